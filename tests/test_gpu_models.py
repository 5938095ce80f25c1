"""Model-level parity on the GPU: ViT encoder, projector and Qwen2 forward/generate through the C ABI
against the oracle (CPU fp32 restatement of the reference) on the same seeded weights and inputs.
fp32 parity mode must agree to 1e-4 (exact-f32 MFMA, different summation order only); the bf16
production mode is compared with bf16-sized tolerances (one rounding = 2^-8 relative)."""
import os

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

VIT = dict(hidden_size=576, intermediate_size=200, num_hidden_layers=2, num_attention_heads=8)  # hd 72, K slab 64
LLM = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
           num_key_value_heads=1, vocab_size=512, image_token_index=500, eos_token_id=499)


def _vit(dev, dtype, mode):
    from cogstream_amd.vision import VisionEncoder
    from cogstream_amd.weights import VisionConfig, random_vit_state
    cfg = VisionConfig(**VIT)
    st = random_vit_state(cfg, seed=3, std=0.05)
    return cfg, st, VisionEncoder(st, cfg, dtype=dtype, device=dev, attn_mode=mode)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("mode", [0, 1])
def test_vit_encode_vs_oracle(dev, dtype, tol, mode):
    from oracle import vision as ov
    cfg, st, enc = _vit(dev, dtype, mode)
    torch.manual_seed(5)
    grid = torch.tensor([[3, 4, 6], [1, 2, 2], [2, 6, 4]])
    merge = torch.tensor([2, 1, 2])
    n = int(grid.prod(1).sum())
    pix = torch.rand(n, 588) * 2 - 1
    ref = ov.encode(st, pix, grid, merge, heads=cfg.num_attention_heads, layers=cfg.num_hidden_layers, mode=mode)
    out = enc(pix.to(dev), grid, merge)
    assert out.shape == ref.shape
    assert rel_err(out.float(), ref) < tol


def test_vit_bf16_pixel_input_and_frame_independence(dev):
    """block-diagonal mode: perturbing one frame must leave every other frame's tokens bit-identical
    (the property that makes frame sharding legal)"""
    cfg, st, enc = _vit(dev, torch.bfloat16, 0)
    torch.manual_seed(6)
    grid, merge = torch.tensor([[4, 4, 4]]), torch.tensor([2])
    pix = (torch.rand(64, 588) * 2 - 1).bfloat16().to(dev)
    a = enc(pix, grid, merge)
    pix2 = pix.clone()
    pix2[16:32] += 0.5
    b = enc(pix2, grid, merge)
    assert torch.equal(a[:4], b[:4]) and torch.equal(a[8:], b[8:]) and not torch.equal(a[4:8], b[4:8])


def test_frame_split_two_stream_encode_is_transparent(dev):
    """cogs_vit_encode cuts a small clip at the frame boundary nearest to half its patches and encodes the halves on two
    streams (frames are independent in block-diagonal mode). Three videos of different grids in ONE call -- the cut falls
    inside the second one, the halves see different video lists, the attention's uniform-segment shortcut is off -- must
    equal (bit for bit) the concatenation of one encode per video, and the oracle within bf16 tolerance; a workspace too
    small for two halves falls back to one stream instead of failing; back-to-back calls on one handle do not race."""
    import ctypes as C
    from cogstream_amd import _lib as L
    from oracle import vision as ov
    cfg, st, enc = _vit(dev, torch.bfloat16, 0)
    torch.manual_seed(61)
    grids = torch.tensor([[3, 8, 12], [5, 6, 10], [2, 4, 6]])
    merges = torch.tensor([2, 2, 2])
    rows = [int(t * a * b) for t, a, b in grids.tolist()]
    pix = (torch.rand(sum(rows), 588) * 2 - 1).bfloat16().to(dev)
    whole = enc(pix, grids, merges)
    parts, r0 = [], 0
    for v in range(3):
        parts.append(enc(pix[r0:r0 + rows[v]], grids[v:v + 1], merges[v:v + 1]))
        r0 += rows[v]
    assert torch.equal(whole, torch.cat(parts))
    again = enc(pix, grids, merges)
    assert torch.equal(whole, again)
    ref = ov.encode(st, pix.float().cpu(), grids, merges, heads=cfg.num_attention_heads, layers=cfg.num_hidden_layers, mode=0)
    assert rel_err(whole.float(), ref) < 3e-2
    # exactly the single-stream workspace (the query adds room for the second set of tables): still fine, same tokens
    need = C.c_size_t()
    n = sum(rows)
    L.check(L.lib.cogs_vit_workspace_bytes(enc.handle.h, n, C.byref(need)))
    ws = torch.empty(need.value - 256 * 1024, dtype=torch.uint8, device=dev)
    out = torch.empty_like(whole)
    gs = (C.c_int64 * 9)(*[int(x) for x in grids.reshape(-1).tolist()])
    ms = (C.c_int64 * 3)(2, 2, 2)
    rc = L.lib.cogs_vit_encode(enc.handle.h, L.current_stream(), pix.data_ptr(), L.dtype_code(pix.dtype), gs, ms, 3, 0,
                               out.data_ptr(), ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    assert rc == L.OK and torch.equal(out, whole)
    # split against UNSPLIT, explicitly: cogs_vit_set_streams(1) keeps the clip on the caller's stream
    try:
        L.check(L.lib.cogs_vit_set_streams(enc.handle.h, 1))
        single = enc(pix, grids, merges)
    finally:
        L.check(L.lib.cogs_vit_set_streams(enc.handle.h, 2))
    assert torch.equal(single, whole)
    for streams in (3, 4):                       # three frame ranges (one per video here) / four (more ranges than videos)
        try:
            L.check(L.lib.cogs_vit_set_streams(enc.handle.h, streams))
            assert torch.equal(enc(pix, grids, merges), whole), streams
        finally:
            L.check(L.lib.cogs_vit_set_streams(enc.handle.h, 2))
    assert L.lib.cogs_vit_set_streams(enc.handle.h, 5) == L.E_INVALID


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 2e-2)])
def test_projector_vs_oracle(dev, dtype, tol):
    from cogstream_amd.vision import Projector
    from cogstream_amd.weights import random_proj_state
    from oracle import vision as ov
    st = random_proj_state(192, 256, std=0.05)
    x = torch.randn(70, 192)
    ref = ov.project(st, x)
    out = Projector(st, dtype=dtype, device=dev)(x.to(dev, dtype))
    assert rel_err(out.float(), ref) < tol


def _llm(dev, dtype):
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    cfg = LlmConfig(**LLM)
    st = random_llm_state(cfg, seed=7, std=0.05)
    return cfg, st, Qwen2Engine(st, cfg, dtype=dtype, device=dev)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_llm_prefill_and_decode_vs_oracle(dev, dtype, tol):
    from oracle import qwen2 as oq
    cfg, st, eng = _llm(dev, dtype)
    kw = dict(heads=cfg.num_attention_heads, kv_heads=cfg.num_key_value_heads, layers=cfg.num_hidden_layers)
    torch.manual_seed(8)
    emb = torch.randn(150, cfg.hidden_size) * 0.5
    hid, kv = oq.forward(st, emb, **kw)
    ref_logits = oq.logits(st, hid[-1])
    cache = eng.new_cache(256)
    res = eng.forward(emb.to(dev, dtype), cache, want_logits=True, want_pooled=True, want_hidden=True)
    assert cache.len == 150
    assert rel_err(res["hidden"].float(), hid) < tol
    assert rel_err(res["logits"], ref_logits) < tol
    assert rel_err(res["pooled"], hid.mean(0)) < tol
    # three decode steps on top of the cache
    for step in range(3):
        e = torch.randn(1, cfg.hidden_size) * 0.5
        hid, kv = oq.forward(st, e, past=kv, **kw)
        r = eng.forward(e.to(dev, dtype), cache)
        assert rel_err(r["logits"], oq.logits(st, hid[-1])) < tol
    # stateless forward (event-summary passes) must equal the cached prefill
    res2 = eng.forward(emb.to(dev, dtype), None, want_logits=False, want_hidden=True)
    assert torch.equal(res2["hidden"], res["hidden"])


def test_llm_greedy_generate_matches_oracle_fp32(dev):
    """token ids are integers: bit-exact against the oracle's greedy search (fp32 parity mode)"""
    from oracle import qwen2 as oq
    cfg, st, eng = _llm(dev, torch.float32)
    kw = dict(heads=cfg.num_attention_heads, kv_heads=cfg.num_key_value_heads, layers=cfg.num_hidden_layers)
    torch.manual_seed(9)
    emb = torch.randn(40, cfg.hidden_size) * 0.5
    ref, first = oq.greedy_generate(st, emb, max_new_tokens=12, eos=[cfg.eos_token_id], rep_penalty=1.05, **kw)
    got = eng.generate(emb.to(dev), max_new_tokens=12, eos_token_id=[cfg.eos_token_id], repetition_penalty=1.05)
    assert got == ref
    allowed = [11, 15, 16, 17, 58, 60, 499]
    ref2, _ = oq.greedy_generate(st, emb, max_new_tokens=6, eos=[499], allowed=allowed, **kw)
    got2 = eng.generate(emb.to(dev), max_new_tokens=6, eos_token_id=[499], allowed_ids=allowed)
    assert got2 == ref2 and all(t in allowed for t in got2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_llm_prefix_kv_reuse_is_transparent(dev, dtype):
    """PrefixKV: a prompt that shares its first rows with the previous one prefills only the rest; the KV rows,
    the logits of the first step and the greedy tokens equal those of a fresh full prefill"""
    from cogstream_amd.llm import PrefixKV
    cfg, st, eng = _llm(dev, dtype)
    torch.manual_seed(21)
    a = (torch.randn(300, cfg.hidden_size) * 0.5).to(dev, dtype)
    b = a.clone()
    b[173:] = (torch.randn(127, cfg.hidden_size) * 0.5).to(dev, dtype)      # differs from row 173 on
    c = torch.cat([a[:90], (torch.randn(45, cfg.hidden_size) * 0.5).to(dev, dtype)])   # shorter, differs from row 90
    slot = PrefixKV(eng)
    d = torch.cat([b, (torch.randn(400, cfg.hidden_size) * 0.5).to(dev, dtype)])   # outgrows the slot's cache
    for emb, want_p in ((a, 0), (a, 298), (b, 173), (d, 300), (c, 90), (c[:50], 48)):
        before = slot.reused
        got = eng.generate(emb, max_new_tokens=8, eos_token_id=[], repetition_penalty=1.05, prefix=slot)
        assert slot.reused - before == want_p
        fresh_cache = eng.new_cache(emb.shape[0] + 8)
        ref = eng.generate(emb, max_new_tokens=8, eos_token_id=[], repetition_penalty=1.05, cache=fresh_cache)
        assert got == ref
        n = emb.shape[0]
        # the reused rows are the same bytes and the re-prefilled rows go through the same kernels as in a full prefill
        assert torch.equal(slot.cache.k[:, :n], fresh_cache.k[:, :n]) and torch.equal(slot.cache.v[:, :n], fresh_cache.v[:, :n])


def test_llm_sampling_runs_and_respects_topk(dev):
    cfg, st, eng = _llm(dev, torch.bfloat16)
    torch.manual_seed(10)
    emb = (torch.randn(20, cfg.hidden_size) * 0.5).to(dev, torch.bfloat16)
    g = torch.Generator().manual_seed(0)
    toks = eng.generate(emb, max_new_tokens=8, do_sample=True, temperature=0.7, top_k=20, top_p=0.8,
                        repetition_penalty=1.05, generator=g, ignore_eos=True)
    assert len(toks) == 8 and all(0 <= t < cfg.vocab_size for t in toks)


def test_processor_gpu_path_equals_host_path(dev):
    """CogStreamProcessor(device=...) returns the same pixel_values (bf16 of the host fp32) and the same text side"""
    from cogstream_amd import processing as pr
    from toy_tokenizer import ToyTokenizer
    tok = ToyTokenizer()
    frames, ts = pr.synthetic_clip(3, 120, 214, kind="drift", clip_idx=2)
    conv = [{"role": "user", "content": [{"type": "video", "video": frames, "timestamps": ts},
                                         {"type": "text", "text": "what moves?"}]}]
    host = pr.CogStreamProcessor(tok)(conversation=conv, add_system_prompt=True, add_generation_prompt=True)
    gpu = pr.CogStreamProcessor(tok, device=dev)(conversation=conv, add_system_prompt=True, add_generation_prompt=True)
    assert gpu["pixel_values"].is_cuda and gpu["pixel_values"].dtype == torch.bfloat16
    assert torch.equal(gpu["pixel_values"].cpu(), host["pixel_values"].bfloat16())
    assert torch.equal(gpu["grid_sizes"], host["grid_sizes"]) and torch.equal(gpu["input_ids"], host["input_ids"])


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 4e-2)])
def test_llm_lora_adapters_vs_unmerged_oracle(dev, dtype, tol):
    """two adapters = two merged weight sets on one handle; each must match the oracle's UNMERGED peft branch
    (result + lora_B(lora_A(x)) * alpha/r), and switching back and forth must not mix them up"""
    from oracle import qwen2 as oq
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import merge_lora, random_lora_state
    cfg, st, base = _llm(dev, dtype)
    kw = dict(heads=cfg.num_attention_heads, kv_heads=cfg.num_key_value_heads, layers=cfg.num_hidden_layers)
    strip = lambda d: {k.replace("base_model.model.model.", ""): v for k, v in d.items()}
    loras = [random_lora_state(cfg, seed=s) for s in (21, 22)]
    engines = [Qwen2Engine(merge_lora(st, None, l, cfg)[0], cfg, dtype=dtype, device=dev) for l in loras]
    torch.manual_seed(10)
    emb = torch.randn(70, cfg.hidden_size) * 0.5
    ref_base = oq.forward(st, emb, **kw)[0]
    refs = [oq.forward(st, emb, lora=strip(l), lora_scaling=16.0 / 8, **kw)[0] for l in loras]
    assert rel_err(refs[0], ref_base) > 0.05 and rel_err(refs[0], refs[1]) > 0.05   # the adapters do something
    for order in ((0, 1), (1, 0), (0, 0)):
        for i in order:
            got = engines[i].forward(emb.to(dev, dtype), None, want_logits=False, want_hidden=True)["hidden"].float()
            assert rel_err(got, refs[i]) < tol
    got = base.forward(emb.to(dev, dtype), None, want_logits=False, want_hidden=True)["hidden"].float()
    assert rel_err(got, ref_base) < tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 4e-2)])
def test_lora_adapters_vs_reference_fixture(dev, dtype, tol):
    """the product's adapter path (merged weight sets on the GPU) against tests/golden/lora.npz -- the reference's model
    object carrying peft-style LoRA modules on the reference's target list (tests/golden/make_golden.py::golden_lora)"""
    from test_oracle_golden import _lora_case
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.vision import Projector
    from cogstream_amd.weights import merge_lora
    g, lcfg, lst, pst, loras, _ = _lora_case()
    emb, vis = torch.from_numpy(g["embeds"]).to(dev, dtype), torch.from_numpy(g["vis"]).to(dev, dtype)
    for a, lo in loras.items():
        ml, mp = merge_lora(lst, pst, lo, lcfg, lora_alpha=float(g["lora_alpha"]))
        eng = Qwen2Engine(ml, lcfg, dtype=dtype, device=dev)
        res = eng.forward(emb, None, want_hidden=True)
        assert rel_err(res["hidden"].float(), torch.from_numpy(g[f"{a}_hidden"])) < tol
        assert rel_err(res["logits"], torch.from_numpy(g[f"{a}_logits"])) < tol
        assert rel_err(Projector(mp, dtype=dtype, device=dev)(vis).float(), torch.from_numpy(g[f"{a}_projected"])) < tol


def test_cogreasoner_set_adapter_switches_llm_and_projector(dev):
    """peft surface of evaluate/answer_generate.py:71-73,181-182 on the host mirror"""
    from oracle import vision as ov
    from cogstream_amd.chat import CogReasoner
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.vision import Projector
    from cogstream_amd.weights import LlmConfig, random_llm_state, random_lora_state, random_proj_state
    cfg = LlmConfig(**LLM)
    st = random_llm_state(cfg, seed=7, std=0.05)
    pst = random_proj_state(576, cfg.hidden_size, seed=4, std=0.05)
    _, _, enc = _vit(dev, torch.float32, 0)
    model = CogReasoner(enc, Projector(pst, dtype=torch.float32, device=dev), Qwen2Engine(st, cfg, dtype=torch.float32, device=dev))
    lora = random_lora_state(cfg, seed=31, proj_dims=(576, cfg.hidden_size))
    model.load_adapter(st, pst, lora, "full_module")
    model.load_adapter(st, pst, random_lora_state(cfg, seed=32), "language_module")     # LLM-only adapter
    with pytest.raises(ValueError):
        model.set_adapter("nope")
    torch.manual_seed(11)
    x = torch.randn(24, 576)
    s = 16.0 / 8
    a0, b0 = lora["base_model.model.model.mm_projector.readout.0.lora_A.weight"], lora["base_model.model.model.mm_projector.readout.0.lora_B.weight"]
    a2, b2 = lora["base_model.model.model.mm_projector.readout.2.lora_A.weight"], lora["base_model.model.model.mm_projector.readout.2.lora_B.weight"]
    F = torch.nn.functional
    h = F.linear(x, pst["readout.0.weight"], pst["readout.0.bias"]) + F.linear(F.linear(x, a0), b0) * s
    h = F.gelu(h)
    ref_full = F.linear(h, pst["readout.2.weight"], pst["readout.2.bias"]) + F.linear(F.linear(h, a2), b2) * s
    ref_base = ov.project(pst, x)
    model.set_adapter("full_module")
    assert model.active_adapter == "full_module"
    assert rel_err(model.mm_projector(x.to(dev)).cpu(), ref_full) < 1e-4
    model.set_adapter("language_module")                       # no projector LoRA -> base projector
    assert rel_err(model.mm_projector(x.to(dev)).cpu(), ref_base) < 1e-4
    assert model.llm is not model._adapters["full_module"][0]
    model.set_adapter("base")
    assert rel_err(model.mm_projector(x.to(dev)).cpu(), ref_base) < 1e-4


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 2e-2)])
def test_llm_forward_segments_equals_separate_passes(dev, dtype, tol):
    """cogs_llm_forward_segments (one var-len prefill, per-sequence positions / causal attention / mean pooling)
    against one stateless forward per sequence -- the reference's K event-summary passes + the question pass"""
    from oracle import qwen2 as oq
    cfg, st, eng = _llm(dev, dtype)
    kw = dict(heads=cfg.num_attention_heads, kv_heads=cfg.num_key_value_heads, layers=cfg.num_hidden_layers)
    torch.manual_seed(12)
    lens = [150, 1, 37, 260, 9]                       # ragged, incl. a single token and > 2 attention q-blocks
    emb = torch.randn(sum(lens), cfg.hidden_size) * 0.5
    got = eng.forward_segments(emb.to(dev, dtype), lens)
    assert got.shape == (len(lens), cfg.hidden_size) and got.dtype == torch.float32
    o = 0
    for i, n in enumerate(lens):
        seg = emb[o:o + n]
        one = eng.forward(seg.to(dev, dtype), None, want_logits=False, want_pooled=True)["pooled"]
        assert rel_err(got[i], one) < tol
        if dtype == torch.float32:
            assert rel_err(got[i].cpu(), oq.forward(st, seg, **kw)[0].mean(0)) < 1e-4
        o += n
    # a sequence's mean does not depend on which other sequences share the forward: what lets parallel.
    # pooled_means_sharded spread them over ranks with identical results
    parts = list(emb.to(dev, dtype).split(lens))
    sub = eng.forward_segments(torch.cat([parts[3], parts[0]]), [lens[3], lens[0]])
    assert torch.equal(sub[0], got[3]) and torch.equal(sub[1], got[0])


def test_full_size_encoder_is_frame_separable(dev):
    """BASELINE.json cfg2 at real dimensions (64 x 480p frames, ViT 1152 x 27, projector 3584): encoding frame
    shards separately and concatenating must be BIT-identical to encoding the clip at once -- the property the
    multi-GPU frame sharding rests on -- and GPU pre-processing must be deterministic"""
    from cogstream_amd import processing as pr
    from cogstream_amd.preprocess_gpu import preprocess_videos_gpu
    from cogstream_amd.vision import Projector, VisionEncoder
    from cogstream_amd.weights import VisionConfig, random_proj_state, random_vit_state
    cfg = VisionConfig()
    enc = VisionEncoder(random_vit_state(cfg, 0, dev, torch.bfloat16), cfg, dtype=torch.bfloat16, device=dev)
    proj = Projector(random_proj_state(cfg.hidden_size, 3584, 1, dev, torch.bfloat16), dtype=torch.bfloat16, device=dev)
    frames, _ = pr.synthetic_clip(64, kind="drift")
    d = torch.from_numpy(frames).to(dev)
    f1, f2 = preprocess_videos_gpu([d]), preprocess_videos_gpu([d])
    assert torch.equal(f1["pixel_values"], f2["pixel_values"]) and f1["grid_sizes"].tolist() == [[64, 22, 42]]
    pix, merge = f1["pixel_values"], torch.tensor([2])
    full = proj(enc(pix, f1["grid_sizes"], merge))
    assert full.shape == (64 * 231, 3584) and bool(torch.isfinite(full.float()).all())
    per = 22 * 42
    parts = []
    for b, e in ((0, 24), (24, 25), (25, 64)):                       # ragged shards, incl. a single frame
        parts.append(proj(enc(pix[b * per:e * per], torch.tensor([[e - b, 22, 42]]), merge)))
    assert torch.equal(torch.cat(parts), full)


def test_full_size_llm_decode_as_accurate_as_prefill(dev):
    """Qwen2-7B dimensions, random weights: prefill(S) + one cached decode step against prefill(S+1) -- the GEMV
    path with the fused KV-row write, split-KV decode attention and the fused RMSNorm at full size. Over 28 random
    layers bf16 rounding alone moves the logits by ~5 % of their range, so the yardstick is the fp32 parity engine
    on the same weights: the decode path must be as close to it as the prefill path is."""
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    cfg = LlmConfig()
    st = random_llm_state(cfg, 2, dev, torch.bfloat16)
    eng = Qwen2Engine(st, cfg, dtype=torch.bfloat16, device=dev)
    torch.manual_seed(3)
    S = 2047                      # a 2 048-token prefill over all 28 layers and the real 152 064-entry vocabulary
    emb = (torch.randn(S + 1, cfg.hidden_size, device=dev) * 0.02).to(torch.bfloat16)
    ref = eng.forward(emb, None)["logits"]
    cache = eng.new_cache(S + 8)
    eng.forward(emb[:S], cache, want_logits=False)
    got = eng.forward(emb[S:], cache)["logits"]
    assert cache.len == S + 1
    eng32 = Qwen2Engine({k: v.float() for k, v in st.items()}, cfg, dtype=torch.float32, device=dev)
    truth = eng32.forward(emb.float(), None)["logits"]
    rms = lambda a: float((a - truth).pow(2).mean().sqrt())
    assert rms(ref) < 0.03 * float(truth.abs().max())              # bf16 prefill within bf16 noise of fp32
    assert rms(got) < 1.25 * rms(ref) + 1e-3                       # the decode path is no worse
    assert rel_err(got, ref) < 6e-2
    # production depth, explicit figures: the 28-layer bf16 prefill against the fp32 parity mode of the same kernels
    # (itself pinned to the reference's logits at 5e-6, tests/test_gpu_golden.py) -- max-norm, RMS and direction
    cos = float(torch.nn.functional.cosine_similarity(ref.double(), truth.double(), dim=0))
    print(f"Qwen2-7B dims, S = {S + 1}: bf16 vs fp32 logits max {rel_err(ref, truth):.2e}, "
          f"rms {rms(ref) / float(truth.pow(2).mean().sqrt()):.2e}, cosine {cos:.6f}")
    assert rel_err(ref, truth) < 8e-2 and cos > 0.995
    assert truth.shape == (152064,)
    del eng, eng32, cache
    torch.cuda.empty_cache()


def test_c_abi_error_behaviour(dev):
    """Errors are status codes, never exceptions or device faults (include/cogs.h): entry points refuse to run before
    their weights are loaded, with a missing / short workspace, with shapes the kernels do not take, or with a KV
    cache that is too small -- and the handle stays usable afterwards. The Python host raises CogsError exactly where
    the reference would raise from torch (model/cogreasoner_chat.py error behaviour)."""
    import ctypes as C
    from cogstream_amd import _lib as L
    from cogstream_amd import ops
    INVALID, WORKSPACE = -1, -4
    h = C.c_void_p()
    assert L.lib.cogs_create(0, C.byref(h)) == 0
    st = L.current_stream()
    nbytes = C.c_size_t()
    x = torch.zeros(64, 588, device=dev, dtype=torch.bfloat16)
    grid = (C.c_int64 * 3)(1, 8, 8)
    ms = (C.c_int64 * 1)(2)
    # a fresh handle has no weights
    assert L.lib.cogs_vit_workspace_bytes(h, 64, C.byref(nbytes)) == INVALID
    assert L.lib.cogs_vit_encode(h, st, x.data_ptr(), L.dtype_code(x.dtype), grid, ms, 1, 0, x.data_ptr(), None, 0) == INVALID
    assert L.lib.cogs_llm_workspace_bytes(h, 8, 8, C.byref(nbytes)) == INVALID
    assert L.lib.cogs_project(h, st, x.data_ptr(), 16, x.data_ptr(), None, 0) == INVALID
    assert L.lib.cogs_destroy(h) == 0
    assert L.lib.cogs_create(0, None) == INVALID and L.lib.cogs_destroy(None) == 0      # destroy(NULL) is a no-op, like free()

    cfg, _, eng = _llm(dev, torch.bfloat16)
    hh = eng.handle.h
    emb = (torch.randn(24, cfg.hidden_size, device=dev) * 0.5).to(torch.bfloat16)
    logits = torch.empty(cfg.vocab_size, device=dev, dtype=torch.float32)
    assert L.lib.cogs_llm_workspace_bytes(hh, 24, 24, C.byref(nbytes)) == 0 and nbytes.value > 0
    ws = torch.empty(nbytes.value, device=dev, dtype=torch.uint8)
    args = (hh, st, emb.data_ptr(), 24)
    assert L.lib.cogs_llm_forward(*args, None, logits.data_ptr(), None, None, None, 0) == WORKSPACE
    assert L.lib.cogs_llm_forward(*args, None, logits.data_ptr(), None, None, ws.data_ptr(), nbytes.value // 2) == WORKSPACE
    small = eng.new_cache(16)                                    # 24 rows do not fit 16
    assert L.lib.cogs_llm_forward(*args, C.byref(small.struct), logits.data_ptr(), None, None, ws.data_ptr(), ws.numel()) == INVALID
    assert small.len == 0
    assert L.lib.cogs_llm_forward(hh, st, emb.data_ptr(), 0, None, logits.data_ptr(), None, None, ws.data_ptr(), ws.numel()) == INVALID
    pooled = torch.empty(2, cfg.hidden_size, device=dev, dtype=torch.float32)
    for cu in ((0, 30, 24), (1, 10, 24), (0, 10, 10, 24)):       # not ending at S / not starting at 0 / empty segment
        arr = (C.c_int32 * len(cu))(*cu)
        assert L.lib.cogs_llm_forward_segments(hh, st, emb.data_ptr(), 24, arr, len(cu) - 1, pooled.data_ptr(),
                                               ws.data_ptr(), ws.numel()) == INVALID
    # the handle still works, and the host wrapper turns a status into an exception
    ok = eng.forward(emb)["logits"]
    assert torch.isfinite(ok).all()
    with pytest.raises(L.CogsError):
        eng.forward(emb, eng.new_cache(8))
    with pytest.raises(L.CogsError):
        ops.gemm(torch.zeros(8, 40, device=dev, dtype=torch.bfloat16), torch.zeros(16, 40, device=dev, dtype=torch.bfloat16))  # K % 64
    with pytest.raises(L.CogsError):
        z = torch.zeros(4, 96, device=dev, dtype=torch.bfloat16)
        ops.attention(z, z[:, :64], z[:, :64], hq=3, hkv=2, head_dim=32)   # query heads not a multiple of kv heads


def test_real_dimension_vit_layers_vs_oracle(dev):
    """The production kernels at the production shapes against the (reference-pinned) oracle: ViT at VideoLLaMA3
    dimensions (hidden 1152, 16 heads of 72, MLP 4304 -> padded 4352), 2 layers, 4 frames of the cfg2 grid 22 x 42
    (924 patches per frame, 3696 rows: the ping-pong GEMM with the rotary LUT epilogue, the ragged 924-row attention
    blocks, LayerNorm, the 2x2 merge) + the 1152 -> 3584 projector. bf16 within bf16 rounding of the fp32 oracle, and
    the exact-fp32 mode of the same path within 1e-4."""
    from cogstream_amd.vision import Projector, VisionEncoder
    from cogstream_amd.weights import VisionConfig, random_proj_state, random_vit_state
    from oracle import vision as ov
    cfg = VisionConfig(num_hidden_layers=2)
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads) == (1152, 4304, 16)
    st = random_vit_state(cfg, seed=13, std=0.03)
    pst = random_proj_state(cfg.hidden_size, 3584, seed=14, std=0.02)
    torch.manual_seed(15)
    grid, merge = torch.tensor([[4, 22, 42]]), torch.tensor([2])
    pix = torch.rand(4 * 924, 588) * 2 - 1
    ref_tok = ov.encode(st, pix, grid, merge, heads=16, layers=2, mode=0)
    ref = ov.project(pst, ref_tok)
    for dtype, tol in ((torch.bfloat16, 3e-2), (torch.float32, 1e-4)):
        enc = VisionEncoder(st, cfg, dtype=dtype, device=dev)
        proj = Projector(pst, dtype=dtype, device=dev)
        tok = enc(pix.to(dev, dtype), grid, merge)
        out = proj(tok)
        assert tok.shape == (4 * 231, 1152) and out.shape == (4 * 231, 3584)
        assert rel_err(tok.float(), ref_tok) < tol, dtype
        assert rel_err(out.float(), ref) < tol, dtype


def test_production_depth_vit_27_layers_vs_oracle(dev):
    """All 27 layers at the production width (hidden 1152, 16 heads of 72, MLP 4304), 2 frames of the cfg2 grid 22 x 42
    (1 848 patches), + the projector, against the reference-pinned oracle run in fp32 AND in bf16 (the oracle computes
    in the dtype of its weights, like the reference's .to(bfloat16) model, evaluate/answer_generate.py:176):
      * the exact-fp32 mode of the HIP path within 1e-4 of the fp32 oracle through all 27 layers,
      * the production bf16 path (LayerNorm folded into the GEMMs, pipelined attention) as close to the fp32 oracle as
        the oracle's own bf16 run is (x 1.5), in max-norm and RMS -- the criterion of tests/test_gpu_golden.py at depth."""
    from cogstream_amd.vision import Projector, VisionEncoder
    from cogstream_amd.weights import VisionConfig, random_proj_state, random_vit_state
    from oracle import vision as ov
    from test_gpu_golden import _as_good_as_reference_bf16
    cfg = VisionConfig()
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_hidden_layers) == (1152, 4304, 16, 27)
    st = random_vit_state(cfg, seed=21, std=0.03)
    pst = random_proj_state(cfg.hidden_size, 3584, seed=22, std=0.02)
    torch.manual_seed(23)
    grid, merge = torch.tensor([[2, 22, 42]]), torch.tensor([2])
    pix = (torch.rand(2 * 924, 588) * 2 - 1).bfloat16().float()          # bf16-representable pixels: same input for every run
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref_tok = ov.encode(st, pix, grid, merge, heads=16, layers=27, mode=0)
    ref = ov.project(pst, ref_tok)
    st16 = {k: v.bfloat16() for k, v in st.items()}
    pst16 = {k: v.bfloat16() for k, v in pst.items()}
    r16_tok = ov.encode(st16, pix.bfloat16(), grid, merge, heads=16, layers=27, mode=0)
    r16 = ov.project(pst16, r16_tok)
    enc32 = VisionEncoder(st, cfg, dtype=torch.float32, device=dev)
    tok32 = enc32(pix.to(dev), grid, merge)
    out32 = Projector(pst, dtype=torch.float32, device=dev)(tok32)
    e_tok, e_out = rel_err(tok32, ref_tok), rel_err(out32, ref)
    print(f"27 layers, fp32 parity mode vs fp32 oracle: tokens {e_tok:.2e}, projected {e_out:.2e}")
    assert e_tok < 1e-4 and e_out < 1e-4
    enc = VisionEncoder(st, cfg, dtype=torch.bfloat16, device=dev)
    assert enc.packed.fold_ln                                            # the production configuration
    tok = enc(pix.to(dev, torch.bfloat16), grid, merge)
    out = Projector(pst, dtype=torch.bfloat16, device=dev)(tok)
    _as_good_as_reference_bf16(tok.float(), r16_tok.float(), ref_tok, "27-layer ViT tokens")
    _as_good_as_reference_bf16(out.float(), r16.float(), ref, "27-layer ViT + projector")


@pytest.mark.parametrize("kind", ["outlier_channels", "large_mean"])
def test_ln_fold_with_outlier_channels_and_large_row_means(dev, kind):
    """The LayerNorm fold on a residual stream shaped like a trained SigLIP-style encoder's: a few channels carry
    values 60 x the rest (planted through the patch-embedding bias, with the small LayerNorm gains such channels come
    with), or every row sits far from zero (|mean / std| ~ 10). Real width, 4 layers, 2 frames of the cfg2 grid. The
    folded path must be as accurate against the fp32 oracle as the UNFUSED bf16 path of the same kernels -- no
    data-dependent fallback is needed because the folded weight rows sum to zero exactly (weights.zero_sum_rows), which
    makes the GEMM on x equal the GEMM on x - mean whatever the mean."""
    from cogstream_amd.vision import VisionEncoder
    from cogstream_amd.weights import VisionConfig, random_vit_state
    from oracle import vision as ov
    cfg = VisionConfig(num_hidden_layers=4)
    st = random_vit_state(cfg, seed=31, std=0.03)
    hot = [7, 300, 901]
    b = st["embeddings.patch_embedding.bias"].clone()
    if kind == "outlier_channels":
        b[hot] = torch.tensor([60.0, -75.0, 90.0])
        for i in range(cfg.num_hidden_layers):
            for ln in ("layer_norm1", "layer_norm2"):
                g = st[f"encoder.layers.{i}.{ln}.weight"].clone()
                g[hot] = 0.05
                st[f"encoder.layers.{i}.{ln}.weight"] = g
    else:
        b += 12.0
    st["embeddings.patch_embedding.bias"] = b
    torch.manual_seed(33)
    grid, merge = torch.tensor([[2, 22, 42]]), torch.tensor([2])
    pix = (torch.rand(2 * 924, 588) * 2 - 1).bfloat16().float()
    ref = ov.encode(st, pix, grid, merge, heads=16, layers=4, mode=0)
    # what the rows look like going into layer 0 (for the record)
    x0 = pix @ st["embeddings.patch_embedding.weight"].reshape(1152, -1).t() + b
    ratio = float((x0.mean(1).abs() / x0.std(1)).max())
    peak = float(x0.abs().max() / x0.abs().median())
    print(f"{kind}: max |mean/std| of a row {ratio:.1f}, largest / median magnitude {peak:.0f}")
    assert (peak > 40) if kind == "outlier_channels" else (ratio > 8)
    errs = {}
    for fold in (True, False):
        enc = VisionEncoder(st, cfg, dtype=torch.bfloat16, device=dev, fold_ln=fold)
        assert enc.packed.fold_ln is fold
        tok = enc(pix.to(dev, torch.bfloat16), grid, merge)
        assert bool(torch.isfinite(tok.float()).all())
        # judged on the ORDINARY channels: the planted ones are 300 x larger, and their own bf16 rounding would be all
        # that a max-norm or an RMS over every channel sees
        keep = torch.ones(ref.shape[1], dtype=torch.bool)
        if kind == "outlier_channels":
            keep[hot] = False
        r_, d = ref[:, keep].double(), (tok.float().cpu() - ref)[:, keep].double()
        errs[fold] = (float(d.abs().max() / r_.abs().max()), float(d.pow(2).mean().sqrt() / r_.pow(2).mean().sqrt()))
    print(f"{kind}: folded max {errs[True][0]:.2e} rms {errs[True][1]:.2e} | unfused max {errs[False][0]:.2e} rms {errs[False][1]:.2e}")
    assert errs[True][0] <= 1.5 * errs[False][0] + 1e-3 and errs[True][1] <= 1.5 * errs[False][1] + 1e-4
    # (large_mean: rows of 12 +- 0.4 stored in bf16 carry a quantisation noise of 15 % of their spread -- BOTH paths, and the
    # reference's own bf16 run, sit at ~0.14 of the fp32 result there; the point of the case is that the fold adds nothing)
    assert errs[True][0] < (5e-2 if kind == "outlier_channels" else 0.25)


def test_real_dimension_llm_layer_vs_oracle(dev):
    """Qwen2-7B dimensions (hidden 3584, 28 query / 4 kv heads of 128, MLP 18944) with one layer and a 4096-entry
    vocabulary: a 1100-token prefill (ping-pong GEMMs with the rotary / SwiGLU / residual epilogues, causal GQA
    attention over 9 query blocks) and three decode steps (GEMV path, split-KV attention) against the oracle."""
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    from oracle import qwen2 as oq
    cfg = LlmConfig(num_hidden_layers=1, vocab_size=4096, image_token_index=4000, eos_token_id=4001)
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads) == (3584, 18944, 28, 4)
    st = random_llm_state(cfg, seed=16, std=0.02)
    kw = dict(heads=28, kv_heads=4, layers=1)
    torch.manual_seed(17)
    emb = torch.randn(1103, cfg.hidden_size) * 0.5
    hid, _ = oq.forward(st, emb, **kw)
    eng = Qwen2Engine(st, cfg, dtype=torch.bfloat16, device=dev)
    cache = eng.new_cache(1110)
    res = eng.forward(emb[:1100].to(dev, torch.bfloat16), cache, want_hidden=True)
    assert rel_err(res["hidden"].float(), hid[:1100]) < 3e-2
    assert rel_err(res["logits"], oq.logits(st, hid[1099])) < 3e-2
    for i in range(1100, 1103):
        r = eng.forward(emb[i:i + 1].to(dev, torch.bfloat16), cache)
        assert rel_err(r["logits"], oq.logits(st, hid[i])) < 3e-2


def test_production_depth_qwen2_28_layers_vs_oracle(dev):
    """All 28 decoder layers at the Qwen2-7B width (hidden 3584, 28 query / 4 kv heads of 128, MLP 18944; a 4 096-entry
    vocabulary keeps the host copy of the weights at 26 GB) against the reference-pinned oracle on a 96-token prompt and
    two cached decode steps: the fp32 parity mode within 1e-4 through all 28 layers, the bf16 production path as close
    to the fp32 oracle as the oracle's own bf16 run is (x 1.5; the reference runs the model in bf16 on a GPU,
    evaluate/answer_generate.py:176). Weights are drawn on the GPU and copied to the host for the oracle."""
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    from oracle import qwen2 as oq
    from test_gpu_golden import _as_good_as_reference_bf16
    cfg = LlmConfig(vocab_size=4096, image_token_index=4000, eos_token_id=4001)
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
            cfg.num_key_value_heads) == (3584, 18944, 28, 28, 4)
    st = random_llm_state(cfg, seed=41, device=dev, dtype=torch.float32, std=0.02)
    host = {k: v.cpu() for k, v in st.items()}
    kw = dict(heads=28, kv_heads=4, layers=28)
    torch.manual_seed(43)
    S = 96
    emb = (torch.randn(S + 2, cfg.hidden_size) * 0.5).bfloat16().float()         # bf16-representable: same input everywhere
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    hid, _ = oq.forward(host, emb, **kw)
    want = torch.stack([oq.logits(host, hid[i]) for i in (S - 1, S, S + 1)])
    host16 = {k: v.bfloat16() for k, v in host.items()}
    hid16, _ = oq.forward(host16, emb.bfloat16(), **kw)
    want16 = torch.stack([oq.logits(host16, hid16[i]).float() for i in (S - 1, S, S + 1)])
    del host16

    def run(dtype):
        eng = Qwen2Engine(st, cfg, dtype=dtype, device=dev)
        cache = eng.new_cache(S + 8)
        out = [eng.forward(emb[:S].to(dev, dtype), cache)["logits"].clone()]
        for i in (S, S + 1):
            out.append(eng.forward(emb[i:i + 1].to(dev, dtype), cache)["logits"].clone())
        del eng
        torch.cuda.empty_cache()
        return torch.stack(out).cpu()

    got32 = run(torch.float32)
    e32 = rel_err(got32, want)
    print(f"28 layers, fp32 parity mode vs fp32 oracle (prefill + 2 decode steps): {e32:.2e}")
    assert e32 < 1e-4
    got16 = run(torch.bfloat16)
    _as_good_as_reference_bf16(got16.float(), want16, want, "28-layer Qwen2 logits (prefill + 2 decode steps)")


def test_ragged_frame_shards_equal_whole_clip_bit_for_bit(dev):
    """20 frames of the cfg3 grid (200 patches each) at the real ViT width, 3 layers: 4000 rows whole, 2 x 2000 rows
    sharded -- 2000 is not a multiple of the 256-row GEMM tile, so the last frames of a shard run through the
    ragged-block epilogues (general path, per-row rotary table) while the same rows sit in interior tiles (pair
    epilogue, LDS rotary LUT, LayerNorm statistics / folding) in the whole-clip encode. Frame sharding over GPUs
    relies on the two agreeing bit for bit (every epilogue spells the rotary rotation and the row statistics the same
    way: csrc/gemm_epilogue.h rope_rot / EPI_ROWSTAT)."""
    from cogstream_amd.vision import VisionEncoder
    from cogstream_amd.weights import VisionConfig, random_vit_state
    cfg = VisionConfig(num_hidden_layers=3)
    enc = VisionEncoder(random_vit_state(cfg, 0, dev, torch.bfloat16), cfg, device=dev)
    assert enc.packed.fold_ln                                            # the production configuration
    T, gh, gw = 20, 10, 20
    g = torch.Generator(device=dev).manual_seed(3)
    pix = (torch.rand(T * gh * gw, 588, generator=g, device=dev) * 2 - 1).bfloat16()
    merge = torch.tensor([2])
    whole = enc(pix, torch.tensor([[T, gh, gw]]), merge).clone()
    for cut in (10, 7):
        a = enc(pix[:cut * 200], torch.tensor([[cut, gh, gw]]), merge).clone()
        b = enc(pix[cut * 200:], torch.tensor([[T - cut, gh, gw]]), merge).clone()
        assert torch.equal(whole, torch.cat([a, b])), cut


def test_content_key_of_gpu_resident_clips(dev):
    """processing.content_key fingerprints a clip that already lives on the GPU there (no 300 MB copy back to the host
    per request): equal content -> equal key, any changed byte / swapped frames / other shape -> another key"""
    from cogstream_amd import processing as pr
    clip = torch.from_numpy(pr.synthetic_clip(6, 60, 100, kind="drift", clip_idx=3)[0]).to(dev)
    k0 = pr.content_key(clip)
    assert k0.startswith("gpu:") and k0 == pr.content_key(clip.clone())
    other = clip.clone()
    other[3, 17, 5, 1] ^= 1
    swapped = clip[[1, 0, 2, 3, 4, 5]].contiguous()
    keys = {k0, pr.content_key(other), pr.content_key(swapped), pr.content_key(clip[:5].contiguous()),
            pr.content_key(clip.view(6, 100, 60, 3))}
    assert len(keys) == 5
    proc = pr.CogStreamProcessor(__import__("toy_tokenizer").ToyTokenizer(), device=dev)
    conv = [{"role": "user", "content": [{"type": "video", "video": clip, "timestamps": [0.0, 1, 2, 3, 4, 5]}, {"type": "text", "text": "q?"}]}]
    assert proc(conversation=conv)["video_keys"] == [k0]


def test_encode_project_equals_encoder_then_projector_bit_for_bit(dev):
    """cogs_vit_encode_project (round 6: every frame range projects its own tokens on its own stream) must give the bits of
    cogs_vit_encode followed by cogs_project -- three videos of different grids in one call, 1 / 2 / 3 streams."""
    from cogstream_amd import _lib as L
    from cogstream_amd.vision import Projector, VisionEncoder
    from cogstream_amd.weights import VisionConfig, random_proj_state, random_vit_state
    vcfg = VisionConfig(hidden_size=576, intermediate_size=200, num_hidden_layers=3, num_attention_heads=8)
    enc = VisionEncoder(random_vit_state(vcfg, seed=3, std=0.05), vcfg, dtype=torch.bfloat16, device=dev)
    proj = Projector(random_proj_state(vcfg.hidden_size, 256, std=0.05), dtype=torch.bfloat16, device=dev)
    grids = torch.tensor([[3, 4, 6], [5, 8, 8], [2, 10, 4]])
    merges = torch.tensor([2, 2, 2])
    n = int((grids[:, 0] * grids[:, 1] * grids[:, 2]).sum())
    g = torch.Generator(device=dev).manual_seed(n)
    pix = (torch.rand(n, 588, generator=g, device=dev) * 2 - 1).bfloat16()
    try:
        for s in (1, 2, 3):
            L.check(L.lib.cogs_vit_set_streams(enc.handle.h, s))
            tok = enc(pix, grids, merges)
            want = proj(tok)
            tok2, got = enc.encode_project(pix, grids, merges, proj)
            torch.cuda.synchronize()
            assert torch.equal(tok2, tok), s
            assert torch.equal(got, want), (s, float((got.float() - want.float()).abs().max()))
    finally:
        L.check(L.lib.cogs_vit_set_streams(enc.handle.h, 2))


def test_workspace_sizes_are_the_sum_of_their_buffers(dev):
    """The *_workspace_bytes queries return the one number callers cache their workspaces by: every buffer of the layout,
    each rounded up to 256 bytes, in the tiny bf16 head_dim-128 Qwen2 (tests/test_gpu_rows.py) and the tiny ViT of
    tests/golden/vit_tiny.npz. The split count is test_gpu_rows._nsplit without its cap of 127 (128 for the single-row
    step: no tails there); no case here comes near either cap."""
    import ctypes as C
    from cogstream_amd import _lib as L

    def total(*sizes):
        return sum((int(s) + 255) // 256 * 256 for s in sizes)

    def nsplit(ctx):
        return max(min(max((ctx + 255) // 256, 32), (ctx + 63) // 64), 1)

    def query(fn, *args):
        n = C.c_size_t()
        L.check(fn(*args, C.byref(n)))
        return n.value

    cfg, _, eng = _llm(dev, torch.bfloat16)
    H, I, hq, hkv, hd = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    assert hd == 128
    qd = (hq + 2 * hkv) * hd
    eng._activate()
    for S, ctx in ((1, 1), (5, 5), (1, 300), (24, 24)):
        want = total(S * H * 2, S * H * 2, S * qd * 2, S * hq * hd * 2, S * I * 2,      # x, ln, qkv, attention out, MLP hidden
                     S * (hd // 2) * 2 * 4,                                             # (cos, sin) table
                     nsplit(ctx) * hq * (hd + 2) * 4,                                   # decode-attention partials
                     S * 4, (S + 1) * 4)                                                # row positions, cu_seqlens
        assert query(L.lib.cogs_llm_workspace_bytes, eng.handle.h, S, ctx) == want, (S, ctx)
    for R, prefix in ((1, 1), (3, 40), (16, 300)):
        want = total(R * H * 2, R * H * 2, R * qd * 2, R * hq * hd * 2, R * I * 2, R * (hd // 2) * 2 * 4, R * 4,
                     (nsplit(prefix) + 1) * R * hq * (hd + 2) * 4)                      # prefix partials + one for the tails
        assert query(L.lib.cogs_llm_decode_rows_workspace_bytes, eng.handle.h, R, prefix) == want, (R, prefix)

    vcfg, _, enc = _vit(dev, torch.bfloat16, 0)
    VH, vhd = vcfg.hidden_size, vcfg.hidden_size // vcfg.num_attention_heads
    ipad, ppad = enc.packed.inter_pad, enc.packed.patch_pad
    assert (ipad, ppad) == (256, 640)                                                   # 200 and 588 up to the 64-wide K slab
    enc._activate()
    for N in (4, 64):
        want = total(N * ppad * 2, N * VH * 2, N * VH * 2, N * max(4 * VH, ipad) * 2,   # padded patches, x, ln, [qkv | att] / MLP
                     N * (vhd // 2) * 2 * 4,                                            # (cos, sin) table
                     (N + 1) * 4, N * 4, N * 4,                                         # cu_seqlens (frames <= patches), lo, hi
                     28 * 1024) + 256 * 1024                                            # rotary LUT; tables of further frame ranges
        assert query(L.lib.cogs_vit_workspace_bytes, enc.handle.h, N) == want, N
