"""generate(num_return_sequences=N) on the GPU, layer by layer: the multi-row weight-streaming GEMM (csrc/gemm_rows.hip)
against the fp64 reference of tests/gemm_reference.py, the shared-prefix decode attention (csrc/attn_decode.hip, rows form)
against tests/attn_reference.py, the lockstep step (cogs_llm_decode_rows) teacher-forced against the CPU oracle and against
the single-row decode path, and the host loop of Qwen2Engine.generate / CogReasoner.generate."""
from __future__ import annotations

import ctypes as C
import math

import pytest
import torch

import attn_reference as AR
import gemm_reference as R
import gemv_reference as G

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
TRACE16, TRACE32 = 0x7F7F, 0x7F7F7F7F        # finite tracer patterns, as in test_gpu_gemm_conformance.py
HD = 128


def _L():
    from cogstream_amd import _lib
    return _lib


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


def _filled(shape, dtype, dev):
    n = math.prod(shape)
    if dtype == F32:
        return torch.full((n,), TRACE32, dtype=torch.int32, device=dev).view(F32).view(*shape)
    return torch.full((n,), TRACE16, dtype=torch.int16, device=dev).view(dtype).view(*shape)


# ------------------------------------------------------------------------------------------------- 1. cogs_gemm_rows
def _operands(dev, M, N, K, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    a = (torch.randn(M, K, generator=g, device=dev) * 0.7 + 0.1).to(BF16)
    w = (torch.randn(N, K, generator=g, device=dev) / math.sqrt(K)).to(BF16)
    return a, w, g


def run_rows_cell(dev, M, N, K, *, bias=False, res=None, act=R.ACT_NONE, out_f32=False, rope=False, rope_cols=0, q_cols=0,
                  q_scale=0.125, seed=1, cols=None):
    """one cogs_gemm_rows; every output element (or the columns `cols`) against its own fp64 band; the guard rows above and
    below C and the guard columns beside it keep their bits. res: None | "sep" | "inplace"; rope: per-row interleaved table;
    q_cols > 0: q_scale on the columns below it (2^-3 unless given: an exact multiply, which adds nothing to the band)"""
    from cogstream_amd import ops
    a, w, g = _operands(dev, M, N, K, seed)
    swiglu = act == R.ACT_SWIGLU
    ocols = N // 2 if swiglu else N
    odt = F32 if out_f32 else BF16
    cbuf = _filled((M + 2, ocols + 16), odt, dev)
    cview = cbuf[1:M + 1, 8:8 + ocols]
    inside = torch.zeros(cbuf.shape, dtype=torch.bool, device=dev)
    inside[1:M + 1, 8:8 + ocols] = True
    kw = dict(act=act, out_f32=out_f32, out=cview)
    bias_t = res_t = rope_r = None
    if bias:
        bias_t = torch.randn(N, generator=g, device=dev).to(BF16)
        kw["bias"] = bias_t
    if rope:
        ang = torch.rand(M, HD // 2, generator=g, device=dev) * 6.0          # a different position per row
        cos, sin = ang.cos(), ang.sin()
        kw.update(rope_cos=torch.stack([cos, sin], -1).contiguous(), rope_cols=rope_cols, head_dim=HD)
        rope_r = R.Rope(cos.double(), sin.double(), rope_cols, HD)
    if res == "sep":
        res_t = torch.randn(M, N, generator=g, device=dev).to(BF16)
        kw["residual"] = res_t
    elif res == "inplace":
        res_t = torch.randn(M, N, generator=g, device=dev).to(BF16)
        cview.copy_(res_t)
        kw["residual"] = cview
    sel = slice(None) if cols is None else cols
    acc, bound = R.product_and_bound(a, w[sel])
    if q_cols:
        kw.update(q_scale=q_scale, q_cols=q_cols)
    guard = _bits(cbuf)[~inside].clone()
    ref, tol = R.epilogue(acc, bound, cols=cols, bias=bias_t, rope=rope_r, q_scale=q_scale if q_cols else None, q_cols=q_cols, act=act,
                          residual=res_t[:, sel] if res_t is not None else None, out_f32=out_f32, out_dtype=odt)
    ops.gemm_rows(a, w, **kw)
    torch.cuda.synchronize()
    what = f"gemm_rows M={M} N={N} K={K} bias={bias} res={res} act={act} f32={out_f32} rope={rope} q={q_cols}"
    assert torch.equal(_bits(cbuf)[~inside], guard), what + ": guard rows / columns around C changed"
    R.assert_within(cview[:, sel] if cols is not None else cview, ref, tol, what)


@pytest.mark.parametrize("M", [1, 2, 7, 15, 16])
def test_gemm_rows_n_edges(dev, M):
    """one column block, a ragged last block inside the k-split form, and both sides of the switch to one block per wave
    (1024 column blocks = N 16384)"""
    for N in (16, 132, 16380, 16388):
        run_rows_cell(dev, M, N, 192, seed=N + M)


@pytest.mark.parametrize("M", [1, 2, 7, 15, 16])
def test_gemm_rows_k_edges(dev, M):
    """one k-chunk (seven of the eight k-split waves idle), fewer chunks than a batch, the model's two K"""
    for K in (64, 192, 3584, 18944):
        run_rows_cell(dev, M, 256, K, seed=K + M)


@pytest.mark.parametrize("epi", ["qkv", "qkv model scale", "residual", "residual in place", "swiglu", "fp32"])
def test_gemm_rows_epilogues(dev, epi):
    """M = 7, in the k-split form (N = 640) and in the one-block-per-wave form (N > 16384)"""
    for N in (5 * HD, 129 * HD if epi.startswith("qkv") else 16388):
        kw = {"qkv": dict(bias=True, rope=True, rope_cols=N - HD, q_cols=N - 2 * HD),      # Q heads | one K head | one V head
              "qkv model scale": dict(bias=True, rope=True, rope_cols=N - HD, q_cols=N - 2 * HD, q_scale=G.model_q_scale(HD)),
              "residual": dict(res="sep"), "residual in place": dict(res="inplace"),
              "swiglu": dict(act=R.ACT_SWIGLU), "fp32": dict(out_f32=True)}[epi]
        run_rows_cell(dev, 7, N, 192, seed=3, **kw)


def test_gemm_rows_lm_head_width(dev):
    """152064 x 3584, M = 16, fp32 output (two column blocks per wave): a fixed seeded sample of 2048 columns + the first and
    last 64"""
    N = 152064
    pick = torch.randperm(N, generator=torch.Generator().manual_seed(11))[:2048]
    cols = torch.unique(torch.cat([pick, torch.arange(64), torch.arange(N - 64, N)])).to(dev)
    run_rows_cell(dev, 16, N, 3584, out_f32=True, seed=5, cols=cols)


@pytest.mark.parametrize("N,K", [(132, 3584), (256, 18944)])
def test_gemm_rows_row_independence_is_exact(dev, N, K):
    """M = 5, then M = 5 with the rows permuted and two of them replaced: every unchanged row is bit-identical"""
    from cogstream_amd import ops
    a, w, g = _operands(dev, 5, N, K, 17)
    first = ops.gemm_rows(a, w)
    perm = [3, 0, 4, 1, 2]
    b = a[perm].clone()
    b[1] = (torch.randn(K, generator=g, device=dev) * 3).to(BF16)      # slot 1 held row 0, slot 3 held row 1
    b[3] = (torch.randn(K, generator=g, device=dev) * 3).to(BF16)
    second = ops.gemm_rows(b, w)
    torch.cuda.synchronize()
    for slot, src in enumerate(perm):
        same = torch.equal(_bits(second[slot]), _bits(first[src]))
        assert same == (slot not in (1, 3)), (slot, src)


def test_gemm_rows_status_codes(dev):
    from cogstream_amd import ops
    L = _L()
    a, w, _ = _operands(dev, 4, 64, 64, 1)
    with pytest.raises(L.CogsError, match=rf"\({L.E_UNSUPPORTED}\)"):
        ops.gemm_rows(a.float(), w.float())
    a17 = torch.zeros(17, 64, dtype=BF16, device=dev)
    with pytest.raises(L.CogsError, match=rf"\({L.E_UNSUPPORTED}\)"):
        ops.gemm_rows(a17, w)
    f = torch.zeros(64, dtype=F32, device=dev)
    with pytest.raises(L.CogsError, match=rf"\({L.E_UNSUPPORTED}\)"):
        ops.gemm_rows(a, w, ln_ab=f, col_c=f)
    with pytest.raises(L.CogsError, match=rf"\({L.E_UNSUPPORTED}\)"):
        ops.gemm_rows(a, w, bias=w[0].contiguous(), row_stats=f)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------- 2. cogs_attention_rows
# pairwise covering of rows {1, 2, 3, 16} x (hq, hkv) {(7, 1), (28, 4), (16, 1), (2, 2)} x prefix_len {1, 63, 64, 65, 2100} x
# tail_len {1, 63, 64, 65}: every pair of values of two factors occurs in at least one case
ATTN_CASES = [
    (1, 7, 1, 1, 1), (1, 28, 4, 63, 63), (1, 16, 1, 64, 64), (1, 2, 2, 65, 65),
    (2, 7, 1, 63, 64), (2, 28, 4, 1, 65), (2, 16, 1, 65, 1), (2, 2, 2, 64, 63),
    (3, 7, 1, 64, 65), (3, 28, 4, 65, 64), (3, 16, 1, 1, 63), (3, 2, 2, 63, 1),
    (16, 7, 1, 65, 63), (16, 28, 4, 64, 1), (16, 16, 1, 63, 65), (16, 2, 2, 1, 64),
    (1, 7, 1, 2100, 1), (2, 28, 4, 2100, 63), (3, 16, 1, 2100, 64), (16, 2, 2, 2100, 65),
]
BIG = 3.0e4          # large finite filler: a key read from the wrong row or past tail_len moves the output by O(1)


def _nsplit(ctx):
    """csrc/attn_plan.h::cogs_attn_nsplit (at most 127 here: the tails are one more partial)"""
    return min(max(min(max((ctx + 255) // 256, 32), (ctx + 63) // 64), 1), 127)


@pytest.mark.parametrize("rows,hq,hkv,prefix_len,tail_len", ATTN_CASES)
def test_attention_rows_vs_fp64(dev, rows, hq, hkv, prefix_len, tail_len):
    from cogstream_amd import ops
    g = torch.Generator(device=dev).manual_seed(rows * 1000 + hq * 10 + prefix_len + tail_len)
    kvd, tail_max = hkv * HD, 72
    qbuf = torch.randn(rows, hq * HD + 2 * kvd, generator=g, device=dev).to(BF16)      # Q is a column view of a fused qkv buffer
    q = qbuf[:, :hq * HD]
    k = torch.full((prefix_len + 5, kvd), BIG, dtype=BF16, device=dev)
    v = torch.full((prefix_len + 5, kvd), BIG, dtype=BF16, device=dev)
    k[:prefix_len] = torch.randn(prefix_len, kvd, generator=g, device=dev).to(BF16)
    v[:prefix_len] = torch.randn(prefix_len, kvd, generator=g, device=dev).to(BF16)
    tk = torch.full((rows, tail_max, kvd), BIG, dtype=BF16, device=dev)
    tv = torch.full((rows, tail_max, kvd), -BIG, dtype=BF16, device=dev)
    tk[:, :tail_len] = torch.randn(rows, tail_len, kvd, generator=g, device=dev).to(BF16)      # a different tail per row
    tv[:, :tail_len] = torch.randn(rows, tail_len, kvd, generator=g, device=dev).to(BF16) + \
        torch.arange(rows, device=dev).view(rows, 1, 1).to(BF16)
    nsplit = _nsplit(prefix_len)
    out = ops.attention_rows(q, k, v, tk, tv, prefix_len=prefix_len, tail_len=tail_len, hq=hq, hkv=hkv, nsplit=nsplit)
    torch.cuda.synchronize()
    for r in range(rows):
        kk = torch.cat([k[:prefix_len], tk[r, :tail_len]])
        vv = torch.cat([v[:prefix_len], tv[r, :tail_len]])
        ref, tol = AR.reference(q[r:r + 1], kk, vv, hq=hq, hkv=hkv, hd=HD, scale_log2=1.0, nsplit=nsplit + 1)
        AR.assert_within(out[r:r + 1], ref, tol, f"attention_rows rows={rows} hq={hq} hkv={hkv} prefix={prefix_len} tail={tail_len} row {r}")


# ------------------------------------------------------------------------------------------------- 3. the step
STEP_MODELS = {
    "7 heads, 1 kv head": dict(hidden_size=896, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=7,
                               num_key_value_heads=1, vocab_size=512, image_token_index=500, eos_token_id=499),
    "4 heads, 2 kv heads": dict(hidden_size=512, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4,
                                num_key_value_heads=2, vocab_size=512, image_token_index=500, eos_token_id=499),
}


@pytest.mark.parametrize("name", list(STEP_MODELS))
def test_decode_rows_step_teacher_forced(dev, name):
    """Prompt of 70 tokens, R = 3, six forced steps with different tokens per row. Per row and step, max |logits - oracle|
    (oracle: CPU fp32 on the bf16-rounded weights) of the multi-row step against the same figure of the existing single-row
    decode path on the same history:  err_rows <= 2 * err_single + floor,  floor = 2^-8 max |oracle logits| -- one bf16 step at
    the size of the logits, the error a bf16 path (bf16 hidden states in front of the lm_head) shows under its luckiest
    summation order. Both are bf16 paths that differ in summation order, which the factor covers; a wrong position, tail or
    row gives errors of the size of the logits. Then: identical histories in two slots give identical logits bits."""
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    from oracle import qwen2 as oq
    cfg = LlmConfig(**STEP_MODELS[name])
    assert cfg.head_dim == HD
    st = random_llm_state(cfg, seed=7, std=0.05)
    st_r = {k: v.to(BF16).float() for k, v in st.items()}
    eng = Qwen2Engine(st, cfg, dtype=BF16, device=dev)
    kw = dict(heads=cfg.num_attention_heads, kv_heads=cfg.num_key_value_heads, layers=cfg.num_hidden_layers)
    torch.manual_seed(12)
    P, Rn, steps = 70, 3, 6
    prompt = (torch.randn(P, cfg.hidden_size) * 0.5).to(BF16)
    toks = torch.randint(0, 480, (Rn, steps))
    emb = eng.embed_tokens(toks.reshape(-1).to(dev)).view(Rn, steps, cfg.hidden_size)
    cache = eng.new_cache(P + steps + 2)
    eng.forward(prompt.to(dev), cache)
    _, kv0 = oq.forward(st_r, prompt.float(), **kw)

    kvr, tk, tv = eng.new_rows_kv(cache, Rn, steps)
    rows_logits = torch.stack([eng.decode_rows(emb[:, s].contiguous(), kvr) for s in range(steps)], 1).cpu()    # [R, steps, V]
    assert kvr.tail_len == steps and cache.len == P
    single = torch.empty_like(rows_logits)
    oracle = torch.empty_like(rows_logits)
    for r in range(Rn):
        cache.reset(P)
        past = kv0
        for s in range(steps):
            single[r, s] = eng.forward(emb[r, s:s + 1].contiguous(), cache)["logits"].cpu()
            hid, past = oq.forward(st_r, emb[r, s:s + 1].float().cpu(), past=past, **kw)
            oracle[r, s] = oq.logits(st_r, hid[-1])
    cache.reset(P)
    assert float(oracle.std()) > 0.05, "flat logits would hide a wrong row"
    worst = (0.0, 0.0)
    for r in range(Rn):
        for s in range(steps):
            e_rows = float((rows_logits[r, s] - oracle[r, s]).abs().max())
            e_single = float((single[r, s] - oracle[r, s]).abs().max())
            floor = 2.0 ** -8 * float(oracle[r, s].abs().max())
            print(f"{name}: row {r} step {s}: multi-row {e_rows:.4g} single-row {e_single:.4g} floor {floor:.4g}")
            worst = max(worst, (e_rows, e_single))
            assert e_rows <= 2 * e_single + floor, (name, r, s, e_rows, e_single, floor)
    print(f"{name}: largest multi-row error {worst[0]:.4g} (single-row error there {worst[1]:.4g})")
    # slot independence at the step level: rows 0 and 2 carry one history, row 1 another
    kv2, tk2, tv2 = eng.new_rows_kv(cache, Rn, steps)
    for s in range(steps):
        e = torch.stack([emb[0, s], emb[1, s], emb[0, s]])
        lg = eng.decode_rows(e, kv2)
        assert torch.equal(_bits(lg[0]), _bits(lg[2])) and not torch.equal(_bits(lg[0]), _bits(lg[1])), s
        assert torch.equal(_bits(lg[0].cpu()), _bits(rows_logits[0, s])), s        # and the bits of the first run's row 0


# ------------------------------------------------------------------------------------------------- 4. generate
LLM = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
           vocab_size=512, image_token_index=500, eos_token_id=499)


def _engine(dev, dtype, **kw):
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    cfg = LlmConfig(**LLM)
    return cfg, Qwen2Engine(random_llm_state(cfg, seed=7, std=0.05), cfg, dtype=dtype, device=dev, **kw)


def _prompt(dev, dtype, n=40, seed=9):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, LLM["hidden_size"], generator=g) * 0.5).to(dev, dtype)


SAMPLE = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.05)


def test_generate_one_sequence_is_the_old_call(dev):
    cfg, eng = _engine(dev, BF16)
    emb = _prompt(dev, BF16)
    a = eng.generate(emb, max_new_tokens=12, eos_token_id=[], seed=5, **SAMPLE)
    b = eng.generate(emb, max_new_tokens=12, eos_token_id=[], seed=5, num_return_sequences=1, **SAMPLE)
    assert a == b and isinstance(b[0], int)


def test_generate_top1_rows_are_identical_and_start_greedy(dev):
    cfg, eng = _engine(dev, BF16)
    emb = _prompt(dev, BF16)
    rows = eng.generate(emb, max_new_tokens=10, eos_token_id=[], do_sample=True, top_k=1, repetition_penalty=1.05, seed=1,
                        num_return_sequences=5)
    greedy = eng.generate(emb, max_new_tokens=10, eos_token_id=[], repetition_penalty=1.05)
    assert len(rows) == 5 and all(r == rows[0] for r in rows) and len(rows[0]) == 10
    assert rows[0][0] == greedy[0]


def test_generate_seed_and_eos(dev):
    from cogstream_amd.llm import truncate_at_eos
    cfg, eng = _engine(dev, BF16)
    emb = _prompt(dev, BF16)
    kw = dict(max_new_tokens=20, seed=3, num_return_sequences=4, **SAMPLE)
    free = eng.generate(emb, eos_token_id=[], **kw)
    assert free == eng.generate(emb, eos_token_id=[], **kw)
    assert len({tuple(r) for r in free}) > 1, "sampled rows should differ"
    eos = free[0][2]                                # row 0 stops after at most three tokens
    got = eng.generate(emb, eos_token_id=[eos], **kw)
    assert got == truncate_at_eos(free, [eos])      # rows do not influence one another: the free run, cut at the first EOS
    assert len({len(r) for r in got}) > 1 and all(eos not in r[:-1] for r in got)
    host = dict(kw, sampler="host")
    h1 = eng.generate(emb, eos_token_id=[], generator=torch.Generator().manual_seed(4), **host)
    h2 = eng.generate(emb, eos_token_id=[], generator=torch.Generator().manual_seed(4), **host)
    assert h1 == h2 and len(h1) == 4


def test_cogreasoner_generate_pads_and_reuses_the_prefix(dev):
    from cogstream_amd.chat import CogReasoner
    cfg, eng = _engine(dev, BF16)
    ids = torch.randint(0, 480, (1, 40), generator=torch.Generator().manual_seed(2))
    gen = dict(SAMPLE, eos_token_id=[], pad_token_id=498, seed=3)
    model = CogReasoner(None, None, eng, cfg, generation_config=gen)
    free, _ = model.generate(new_input_ids=ids, max_new_tokens=16, num_return_sequences=4)
    assert free.shape == (4, 16) and free.dtype == torch.int64
    eos = int(free[0, 2])
    model = CogReasoner(None, None, eng, cfg, generation_config=dict(gen, eos_token_id=[eos]))
    model.enable_prefix_cache()
    out, _ = model.generate(new_input_ids=ids, max_new_tokens=16, num_return_sequences=4)
    lens = [free[r].tolist().index(eos) + 1 if eos in free[r].tolist() else 16 for r in range(4)]
    assert out.shape == (4, max(lens)) and len(set(lens)) > 1
    for r in range(4):
        assert out[r, :lens[r]].tolist() == free[r, :lens[r]].tolist() and bool((out[r, lens[r]:] == 498).all())
    again, _ = model.generate(new_input_ids=ids, max_new_tokens=16, num_return_sequences=4)
    assert again.shape[0] == 4
    assert model.prefix_cache_stats()["answer"] == (38, 80)        # second call: all rows but the two that are always prefilled


def test_generate_fp32_fallback_top1_is_greedy(dev):
    cfg, eng = _engine(dev, F32)
    emb = _prompt(dev, F32)
    greedy = eng.generate(emb, max_new_tokens=10, eos_token_id=[cfg.eos_token_id], repetition_penalty=1.05)
    rows = eng.generate(emb, max_new_tokens=10, eos_token_id=[cfg.eos_token_id], do_sample=True, top_k=1,
                        repetition_penalty=1.05, seed=1, num_return_sequences=3)
    assert rows == [greedy] * 3


def test_generate_on_an_fp8_engine_reads_the_dequantised_weights(dev):
    L = _L()
    cfg, eng = _engine(dev, BF16, decode_weights="fp8")
    emb = _prompt(dev, BF16)
    one = eng.generate(emb, max_new_tokens=4, eos_token_id=[], seed=5, **SAMPLE)
    assert len(one) == 4 and L.debug_get("llm_last_decode_fp8") == 1
    rows = eng.generate(emb, max_new_tokens=6, eos_token_id=[], seed=5, num_return_sequences=3, **SAMPLE)
    assert [len(r) for r in rows] == [6, 6, 6] and L.debug_get("llm_last_decode_fp8") == 0
