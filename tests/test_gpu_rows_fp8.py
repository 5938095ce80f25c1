"""The e4m3 multi-row decode step on the GPU: cogs_gemm_rows_fp8 (csrc/gemm_rows.hip) cell by cell against the fp64 reference
of tests/gemm_reference.py AND bit for bit against cogs_gemm_rows on the dequantised matrix -- the kernel's contract --, the
e4m3 decode table through the MFMA path, row independence, the status codes, the lockstep step (cogs_llm_decode_rows[_slots])
and generate / beam_search on an fp8 engine under the debug switch llm_rows_fp8 = 1 and 0."""
from __future__ import annotations

import math

import pytest
import torch

import gemm_reference as R

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
TRACE16, TRACE32 = 0x7F7F, 0x7F7F7F7F        # finite tracer patterns, as in test_gpu_rows.py
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


# ------------------------------------------------------------------------------------------------- 1. cogs_gemm_rows_fp8
def _operands(dev, M, N, K, seed):
    """a bf16 [M, K]; w bf16 ~ N(0, 1/K) with row n scaled by 2^(-12 + 7n mod 19) -- magnitudes over 2^-12 .. 2^6, never the
    same in two neighbouring rows -- and one all-zero row; codes / scale / wd = the device quantiser's codes, scales and
    dequantised matrix"""
    from cogstream_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    a = (torch.randn(M, K, generator=g, device=dev) * 0.7 + 0.1).to(BF16)
    w = torch.randn(N, K, generator=g, device=dev) / math.sqrt(K)
    ex = (torch.arange(N, device=dev) * 7) % 19 - 12
    w = (w * torch.exp2(ex.float())[:, None]).to(BF16)
    zero_row = N // 2
    w[zero_row] = 0
    wd = torch.empty_like(w)
    codes, scale = ops.quantize_fp8_rows(w, dequant=wd)
    assert float(scale[zero_row]) == 1.0
    if N > 2:
        live = torch.ones(N - 1, dtype=torch.bool, device=dev)
        live[zero_row - 1:zero_row + 1] = False
        assert bool((scale[1:] != scale[:-1])[live].all()), "neighbouring rows should have different scales"
    return a, codes, scale, wd, g


def run_cell(dev, M, N, K, *, bias=False, res=None, act=R.ACT_NONE, out_f32=False, rope=False, rope_cols=0, q_cols=0, seed=1):
    """one cogs_gemm_rows_fp8 on (codes, scale) and one cogs_gemm_rows on the dequantised matrix wd, each into its own
    C with guard rows above and below and guard columns beside it:
    (a) every fp8 output element inside its own fp64 band of product_and_bound(a, wd) through R.epilogue,
    (b) the two C buffers hold the same bits,
    (c) the guards keep their tracer bits.
    res: None | "sep" | "inplace"; rope: per-row interleaved table; q_cols > 0: q_scale = 2^-3 on the columns below it (a power
    of two commutes with every rounding: the reference runs on pre-scaled columns; test_gpu_rows.py has the cell at the model's factor)"""
    from cogstream_amd import ops
    a, codes, scale, wd, g = _operands(dev, M, N, K, seed)
    swiglu = act == R.ACT_SWIGLU
    ocols = N // 2 if swiglu else N
    odt = F32 if out_f32 else BF16
    bias_t = res_t = rope_r = None
    common = dict(act=act, out_f32=out_f32)
    if bias:
        bias_t = torch.randn(N, generator=g, device=dev).to(BF16)
        common["bias"] = bias_t
    if rope:
        ang = torch.rand(M, HD // 2, generator=g, device=dev) * 6.0          # a different position per row
        cos, sin = ang.cos(), ang.sin()
        common.update(rope_cos=torch.stack([cos, sin], -1).contiguous(), rope_cols=rope_cols, head_dim=HD)
        rope_r = R.Rope(cos.double(), sin.double(), rope_cols, HD)
    if res is not None:
        res_t = torch.randn(M, N, generator=g, device=dev).to(BF16)
    if q_cols:
        common.update(q_scale=0.125, q_cols=q_cols)

    def buffers():
        cbuf = _filled((M + 2, ocols + 16), odt, dev)
        cview = cbuf[1:M + 1, 8:8 + ocols]
        kw = dict(common, out=cview)
        if res == "sep":
            kw["residual"] = res_t
        elif res == "inplace":
            cview.copy_(res_t)
            kw["residual"] = cview
        return cbuf, cview, kw

    inside = torch.zeros((M + 2, ocols + 16), dtype=torch.bool, device=dev)
    inside[1:M + 1, 8:8 + ocols] = True
    acc, bound = R.product_and_bound(a, wd)
    bias_ref = bias_t
    if q_cols:
        colscale = torch.where(torch.arange(N, device=dev) < q_cols, 0.125, 1.0).double()
        acc, bound = acc * colscale[None], bound * colscale[None]
        bias_ref = bias_t.double() * colscale if bias_t is not None else None
    ref, tol = R.epilogue(acc, bound, bias=bias_ref, rope=rope_r, act=act, residual=res_t, out_f32=out_f32, out_dtype=odt)
    c8, v8, kw8 = buffers()
    cd, vd, kwd = buffers()
    guard = _bits(c8)[~inside].clone()
    ops.gemm_rows_fp8(a, codes, scale, **kw8)
    ops.gemm_rows(a, wd, **kwd)
    torch.cuda.synchronize()
    what = f"gemm_rows_fp8 M={M} N={N} K={K} bias={bias} res={res} act={act} f32={out_f32} rope={rope} q={q_cols}"
    assert torch.equal(_bits(c8)[~inside], guard), what + ": guard rows / columns around C changed"
    R.assert_within(v8, ref, tol, what)
    diff = _bits(v8) != _bits(vd)
    assert not bool(diff.any()), what + f": {int(diff.sum())} elements differ from gemm_rows on the dequantised matrix, first at " \
        f"{diff.nonzero()[0].tolist()}"
    assert torch.equal(_bits(cd)[~inside], guard), what + ": the bf16 kernel changed its guards"


@pytest.mark.parametrize("M", [1, 2, 7, 15, 16])
def test_gemm_rows_fp8_n_edges(dev, M):
    """one column block, a ragged last block inside the k-split form, and both sides of both form thresholds (1024 column
    blocks = N 16384: one block per wave; 4096 = N 65536: two blocks per wave)"""
    for N in (16, 132, 16380, 16388, 65532, 65540):
        run_cell(dev, M, N, 192, seed=N + M)


@pytest.mark.parametrize("M", [1, 7, 16])
def test_gemm_rows_fp8_k_edges(dev, M):
    """one k-chunk (seven of the eight k-split waves idle), fewer chunks than a batch, the model's two K"""
    for K in (64, 192, 3584, 18944):
        run_cell(dev, M, 256, K, seed=K + M)


@pytest.mark.parametrize("epi", ["qkv", "residual", "residual in place", "swiglu", "fp32"])
def test_gemm_rows_fp8_epilogues(dev, epi):
    """M = 7, in the k-split form (N = 640) and in the one-block-per-wave form (N = 16388). qkv: Q heads | one K head | the V
    columns (128, or the 132 that are left of 16388), rotary on Q and K, q_scale on Q"""
    for N in (5 * HD, 16388):
        kw = {"qkv": dict(bias=True, rope=True, rope_cols=(N // HD - 1) * HD, q_cols=(N // HD - 2) * HD),
              "residual": dict(res="sep"), "residual in place": dict(res="inplace"),
              "swiglu": dict(act=R.ACT_SWIGLU), "fp32": dict(out_f32=True)}[epi]
        run_cell(dev, 7, N, 192, seed=3, **kw)


@pytest.mark.parametrize("N", [16388, 65540])
def test_gemm_rows_fp8_many_chunks_without_k_split(dev, N):
    """the model's K = 3584 (56 chunks per wave, many batches) in the two forms without a k split, M = 16, fp32 output"""
    run_cell(dev, 16, N, 3584, out_f32=True, seed=N)


def _e4m3_table():
    """value of every OCP e4m3fn code (0x7F / 0xFF, the NaNs, as 0: the test leaves them out)"""
    t = []
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        v = math.ldexp(8 + m, e - 10) if e else math.ldexp(m, -9)
        t.append(0.0 if c & 0x7F == 0x7F else (-v if c & 0x80 else v))
    return torch.tensor(t, dtype=torch.float64)


@pytest.mark.parametrize("N", [256, 16384, 65536])
def test_e4m3_decode_table_through_the_mfma_path(dev, N):
    """K = 64 (one chunk), every form. Row n holds the single code n % 256 at k = n % 64; A[m][k] = (k % 16 == m), M = 16:
    C[m][n] = table[code] * scale[n] exactly where (n % 64) % 16 == m and 0 elsewhere -- a code converted from the wrong byte
    of its dword lands in another row m, a scale taken from another row changes the value"""
    from cogstream_amd import ops
    K, M = 64, 16
    n = torch.arange(N)
    code = n % 256
    code = torch.where((code & 0x7F) == 0x7F, torch.zeros_like(code), code)
    codes = torch.zeros(N, K, dtype=torch.uint8)
    codes[n, n % 64] = code.to(torch.uint8)
    a = ((torch.arange(K)[None, :] % 16) == torch.arange(M)[:, None]).to(BF16)
    table = _e4m3_table()
    hit = ((n % 64) % 16)[None, :] == torch.arange(M)[:, None]                     # [M, N]
    codes, a = codes.to(dev), a.to(dev)
    mixed = torch.exp2(((n * 5) % 13 - 6).double())
    for name, sc in (("2^-9", torch.full((N,), 2.0 ** -9, dtype=torch.float64)), ("1", torch.ones(N, dtype=torch.float64)),
                     ("2^3", torch.full((N,), 8.0, dtype=torch.float64)), ("mixed", mixed)):
        want = torch.where(hit, (table[code] * sc)[None, :], torch.zeros((), dtype=torch.float64))
        got = ops.gemm_rows_fp8(a, codes, sc.float().to(dev), out_f32=True).cpu().double()
        bad = got != want
        assert not bool(bad.any()), f"N={N} scale {name}: {int(bad.sum())} wrong, first (m, n) = {bad.nonzero()[0].tolist()}: " \
            f"got {float(got[bad][0])} want {float(want[bad][0])}"


@pytest.mark.parametrize("N,K", [(132, 3584), (256, 18944)])
def test_gemm_rows_fp8_row_independence_is_exact(dev, N, K):
    """M = 5, then M = 5 with the rows permuted and two of them replaced: every unchanged row is bit-identical"""
    from cogstream_amd import ops
    a, codes, scale, _, g = _operands(dev, 5, N, K, 17)
    first = ops.gemm_rows_fp8(a, codes, scale)
    perm = [3, 0, 4, 1, 2]
    b = a[perm].clone()
    b[1] = (torch.randn(K, generator=g, device=dev) * 3).to(BF16)      # slot 1 held row 0, slot 3 held row 1
    b[3] = (torch.randn(K, generator=g, device=dev) * 3).to(BF16)
    second = ops.gemm_rows_fp8(b, codes, scale)
    torch.cuda.synchronize()
    for slot, src in enumerate(perm):
        same = torch.equal(_bits(second[slot]), _bits(first[src]))
        assert same == (slot not in (1, 3)), (slot, src)


def test_gemm_rows_fp8_status_codes(dev):
    """every refusal comes back before a launch: the output keeps its tracer bits"""
    from cogstream_amd import ops
    L = _L()
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.randn(4, 64, generator=g, device=dev).to(BF16)
    codes = torch.randint(0, 0x70, (64, 64), generator=g, device=dev, dtype=torch.uint8)
    scale = torch.ones(64, dtype=F32, device=dev)
    out = _filled((17, 64), BF16, dev)
    tracer = _bits(out).clone()
    ops.gemm_rows_fp8(a, codes, scale, out=_filled((4, 64), BF16, dev))              # the base call itself is fine
    inv, uns = rf"\({L.E_INVALID}\)", rf"\({L.E_UNSUPPORTED}\)"
    with pytest.raises(L.CogsError, match=inv):
        ops.gemm_rows_fp8(a, codes, None, out=out[:4])
    wide = torch.zeros(64, 72, dtype=torch.uint8, device=dev)
    with pytest.raises(L.CogsError, match=inv):
        ops.gemm_rows_fp8(a, wide[:, :64], scale, out=out[:4])                       # ldw = 72: not whole 16-byte chunks
    a96 = torch.zeros(4, 96, dtype=BF16, device=dev)
    with pytest.raises(L.CogsError, match=inv):
        ops.gemm_rows_fp8(a96, torch.zeros(64, 96, dtype=torch.uint8, device=dev), scale, out=out[:4])
    with pytest.raises(L.CogsError, match=uns):
        ops.gemm_rows_fp8(a.float(), codes, scale, out=out[:4])
    with pytest.raises(L.CogsError, match=uns):
        ops.gemm_rows_fp8(torch.zeros(17, 64, dtype=BF16, device=dev), codes, scale, out=out)
    f = torch.zeros(64, dtype=F32, device=dev)
    with pytest.raises(L.CogsError, match=uns):
        ops.gemm_rows_fp8(a, codes, scale, ln_ab=f, col_c=f, out=out[:4])
    with pytest.raises(L.CogsError, match=uns):
        ops.gemm_rows_fp8(a, codes, scale, bias=a[0].contiguous(), row_stats=f, out=out[:4])
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), tracer)


# ------------------------------------------------------------------------------------------------- 2. the step
STEP_MODELS = {          # the two dimension sets of test_gpu_rows.py
    "7 heads, 1 kv head": dict(hidden_size=896, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=7,
                               num_key_value_heads=1, vocab_size=512, image_token_index=500, eos_token_id=499),
    "4 heads, 2 kv heads": dict(hidden_size=512, intermediate_size=768, num_hidden_layers=2, num_attention_heads=4,
                                num_key_value_heads=2, vocab_size=512, image_token_index=500, eos_token_id=499),
}


@pytest.mark.parametrize("name", list(STEP_MODELS))
def test_decode_rows_step_on_codes_and_on_the_dequantised_weights(dev, name):
    """fp8 engine, prompt of 70 tokens, R = 3, four teacher-forced steps: the logits under llm_rows_fp8 = 1 and 0 are the same
    bits, the reporter says which ran, llm_last_decode_fp8 stays the single-token reporter (0 after both); once more with a
    slot table in which every row reads its earlier tail positions from its neighbour's slot; a plain engine reports 0"""
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    L = _L()
    cfg = LlmConfig(**STEP_MODELS[name])
    assert cfg.head_dim == HD
    st = random_llm_state(cfg, seed=7, std=0.05)
    eng = Qwen2Engine(st, cfg, dtype=BF16, device=dev, decode_weights="fp8")
    torch.manual_seed(12)
    P, Rn, steps = 70, 3, 4
    prompt = (torch.randn(P, cfg.hidden_size) * 0.5).to(BF16)
    toks = torch.randint(0, 480, (Rn, steps))
    emb = eng.embed_tokens(toks.reshape(-1).to(dev)).view(Rn, steps, cfg.hidden_size)
    cache = eng.new_cache(P + steps + 2)
    eng.forward(prompt.to(dev), cache)

    def run(sw, slots):
        cache.reset(P)
        out = []
        with L.debug_switch("llm_rows_fp8", sw):
            if slots:
                kvr, tk, tv, table = eng.new_rows_kv(cache, Rn, steps, slots=True)
            else:
                (kvr, tk, tv), table = eng.new_rows_kv(cache, Rn, steps), None
            for s in range(steps):
                if slots:
                    table[:, :s] = ((torch.arange(Rn, device=dev, dtype=torch.int32) + 1) % Rn)[:, None]
                    table[:, s] = torch.arange(Rn, device=dev, dtype=torch.int32)
                out.append(eng.decode_rows(emb[:, s].contiguous(), kvr, tail_slot=table))
                assert L.debug_get("llm_last_rows_fp8") == sw and L.debug_get("llm_last_decode_fp8") == 0
            torch.cuda.synchronize()
        assert kvr.tail_len == steps
        return torch.stack(out, 1)                       # [R, steps, V]

    for slots in (False, True):
        on, off = run(1, slots), run(0, slots)
        assert float(on.std()) > 0.05 and bool(torch.isfinite(on).all())
        assert torch.equal(_bits(on), _bits(off)), (name, slots)
    assert not torch.equal(_bits(run(1, False)), _bits(run(1, True))), "the slot table should change what the rows read"

    plain = Qwen2Engine(st, cfg, dtype=BF16, device=dev)
    pc = plain.new_cache(P + 2)
    plain.forward(prompt.to(dev), pc)
    with L.debug_switch("llm_rows_fp8", 1):
        kvr, tk, tv = plain.new_rows_kv(pc, Rn, 1)
        plain.decode_rows(emb[:, 0].contiguous(), kvr)
        torch.cuda.synchronize()
        assert L.debug_get("llm_last_rows_fp8") == 0


# ------------------------------------------------------------------------------------------------- 3. generate / beam search
LLM = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
           vocab_size=512, image_token_index=500, eos_token_id=499)
SAMPLE = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.05)


def test_generate_and_beam_search_on_an_fp8_engine_do_not_depend_on_the_switch(dev):
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    L = _L()
    cfg = LlmConfig(**LLM)
    eng = Qwen2Engine(random_llm_state(cfg, seed=7, std=0.05), cfg, dtype=BF16, device=dev, decode_weights="fp8")
    emb = (torch.randn(40, LLM["hidden_size"], generator=torch.Generator().manual_seed(9)) * 0.5).to(dev, BF16)
    got = {}
    for sw in (1, 0):
        with L.debug_switch("llm_rows_fp8", sw):
            rows = eng.generate(emb, max_new_tokens=6, eos_token_id=[], seed=5, num_return_sequences=3, **SAMPLE)
            assert L.debug_get("llm_last_rows_fp8") == sw
            seqs, scores = eng.beam_search(emb, num_beams=4, max_new_tokens=8, eos_token_id=[])
            assert L.debug_get("llm_last_rows_fp8") == sw
            with L.debug_switch("beam_gather_tails", 1):
                gathered = eng.beam_search(emb, num_beams=4, max_new_tokens=8, eos_token_id=[])
            got[sw] = (rows, seqs, [float(s) for s in scores], gathered[0], [float(s) for s in gathered[1]])
    rows, seqs, scores, gseqs, gscores = got[1]
    assert [len(r) for r in rows] == [6, 6, 6] and len(seqs[0]) == 8
    assert got[1] == got[0]
    assert (gseqs, gscores) == (seqs, scores)
