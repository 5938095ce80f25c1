"""The decode GEMV (gemv_kernel of csrc/gemv.hip: bf16 / fp32 weights, every single-token linear of the Qwen2 layers) cell by
cell through cogs_gemm_fused (include/cogs.h) at M = 1, against the fp64 reference of tests/gemm_reference.py and
tests/gemv_reference.py: the K loop (pre-issued first batch, unrolled main loop, ragged tail) on both (rows per wave,
chunks in flight) instances, the fused Qwen2RMSNorm prologue in its three forms, the K / V row redirect, the Q pre-scale,
and the status contract. Laid out like test_gpu_gemm_conformance.py: every output buffer -- C and both cache rows -- is a
view into a buffer of finite tracer values compared bit for bit afterwards, every cell asserts gemm_last_body == 6, and the
last test checks the cells reached a required list. No element of any output is left out of a comparison.

Instances are forced with debug switches only: gemv_small_n = 1 << 30 -> 2 rows per wave, 4 chunks in flight per row
("R2U4"); gemv_small_n = 0 -> 4 rows, 2 chunks ("R4U2"); gemv_dot2 1 / 0 -> the bf16 products on v_dot2c_f32_bf16 or on fp32
fma (fp32 weights have one form)."""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import pytest
import torch

import gemm_reference as R
import gemv_reference as G

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
TRACE16, TRACE32 = 0x7F7F, 0x7F7F7F7F        # finite tracer patterns, as in test_gpu_gemm_conformance.py
HD = 128
EPS = 1e-6
LOW = 2e-3                                   # tests/test_gemv_reference.py: the magnitude at which a dropped epsilon shows
INST = {"R2U4": 1 << 30, "R4U2": 0}
GUARD = 64

# K by 16-byte chunk count nch (8 bf16 / 4 fp32 elements per chunk): what each count hits is listed in test_k_loop
NCH = [8, 64, 96, 128, 136, 224, 256, 264, 448, 456, 2368]
K_OF = {BF16: [8 * n for n in NCH], F32: [4 * n for n in NCH] + [3584, 18944]}
RMS_K = [3584, 3520, 3648, 1088, 64]
KV_SHAPES = {"7b": (4608, 3584, 512), "small": (6 * HD + 4 * HD, 6 * HD, 2 * HD), "ragged": (132, 92, 20)}   # N, kv_col0, kv_dim


def _tn(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def _variants(dtype):
    """(instance, dot2) pairs of one type"""
    return [(i, d) for i in INST for d in ((1, 0) if dtype == BF16 else (1,))]


REACHED: set = set()
WORST: dict = {}                             # family -> largest |out - ref| / tol seen (printed by the last test)
REQUIRED = (
    [(6, f"{kind} K={K} {_tn(dt)} {i} dot2={d}") for dt in (BF16, F32) for K in K_OF[dt] for i, d in _variants(dt)
     for kind in ("bias+res", "exact f32out")]
    + [(6, f"rms {form} K={K} {_tn(dt)} {i} dot2={d}") for dt in (BF16, F32) for K in RMS_K for i, d in _variants(dt)
       for form in ("qkv", "gate_up", "lm_head")]
    + [(6, f"rms low lm_head K={K} {_tn(dt)}") for dt in (BF16, F32) for K in (3584, 1088)]
    + [(6, f"kv {shape} rope={rope} {_tn(dt)} {i}") for dt in (BF16, F32) for i in INST
       for shape, rope in (("7b", "inter"), ("7b", "sep"), ("small", "inter"), ("small", "sep"), ("ragged", None))]
    + [(6, f"q_scale q_cols={q} rope={rope} {_tn(dt)} {i}") for dt in (BF16, F32) for i in INST for q in (6 * HD, 292)
       for rope in ("inter", "sep")]
    + [(6, "status")]
)


def _L():
    from cogstream_amd import _lib
    return _lib


@contextlib.contextmanager
def switches(**kw):
    L = _L()
    with contextlib.ExitStack() as st:
        for k, v in kw.items():
            st.enter_context(L.debug_switch(k, v))
        yield


def _filled(n, dtype, dev):
    if dtype == F32:
        return torch.full((n,), TRACE32, dtype=torch.int32, device=dev).view(F32)
    return torch.full((n,), TRACE16, dtype=torch.int16, device=dev).view(dtype)


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


# ----------------------------------------------------------------------------------------------------------- data
_cache: dict = {}


def _operands(dev, N, K, dtype, kind, seed):
    """x [K], W [N, K] on the device; the last few are cached (one pair serves every instance of a cell)"""
    key = (N, K, dtype, kind, seed)
    if key in _cache:
        return _cache[key]
    if len(_cache) >= 4:
        _cache.pop(next(iter(_cache)))
    g = torch.Generator(device=dev).manual_seed(seed)
    if kind == "exact":
        # dense small integers: |sum| <= 2 K < 2^24, so every partial sum in every order is exact in fp32
        x = torch.randint(-2, 3, (K,), generator=g, device=dev).to(dtype)
        w = torch.randint(-1, 2, (N, K), generator=g, device=dev).to(dtype)
    else:
        x = ((torch.randn(K, generator=g, device=dev) * 0.7 + 0.1) * (LOW if kind == "low" else 1.0)).to(dtype)
        w = (torch.randn(N, K, generator=g, device=dev) / math.sqrt(K)).to(dtype)
    _cache[key] = (x, w)
    return x, w


# ----------------------------------------------------------------------------------------------------------- one cell
def run_cell(dev, N, K, label, family, *, dtype=BF16, inst="R4U2", dot2=1, kind="random", rms=False, bias=False, res=None,
             act=R.ACT_NONE, out_f32=False, rope=None, rope_cols=0, hd=HD, q_cols=0, kv=None, seed=1):
    """One GEMV through cogs_gemm_fused (M = 1): the status, the body, every output element against its own fp64 band (or bit
    for bit against the integer result: kind = "exact"), the guards around C and both cache rows, and -- kv = (kv_col0, kv_dim)
    -- the tracer bits of the columns of C the K / V rows replace. res: None | "sep" | "inplace"; rope: None | "inter" | "sep";
    q_cols > 0: the model's q_scale for head_dim hd on the columns below it. Returns the worst |out - ref| / tol."""
    L = _L()
    x, w = _operands(dev, N, K, dtype, kind, seed)
    g = torch.Generator(device=dev).manual_seed(seed + 7919)
    swiglu = act == R.ACT_SWIGLU
    ocols = N // 2 if swiglu else N
    odt = F32 if (out_f32 or dtype == F32) else dtype
    d, f = L.GemmDesc(), L.GemmFusedArgs()
    d.dtype = L.dtype_code(dtype)
    d.A, d.lda, d.W, d.ldw = x.data_ptr(), K, w.data_ptr(), K
    d.M, d.N, d.K, d.act, d.out_f32 = 1, N, K, act, int(out_f32)
    keep, rkw = [], {}
    if rms:
        gamma = (1 + 0.1 * torch.randn(K, generator=g, device=dev)).to(dtype)
        f.rms_gamma, f.rms_eps = gamma.data_ptr(), EPS
        rkw["rms"] = (gamma, EPS)
    if bias:
        bias_t = torch.randn(N, generator=g, device=dev).to(dtype)
        d.bias = bias_t.data_ptr()
        rkw["bias"] = bias_t
    if rope:
        ang = torch.rand(1, hd // 2, generator=g, device=dev) * 6.0
        cos, sin = ang.cos(), ang.sin()
        if rope == "sep":
            tc, ts = cos.contiguous(), sin.contiguous()
            d.rope_cos, d.rope_sin = tc.data_ptr(), ts.data_ptr()
            keep += [tc, ts]
        else:
            tc = torch.stack([cos, sin], -1).contiguous()
            d.rope_cos = tc.data_ptr()
            keep.append(tc)
        d.rope_cols, d.head_dim = rope_cols, hd
        rkw["rope"] = R.Rope(cos.double(), sin.double(), rope_cols, hd)
    if q_cols:
        q = G.model_q_scale(hd)
        f.q_scale, f.q_cols = q, q_cols
        rkw.update(q_scale=q, q_cols=q_cols)
    cbuf = _filled(GUARD + ocols + GUARD, odt, dev)
    cview = cbuf[GUARD:GUARD + ocols]
    d.C, d.ldc = cview.data_ptr(), ocols
    inside = torch.zeros(cbuf.numel(), dtype=torch.bool, device=dev)
    inside[GUARD:GUARD + ocols] = True
    if res is not None:
        res_t = torch.randn(N, generator=g, device=dev).to(dtype)
        rkw["residual"] = res_t
        if res == "inplace":
            cview.copy_(res_t)
            d.residual, d.ldr = cview.data_ptr(), N
        else:
            d.residual, d.ldr = res_t.data_ptr(), N
    kvbuf = kk = vv = None
    if kv is not None:
        c0, kd = kv
        kvbuf = _filled(2 * (GUARD + kd + GUARD), dtype, dev)
        v0 = GUARD + kd + 2 * GUARD
        kk, vv = kvbuf[GUARD:GUARD + kd], kvbuf[v0:v0 + kd]
        f.kv_k, f.kv_v, f.kv_col0, f.kv_dim = kk.data_ptr(), vv.data_ptr(), c0, kd
        kv_inside = torch.zeros(kvbuf.numel(), dtype=torch.bool, device=dev)
        kv_inside[GUARD:GUARD + kd] = True
        kv_inside[v0:v0 + kd] = True
        kv_guard = _bits(kvbuf)[~kv_inside].clone()
        inside[GUARD + c0:GUARD + N] = False                                # those columns of C must keep their tracer bits
    guard = _bits(cbuf)[~inside].clone()
    what = f"gemv {label} N={N}"
    with switches(gemv_small_n=INST[inst], gemv_dot2=dot2):
        st = L.lib.cogs_gemm_fused(L.current_stream(), C.byref(d), C.byref(f))
        body = L.debug_get("gemm_last_body")
    torch.cuda.synchronize()
    assert st == L.OK, (what, st)
    assert body == 6, f"{what}: ran body {body}"
    assert torch.equal(_bits(cbuf)[~inside], guard), what + ": elements outside C (or its K / V columns) changed"
    kv_arg = None
    if kv is not None:
        assert torch.equal(_bits(kvbuf)[~kv_inside], kv_guard), what + ": guard elements around the K / V rows changed"
        kv_arg = (kk, vv, *kv)
    if kind == "exact":
        assert out_f32 and kv is None and not rkw
        want = (x.double().view(1, K) @ w.double().t()).view(-1)
        assert float(want.abs().max()) < 2.0 ** 24
        bad = cview.double() != want
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ from the exact integer result"
        ratio = 0.0
    else:
        ref, tol = G.reference(x, w, act=act, out_f32=out_f32, **rkw)
        ratio = G.worst_ratio(cview, ref, tol, kv=kv_arg)
        print(f"{what}: worst |out - ref| / tol = {ratio:.3f}")
        G.assert_row(cview, ref, tol, what, kv=kv_arg)
    del keep
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    REACHED.add((6, label))
    return ratio


# ----------------------------------------------------------------------------------------------------------- K loop
@pytest.mark.parametrize("dtype,K", [(dt, K) for dt in (BF16, F32) for K in K_OF[dt]], ids=lambda v: _tn(v) if isinstance(v, torch.dtype) else str(v))
def test_k_loop(dev, dtype, K):
    """nch = K / (elements per 16-byte chunk); U = 2 is R4U2, U = 4 is R2U4. A lane takes the pre-issued first batch when
    lane + 64 (U - 1) < nch, the main loop runs while whole batches of 64 U chunks remain, the tail takes 64 chunks at a time:
      8 fewer chunks than lanes; 64 one chunk per lane; 96 U = 2: only lanes 0..31 take the first batch; 128 U = 2: the first
      batch exactly; 136 U = 2: first batch + ragged tail; 224 U = 4: only lanes 0..31 take the first batch; 256 U = 4: first
      batch exactly, U = 2: first batch + one loop trip; 264 both + a ragged tail; 448 the bf16 count of the hidden size
      (K = 3584); 456 one tile past it; 2368 the down projection (K = 18944). fp32 also at K = 3584 and 18944 themselves.
    Each K once with random data against the fp64 band (bias + residual) and once with dense integers, bit for bit."""
    N = 264
    for inst, dot2 in _variants(dtype):
        tag = f"K={K} {_tn(dtype)} {inst} dot2={dot2}"
        run_cell(dev, N, K, "bias+res " + tag, f"K loop, random, {_tn(dtype)}", dtype=dtype, inst=inst, dot2=dot2, bias=True,
                 res="sep", seed=K)
        run_cell(dev, N, K, "exact f32out " + tag, "K loop, exact", dtype=dtype, inst=inst, dot2=dot2, kind="exact",
                 out_f32=True, seed=K + 1)


# ----------------------------------------------------------------------------------------------------------- fused RMSNorm
@pytest.mark.parametrize("K", RMS_K)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_fused_rmsnorm(dev, K, dtype):
    """the Qwen2RMSNorm prologue: register-resident at K = 3584 in bf16 (with and without the dot2 product), the generic
    two-pass form on both sides of it (3520, 3648), behind a ragged tail (1088), with fewer chunks than lanes (64) and for
    fp32 -- in the three forms the model uses: qkv (bias + interleaved rotary + q_scale + K / V row), gate / up (SwiGLU),
    lm_head (fp32 output)"""
    kvd = 2 * HD
    N = 6 * HD + 2 * kvd
    for inst, dot2 in _variants(dtype):
        tag = f"K={K} {_tn(dtype)} {inst} dot2={dot2}"
        fam = f"fused RMSNorm, {_tn(dtype)}"
        run_cell(dev, N, K, "rms qkv " + tag, fam, dtype=dtype, inst=inst, dot2=dot2, rms=True, bias=True, rope="inter",
                 rope_cols=N - kvd, q_cols=N - 2 * kvd, kv=(N - 2 * kvd, kvd), seed=K + 1)
        run_cell(dev, 1032, K, "rms gate_up " + tag, fam, dtype=dtype, inst=inst, dot2=dot2, rms=True, act=R.ACT_SWIGLU, seed=K + 2)
        run_cell(dev, 1028, K, "rms lm_head " + tag, fam, dtype=dtype, inst=inst, dot2=dot2, rms=True, out_f32=True, seed=K + 3)


@pytest.mark.parametrize("K", [3584, 1088])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_fused_rmsnorm_epsilon(dev, K, dtype):
    """x at 2e-3 of the ordinary magnitude: the mean square (~2e-6) is of the order of rms_eps, so an rstd computed without
    it (or with another one) leaves the band on nearly every element (tests/test_gemv_reference.py: > half of 264, against 0
    at the ordinary magnitude)"""
    for inst, dot2 in _variants(dtype):
        run_cell(dev, 264, K, f"rms low lm_head K={K} {_tn(dtype)}", "fused RMSNorm, low magnitude", dtype=dtype, inst=inst,
                 dot2=dot2, kind="low", rms=True, out_f32=True, seed=K + 4)


def test_fused_rmsnorm_is_refused_for_two_rows(dev):
    _status_cells(dev, only="rms_gamma, M = 2")


# ----------------------------------------------------------------------------------------------------------- K / V row
@pytest.mark.parametrize("shape", list(KV_SHAPES))
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_kv_row(dev, shape, dtype):
    """the epilogue redirect: columns [kv_col0, kv_col0 + kv_dim) into the K row, the next kv_dim into the V row, C left alone
    there -- the 7B split (at its own K, with the fused norm: the production call), 6 + 2 x 2 heads, and a split whose
    boundaries (92, 112) are multiples of 4 but not of 8 (no rotary), with both table forms and on both instances"""
    N, c0, kd = KV_SHAPES[shape]
    for inst in INST:
        for rope in ((None,) if shape == "ragged" else ("inter", "sep")):
            kw = dict(bias=True, kv=(c0, kd))
            if rope:
                kw.update(rope=rope, rope_cols=c0 + kd, q_cols=c0)
            K = 3584 if shape == "7b" else 256
            run_cell(dev, N, K, f"kv {shape} rope={rope} {_tn(dtype)} {inst}", "K / V row", dtype=dtype, inst=inst,
                     rms=shape == "7b", seed=N, **kw)


# ----------------------------------------------------------------------------------------------------------- Q pre-scale
@pytest.mark.parametrize("q_cols", [6 * HD, 292])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_q_prescale(dev, q_cols, dtype):
    """q_scale on columns < q_cols in epilogue4 (R4U2) and epilogue2 (R2U4), with q_cols at the end of the Q heads and at a
    multiple of 4 inside a head (292 = 2 heads + 36), at the factor the model passes"""
    N = 6 * HD + 4 * HD
    for inst in INST:
        for rope in ("inter", "sep"):
            run_cell(dev, N, 256, f"q_scale q_cols={q_cols} rope={rope} {_tn(dtype)} {inst}", "Q pre-scale", dtype=dtype,
                     inst=inst, bias=True, rope=rope, rope_cols=8 * HD, q_cols=q_cols, seed=q_cols)


# ----------------------------------------------------------------------------------------------------------- status contract
def _status_cells(dev, only=None):
    """descriptors include/cogs.h declares invalid or unsupported, on valid allocations: the documented status before any
    launch, C and both cache rows keep their bits"""
    L = _L()
    N, K, kvd = 6 * HD + 4 * HD, 128, 2 * HD
    c0 = N - 2 * kvd
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(2, K, generator=g, device=dev).bfloat16()
    w = (torch.randn(N, K, generator=g, device=dev) / math.sqrt(K)).bfloat16()
    bias = torch.randn(N, generator=g, device=dev).bfloat16()
    gamma = torch.ones(K, device=dev).bfloat16()
    tab = torch.zeros(2, HD // 2, 2, device=dev)
    out = _filled(2 * N + 2 * GUARD, BF16, dev)
    kvbuf = _filled(2 * (kvd + 2 * GUARD), BF16, dev)
    kp, vp = kvbuf[GUARD:].data_ptr(), kvbuf[kvd + 3 * GUARD:].data_ptr()
    before, kv_before = _bits(out).clone(), _bits(kvbuf).clone()

    def call(dkw=None, **fkw):
        d, f = L.GemmDesc(), L.GemmFusedArgs()
        d.dtype = L.DT_BF16
        d.A, d.lda, d.W, d.ldw, d.C, d.ldc = x.data_ptr(), K, w.data_ptr(), K, out[GUARD:].data_ptr(), N
        d.M, d.N, d.K = 1, N, K
        d.bias, d.rope_cos, d.rope_cols, d.head_dim = bias.data_ptr(), tab.data_ptr(), c0 + kvd, HD
        for k, v in (dkw or {}).items():
            setattr(d, k, v)
        for k, v in fkw.items():
            setattr(f, k, v)
        return L.lib.cogs_gemm_fused(L.current_stream(), C.byref(d), C.byref(f))

    KV = dict(kv_k=kp, kv_v=vp, kv_col0=c0, kv_dim=kvd)
    Q = dict(q_scale=G.model_q_scale(HD), q_cols=c0)
    NO_ROPE = dict(rope_cos=None, rope_cols=0, head_dim=0)
    UNS, INV = L.E_UNSUPPORTED, L.E_INVALID
    cases = [
        ("kv_col0 % 4", INV, {}, dict(KV, kv_col0=c0 + 2, kv_dim=kvd - 1)),
        ("kv_dim % 4", INV, {}, dict(KV, kv_col0=c0 + 4, kv_dim=kvd - 2)),
        ("kv_v NULL", INV, {}, dict(KV, kv_v=None)),
        ("kv_col0 + 2 kv_dim < N", INV, {}, dict(KV, kv_dim=kvd - 4)),
        ("kv_col0 + 2 kv_dim > N", INV, {}, dict(KV, kv_dim=kvd + 4)),
        ("kv_k + out_f32", INV, dict(out_f32=1), KV),
        ("kv_k + SwiGLU", INV, dict(NO_ROPE, bias=None, act=L.ACT_SWIGLU), KV),
        ("kv_k, M = 2", UNS, dict(M=2), KV),
        ("rms_gamma, M = 2", UNS, dict(M=2), dict(rms_gamma=gamma.data_ptr(), rms_eps=EPS)),
        ("q_scale without rotary", INV, NO_ROPE, Q),
        ("q_cols % 4", INV, {}, dict(Q, q_cols=c0 + 2)),
        ("q_cols > rope_cols", INV, {}, dict(Q, q_cols=c0 + kvd + 4)),
        ("q_scale without rotary, M = 2", INV, dict(NO_ROPE, M=2), Q),
        ("NULL args", INV, None, None),
    ]
    for name, want, dkw, fkw in cases:
        if only is not None and name != only:
            continue
        if fkw is None:
            d = L.GemmDesc()
            got = L.lib.cogs_gemm_fused(L.current_stream(), C.byref(d), None)
        else:
            got = call(dkw, **fkw)
        assert got == want, (name, got, want)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), before), "a rejected descriptor wrote to C"
    assert torch.equal(_bits(kvbuf), kv_before), "a rejected descriptor wrote to the cache rows"
    if only is None:
        # the base descriptor with everything on is accepted and writes exactly its three regions
        assert call({}, **KV, **Q, rms_gamma=gamma.data_ptr(), rms_eps=EPS) == L.OK
        assert L.debug_get("gemm_last_body") == 6
        torch.cuda.synchronize()
        changed = _bits(out) != before
        assert bool(changed[GUARD:GUARD + c0].all()) and int(changed.sum()) == c0
        kchanged = _bits(kvbuf) != kv_before
        assert int(kchanged.sum()) == 2 * kvd and bool(kchanged[GUARD:GUARD + kvd].all())
        REACHED.add((6, "status"))


def test_rejected_descriptors_return_their_status_and_write_nothing(dev):
    _status_cells(dev)


# ----------------------------------------------------------------------------------------------------------- coverage
def test_zz_required_coverage(dev):
    """the cells above reached every required cell -- one that is renamed, dropped or rerouted fails here"""
    for fam in sorted(WORST):
        print(f"worst |out - ref| / tol, {fam}: {WORST[fam]:.3f}")
    missing = [p for p in REQUIRED if p not in REACHED]
    assert not missing, f"not reached: {missing[:12]} ({len(missing)} in all)"
