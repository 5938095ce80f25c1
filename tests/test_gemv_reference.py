"""The reference of tests/gemv_reference.py (and the q_scale step of tests/gemm_reference.py) held to account without a
GPU: csrc/gemv.hip's arithmetic restated in torch fp32 -- lanes striding over 16-byte chunks, sequential sums per lane, a
butterfly, the fused RMSNorm prologue, the epilogue, the K / V row redirect -- passes every element of a handful of cells,
and each planted error of the kind the GPU cells are there to catch fails on the cell that is meant to catch it."""
from __future__ import annotations

import math

import pytest
import torch

import gemm_reference as R
import gemv_reference as G

BF16, F32 = torch.bfloat16, torch.float32
HD = 128
EPS = 1e-6
LOW = 2e-3              # x scaled so that its mean square (~2e-6) is of the order of eps: the epsilon cells


def _butterfly(v):
    """the 64-lane xor butterfly on the last dimension; every lane ends with the total, lane 0 is returned"""
    lanes = torch.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ s]
    return v[..., 0]


def emulate(x, w, *, rms=None, bias=None, rope=None, q_scale=None, q_cols=0, act=R.ACT_NONE, residual=None, out_f32=False,
            kv=None, mut=None):
    """gemv_kernel in torch fp32. x [K], w [N, K] in bf16 / fp32; rope = (cos, sin fp32 [hd / 2], rope_cols, hd); kv =
    (kv_col0, kv_dim). Returns (c, k_row, v_row): with kv, only c[:kv_col0] is written (the rest stays NaN).
    mut: None | "drop_tail" | "no_eps" | "k_minus_8" | "q_beyond" | "kv_swapped" | "k_shifted" """
    dt = x.dtype
    N, K = w.shape
    epc = 16 // x.element_size()
    nch = K // epc
    iters = (nch + 63) // 64
    pad = iters * 64 * epc - K
    xs = torch.cat([x.float(), torch.zeros(pad)]).view(iters, 64, epc)
    ws = torch.cat([w.float(), torch.zeros(N, pad)], 1).view(N, iters, 64, epc)
    if rms is not None:
        gamma, eps = rms
        ss = torch.zeros(64)
        for it in range(iters):
            for e in range(epc):
                ss = ss + xs[it, :, e] * xs[it, :, e]
        ms = _butterfly(ss) / torch.tensor(float(K - 8 if mut == "k_minus_8" else K), dtype=F32)
        rstd = torch.rsqrt(ms + torch.tensor(0.0 if mut == "no_eps" else eps, dtype=F32))
        n = xs * rstd
        if dt == BF16:
            n = n.to(BF16).float()
        n = torch.cat([gamma.float(), torch.zeros(pad)]).view(iters, 64, epc) * n
        if dt == BF16:
            n = n.to(BF16).float()
        xs = n
    acc = torch.zeros(N, 64)
    whole = nch // 64 if (mut == "drop_tail" and nch % 64) else iters
    for it in range(whole):
        for e in range(epc):
            acc = acc + ws[:, it, :, e] * xs[it, :, e]
    v = _butterfly(acc)
    cols = torch.arange(N)
    if bias is not None:
        v = v + bias.float()
    if rope is not None:
        cos, sin, rope_cols, hd = rope
        pi = (cols[0::2] % hd) // 2
        c, s = cos.float()[pi], sin.float()[pi]
        v0, v1 = v[0::2], v[1::2]
        on = cols[0::2] < rope_cols
        r0, r1 = v0 * c - v1 * s, v1 * c + v0 * s
        v = torch.stack([torch.where(on, r0, v0), torch.where(on, r1, v1)], 1).reshape(-1)
    if q_scale is not None and q_cols > 0:
        v = torch.where(cols < q_cols + (4 if mut == "q_beyond" else 0), v * torch.tensor(q_scale, dtype=F32), v)
    if act == R.ACT_SWIGLU:
        v = v[0::2] * torch.sigmoid(v[0::2]) * v[1::2]
    elif act == R.ACT_GELU_TANH:
        v = torch.nn.functional.gelu(v, approximate="tanh")
    if residual is not None:
        v = v + residual.float()
    out = v if (out_f32 or dt == F32) else v.to(BF16)
    if kv is None:
        return out, None, None
    c0, kd = kv
    k_row, v_row = out[c0:c0 + kd].clone(), out[c0 + kd:].clone()
    if mut == "kv_swapped":
        k_row, v_row = v_row, k_row
    if mut == "k_shifted":
        k_row = torch.roll(k_row, 4)
    c = out.clone()
    c[c0:] = float("nan")
    return c, k_row, v_row


def _cell(form, K, dtype, *, seed=0, scale=1.0, N=None):
    """(emulate / reference keyword sets, x, w) of one cell. form: "loop" bias + residual; "qkv" fused norm, bias,
    interleaved rotary, the model's q_scale, K / V row; "gate_up" fused norm + SwiGLU; "lm_head" fused norm + fp32 output"""
    g = torch.Generator().manual_seed(seed * 1000 + K)
    N = N or (6 * HD + 2 * 2 * HD if form == "qkv" else 264)
    x = ((torch.randn(K, generator=g) * 0.7 + 0.1) * scale).to(dtype)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype)
    kw, rkw, kv = {}, {}, None
    if form != "loop":
        gamma = (1 + 0.1 * torch.randn(K, generator=g)).to(dtype)
        kw["rms"] = rkw["rms"] = (gamma, EPS)
    if form == "loop":
        bias, res = torch.randn(N, generator=g).to(dtype), torch.randn(N, generator=g).to(dtype)
        kw.update(bias=bias, residual=res)
        rkw.update(bias=bias, residual=res)
    elif form == "qkv":
        kvd = 2 * HD
        bias = torch.randn(N, generator=g).to(dtype)
        ang = torch.rand(1, HD // 2, generator=g) * 6.0
        cos, sin = ang.cos(), ang.sin()
        q = G.model_q_scale(HD)
        kv = (N - 2 * kvd, kvd)
        kw.update(bias=bias, rope=(cos[0], sin[0], N - kvd, HD), q_scale=q, q_cols=N - 2 * kvd, kv=kv)
        rkw.update(bias=bias, rope=R.Rope(cos.double(), sin.double(), N - kvd, HD), q_scale=q, q_cols=N - 2 * kvd)
    elif form == "gate_up":
        kw.update(act=R.ACT_SWIGLU)
        rkw.update(act=R.ACT_SWIGLU)
    elif form == "lm_head":
        kw.update(out_f32=True)
        rkw.update(out_f32=True)
    return x, w, kw, rkw, kv


def _violations(x, w, kw, rkw, kv, mut=None):
    ref, tol = G.reference(x, w, **rkw)
    c, k_row, v_row = emulate(x, w, mut=mut, **kw)
    n = G.count_violations(c, ref, tol, kv=None if kv is None else (k_row, v_row, *kv))
    if mut is None:
        G.assert_row(c, ref, tol, "clean emulation", kv=None if kv is None else (k_row, v_row, *kv))
    return n, ref.numel()


# the clean cells: every form, both types, K = fewer chunks than lanes / a ragged tail behind whole batches / the model's
CLEAN = [(form, K) for form in ("loop", "qkv", "gate_up", "lm_head") for K in (64, 1088, 3584)]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("form,K", CLEAN)
def test_clean_emulation_passes_every_element(form, K, dtype):
    n, total = _violations(*_cell(form, K, dtype))
    assert n == 0, (n, total)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K", [1088, 3584])
def test_clean_emulation_passes_at_low_magnitude(K, dtype):
    n, total = _violations(*_cell("lm_head", K, dtype, scale=LOW))
    assert n == 0, (n, total)


# (planted error, form, K, x scale): the cell that has to catch it
PLANTED = [
    ("drop_tail", "loop", 1088, 1.0),          # nch = 136 (bf16) / 272 (fp32): the last 8 / 16 chunks are a ragged group
    ("drop_tail", "qkv", 1088, 1.0),
    ("no_eps", "lm_head", 1088, LOW),
    ("no_eps", "lm_head", 3584, LOW),
    ("k_minus_8", "lm_head", 64, 1.0),
    ("k_minus_8", "lm_head", 1088, 1.0),
    ("k_minus_8", "qkv", 64, 1.0),
    ("q_beyond", "qkv", 1088, 1.0),
    ("q_beyond", "qkv", 3584, 1.0),
    ("kv_swapped", "qkv", 1088, 1.0),
    ("k_shifted", "qkv", 1088, 1.0),
    ("k_shifted", "qkv", 3584, 1.0),
]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mut,form,K,scale", PLANTED)
def test_each_planted_error_fails(mut, form, K, scale, dtype):
    cell = _cell(form, K, dtype, scale=scale)
    clean, total = _violations(*cell)
    bad, _ = _violations(*cell, mut=mut)
    print(f"{mut} on {form} K={K} {dtype}: {bad} of {total} elements outside the band (clean: {clean})")
    assert clean == 0 and bad > 0, (mut, bad, total)
    if mut == "no_eps":
        assert 2 * bad > total, (bad, total)             # the dropped epsilon moves every element, not a few near a boundary


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_dropped_epsilon_is_invisible_at_ordinary_magnitude(dtype):
    """why the epsilon cells use LOW: at mean square ~0.5 a missing 1e-6 changes rstd by 1e-6, far inside every band"""
    for K in (1088, 3584):
        bad, total = _violations(*_cell("lm_head", K, dtype), mut="no_eps")
        assert bad == 0, (K, bad, total)


def test_q_scale_step_of_the_reference():
    """with a power of two the step commutes with every rounding around it: the reference with q_scale must equal the
    reference run on pre-scaled columns (what the GEMV files did before the step existed); with the model's factor a result
    that skips the scale, or scales four more columns, is outside the band"""
    torch.manual_seed(2)
    N, K = 96, 128
    a = torch.randn(1, K).bfloat16()
    w = (torch.randn(N, K) / math.sqrt(K)).bfloat16()
    b = torch.randn(N).bfloat16()
    ang = torch.rand(1, 8) * 6
    rope = R.Rope(ang.cos().double(), ang.sin().double(), 64, 16)
    acc, bound = R.product_and_bound(a, w)
    ref, tol = R.epilogue(acc, bound, bias=b, rope=rope, q_scale=0.125, q_cols=32)
    cs = torch.where(torch.arange(N) < 32, 0.125, 1.0).double()
    ref2, tol2 = R.epilogue(acc * cs, bound * cs, bias=b.double() * cs, rope=rope)
    assert torch.equal(ref, ref2)
    assert torch.allclose(tol, tol2, rtol=1e-12, atol=0)
    for hd in (128, 72):
        q = G.model_q_scale(hd)
        assert abs(q - 1.4426950408889634 / math.sqrt(hd)) < 2.0 ** -23 * q and q == float(torch.tensor(q, dtype=F32))
        ref, tol = R.epilogue(acc, bound, bias=b, rope=rope, q_scale=q, q_cols=32)
        plain, ptol = R.epilogue(acc, bound, bias=b, rope=rope)
        # the band of a scaled column: the unscaled one times q, plus the one multiply (through the store's 1 + u_out)
        want = q * ptol[:, :32] + (1 + R.U_BF16) * R.U32 * ref[:, :32].abs()
        assert torch.allclose(tol[:, :32], want, rtol=1e-9, atol=0) and torch.equal(tol[:, 32:], ptol[:, 32:])
        assert torch.equal(ref[:, 32:], plain[:, 32:]) and torch.equal(ref[:, :32], plain[:, :32] * q)
        good = ref.float().bfloat16()
        assert R.violations(good, ref, tol).sum() == 0
        assert R.violations(plain.float().bfloat16(), ref, tol)[:, :32].sum() > 24        # no scale at all
        beyond = good.clone()
        beyond[:, 32:36] = (ref[:, 32:36] * q).float().bfloat16()
        assert R.violations(beyond, ref, tol).sum() >= 3
