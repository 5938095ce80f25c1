"""What the two GEMV conformance files (tests/test_gpu_gemv_conformance.py: csrc/gemv.hip, bf16 / fp32 weights;
tests/test_gpu_fp8.py: csrc/gemv_fp8.hip, e4m3 weights) and tests/test_gemv_reference.py share on top of
tests/gemm_reference.py: the fused Qwen2RMSNorm prologue with its rstd band, the model's Q pre-scale, and the comparison of
one output row that is split between C and the K / V cache rows.

The rstd band. Both kernels compute the statistics the same way: a lane adds the squares of its K / 64 elements in
sequence (16-byte chunks lane, lane + 64, ...; the register-resident K = 3584 form of csrc/gemv.hip keeps the same order),
six butterfly levels join the 64 lanes, then one division by K, the addition of eps and v_rsq_f32 (1 ulp). The squares of
bf16 values are exact in fp32; the square of an fp32 value is rounded once unless it is contracted into the addition, and
since every term is positive that moves the sum by at most one more relative 2^-24. So the mean square carries at most
K / 64 + 6 + 2 roundings, + 1 for the fp32 squares: (K / 64 + 9) 2^-24. The inverse square root halves a relative error,
and the instruction and the final rounding add 2^-23 + 2^-24:

    |rstd_device / rstd_exact - 1| <= rel(K) = 0.5 (K / 64 + 9) 2^-24 + 2^-23 + 2^-24.

That scales the normalised row (fp32), or moves an element by a bf16 step where x * rstd lies that close to a rounding
boundary (bf16; both roundings are monotonic in rstd, so the two ends of the interval decide). What the ends change enters
the tolerance through |W|: extra[n] = sum_k |a_hi[k] - a_lo[k]| |W[n][k]|, nothing where no element is near a boundary.
The bf16 / fp32 kernel's prologue has the same summation shape as the e4m3 kernel's, so one band serves both files."""
from __future__ import annotations

import numpy as np
import torch

import gemm_reference as R

BF16, F32 = torch.bfloat16, torch.float32


def model_q_scale(head_dim: int) -> float:
    """the factor llm_layer passes as q_scale: fp32(1 / sqrt(head_dim)) * 1.4426950408889634f, evaluated in fp32"""
    s = np.float32(1.0) / np.sqrt(np.float32(head_dim))
    return float(np.float32(s * np.float32(1.4426950408889634)))


def rstd_rel(K: int) -> float:
    return 0.5 * (K / 64 + 9) * 2.0 ** -24 + 2.0 ** -23 + 2.0 ** -24


def rmsnorm_row(x, gamma, eps, rel=0.0):
    """Qwen2RMSNorm of the single row x in the kernels' arithmetic (csrc/norm.hip): rstd in fp32 from the fp64 mean square,
    times (1 + rel); bf16: weight * (x * rstd).to(bf16), rounded to bf16 again; fp32: weight * (x * rstd)"""
    rstd = (1.0 / torch.sqrt(x.double().pow(2).mean() + eps) * (1.0 + rel)).float()
    n = x.float() * rstd
    if x.dtype == BF16:
        n = n.to(BF16).float()
    n = gamma.float() * n
    return n.to(x.dtype)


def rms_operand(x, gamma, eps, w):
    """(a [1, K] in x's type, extra [1, N] fp64): the normalised row at the exact rstd, and what the rstd band can move the
    products by (see the module docstring). w [N, K]: the weights the products run on (dequantised for e4m3)."""
    K = x.numel()
    rel = rstd_rel(K)
    a = rmsnorm_row(x, gamma, eps, 0.0).view(1, K)
    lo, hi = rmsnorm_row(x, gamma, eps, -rel), rmsnorm_row(x, gamma, eps, rel)
    extra = (hi.double() - lo.double()).abs().view(1, K) @ w.double().abs().t()
    return a, extra


def reference(x, w, *, rms=None, bias=None, rope=None, q_scale=None, q_cols=0, act=R.ACT_NONE, residual=None, out_f32=False):
    """fp64 (reference, tolerance) [1, N or N / 2] of one GEMV row: x [K] and w [N, K] in the activations' type (the exact
    values the kernel reads), rms = (gamma [K], eps) or None, the rest as gemm_reference.epilogue"""
    a = x.view(1, -1)
    extra = None
    if rms is not None:
        a, extra = rms_operand(x, rms[0], rms[1], w)
    acc, bound = R.product_and_bound(a, w)
    if extra is not None:
        bound = bound + extra
    return R.epilogue(acc, bound, bias=bias, rope=rope, q_scale=q_scale, q_cols=q_cols, act=act,
                      residual=None if residual is None else residual.view(1, -1), out_f32=out_f32, out_dtype=x.dtype)


def count_violations(c, ref, tol, *, kv=None):
    """elements outside their band, over the WHOLE output row: c [N or N / 2] alone, or -- kv = (k_row, v_row, kv_col0,
    kv_dim) -- columns < kv_col0 of c, then the K row, then the V row"""
    if kv is None:
        return int(R.violations(c.view(1, -1), ref, tol).sum())
    k, v, c0, kd = kv
    assert c0 + 2 * kd == ref.shape[1] and k.numel() == kd and v.numel() == kd
    return (int(R.violations(c[:c0].view(1, -1), ref[:, :c0], tol[:, :c0]).sum())
            + int(R.violations(k.view(1, -1), ref[:, c0:c0 + kd], tol[:, c0:c0 + kd]).sum())
            + int(R.violations(v.view(1, -1), ref[:, c0 + kd:], tol[:, c0 + kd:]).sum()))


def assert_row(c, ref, tol, what, *, kv=None):
    """count_violations == 0, naming the worst elements of the part that fails"""
    if kv is None:
        R.assert_within(c.view(1, -1), ref, tol, what)
        return
    k, v, c0, kd = kv
    assert c0 + 2 * kd == ref.shape[1] and k.numel() == kd and v.numel() == kd
    R.assert_within(c[:c0].view(1, -1), ref[:, :c0], tol[:, :c0], what + " (C)")
    R.assert_within(k.view(1, -1), ref[:, c0:c0 + kd], tol[:, c0:c0 + kd], what + " (K row)")
    R.assert_within(v.view(1, -1), ref[:, c0 + kd:], tol[:, c0 + kd:], what + " (V row)")


def worst_ratio(c, ref, tol, *, kv=None) -> float:
    """largest |out - ref| / tol over the row (for the figures a cell prints)"""
    if kv is None:
        out = c.view(1, -1).double()
    else:
        k, v, c0, kd = kv
        out = torch.cat([c[:c0].double(), k.double(), v.double()]).view(1, -1)
    return float(((out.to(ref.device) - ref).abs() / tol.clamp_min(1e-300)).max())
