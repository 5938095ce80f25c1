"""fp64 reference and per-element tolerance for cogs_gemm (include/cogs.h), used by tests/test_gpu_gemm_conformance.py.

The reference is computed from the EXACT rounded inputs (the bf16 / fp32 values the kernel reads, widened to fp64), and
the epilogue is applied in fp64 in the order of csrc/gemm_epilogue.h:

    y = acc                       acc[m][n] = sum_k A[m][k] W[n][k]
    y = rstd[m] * y + col_c[n]    (LN fold; replaces the bias)        or   y = y + bias[n]
    y = rotary(y)                 pair (2i, 2i+1) of a head: (y0 c - y1 s, y1 c + y0 s), (c, s) of row m and pair i
    y = q * y                     columns < q_cols only (the Q heads, pre-scaled for the attention kernels); q is the fp32
                                  value the kernel multiplies by
    y = act(y)                    GELU (tanh / erf), or SwiGLU  out[j] = silu(y[2j]) * y[2j+1]
    y = y + R[m][n]
    store (one rounding to the output type)

Tolerance, per element, no normalisation by the tensor maximum. Let u = 2^-24 (fp32 unit roundoff) and let E be a bound
on |y_fp32 - y_fp64| carried through the steps:

  * dot product: every product of two bf16 values is exact in fp32, fp32 products of fp32 inputs are rounded once, and
    K additions are rounded; the classical bound gives |acc_fp32 - acc| <= gamma_K (|A||W|^T)[m][n] with
    gamma_K ~ K u. We use E_acc = K 2^-23 (|A||W|^T)[m][n], i.e. twice that, which also covers the order of the MFMA
    partial sums.
  * LN fold (one fma): E = rstd E_acc + 2u (|rstd acc| + |col_c|).  Bias (one add): E = E_acc + u |y|.
  * rotary mixes the two columns of a pair with the row's factors: E'_0 = |c| E_0 + |s| E_1 + 2u (|y_0 c| + |y_1 s|),
    and the same for the second column with the roles swapped.
  * q_scale (one fp32 multiply by the fp32 constant q, columns < q_cols): E = |q| E + u |q y|; a power of two is an
    exact multiply and adds nothing.
  * activations: the local slope bounds how E grows (GELU: |gelu'| <= 1.13; SiLU: |silu'| <= 1.1), plus the error of
    the device formulas themselves (x * sigmoid(.) through v_exp_f32 / v_rcp_f32 and erff: a few fp32 ulps, and the
    relative error of 2^t grows with |t|): 2^-16 |y_out| + 2^-20 |y_in|.
    SwiGLU: E = 1.1 E_g |u| + |silu(g)| E_u + E_g E_u + 2^-16 |out|.
  * residual (one add): E = E + u |y|.
  * the store: one rounding to the output type, half an ulp = u_out |y| with u_out = 2^-8 (bf16) or 2^-24 (fp32):
        |out - y| <= u_out |y| + (1 + u_out) E.

A wrong element passes only if it lands within that band around its OWN exact value, which for a bf16 output is about
one output ulp plus the dot-product bound of that element: a value that is small next to the tensor maximum, a wrong
column of v next to large q values, or a row that got another row's rotary factors all fail.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

U32 = 2.0 ** -24           # fp32 unit roundoff
U_BF16 = 2.0 ** -8         # bf16 unit roundoff (8 significant bits)
GELU_SLOPE, SILU_SLOPE = 1.13, 1.1
ACT_SLACK_OUT, ACT_SLACK_IN = 2.0 ** -16, 2.0 ** -20
ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_SWIGLU = 0, 1, 2, 3      # COGS_ACT_* (include/cogs.h)


@dataclass
class Rope:
    """rotary factors of the selected rows: cos / sin [rows, head_dim / 2] (fp64), applied to columns < cols"""
    cos: torch.Tensor
    sin: torch.Tensor
    cols: int
    head_dim: int


def product_and_bound(a: torch.Tensor, w: torch.Tensor):
    """(acc, E_acc) in fp64 on a's device: acc = A . W^T of the rounded inputs, E_acc = K 2^-23 (|A||W|^T). The bound is
    a magnitude, so its own GEMM runs in fp32 (relative error ~K u, far below the factor 2 the bound already carries)."""
    K = a.shape[1]
    acc = a.double() @ w.double().t()
    bound = (a.float().abs() @ w.float().abs().t()).double() * (K * 2.0 ** -23)
    return acc, bound


def epilogue(acc: torch.Tensor, bound: torch.Tensor, *, cols: Optional[torch.Tensor] = None,
             bias: Optional[torch.Tensor] = None, rstd: Optional[torch.Tensor] = None,
             col_c: Optional[torch.Tensor] = None, rope: Optional[Rope] = None, q_scale: Optional[float] = None,
             q_cols: int = 0, act: int = ACT_NONE, residual: Optional[torch.Tensor] = None, out_f32: bool = False, out_dtype=torch.bfloat16):
    """fp64 (reference, tolerance) of the output columns `cols` (all when None) from acc / bound [rows, len(cols)].
    bias / col_c are full [N] vectors (indexed by cols), rstd [rows], residual [rows, len(cols)]; rotary and SwiGLU need
    whole aligned pairs among the selected columns. q_scale: the fp32 factor of the columns < q_cols (None / q_cols 0: off). SwiGLU returns [rows, len(cols) / 2]."""
    dev = acc.device
    N_sel = acc.shape[1]
    if cols is None:
        cols = torch.arange(N_sel, device=dev)
    cols = cols.to(dev)
    y, e = acc.clone(), bound.clone()
    if rstd is not None:
        r = rstd.double().to(dev)[:, None]
        c = col_c.double().to(dev)[cols][None, :]
        e = r * e + 2 * U32 * ((r * y).abs() + c.abs())
        y = r * y + c
    elif bias is not None:
        y = y + bias.double().to(dev)[cols][None, :]
        e = e + U32 * y.abs()
    if rope is not None:
        assert N_sel % 2 == 0 and bool((cols[0::2] % 2 == 0).all()) and bool((cols[1::2] == cols[0::2] + 1).all())
        pi = ((cols[0::2] % rope.head_dim) // 2).long()
        on = (cols[0::2] < rope.cols)[None, :]
        c, s = rope.cos.double().to(dev)[:, pi], rope.sin.double().to(dev)[:, pi]
        y0, y1, e0, e1 = y[:, 0::2], y[:, 1::2], e[:, 0::2], e[:, 1::2]
        r0, r1 = y0 * c - y1 * s, y1 * c + y0 * s
        f0 = c.abs() * e0 + s.abs() * e1 + 2 * U32 * ((y0 * c).abs() + (y1 * s).abs())
        f1 = c.abs() * e1 + s.abs() * e0 + 2 * U32 * ((y1 * c).abs() + (y0 * s).abs())
        y, e = y.clone(), e.clone()
        y[:, 0::2], y[:, 1::2] = torch.where(on, r0, y0), torch.where(on, r1, y1)
        e[:, 0::2], e[:, 1::2] = torch.where(on, f0, e0), torch.where(on, f1, e1)
    if q_scale is not None and q_cols > 0:
        q = float(torch.tensor(q_scale, dtype=torch.float32))                # the fp32 value, widened
        on = (cols < q_cols)[None, :]
        exact = math.frexp(abs(q))[0] == 0.5                                 # a power of two: the multiply rounds nothing
        e = torch.where(on, abs(q) * e + (0.0 if exact else U32) * (q * y).abs(), e)
        y = torch.where(on, q * y, y)
    if act == ACT_GELU_TANH or act == ACT_GELU_ERF:
        x = y
        if act == ACT_GELU_TANH:
            y = 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
        else:
            y = 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))
        e = GELU_SLOPE * e + ACT_SLACK_OUT * y.abs() + ACT_SLACK_IN * x.abs()
    elif act == ACT_SWIGLU:
        assert N_sel % 2 == 0 and bool((cols[0::2] % 2 == 0).all()) and bool((cols[1::2] == cols[0::2] + 1).all())
        g, u, eg, eu = y[:, 0::2], y[:, 1::2], e[:, 0::2], e[:, 1::2]
        sg = g * torch.sigmoid(g)
        y = sg * u
        e = SILU_SLOPE * eg * u.abs() + sg.abs() * eu + eg * eu + ACT_SLACK_OUT * y.abs() + ACT_SLACK_IN * g.abs()
    if residual is not None:
        y = y + residual.double().to(dev)
        e = e + U32 * y.abs()
    u_out = U32 if (out_f32 or out_dtype == torch.float32) else U_BF16
    return y, u_out * y.abs() + (1.0 + u_out) * e


def violations(out: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor):
    """boolean mask of the elements outside their band (NaN / Inf in `out` count as outside)"""
    err = (out.double().to(ref.device) - ref).abs()
    return ~(err <= tol)


def assert_within(out: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor, what: str = "") -> None:
    """every element of `out` within its own tolerance of the fp64 reference; the message names the worst ones"""
    bad = violations(out, ref, tol)
    n = int(bad.sum())
    if n == 0:
        return
    o = out.double().to(ref.device)
    ratio = torch.where(bad, (o - ref).abs() / tol.clamp_min(1e-300), torch.zeros_like(ref))
    worst = torch.topk(ratio.reshape(-1), min(n, 5)).indices
    shape = list(ref.shape)
    lines = []
    for flat in worst.tolist():
        idx, rem = [], flat
        for d in reversed(shape):
            idx.append(rem % d)
            rem //= d
        idx = tuple(reversed(idx))
        lines.append(f"  at {idx}: out {float(o[idx]):.8g} ref {float(ref[idx]):.8g} tol {float(tol[idx]):.3g}")
    raise AssertionError(f"{what}: {n} of {ref.numel()} elements outside the fp64 band\n" + "\n".join(lines))


def row_stats_reference(stored: torch.Tensor):
    """(sum, sum of squares) per row and 64-column block of the STORED output [M, N] (what cogs_gemm_desc.row_stats holds),
    in fp64, with the tolerance of 64-term fp32 sums: 2^-17 sum |x| and 2^-17 sum x^2"""
    x = stored.double()
    M, N = x.shape
    blocks = x.view(M, N // 64, 64)
    ref = torch.stack([blocks.sum(-1), (blocks ** 2).sum(-1)], -1)
    tol = torch.stack([blocks.abs().sum(-1), (blocks ** 2).sum(-1)], -1) * 2.0 ** -17 + 1e-30
    return ref, tol
