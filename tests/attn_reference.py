"""fp64 reference and per-element tolerance for cogs_attention (include/cogs.h), used by tests/test_gpu_attn_conformance.py.

The reference is computed from the EXACT values the kernel reads (bf16 / fp32 widened to fp64), in log2 units as the
kernels compute it. Query row i of head h reads kv head h // (hq / hkv); key j is visible to row i iff it lies in the
row's key range (the row's cu_seqlens segment, else [0, kv_len)) and, with `causal`, j - ks <= (i - qs) + q_pos0 (ks, qs
= the first key / row of the segment). Scores:

    s_ij = scale_log2 * (q_i . k_j)  [+ bias_log2 for keys in [row_lo[i], row_hi[i])]
    p_ij = 2^(s_ij - max_j s_ij),   o_i = sum_j p_ij v_j / sum_j p_ij          (0 for a row with no visible key)

scale_log2 is the fp32 value the dispatcher derives (fp32(scale) * fp32(log2 e) rounded to fp32, or 1 for pre-scaled Q),
bias_log2 = fp32(bias) * fp32(log2 e) the same way: the rounding of the scale is part of the operation, not of the error.
Everything is evaluated on the inputs' device, chunked over heads and query rows (a 15k-token cell never holds a full
score matrix).

Tolerance, per element, |out - ref| <= tol, never normalised by a tensor or row maximum. u = 2^-24 (fp32 unit roundoff),
u_out = 2^-8 (bf16 output) or 2^-24 (fp32), n = visible keys of the row, nt = ceil(n / 64), hd = head_dim.

MFMA kernels (general 1, ViT 2 / 3 / 8, decode 4 + combine, prompt 5), log2 domain with v_exp_f32:
  * scores: fp32 sums of exact bf16 products, the running reference -m folded into the accumulator (pre-scaled kernels) or
    subtracted by one fma (classic). With a_ij = |scale_log2| (|q_i| . |k_j|) and M_i = max over visible j of |s_ij|:
        |ds_ij| <= C_DOT (a_ij + M_i + 8),   C_DOT = (hd + 8) 2^-23
    (the gamma_hd bound of the GEMM reference, doubled; +8 covers the reference offset of the deferred maximum, <= 2^6 above
    the row maximum by PREFILL_THR / RESCALE_THR = 6, and the bf16 rounding of the ViT kernel's reference).
    A score error ds moves p_ij by a relative ln 2 * ds.
  * exp2: v_exp_f32 is accurate to 1 ulp; EXP_ERR = 2^-22 (two fp32 ulps) relative per exponential.
  * P -> bf16 before the PV MFMA, round-to-nearest-even (pack_bf2, csrc/common.h): relative U_BF16 = 2^-8. P <= 2^6 under
    the deferred maximum, far inside the bf16 range, so the relative bound holds.
  * the row sum l: with hd % 16 == 0 the kernels add the UNROUNDED P (fp32), so the bf16 rounding of P enters the
    numerator only; with SUM_IN_V (hd 72) l is the ones column of V, i.e. it adds the ROUNDED P, and the rounding enters
    numerator and denominator alike.
  * accumulation: O and l are fp32 sums over 2 nt MFMA steps of <= 32 products each plus the cross-lane / cross-split /
    cross-wave merges: N_ACC = 2 nt + 48 + nsplit roundings, each <= u of the magnitude sum.
  * rescale factors 2^-d (running maximum moved): one exp2 and one multiply of O and l each, at most once per tile and
    once per split in the combine: N_RESC = nt + 2 factors, each EXP_ERR + u relative, on both O and l.
  * the final o * (1 / l) (or o / L in the combine): 2 u |o|.
  * one rounding to the output type: u_out |o|.
  Together, with (P x)_i = sum_j p_ij x_ij / l_i (the same attention applied to x):
        c1_ij = ln2 C_DOT (a_ij + M_i + 8) + EXP_ERR + U_BF16 + (N_ACC + N_RESC) u + N_RESC EXP_ERR
        c2_ij = the same without U_BF16, unless SUM_IN_V
        E_i   = (1 + 2^-4) [ (P (c1 |v|))_i + (P c2)_i |o_i| + 2 u |o_i| ]
        tol   = u_out |o| + (1 + u_out) E
  The factor 1 + 2^-4 covers the second-order products of the first-order terms (each is below 2^-7).

Row-wise kernel (7, csrc/attn.hip attn_rowwise_kernel), natural-log domain with expf, one wave per (row, head):
  * scores: sequential fp32 dot products of hd terms (fp32 inputs: each product rounded too), times the fp32 natural scale
    fp32(scale_log2 / log2 e) (two more roundings against scale_log2 ln 2), plus the bias: in natural units
        |ds_ij| <= C_DOT_RW (a_ij ln2 + M_i ln2 + 1),   C_DOT_RW = (2 hd + 8) 2^-24
  * expf: EXPF_ERR = 2^-21 relative (a few ulps of the device libm), twice per key (pass 1 and pass 2).
  * l: per-lane sums of ~n / 64 terms, each rescaled by an expf factor, and a 64-lane tree: (n / 64 + 8) (u + EXPF_ERR).
  * o: every lane sums all n products p_j v_j in sequence, p_j = expf(.) * (1 / l): n + 2 roundings of the magnitude sum.
        c1_ij = ds_ij + 2 EXPF_ERR + (n + 4) u,   c2_ij = ds_ij + 2 EXPF_ERR + (n / 64 + 8)(u + EXPF_ERR)
  and E, tol as above.

Exact data (exact_cell below): integer scores that only differ by 0..6 among the live keys of a row and by >= 250 from
every other key, small-integer V, few live keys. Every live p is a power of two (exact in fp32 and in bf16), every dead p
is exactly 0 after exp2, every sum is exact in fp32, so the kernels' o is fp32(O * fp32(1 / l)) of the exact O and l,
rounded once more to the output type: |out - ref| <= (u_out + 4 u) |ref| + 2^-200 (the fp64 reference still gives the dead
keys weights of 2^-250 and below). This relies on v_exp_f32 returning exact powers of two for integer arguments in
[-12, 6] and 0 below -149; the exact cells themselves measure that on the device (a device that disagreed would fail every
exact cell, by a bounded amount that the message shows). With scale = fp32(ln 2) the classic path is exact as well:
fp32(ln 2) * fp32(log2 e) rounds to 1.0f.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from gemm_reference import assert_within, violations  # noqa: F401  (re-exported for the attention tests)

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
EXP_ERR = 2.0 ** -22
EXPF_ERR = 2.0 ** -21
LN2 = math.log(2.0)
SECOND_ORDER = 1.0 + 2.0 ** -4
EXACT_SLACK_REL, EXACT_SLACK_ABS = 4 * U32, 2.0 ** -200
LOG2E_F32 = 1.4426950408889634        # the dispatcher's constant (csrc/attn.hip), as fp32


def f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def scale_log2_of(scale: float, q_prescaled: bool) -> float:
    """the fp32 scale (log2 units) cogs_k_attention derives from the descriptor"""
    return 1.0 if q_prescaled else f32(f32(scale) * f32(LOG2E_F32))


def _segments(n_rows: int, cu: Optional[Sequence[int]], kv_len: int):
    """per query row: (qs, ks, ke) of its segment"""
    if cu is None:
        z = torch.zeros(n_rows, dtype=torch.long)
        return z, z.clone(), torch.full((n_rows,), kv_len, dtype=torch.long)
    cu_t = torch.tensor(list(cu), dtype=torch.long)
    rows = torch.arange(n_rows)
    seg = torch.bucketize(rows, cu_t[1:], right=True)
    return cu_t[seg], cu_t[seg], cu_t[seg + 1]


def reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, hq: int, hkv: int, hd: int, scale_log2: float = 1.0,
              cu: Optional[Sequence[int]] = None, cu_k: Optional[Sequence[int]] = None, causal: bool = False,
              q_pos0: int = 0, row_lo: Optional[torch.Tensor] = None, row_hi: Optional[torch.Tensor] = None,
              bias_log2: float = 0.0, kv_len: Optional[int] = None, rows: Optional[torch.Tensor] = None,
              kv_head: Optional[Sequence[int]] = None, dup_last: bool = False, bound: Optional[str] = "mfma",
              sum_in_v: bool = False, out_dtype=torch.bfloat16, nsplit: int = 1, chunk: int = 1024):
    """(ref, tol) in fp64, [len(rows), hq * hd], on q's device. q [Lq, hq*hd], k / v [Lk, hkv*hd] token-major (exact values).
    bound: "mfma" / "rowwise" (the derivations above), "exact" (exact data), None (tol = 0).
    Perturbations for the tests of the tests: cu_k = other key-side segment bounds, kv_head = the kv head of every query
    head, dup_last = the last key of every row's key range counted twice (a padding row fetched from the last row and given
    weight)."""
    dev = q.device
    Lq, Lk = q.shape[0], k.shape[0]
    kv_len = Lk if kv_len is None else kv_len
    rows = torch.arange(Lq) if rows is None else rows.cpu().long()
    qs, ks, ke = _segments(Lq, cu, kv_len)
    if cu_k is not None:
        _, ks2, ke2 = _segments(Lq, cu_k, kv_len)
        ks, ke = ks2, ke2
    gsz = hq // hkv
    kvh = list(kv_head) if kv_head is not None else [h // gsz for h in range(hq)]
    u_out = U_BF16 if out_dtype == torch.bfloat16 else U32
    R = rows.numel()
    ref = torch.zeros(R, hq * hd, dtype=torch.float64, device=dev)
    tol = torch.zeros_like(ref)
    keys = torch.arange(Lk, device=dev)
    for c0 in range(0, R, chunk):
        rr = rows[c0:c0 + chunk]
        rd = rr.to(dev)
        lo_k, hi_k = ks[rr].to(dev)[:, None], ke[rr].to(dev)[:, None]
        allow = (keys[None, :] >= lo_k) & (keys[None, :] < hi_k)
        if causal:
            allow &= (keys[None, :] - lo_k) <= (rd - qs[rr].to(dev))[:, None] + q_pos0
        mult = torch.ones(allow.shape, dtype=torch.float64, device=dev)
        if dup_last:
            last = torch.where(allow, keys[None, :], torch.full_like(keys[None, :], -1)).amax(1)
            mult[torch.arange(len(rr), device=dev)[last >= 0], last[last >= 0]] = 2.0
        inb = None
        if row_lo is not None:
            inb = (keys[None, :] >= row_lo.to(dev)[rd][:, None].long()) & (keys[None, :] < row_hi.to(dev)[rd][:, None].long())
        n_vis = allow.sum(1).double()
        for h in range(hq):
            qh = q[rd, h * hd:(h + 1) * hd].double()
            kh = k[:, kvh[h] * hd:(kvh[h] + 1) * hd].double()
            vh = v[:, kvh[h] * hd:(kvh[h] + 1) * hd].double()
            s = (qh @ kh.t()) * scale_log2
            if inb is not None:
                s = s + inb.double() * bias_log2
            s_m = s.masked_fill(~allow, float("-inf"))
            m = s_m.amax(1, keepdim=True)
            m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
            p = torch.exp2(s_m - m) * mult
            l = p.sum(1, keepdim=True)
            safe_l = torch.where(l > 0, l, torch.ones_like(l))
            o = (p @ vh) / safe_l
            o = torch.where(l > 0, o, torch.zeros_like(o))
            ref[c0:c0 + len(rr), h * hd:(h + 1) * hd] = o
            if bound is None:
                continue
            if bound == "exact":
                tol[c0:c0 + len(rr), h * hd:(h + 1) * hd] = (u_out + EXACT_SLACK_REL) * o.abs() + EXACT_SLACK_ABS
                continue
            a = (qh.abs() @ kh.abs().t()) * abs(scale_log2)
            big_m = s_m.abs().masked_fill(~allow, 0.0).amax(1, keepdim=True)
            nv = n_vis[:, None]
            nt = torch.ceil(nv / 64)
            av = vh.abs()
            w = p / safe_l                                     # normalised weights
            if bound == "mfma":
                c_dot = (hd + 8) * 2.0 ** -23
                n_acc, n_resc = 2 * nt + 48 + nsplit, nt + 2
                base = EXP_ERR + (n_acc + n_resc) * U32 + n_resc * EXP_ERR
                ds = LN2 * c_dot * (a + big_m + 8)
                c1_const = base + U_BF16
                c2_const = base + (U_BF16 if sum_in_v else 0.0)
            elif bound == "rowwise":
                c_dot = (2 * hd + 8) * U32
                ds = c_dot * (a * LN2 + big_m * LN2 + 1)
                c1_const = 2 * EXPF_ERR + (nv + 4) * U32
                c2_const = 2 * EXPF_ERR + (nv / 64 + 8) * (U32 + EXPF_ERR)
            else:
                raise ValueError(bound)
            e1 = (w * ds) @ av + c1_const * (w @ av)
            e2 = (w * ds).sum(1, keepdim=True) + c2_const * w.sum(1, keepdim=True)
            e = SECOND_ORDER * (e1 + e2 * o.abs() + 2 * U32 * o.abs())
            tol[c0:c0 + len(rr), h * hd:(h + 1) * hd] = u_out * o.abs() + (1 + u_out) * e
    return ref, tol


# ----------------------------------------------------------------------------------------------------------- exact data
CODE_B = 8          # the last 8 dims of a head carry the B part of a key's two-hot code


def key_code(j, hd: int, head: int):
    """(a, b) of key j under kv head `head`: a in [0, hd - 8), b in [0, 8); period 8 (hd - 8). Every kv head has its own
    offset, so a query head mapped to the neighbouring kv head scores other keys."""
    A = hd - CODE_B
    jj = j + 37 * head + 11
    return jj % A, A + (jj // A) % CODE_B


def exact_kv(Lk: int, hkv: int, hd: int, gen: torch.Generator, v_range: int = 8):
    """K [Lk, hkv*hd]: two-hot codes; V: integers in [-v_range, v_range] (exact in bf16 and fp32)"""
    k = torch.zeros(Lk, hkv * hd)
    j = torch.arange(Lk)
    for h in range(hkv):
        a, b = key_code(j, hd, h)
        k[j, h * hd + a] = 1.0
        k[j, h * hd + b] = 1.0
    v = torch.randint(-v_range, v_range + 1, (Lk, hkv * hd), generator=gen).float()
    return k, v


def exact_q(keys: torch.Tensor, g: torch.Tensor, hq: int, hkv: int, hd: int):
    """Q [Lq, hq*hd]: row i aims at the targets keys[i, :] (int64, [Lq, T]) with offsets g[i, :] in 0..6: q = sum (256 - g)
    e_a + 512 e_b over the targets' codes (two targets on one a-dim keep the smaller g). A target scores 768 - g, a key that
    shares only one half of a target's code <= 512, every other key 0. Keys whose code equals a target's (the period, or a
    cross code (a_r, b_s) of two targets) score the same and are live too; the reference counts them. The same targets for
    every query head, coded under that head's kv head."""
    Lq, T = keys.shape
    q = torch.zeros(Lq, hq * hd)
    gsz = hq // hkv
    rows = torch.arange(Lq)[:, None].expand(Lq, T)
    for h in range(hq):
        a, b = key_code(keys, hd, h // gsz)
        blk = torch.zeros(Lq * hd)
        blk.scatter_reduce_(0, (rows * hd + a).reshape(-1), (256.0 - g.float()).reshape(-1), reduce="amax")
        blk[(rows * hd + b).reshape(-1)] = 512.0
        blk = blk.view(Lq, hd)
        q[:, h * hd:(h + 1) * hd] = blk
    return q


def live_counts(q, k, hq, hkv, hd, rows) -> torch.Tensor:
    """largest number of keys per row that score within 8 of the row's best (any visibility): the exactness premise"""
    gsz = hq // hkv
    worst = 0
    for h in range(hq):
        s = q[rows, h * hd:(h + 1) * hd].double() @ k[:, (h // gsz) * hd:(h // gsz + 1) * hd].double().t()
        worst = max(worst, int((s >= s.amax(1, keepdim=True) - 8).sum(1).max()))
    return worst
