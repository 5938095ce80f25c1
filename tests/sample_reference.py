"""fp64 reference, Philox reference and per-element tolerance for cogs_sample, cogs_argmax, cogs_topk and
cogs_logits_process (include/cogs.h), used by tests/test_sample_reference.py and tests/test_gpu_sample_conformance.py.
Plain numpy; it does not import the library.

The operation (transformers 4.46.3: TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, softmax, multinomial):

    v_i  = fp32(logit_i / fp32(temperature))                 one IEEE division, as the kernels do -- part of the operation
    top-k: keep v_i >= the k-th largest v (IEEE comparison: -0 == +0); off for top_k == 0 or top_k >= n
    p    = softmax over the kept v                            fp64 here
    top-p: sort ascending, remove the prefix whose inclusive cumulative p is <= fp32(1 - top_p), always keep the largest
    p'   = softmax over the survivors; token = argmax_i p'_i / q_i, q_i ~ Exp(1), lower id on equal scores

Entries at -inf (masked) are never candidates and never reported. Where HF leaves the outcome to its unstable sort the
project fixes it (include/cogs.h, cogs_sample): the kept list is ordered by descending v, equal v by ascending id; the slice
path (1) cuts top-p by POSITION in that list (the kept count is HF's, a cut inside a block of equal v keeps the lower ids);
the whole-row path (2) thresholds on the VALUE (every entry equal to the boundary value stays). `warp` returns both.

Tolerance of a kept probability, per element, |p_dev - p_ref| <= prob_tol(D, m, path), never a norm over the row.
u = 2^-24 (fp32 unit roundoff), D_j = |v_j - max v| (in fp64, of the fp32 v), m = number of terms in the final sum.
  * e_j = expf(fl(v_j - max)): the subtraction rounds once, |d - (v_j - max)| <= u D_j, which the exponential turns into a
    relative u D_j; expf itself EXPF_ERR = 2^-23 relative: the HIP math API documents expf (and logf) at a maximum error
    of 1 ulp, and one fp32 ulp is at most 2^-23 of the value. (attn_reference.py allows its row-wise kernel 2^-21; here the
    documented figure is taken, because a bound of 8 u from the exponentials alone could not reject an 8-ulp error.)
  * the sum S = sum_i e_i: every term carries its own relative error u D_i + EXPF_ERR, so S carries their p-weighted mean.
    sum_i p_i D_i = H(p) - ln Z <= ln m (H the entropy of p, Z = sum_i exp(-D_i) >= 1 because the maximum contributes 1), so
    the terms contribute at most u ln m + EXPF_ERR. The summation itself: path 1 adds m positive fp32 terms in sequence,
    (m - 1) u relative; path 2 adds them in fp64 (m 2^-53 <= 2^-35, absorbed) and rounds the total to fp32 once; the 16
    partial sums are fp64 too: 2 u covers it.
  * one division p_j = e_j / S: u.
        rel(D, m, 1) = (1 + 2^-10) (u D + 2 EXPF_ERR + u ln m + (m - 1) u + u)      = about (D + ln m + m + 4) u
        rel(D, m, 2) = (1 + 2^-10) (u D + 2 EXPF_ERR + u ln m + 2 u + u)            = about (D + ln m + 7) u
        prob_tol     = rel * p_ref + 2^-126
    1 + 2^-10 covers the products of the first-order terms (each below 2^-11 for m <= 1024, D <= 2^12); 2^-126 covers an
    exponential or a quotient in the subnormal range being flushed.
torch's fp32 softmax (the fixture's probabilities) does the same steps in another summation order; (m - 1) u bounds any
order, so the fixture is held to rel(D, m, 1).

The top-p cut compares cumulative sums of p (over the m0 entries top-k kept) with fp32(1 - top_p). Their absolute error,
with cum <= 1 and the same weighted-mean argument for the terms:
        cum_err(m0, 1) = (1 + 2^-10) (2 u ln m0 + 2 EXPF_ERR + (m0 - 1) u + u) + (m0 - 1) u      fp32 running sum
        cum_err(m0, 2) = (1 + 2^-10) (2 u ln m0 + 2 EXPF_ERR + 3 u) + 2^-40                       fp64 digit sums
A row is usable by a GPU test when its margin -- the smallest |cum - fp32(1 - top_p)| over every cumulative sum the cut can
compare -- is at least 100 cum_err (test_sample_reference.py asserts that for every row of the GPU file).

Scores p_i / q_i. Handed-over draws are exact inputs: rel(D_i, m, path) + u for the division. Device draws are
q = -logf(u32), u32 = ((x >> 8) + 1) 2^-24 exact in fp32, against -log(u32) in fp64 here: LOGF_ERR = 2^-23 relative, plus
an absolute 2^-26 for an implementation that is only absolutely accurate near u32 -> 1 (q -> 0, where the smallest nonzero
q is 2^-24): score_err = rel + u + 2^-23 + 2^-26 / q. A draw decides the token safely when the relative gap between the
best and the second-best score exceeds the sum of their two score_err; the few others are listed by the CPU test and left
out of the device comparison (at most 1 % of a row's draws, asserted).

cogs_argmax / cogs_topk / cogs_logits_process are selections and single fp32 IEEE operations: compared bit for bit.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

U = 2.0 ** -24
EXPF_ERR = 2.0 ** -23
LOGF_ERR = 2.0 ** -23
SECOND = 1.0 + 2.0 ** -10
MARGIN_FACTOR = 100.0


# ---------------------------------------------------------------------------------------------------------------- bounds
def prob_rel(D, m: int, path: int):
    """relative bound on a kept probability; D = |v_j - max v| (scalar or array), m terms in the sum"""
    s = (max(m, 1) - 1) * U if path == 1 else 2 * U
    return SECOND * (U * np.asarray(D, np.float64) + 2 * EXPF_ERR + U * math.log(max(m, 1)) + s + U)


def prob_tol(p_ref, D, m: int, path: int):
    return prob_rel(D, m, path) * np.asarray(p_ref, np.float64) + 2.0 ** -126


def cum_err(m0: int, path: int) -> float:
    m0 = max(m0, 1)
    if path == 1:
        return SECOND * (2 * U * math.log(m0) + 2 * EXPF_ERR + (m0 - 1) * U + U) + (m0 - 1) * U
    return SECOND * (2 * U * math.log(m0) + 2 * EXPF_ERR + 3 * U) + 2.0 ** -40


def score_err(D, m: int, path: int, q=None):
    """relative bound on p_i / q_i; q = the fp64 device draws (None: handed-over fp32 draws, exact inputs)"""
    e = prob_rel(D, m, path) + U
    if q is not None:
        with np.errstate(divide="ignore"):
            e = e + LOGF_ERR + 2.0 ** -26 / np.asarray(q, np.float64)
    return e


# ------------------------------------------------------------------------------------------------------------------ warp
@dataclass
class Warped:
    v: np.ndarray            # fp32 [n]: logits / temperature
    m0: int                  # entries top-k kept (finite ones)
    topk_above: np.ndarray   # ids strictly above the k-th value (empty when top-k is off)
    topk_tied: np.ndarray    # ids equal to the k-th value (IEEE ==), ascending
    ids: np.ndarray          # survivors by POSITION (path 1, HF's count): descending v, equal v by ascending id
    probs: np.ndarray        # fp64, renormalised over ids
    ids_all: np.ndarray      # survivors by VALUE (path 2): topp_above + every id tied at the boundary, same order
    probs_all: np.ndarray
    topp_above: np.ndarray   # survivors strictly above the boundary value (the smallest surviving v)
    topp_tied: np.ndarray    # ids equal to the boundary value among what top-k kept
    hf_count: int            # len(ids)
    margin: float            # min |cum - fp32(1 - top_p)| over every cumulative sum the cut compares (inf: no cut)
    lim: float               # fp32(1 - top_p) as fp64 (0: top-p off)
    D: np.ndarray            # |v - max| of ids
    D_all: np.ndarray

    @property
    def tie_free(self) -> bool:
        return len(self.ids) == len(self.ids_all)


def _softmax64(v64: np.ndarray) -> np.ndarray:
    e = np.exp(v64 - v64.max())
    return e / e.sum()


def warp(logits_f32, temperature: float, top_k: int, top_p: float) -> Warped:
    x = np.asarray(logits_f32, dtype=np.float32)
    n = x.size
    v = (x / np.float32(temperature)).astype(np.float32)
    v64 = v.astype(np.float64)
    finite = v64 > -np.inf
    empty = np.zeros(0, np.int64)
    if 0 < top_k < n:
        kth = np.sort(v64)[n - top_k]
        keep = (v64 >= kth) & finite                       # IEEE: -0 >= +0
        above = np.flatnonzero((v64 > kth) & finite)
        tied = np.flatnonzero((v64 == kth) & finite)
    else:
        keep, above, tied = finite, empty, empty
    cand = np.flatnonzero(keep)
    if cand.size == 0:
        z = np.zeros(0, np.float64)
        return Warped(v, 0, above, tied, empty, z, empty, z, empty, empty, 0, math.inf, 0.0, z, z)
    order = np.lexsort((cand, -(v64[cand] + 0.0)))         # descending v (-0 as +0), ascending id
    ids = cand[order]
    vs = v64[ids]
    p = _softmax64(vs)
    m0 = ids.size
    lim = 0.0 if top_p >= 1.0 else float(np.float32(1.0 - top_p))
    keep_n, margin = m0, math.inf
    if lim > 0.0 and m0 > 1:
        cum = np.cumsum(p[::-1])[:-1]                      # ascending, inclusive, the largest entry never compared
        keep_n = m0 - int(np.count_nonzero(cum <= lim))
        margin = float(np.abs(cum - lim).min())
    elif lim > 0.0:
        keep_n = 1
    pos_ids = ids[:keep_n]
    bval = vs[keep_n - 1]
    all_n = int(np.count_nonzero(vs >= bval))
    all_ids = ids[:all_n]
    t_above = ids[vs > bval]
    t_tied = np.sort(ids[vs == bval])
    mx = vs[0]
    return Warped(v, m0, above, tied, pos_ids, _softmax64(vs[:keep_n]), all_ids, _softmax64(vs[:all_n]), t_above, t_tied,
                  keep_n, margin, lim, mx - vs[:keep_n], mx - vs[:all_n])


# ---------------------------------------------------------------------------------------------------------------- Philox
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def _philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC 2011) on uint64 arrays holding 32-bit words -> the four output words"""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & _MASK for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(_M0) * c0
        p1 = np.uint64(_M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & _MASK, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & _MASK)
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox4x32_10(counter: Sequence[int], key: Sequence[int]):
    """counter: 4 words, key: 2 words -> 4 words (python ints)"""
    return tuple(int(w) for w in _philox(*counter, *key))


def device_word(seed: int, offset: int, i):
    """the 32-bit word cogs_sample draws for vocabulary entry i: counter (i, offset lo, offset hi, 0), key (seed lo, seed hi),
    first output word"""
    i = np.asarray(i, np.uint64)
    z = np.zeros_like(i)
    return _philox(i, z + np.uint64(offset & 0xFFFFFFFF), z + np.uint64((offset >> 32) & 0xFFFFFFFF), z,
                   seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]


def device_draw(seed: int, offset: int, i) -> np.ndarray:
    """q_i = -log(u), u = ((x >> 8) + 1) 2^-24 in (0, 1], in fp64"""
    x = device_word(seed, offset, i)
    u = ((x >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    return -np.log(u)


def pick(ids, probs_f64, q_f64):
    """argmax of p / q, lower id on equal scores -> (token, relative gap between the best and the second-best score,
    position of the best, position of the second best); gap = inf for a single candidate"""
    ids = np.asarray(ids)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.asarray(probs_f64, np.float64) / np.asarray(q_f64, np.float64)
    order = np.lexsort((ids, -sc))
    b = int(order[0])
    if ids.size == 1:
        return int(ids[b]), math.inf, b, b
    s = int(order[1])
    gap = 0.0 if sc[b] == sc[s] else (1.0 if np.isinf(sc[b]) else float(1.0 - sc[s] / sc[b]))
    return int(ids[b]), gap, b, s


def draw_is_safe(D, m: int, path: int, probs, q, device: bool) -> bool:
    """the best / second-best gap of this draw exceeds what the device's rounding can move (module docstring)"""
    _, gap, b, s = pick(np.arange(len(probs)), probs, q)
    if b == s:
        return True
    err = score_err(np.asarray(D)[[b, s]], m, path, np.asarray(q, np.float64)[[b, s]] if device else None)
    return bool(gap > float(np.sum(err)))


# --------------------------------------------------------------------------------------------------------------- checker
def compare_kept(ref_ids, ref_probs, D, m: int, path: int, got_ids, got_probs, ordered: bool):
    """the comparison of the GPU tests -> (list of failures, worst observed / bound). ordered: got_ids has to BE ref_ids
    (path 1); else the same set in any order (path 2). Probabilities per element against prob_tol."""
    ref_ids, got_ids = np.asarray(ref_ids, np.int64), np.asarray(got_ids, np.int64)
    got_probs = np.asarray(got_probs, np.float32)
    bad = []
    if got_ids.size != ref_ids.size:
        return [f"kept {got_ids.size} ids, reference {ref_ids.size}: got {got_ids[:40].tolist()} want {ref_ids[:40].tolist()}"], math.inf
    if ordered:
        if not np.array_equal(got_ids, ref_ids):
            w = int(np.flatnonzero(got_ids != ref_ids)[0])
            return [f"kept_idx[{w}] = {got_ids[w]}, reference {ref_ids[w]} (descending score, equal scores by ascending id)"], math.inf
        perm = np.arange(ref_ids.size)
    else:
        if np.unique(got_ids).size != got_ids.size or not np.array_equal(np.sort(got_ids), np.sort(ref_ids)):
            return [f"survivor set differs: only device {np.setdiff1d(got_ids, ref_ids)[:20].tolist()}, "
                    f"only reference {np.setdiff1d(ref_ids, got_ids)[:20].tolist()}"], math.inf
        perm = np.argsort(got_ids, kind="stable")[np.argsort(np.argsort(ref_ids, kind="stable"), kind="stable")]
    gp = got_probs.astype(np.float64)[perm]
    tol = prob_tol(ref_probs, D, m, path)
    ratio = np.abs(gp - np.asarray(ref_probs, np.float64)) / tol
    worst = float(ratio.max()) if ratio.size else 0.0
    if not np.all(ratio <= 1.0):                                                      # NaN fails too
        w = int(np.flatnonzero(~(ratio <= 1.0))[0])
        bad.append(f"prob of id {ref_ids[w]}: {gp[w]!r} vs {ref_probs[w]!r}, {ratio[w]:.2f} x the bound {tol[w]:.3e}")
    return bad, worst


def compare_token(token: int, want: int):
    return [] if int(token) == int(want) else [f"token {int(token)}, reference {int(want)}"]


# ------------------------------------------------------------------------------------- argmax / topk / logits processors
def argmax_first(x) -> int:
    """first maximum under IEEE == (+0 == -0); 0 on a row of -inf"""
    return int(np.argmax(np.asarray(x, np.float32)))


def topk_stable(x, k: int):
    """the k largest, descending, equal values (IEEE ==) by ascending index; past the finite entries the tail is
    (-inf, -1) -> (values fp32 [k], indices int32 [k])"""
    x = np.asarray(x, np.float32)
    order = np.argsort(-(x.astype(np.float64) + 0.0), kind="stable")
    order = order[x[order] > -np.inf][:k]
    val = np.full(k, -np.inf, np.float32)
    idx = np.full(k, -1, np.int32)
    val[:order.size] = x[order]
    idx[:order.size] = order
    return val, idx


def penalty_mask_temperature(logits, prev: Optional[Sequence[int]], penalty: float, allowed: Optional[Sequence[int]],
                             temperature: float) -> np.ndarray:
    """RepetitionPenaltyLogitsProcessor (every id of the history once: s < 0 ? s * pen : s / pen), then the allowed-id mask
    (everything else -inf), then TemperatureLogitsWarper -- each one fp32 IEEE operation"""
    x = np.array(logits, dtype=np.float32, copy=True)
    pen, t = np.float32(penalty), np.float32(temperature)
    if prev is not None and len(prev) > 0 and pen != np.float32(1.0):
        ids = np.unique(np.asarray(prev, np.int64))
        s = x[ids]
        with np.errstate(invalid="ignore"):
            x[ids] = np.where(s < 0, s * pen, s / pen).astype(np.float32)
    if allowed is not None and len(allowed) > 0:
        keep = np.zeros(x.size, bool)
        keep[np.asarray(allowed, np.int64)] = True
        x[~keep] = -np.inf
    if t != np.float32(1.0):
        x = (x / t).astype(np.float32)
    return x
