"""References and comparison rules for the row kernels between the ViT and the LLM: the norms of csrc/norm.hip, the
compression helpers of csrc/compress.hip, pack_rows of csrc/vision_misc.hip and the k-means steps of csrc/kmeans.hip. Used
by tests/test_rowops_reference.py (CPU) and tests/test_gpu_rowops_conformance.py. Plain numpy: no torch, no library.

Three kinds of reference live here.
  * fp64 arithmetic on the given inputs (norms, means, cosine, distances, shift): what the operation IS.
  * round_bf16, round to nearest even on the fp32 bit pattern, and bf16_bracket, the two bf16 neighbours of an fp64 value
    taken in fp64 (no detour through fp32, so no double rounding): what a bf16 output may be.
  * fp32 operation-by-operation emulation where a kernel promises torch's fp32 operations one by one (the keep-mask chain,
    the k-means assignment, the k-means++ draw, the centre means): numpy float32 scalars / arrays round every operation
    to nearest even like the device's __f*_rn intrinsics; sqrt of a float32 is correctly rounded in both.

Comparison rules (the GPU file calls exactly these, the CPU file plants errors into them):
  * yardstick cells: err(got) = max |got - ref| / unit elementwise; a cell passes when err(kernel) <= 4 * err(plain fp32
    implementation of the same operation on the same inputs). FLOOR = 2^-25 (half an fp32 ulp at 1, the error of ONE
    correctly rounded operation) replaces a yardstick that happens to be smaller -- an input on which the plain
    implementation is exact (D = 1 cosine) would otherwise demand an exact kernel.
  * nearest-bf16 cells: got must be the bf16 nearest to the fp64 reference; where the reference lies within delta of the
    midpoint of its two neighbours either passes. Inner roundings (RMSNorm's (x * rstd).to(bf16), ln_merge's stored
    post-LayerNorm rows) follow the same rule and the final value is recomputed from the admissible inner values.
  * exact cells: bit equality.
"""
from __future__ import annotations

import itertools

import numpy as np

U = 2.0 ** -24           # fp32 unit roundoff
FLOOR = 2.0 ** -25
FACTOR = 4.0
F32 = np.float32


# ------------------------------------------------------------------------------------------------ bf16
def round_bf16(x) -> np.ndarray:
    """fp32 -> the fp32 value of the nearest bf16, ties to even, on the bit pattern; NaN stays NaN (quiet), inf stays inf"""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, ((b | 0x00400000) & 0xFFFF0000).astype(np.uint32), r)
    return r.view(F32).reshape(np.shape(x))


def bf16_bits(x) -> np.ndarray:
    """fp32 values that are exact in bf16 -> their 16-bit patterns"""
    b = np.ascontiguousarray(x, F32).view(np.uint32)
    assert np.all((b & 0xFFFF) == 0), "not a bf16 value"
    return (b >> 16).astype(np.uint16).reshape(np.shape(x))


def from_bf16_bits(h) -> np.ndarray:
    return (np.ascontiguousarray(h).view(np.uint16).astype(np.uint32) << 16).view(F32).reshape(np.shape(h))


def bf16_bracket(ref):
    """fp64 -> (lo, hi): the bf16 values (as fp64) with |lo| <= |ref| <= |hi|, one bf16 step apart (lo == hi == ref when ref
    is itself a bf16 value is NOT special-cased: then lo = ref, hi = the next one out)"""
    ref = np.asarray(ref, np.float64)
    a = np.abs(ref)
    _, e = np.frexp(a)                                    # a = m 2^e, 0.5 <= m < 1
    e = np.maximum(e - 1, -126)                           # exponent of the leading bit; denormals share 2^-126
    step = np.ldexp(1.0, e - 7)
    lo = np.floor(a / step) * step
    s = np.where(np.signbit(ref), -1.0, 1.0)
    return s * lo, s * (lo + step)


def nearest_bf16(ref, delta):
    """-> (main, other, near): main the bf16 nearest to the fp64 ref (ties to even), other the second neighbour, near =
    ref within delta of their midpoint (delta broadcast against ref)"""
    ref = np.asarray(ref, np.float64)
    lo, hi = bf16_bracket(ref)
    mid = 0.5 * (lo + hi)
    d = np.abs(ref) - np.abs(mid)
    even_lo = (np.round(np.abs(lo) / (np.abs(hi) - np.abs(lo))) % 2) == 0
    take_hi = (d > 0) | ((d == 0) & ~even_lo)
    main = np.where(take_hi, hi, lo)
    other = np.where(take_hi, lo, hi)
    near = np.abs(d) <= delta
    return main, other, near


def bf16_window(ref, delta):
    """-> (lo, hi, wide): every bf16 value that is the nearest bf16 of SOME value within delta of ref lies in [lo, hi]
    (numerically ordered); wide = the window holds more than one value. For delta below half a bf16 step this is the rule
    "the nearest bf16, either neighbour within delta of a midpoint"; for an element whose own magnitude is far below delta (a
    LayerNorm output where gamma xhat and beta cancel) it is the only form of that rule a finite-precision kernel can meet."""
    ref = np.asarray(ref, np.float64)
    a, b = nearest_bf16(ref - delta, 0.0)[0], nearest_bf16(ref + delta, 0.0)[0]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return lo, hi, lo != hi


def check_nearest_bf16(got, ref, delta, cap=0.01):
    """got: fp32 values of the bf16 outputs. -> (list of complaints, share of excepted elements)"""
    got = np.asarray(got, np.float64)
    lo, hi, wide = bf16_window(ref, delta)
    ok = (got >= lo) & (got <= hi)
    bad = []
    if not np.all(ok):
        i = np.flatnonzero(~ok.ravel())
        bad.append(f"{i.size} elements are not the nearest bf16, first {i[:5].tolist()}: got {got.ravel()[i[:5]].tolist()} "
                   f"reference {np.asarray(ref).ravel()[i[:5]].tolist()}")
    share = float(np.mean(wide)) if wide.size else 0.0
    if share > cap:
        bad.append(f"{share:.4f} of the elements lie within delta of a midpoint (cap {cap})")
    return bad, share


def mismatch(got, want):
    """bit-for-bit comparison of two arrays of the same shape -> the indices [n, ndim] at which they differ (a NaN equals
    the same NaN pattern, +0 differs from -0)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (got.shape, want.shape, got.dtype, want.dtype)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.argwhere(got.view(u) != want.view(u))


def yardstick_ratio(got, plain, ref, unit):
    """-> (kernel worst, yardstick worst (floored), ratio) in the given unit; unit == 0 elements must be exact"""
    ref = np.asarray(ref, np.float64)
    unit = np.broadcast_to(np.asarray(unit, np.float64), ref.shape)

    def worst(v):
        e = np.abs(np.asarray(v, np.float64) - ref)
        if not np.all(np.isfinite(e)):
            return float("inf")
        z = unit == 0
        if np.any(e[z] != 0):
            return float("inf")
        return float(np.max(e[~z] / unit[~z])) if np.any(~z) else 0.0
    k, y = worst(got), max(worst(plain), FLOOR)
    return k, y, k / y


# ------------------------------------------------------------------------------------------------ norms
def layernorm64(x, gamma, beta, eps):
    """-> (y, unit): nn.LayerNorm in fp64 (biased variance), unit = |gamma xhat| + |beta| per element"""
    x = np.asarray(x, np.float64)
    g, b = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    xhat = (x - mean) / np.sqrt(var + float(eps))
    return xhat * g + b, np.abs(xhat * g) + np.abs(b)


def rmsnorm64(x, gamma, eps):
    """-> (inner, y, unit): Qwen2RMSNorm in fp64: inner = x rsqrt(mean x^2 + eps), y = gamma inner"""
    x = np.asarray(x, np.float64)
    g = np.asarray(gamma, np.float64)
    inner = x / np.sqrt((x * x).mean(axis=1, keepdims=True) + float(eps))
    return inner, inner * g, np.abs(inner * g)


def ln_merge64(x, gamma, beta, group, eps):
    """post-LayerNorm of every row, then the mean of each `group` consecutive rows -> (rows [R, H], y, unit)"""
    rows, unit = layernorm64(x, gamma, beta, eps)
    H = rows.shape[1]
    return rows, rows.reshape(-1, group, H).mean(axis=1), unit.reshape(-1, group, H).mean(axis=1)


def check_rmsnorm_bf16(got, x, gamma, eps, delta_rel, cap=0.01):
    """Qwen2's two roundings: got == round_bf16(gamma * round_bf16(x rstd)); an inner value within delta of a midpoint may take
    its other neighbour. gamma and both candidates are bf16 values, so the product is exact in fp32 and the outer
    rounding has one answer. delta = delta_rel * |inner| (the unit of the fp32 cell without gamma)."""
    inner, y, _ = rmsnorm64(x, gamma, eps)
    g64 = np.asarray(gamma, F32)[None, :].astype(np.float64)
    lo, hi, wide = bf16_window(inner, delta_rel * np.abs(inner))
    want = round_bf16((g64 * lo).astype(F32)).astype(np.float64)
    alt = round_bf16((g64 * hi).astype(F32)).astype(np.float64)
    got = np.asarray(got, np.float64)
    ok = (got == want) | (got == alt)
    bad = []
    if not np.all(ok):
        i = np.flatnonzero(~ok.ravel())
        bad.append(f"{i.size} elements differ from round(gamma * round(x rstd)), first {i[:5].tolist()}: got "
                   f"{got.ravel()[i[:5]].tolist()} want {want.ravel()[i[:5]].tolist()}")
    share = float(np.mean(wide))
    if share > cap:
        bad.append(f"{share:.4f} of the inner values lie within delta of a midpoint (cap {cap})")
    return bad, share


def merge_final(inner, group):
    """inner [R, group, H] bf16 values -> the stored average: fp32 sum in row order, times fp32(1 / group), rounded to bf16.
    The sum of a few bf16 values is exact in fp32 but for stray low bits, 1 / group is exact for the model's 2 x 2 merge;
    for group 3 the product is the one fp32 operation whose rounding the average inherits"""
    acc = seq_sum32(np.moveaxis(np.asarray(inner, F32), 1, 0))
    return round_bf16((acc * (F32(1.0) / F32(group))).astype(F32))


def check_ln_merge_bf16(got, x, gamma, beta, group, eps, delta_rel, cap=0.01):
    """every normalised row is rounded to bf16 before the average (the stored post_layernorm output): each inner value follows
    the nearest-bf16 rule, and the output must be merge_final of one admissible choice of inner values"""
    rows, unit = layernorm64(x, gamma, beta, eps)
    H = rows.shape[1]
    R_ = rows.shape[0] // group
    lo, hi, wide = (a.reshape(R_, group, H) for a in bf16_window(rows, delta_rel * unit))
    main = nearest_bf16(rows, 0.0)[0].reshape(R_, group, H)
    got = np.asarray(got, F32)
    ok = got == merge_final(main, group)
    for r, h in zip(*np.nonzero(wide.any(axis=1) & ~ok)):        # few: try the other admissible inner values
        choices = [sorted({lo[r, g, h], hi[r, g, h], main[r, g, h]}) for g in range(group)]
        for combo in itertools.product(*choices):
            if got[r, h] == merge_final(np.array(combo, F32).reshape(1, group, 1), group)[0, 0]:
                ok[r, h] = True
                break
    bad = []
    if not np.all(ok):
        i = np.flatnonzero(~ok.ravel())
        bad.append(f"{i.size} elements are not the rounded mean of the rounded rows, first {i[:5].tolist()}: got "
                   f"{got.ravel()[i[:5]].tolist()} want {merge_final(main, group).ravel()[i[:5]].tolist()}")
    share = float(np.mean(wide.any(axis=1)))
    if share > cap:
        bad.append(f"{share:.4f} of the elements have an inner value within delta of a midpoint (cap {cap})")
    return bad, share


def ln_finalize64(part, H, eps):
    """part [rows, tiles, 2] fp32 (sum, sum of squares) -> (rstd, -rstd mean) in fp64, biased variance clamped at 0"""
    p = np.asarray(part, F32).astype(np.float64)
    s1, s2 = p[..., 0].sum(axis=1), p[..., 1].sum(axis=1)
    mean = s1 / H
    var = np.maximum(s2 / H - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + float(F32(eps)))
    return np.stack([rstd, -rstd * mean], axis=1)


def ulps32(got, ref) -> float:
    """max |got - ref| in fp32 ulps of ref"""
    ref = np.asarray(ref, np.float64)
    ulp = np.spacing(np.abs(ref).astype(F32)).astype(np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / ulp)) if ref.size else 0.0


# ------------------------------------------------------------------------------------------------ keep-mask
PIX_UNIT = 2.0 ** -7
# the mean of the chain: "mul" = sum * fp32(1 / E), what torch's mean computes on the device (its reduction scales the sum by
# a precomputed factor) and what the kernel does; "div" = sum / E, torch's mean on the CPU. They differ by one fp32 ulp for
# some sums; the discriminating cells of rowops_cells.py sit on such sums
MEAN_BY = "mul"


def _rnd(v, bf16):
    return round_bf16(v) if bf16 else np.asarray(v, F32)


def pixdiff_chain(units, E, thr, bf16, mean_by=None):
    """keep decision of rows whose sum of |differences| is units * 2^-7 (exact in fp32 below 2^13): fp32 mean (MEAN_BY),
    rounded in the input dtype; times 255, rounded in the input dtype; strictly above
    the threshold rounded to the input dtype"""
    s = (np.asarray(units, np.float64) * PIX_UNIT).astype(F32)
    assert np.all(np.asarray(units) * PIX_UNIT < 2.0 ** 13)
    mean = s / F32(E) if (mean_by or MEAN_BY) == "div" else s * (F32(1.0) / F32(E))
    mean = _rnd(mean.astype(F32), bf16)
    v = _rnd((mean * F32(255.0)).astype(F32), bf16)
    return v > _rnd(np.array(thr, F32), bf16)


def pixdiff_boundary(E, thr, bf16, mean_by=None, limit=None):
    """scan the chain: the smallest unit count that is kept (the chain is monotone in the sum)"""
    limit = limit or min(128 * E, (1 << 20) - 1)
    keep = pixdiff_chain(np.arange(limit + 1), E, thr, bf16, mean_by)
    assert keep[-1] and np.all(np.diff(keep.astype(np.int8)) >= 0), "the chain is not monotone up to the limit"
    return int(np.argmax(keep))


def pixdiff_mask(pix_units, t, P, E, thr, min_tokens, minor, bf16, mean_by=None):
    """pix_units: integer pixel values in units of 2^-7, [t * P, E] -> uint8 keep-mask [t * P]
    (frame 0 whole; frames below min_tokens get their first min_tokens; a minor frame keeps token 0 only)"""
    p = np.asarray(pix_units, np.int64).reshape(t, P, E)
    m = np.ones((t, P), bool)
    if t > 1:
        sums = np.abs(p[1:] - p[:-1]).sum(axis=2)
        m[1:] = pixdiff_chain(sums, E, thr, bf16, mean_by)
    short = m.sum(axis=1) < min_tokens
    m[short, :min_tokens] = True
    if minor is not None:
        for f in np.flatnonzero(np.asarray(minor)):
            m[f, 0] = True
            m[f, 1:] = False
    return m.reshape(-1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ small helpers
def frame_mean64(feats, P, frames):
    """-> {frame: fp64 column mean of its P rows}"""
    f = np.asarray(feats, np.float64)
    return {int(fr): f[fr * P:(fr + 1) * P].mean(axis=0) for fr in frames}


def gather_rows(ta, tb, idx):
    return np.stack([ta[i] if i >= 0 else tb[-i - 1] for i in np.asarray(idx).tolist()])


def mean_rows64(x):
    return np.asarray(x, np.float64).mean(axis=0)


def seq_sum32(x, axis=0):
    """sequential fp32 sum along an axis: the plain implementation the sums are measured against"""
    x = np.moveaxis(np.asarray(x, F32), axis, 0)
    acc = np.zeros(x.shape[1:], F32)
    for row in x:
        acc = (acc + row).astype(F32)
    return acc


def cosine64(a, b):
    """a . b_i / max(|a| |b_i|, 1e-8), the contract of csrc/compress.hip"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (b @ a) / np.maximum(np.sqrt(a @ a) * np.sqrt((b * b).sum(axis=1)), 1e-8)


def pack_rows(x, cols_out, out_bf16):
    """x [rows, cols_in] fp32 values (bf16 inputs as their fp32 values) -> [rows, cols_out] fp32 values of the output:
    round_bf16 or exact, +0.0 in the padding columns"""
    x = np.asarray(x, F32)
    out = np.zeros((x.shape[0], cols_out), F32)
    out[:, :x.shape[1]] = round_bf16(x) if out_bf16 else x
    return out


# ------------------------------------------------------------------------------------------------ k-means
SL = 512


def sqdist64(x, c):
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return np.stack([((x - ck) ** 2).sum(axis=1) for ck in c], axis=1)


def sqdist_scheme32(x, c):
    """the documented scheme in its plain form: sequential fp32 within a 512-column slice, fp64 across slices, fp32 result"""
    x, c = np.asarray(x, F32), np.asarray(c, F32)
    T, PD = x.shape
    tot = np.zeros((T, c.shape[0]), np.float64)
    for j0 in range(0, PD, SL):
        acc = np.zeros((T, c.shape[0]), F32)
        for j in range(j0, min(PD, j0 + SL)):
            d = (x[:, j, None] - c[None, :, j]).astype(F32)
            acc = (acc + (d * d).astype(F32)).astype(F32)
        tot += acc
    return tot.astype(F32)


def assign_fp32(dist2, ts, cts, alpha):
    """kmeans_with_time.py:76-104 in torch's fp32 operations one by one -> (assign int64 [T], final [T, K] fp32).
    sqrt, |.|, per-row min / max, (d - min) / (max - min) or 0, sqrt(nf nf + alpha (nt nt)), first minimum; a row whose
    final distances are all NaN takes cluster 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        d2 = np.asarray(dist2, F32)
        df = np.sqrt(d2).astype(F32)
        dt = np.abs((np.asarray(ts, F32)[:, None] - np.asarray(cts, F32)[None, :]).astype(F32))

        def norm(d):
            lo, hi = np.fmin.reduce(d, axis=1)[:, None], np.fmax.reduce(d, axis=1)[:, None]
            n = ((d - lo).astype(F32) / (hi - lo).astype(F32)).astype(F32)
            return np.where(hi > lo, n, F32(0)).astype(F32)
        nf, nt = norm(df), norm(dt)
        fin = np.sqrt(((nf * nf).astype(F32) + (F32(alpha) * (nt * nt).astype(F32)).astype(F32)).astype(F32)).astype(F32)
    out = np.zeros(fin.shape[0], np.int64)
    for t, row in enumerate(fin):
        best, bk = np.inf, 0
        for k, v in enumerate(row.tolist()):
            if v < best:
                best, bk = v, k
        out[t] = bk
    return out, fin


def margin64(dist2, ts, cts, alpha, t):
    """the decision margin of row t as cogs_kmeans_margins defines it (csrc/kmeans.hip, reduce_assign_kernel): 2 e*, e* the
    relative change of the feature distances that closes the gap between the winner and the runner-up"""
    a, fin = assign_fp32(dist2, ts, cts, alpha)
    df = np.sqrt(np.asarray(dist2, np.float64)[t])
    f = fin[t].astype(np.float64)
    k1 = int(a[t])
    k2 = int(np.argmin(np.where(np.arange(f.size) == k1, np.inf, f)))
    R = df.max() - df.min()
    if R <= 0:
        return float("inf")
    nf = (df - df.min()) / R
    s = [(nf[k] / f[k] if f[k] > 0 else 1.0) * df[k] / R for k in (k1, k2)]
    return max(0.0, 2.0 * (f[k2] - f[k1]) / (s[0] + s[1])) if s[0] + s[1] > 0 else float("inf")


def update_ref(x, ts, assign, K, reseed, old_c, old_ct, drop=None):
    """-> (centres fp32 [K, PD], centre times fp32 [K], shift fp64). Centres: fp32 sum over the members in ascending order,
    divided by fp32(n) (exact sums: one correctly rounded division); an empty cluster takes row reseed[k]. Centre times:
    sequential fp32 sum in ascending member order / fp32(n). Shift: sum_k |new_k - old_k|_2 + |new times - old times|_2 in
    fp64 on those fp32 values. drop=(k, i) leaves member i of cluster k out of the mean (the CPU file's planted error)."""
    x, ts = np.asarray(x, F32), np.asarray(ts, F32)
    c = np.zeros((K, x.shape[1]), F32)
    ct = np.zeros(K, F32)
    for k in range(K):
        m = np.flatnonzero(np.asarray(assign) == k)
        if drop is not None and drop[0] == k:
            m = np.delete(m, drop[1])
        if m.size == 0:
            c[k], ct[k] = x[reseed[k]], ts[reseed[k]]
            continue
        c[k] = (seq_sum32(x[m]) / F32(m.size)).astype(F32)
        ct[k] = F32(seq_sum32(ts[m]) / F32(m.size))
    d = c.astype(np.float64) - np.asarray(old_c, np.float64)
    dt = ct.astype(np.float64) - np.asarray(old_ct, np.float64)
    return c, ct, float(np.sqrt((d * d).sum(axis=1)).sum() + np.sqrt((dt * dt).sum()))


def kpp_select(nearest2, q):
    """one k-means++ draw from the folded distances -> (row, zero_sum, relative gap between the best and the second-best
    DISTINCT ratio, rows that hold the best ratio). probs = fp32(sqrt(n2))^2, total = fp32 of their fp64 sum,
    ratio = fp32(fp32(p / total) / q), first maximum"""
    n2 = np.asarray(nearest2, F32)
    d = np.sqrt(n2).astype(F32)
    p = (d * d).astype(F32)
    total = F32(p.astype(np.float64).sum())
    if total == 0:
        return 0, True, float("inf"), []
    with np.errstate(divide="ignore"):
        r = ((p / total).astype(F32) / np.asarray(q, F32)).astype(F32)
    best = int(np.argmax(r))
    top = r[best]
    rest = r[r < top]
    gap = float((top - rest.max()) / top) if rest.size and top > 0 else float("inf")
    return best, False, gap, np.flatnonzero(r == top).tolist()
