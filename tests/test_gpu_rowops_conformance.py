"""The row kernels between the ViT and the LLM against the numpy references of tests/rowops_reference.py, on the cells of
tests/rowops_cells.py (held to their promises on the CPU by tests/test_rowops_reference.py): cogs_layernorm, cogs_rmsnorm,
cogs_ln_merge, cogs_ln_finalize (csrc/norm.hip); cogs_pixdiff_mask, cogs_frame_mean_to_slot0, cogs_gather_rows,
cogs_mean_rows, cogs_cosine (csrc/compress.hip); cogs_pack_rows (csrc/vision_misc.hip); cogs_kmeans_sqdist, cogs_kmeans_assign,
cogs_kmeans_lloyd(max_iter = 1), cogs_kmeans_margins, cogs_kmeans_update, cogs_kmeans_pp (csrc/kmeans.hip).

Conventions. Every call goes through ctypes and the test owns every buffer: each input, output and workspace sits inside a
tracer-filled allocation with GUARD tracer elements before and after (floating-point tracers are NaN patterns, so a read
outside the payload poisons the result; the gap columns of a strided input are tracer too). Every cell asserts the status,
that all guards kept their bits and that the inputs are unchanged, and records its (kernel, path) pairs in REACHED;
test_zz_required_coverage asserts the list. Exact cells demand bit equality; numeric cells print the kernel's worst
elementwise error, the plain fp32 implementation's worst and their ratio (at most 4), bf16 outputs must be the bf16 nearest to
the fp64 reference (tests/rowops_reference.py states the rules).

Measured on an MI355X (worst cell per kernel and dtype: the kernel's worst elementwise error, the plain fp32 implementation's
worst on the same cell, their ratio; the bound is 4):
    cogs_layernorm                     f32    1.233e-07  9.079e-08   1.358   H3584 rows3
    cogs_rmsnorm                       f32    1.622e-07  1.176e-07   1.379   H2048 rows1
    cogs_ln_merge                      f32    6.704e-08  3.684e-08   1.820   H8 group1 out1
    cogs_frame_mean_to_slot0           f32    3.497e-07  1.372e-07   2.549   D252 P64
    cogs_mean_rows                     f32    1.138e-07  3.471e-08   3.279   D4 rows9
    cogs_mean_rows                     bf16   9.950e-08  5.061e-08   1.966   D128 rows7 ldx D+4
    cogs_cosine                        f32    6.273e-08  2.980e-08   2.105   D64 n1 (the yardstick is the 2^-25 floor)
    cogs_kmeans_sqdist                 f32    8.867e-08  4.218e-07   0.210   T40 PD2568 K5
    cogs_kmeans_sqdist                 bf16   8.475e-08  5.167e-07   0.164   T40 PD2568 K5
    cogs_kmeans_update shift           f32    8.643e-08  2.980e-08   2.900   T1025 PD2056 K9 (floor)
    cogs_kmeans_update shift           bf16   5.964e-08  5.964e-08   1.000   T16385 PD8 K3
    cogs_ln_finalize: worst 1.38 fp32 ulps (bound 2). bf16 norm cells: every output inside its window, at most 0.154 % of a
    cell excepted (cap 1 %). cogs_kmeans_margins: device minimum 3.999e-04, 1 row below 1e-3; reference 4.000e-04, 1 row.
Two kernels were wrong before this file and are fixed with it. ln_finalize_kernel multiplied the fp64 sums by an fp32 1 / H:
63 (H 1152) and 348 (H 3584) ulps of rstd at mean / std = 30; it divides by H in fp64 now. pixdiff_kernel divided the row sum
by E where torch's mean on the device multiplies by fp32(1 / E): on the planted sums where the two differ by an ulp (E 520,
129 units, fp32: kernel 0, torch on the device 1; E 504, 16695 units, bf16: kernel 0, torch 1) the masks differed; the kernel
and the numpy chain (MEAN_BY) multiply now and agree with torch on the device on every row of every cell.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import rowops_cells as S
import rowops_reference as R

pytestmark = pytest.mark.gpu

GUARD = 64
F32 = np.float32
_ST = S.status_codes()
OK, E_INVALID, E_UNSUPPORTED, E_WORKSPACE = _ST["OK"], _ST["E_INVALID"], _ST["E_UNSUPPORTED"], _ST["E_WORKSPACE"]
DT = {"bf16": 0, "f32": 1}
ITEM = {"f32": (torch.int32, np.int32, 0x7FC5A5A5), "bf16": (torch.int16, np.int16, 0x7FC5), "u8": (torch.uint8, np.uint8, 0x5A),
        "i32": (torch.int32, np.int32, 0x5A5A5A5A), "i64": (torch.int64, np.int64, 0x5A5A5A5A5A5A5A5A)}

REACHED = set()
TABLE = {}            # (kernel, dtype) -> [worst kernel error, yardstick at that cell, worst ratio]


def _L():
    from cogstream_amd import _lib
    return _lib


def _bits(data, kind):
    """numpy values -> the raw integer patterns a buffer of this kind holds"""
    if kind == "f32":
        return np.ascontiguousarray(data, F32).view(np.int32)
    if kind == "bf16":
        return R.bf16_bits(data).view(np.int16)
    return np.ascontiguousarray(data, ITEM[kind][1])


class Buf:
    """n elements with GUARD tracer elements before and after; the payload is tracer until data is given"""

    def __init__(self, dev, n, kind, data=None):
        tdt, _, tracer = ITEM[kind]
        self.n, self.kind = int(n), kind
        self.buf = torch.full((self.n + 2 * GUARD,), tracer, dtype=tdt, device=dev)
        if data is not None:
            bits = _bits(data, kind).reshape(-1)
            assert bits.size == self.n, (bits.size, self.n)
            if self.n:
                self.buf[GUARD:GUARD + self.n].copy_(torch.from_numpy(bits.copy()))
        self.before = self.buf.cpu().numpy().copy()

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def bits(self):
        return self.buf.cpu().numpy()[GUARD:GUARD + self.n]

    def vals(self):
        b = self.bits()
        if self.kind == "f32":
            return b.view(F32)
        if self.kind == "bf16":
            return R.from_bf16_bits(b.view(np.uint16))
        return b

    def guards_intact(self):
        now = self.buf.cpu().numpy()
        return now[:GUARD].tobytes() == self.before[:GUARD].tobytes() and now[GUARD + self.n:].tobytes() == self.before[GUARD + self.n:].tobytes()

    def untouched(self):
        return self.buf.cpu().numpy().tobytes() == self.before.tobytes()

    def freeze(self):
        """what the buffer holds now is what untouched() compares with from here on (an output that becomes an input)"""
        self.before = self.buf.cpu().numpy().copy()
        return self


def strided(dev, x, ld, kind):
    """x [rows, cols] inside rows of length ld; the gap columns hold the tracer"""
    rows, cols = x.shape
    full = np.full((rows, ld), ITEM[kind][2], ITEM[kind][1])
    full[:, :cols] = _bits(x, kind).reshape(rows, cols)
    b = Buf(dev, rows * ld, kind)
    if rows:
        b.buf[GUARD:GUARD + rows * ld].copy_(torch.from_numpy(full.reshape(-1)))
    return b.freeze()


def call(fn, *args):
    L = _L()
    st = getattr(L.lib, fn)(L.current_stream(), *args)
    torch.cuda.synchronize()
    return st


def clean(label, inputs=(), outputs=()):
    for b in inputs:
        assert b is None or b.untouched(), f"{label}: an input changed"
    for b in outputs:
        assert b.guards_intact(), f"{label}: a write outside an output"


def reach(c, *extra):
    for p in c.paths + tuple(extra):
        REACHED.add((c.kernel, p))


def yard(c, got, plain, ref, unit, what=""):
    k, y, r = R.yardstick_ratio(got, plain, ref, unit)
    print(f"{c.id}{what}: kernel worst {k:.3e}, yardstick worst {y:.3e}, ratio {r:.3f}")
    row = TABLE.setdefault((c.kernel + what, c.dtype), [0.0, 0.0, 0.0])
    if r >= row[2]:
        row[:] = [k, y, r]
    assert r <= R.FACTOR, f"{c.id}{what}: kernel worst {k:.3e} is {r:.2f} times the plain fp32 implementation's {y:.3e}"


def ids(cells):
    return [c.id for c in cells]


# ------------------------------------------------------------------------------------------------ norms
NORM = S.norm_cells()


def _run_norm(dev, c, x, gamma, beta, rows=None, H=None):
    kind = c.dtype
    bx, bg, bb = Buf(dev, x.size, kind, x), Buf(dev, gamma.size, kind, gamma), Buf(dev, beta.size, kind, beta)
    H = x.shape[1] if H is None else H
    if c.kernel == "cogs_ln_merge":
        out_rows = c.p["out_rows"] if rows is None else rows
        by = Buf(dev, max(out_rows, 1) * x.shape[1], kind)
        st = call("cogs_ln_merge", DT[kind], bx.ptr, by.ptr, bg.ptr, bb.ptr, out_rows, c.p["group"], H, S.EPS)
    elif c.kernel == "cogs_rmsnorm":
        n = x.shape[0] if rows is None else rows
        by = Buf(dev, x.size, kind)
        st = call("cogs_rmsnorm", DT[kind], bx.ptr, by.ptr, bg.ptr, n, H, S.EPS)
    else:
        n = x.shape[0] if rows is None else rows
        by = Buf(dev, x.size, kind)
        st = call("cogs_layernorm", DT[kind], bx.ptr, by.ptr, bg.ptr, bb.ptr, n, H, S.EPS)
    clean(c.id, (bx, bg, bb), (by,))
    return st, by


@pytest.mark.parametrize("ci", range(len(NORM)), ids=ids(NORM))
def test_norm_cell(dev, ci):
    """LayerNorm, RMSNorm and LayerNorm + group mean: fp32 against the yardstick in units of |gamma xhat| + |beta|; bf16 must be the
    nearest bf16 (RMSNorm: Qwen2's two roundings; ln_merge: every normalised row rounded before the average)"""
    c = NORM[ci]
    x, gamma, beta = S.build_norm(c)
    st, by = _run_norm(dev, c, x, gamma, beta)
    assert st == OK, (c.id, st)
    ref, unit = S.norm_reference(c, x, gamma, beta)
    got = by.vals().reshape(ref.shape)
    if not c.bf16:
        yard(c, got, S.norm_plain(c, x, gamma, beta), ref, unit)
    else:
        delta = S.norm_delta(c, x, gamma, beta)
        if c.kernel == "cogs_layernorm":
            bad, share = R.check_nearest_bf16(got, ref, delta * unit)
        elif c.kernel == "cogs_rmsnorm":
            bad, share = R.check_rmsnorm_bf16(got, x, gamma, S.EPS, delta)
        else:
            bad, share = R.check_ln_merge_bf16(got, x, gamma, beta, c.p["group"], S.EPS, delta)
        print(f"{c.id}: delta {delta:.3e} of the unit, excepted share {share:.5f}")
        assert not bad, (c.id, bad)
    reach(c)


@pytest.mark.parametrize("kernel", ["cogs_layernorm", "cogs_rmsnorm", "cogs_ln_merge"])
@pytest.mark.parametrize("dtype", S.DTYPES)
def test_norm_status(dev, kernel, dtype):
    """H % 8 != 0 is invalid, H = 4104 (cpl 9) unsupported, rows = 0 fine; no output byte changes in any of them"""
    c = S.Cell(kernel, "status", dict(H=4104, rows=2, group=2, out_rows=1), (), 1, dtype)
    x, gamma, beta = S.build_norm(c)
    for H, rows, want, label in ((12, None, E_INVALID, "H % 8 != 0"), (4104, None, E_UNSUPPORTED, "H > 4096"), (4104, 0, OK, "rows = 0")):
        st, by = _run_norm(dev, c, x, gamma, beta, rows=rows, H=H)
        assert st == want, (kernel, label, st)
        assert by.untouched(), (kernel, label, "the output changed")
        REACHED.add((kernel, "status " + label))


FIN = S.finalize_cells()


@pytest.mark.parametrize("ci", range(len(FIN)), ids=ids(FIN))
def test_ln_finalize_cell(dev, ci):
    """(rstd, -rstd mean) from the given partial sums against the same formula in fp64: 2 fp32 ulps per output"""
    c = FIN[ci]
    part = S.build_finalize(c)
    bp, bo = Buf(dev, part.size, "f32", part), Buf(dev, 2 * c.p["rows"], "f32")
    st = call("cogs_ln_finalize", bp.ptr, c.p["rows"], c.p["H"], S.EPS, bo.ptr)
    assert st == OK
    clean(c.id, (bp,), (bo,))
    ref = R.ln_finalize64(part, c.p["H"], S.EPS)
    got = bo.vals().reshape(ref.shape)
    ratio = np.arange(c.p["rows"]) % 3
    for r, name in enumerate(S.FIN_RATIOS):
        if np.any(ratio == r):
            print(f"{c.id}: mean / std {name}: worst {R.ulps32(got[ratio == r], ref[ratio == r]):.2f} ulps")
    worst = R.ulps32(got, ref)
    row = TABLE.setdefault(("cogs_ln_finalize (ulps)", "f32"), [0.0, 2.0, 0.0])
    row[0], row[2] = max(row[0], worst), max(row[0], worst) / 2.0
    assert worst <= 2.0, f"{c.id}: {worst:.2f} ulps"
    reach(c)


def test_ln_finalize_status(dev):
    part = S.build_finalize(FIN[0])
    bp, bo = Buf(dev, 2 * 2 * 4, "f32", np.resize(part, 16)), Buf(dev, 8, "f32")
    assert call("cogs_ln_finalize", bp.ptr, 4, 100, S.EPS, bo.ptr) == E_INVALID and bo.untouched()
    REACHED.add(("cogs_ln_finalize", "status H % 64 != 0"))


# ------------------------------------------------------------------------------------------------ keep-mask
PIX = S.pix_cells()


def _device_expression(dev, c, pix, minor):
    """_get_compression_mask as oracle/compress.py states it, by torch on the same device in the same dtype"""
    from oracle.compress import compression_mask
    t, P, E = c.p["t"], c.p["P"], c.p["E"]
    pt = torch.from_numpy((pix * R.PIX_UNIT).astype(F32)).to(dev).to(torch.bfloat16 if c.bf16 else torch.float32)
    m = compression_mask(pt, torch.tensor([[t, P, 1]]), torch.tensor([1]), ["video"], threshold=c.p["thr"], min_tokens=c.p["min_tokens"],
                         minor_frame_indices=np.flatnonzero(minor).tolist() if minor is not None else None)
    return m.cpu().numpy().astype(np.uint8)


@pytest.mark.parametrize("ci", range(len(PIX)), ids=ids(PIX))
def test_pixdiff_mask_cell(dev, ci):
    """exact data (multiples of 2^-7, row sums exact in fp32): the mask equals the numpy chain and the project's own expression run
    by torch on the device, on every element; the planted rows sit one step either side of the threshold"""
    c = PIX[ci]
    pix, minor, planted = S.build_pix(c)
    t, P, E = c.p["t"], c.p["P"], c.p["E"]
    bp = Buf(dev, pix.size, c.dtype, (pix * R.PIX_UNIT).astype(F32))
    bm = Buf(dev, t * P, "u8")
    bn = Buf(dev, t, "u8", minor) if minor is not None else None
    st = call("cogs_pixdiff_mask", DT[c.dtype], bp.ptr, t, P, E, c.p["thr"], c.p["min_tokens"], bn.ptr if bn else None, bm.ptr)
    assert st == OK
    clean(c.id, (bp, bn), (bm,))
    got = bm.bits()
    ref = R.pixdiff_mask(pix, t, P, E, c.p["thr"], c.p["min_tokens"], minor, c.bf16)
    raw = R.pixdiff_mask(pix, t, P, E, c.p["thr"], 0, None, c.bf16)
    other = R.pixdiff_mask(pix, t, P, E, c.p["thr"], 0, None, c.bf16, mean_by="mul" if R.MEAN_BY == "div" else "div")
    dev_mask = _device_expression(dev, c, pix, minor)
    for row, units in planted.items():
        print(f"{c.id}: planted row {row} sum {units} units: kernel {got[row]} chain {ref[row]} (before the fixes {raw[row]}, other mean form "
              f"{other[row]}) torch on the device {dev_mask[row]}")
    d1, d2 = R.mismatch(got, dev_mask).ravel(), R.mismatch(got, ref).ravel()
    assert d1.size == 0, f"{c.id}: kernel and torch on the device differ on rows {d1[:10].tolist()} (planted {sorted(planted)})"
    assert d2.size == 0, f"{c.id}: kernel and the numpy chain differ on rows {d2[:10].tolist()} (planted {sorted(planted)})"
    reach(c)


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_pixdiff_mask_status(dev, dtype):
    bp, bm = Buf(dev, 2 * 16, dtype, np.zeros(32, F32)), Buf(dev, 2, "u8")
    assert call("cogs_pixdiff_mask", DT[dtype], bp.ptr, 2, 1, 12, 0.1, 1, None, bm.ptr) == E_INVALID and bm.untouched()
    assert call("cogs_pixdiff_mask", DT[dtype], bp.ptr, 0, 1, 16, 0.1, 1, None, bm.ptr) == OK and bm.untouched()
    REACHED.add(("cogs_pixdiff_mask", "status E % 8 != 0")), REACHED.add(("cogs_pixdiff_mask", "status t = 0"))


# ------------------------------------------------------------------------------------------------ frame mean
FMEAN = S.fmean_cells()


@pytest.mark.parametrize("ci", range(len(FMEAN)), ids=ids(FMEAN))
def test_frame_mean_cell(dev, ci):
    """token 0 of every listed frame <- the column mean of its P tokens; every other row keeps its bits"""
    c = FMEAN[ci]
    x = S.build_fmean(c)
    P, D, frames = c.p["P"], c.p["D"], c.p["frames"]
    bx = Buf(dev, x.size, c.dtype, x)
    bf = Buf(dev, len(frames), "i32", np.array(frames, np.int32))
    st = call("cogs_frame_mean_to_slot0", DT[c.dtype], bx.ptr, P, D, bf.ptr, len(frames))
    assert st == OK
    clean(c.id, (bf,), (bx,))
    slot = np.zeros(x.shape[0], bool)
    slot[[f * P for f in frames]] = True
    before = bx.before[GUARD:GUARD + x.size].reshape(x.shape)
    now = bx.bits().reshape(x.shape)
    assert np.array_equal(now[~slot], before[~slot]), f"{c.id}: a row outside the listed slots changed"
    got = bx.vals().reshape(x.shape)
    for f, mean in R.frame_mean64(x, P, frames).items():
        g = got[f * P]
        if c.p["exact"]:
            assert _bits(mean.astype(F32), c.dtype).tobytes() == now[f * P].tobytes(), f"{c.id}: frame {f} is not the exact mean"
        elif c.bf16:
            bad, share = R.check_nearest_bf16(g, mean, 2.0 * np.spacing(np.abs(mean).astype(F32)).astype(np.float64))
            assert not bad, (c.id, f, bad)
        else:
            yard(c, g, S.means_plain(x[f * P:(f + 1) * P]), mean, np.abs(x[f * P:(f + 1) * P]).astype(np.float64).mean(axis=0))
    reach(c)


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_frame_mean_status(dev, dtype):
    bx, bf = Buf(dev, 4 * 6, dtype, np.ones(24, F32)), Buf(dev, 1, "i32", np.array([1], np.int32))
    assert call("cogs_frame_mean_to_slot0", DT[dtype], bx.ptr, 2, 6, bf.ptr, 1) == E_INVALID and bx.untouched()
    REACHED.add(("cogs_frame_mean_to_slot0", "status D % 4 != 0"))


# ------------------------------------------------------------------------------------------------ gather
GATHER = S.gather_cells()


@pytest.mark.parametrize("ci", range(len(GATHER)), ids=ids(GATHER))
def test_gather_rows_cell(dev, ci):
    c = GATHER[ci]
    ta, tb, idx = S.build_gather(c)
    D, rows = c.p["D"], c.p["rows"]
    ba, bi, bo = Buf(dev, ta.size, c.dtype, ta), Buf(dev, rows, "i64", idx), Buf(dev, rows * D, c.dtype)
    bb = None if c.p["null_b"] else Buf(dev, tb.size, c.dtype, tb)
    st = call("cogs_gather_rows", DT[c.dtype], ba.ptr, bb.ptr if bb else None, bi.ptr, bo.ptr, rows, D)
    assert st == OK
    clean(c.id, (ba, bb, bi), (bo,))
    assert rows < 4 or {0, S.GATHER_A - 1} <= set(idx.tolist()) and (c.p["null_b"] or {-1, -S.GATHER_B} <= set(idx.tolist()))
    assert idx.min() >= (0 if c.p["null_b"] else -S.GATHER_B) and idx.max() < S.GATHER_A
    assert bo.bits().tobytes() == _bits(R.gather_rows(ta, tb, idx), c.dtype).tobytes(), f"{c.id}: the gathered rows differ"
    reach(c)


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_gather_rows_status(dev, dtype):
    ba, bi, bo = Buf(dev, 24, dtype, np.ones(24, F32)), Buf(dev, 1, "i64", np.array([1], np.int64)), Buf(dev, 12, dtype)
    assert call("cogs_gather_rows", DT[dtype], ba.ptr, None, bi.ptr, bo.ptr, 1, 12) == E_INVALID and bo.untouched()
    REACHED.add(("cogs_gather_rows", "status D % 8 != 0"))


# ------------------------------------------------------------------------------------------------ column means
MEANROWS = S.meanrows_cells()


@pytest.mark.parametrize("ci", range(len(MEANROWS)), ids=ids(MEANROWS))
def test_mean_rows_cell(dev, ci):
    c = MEANROWS[ci]
    x = S.build_meanrows(c)
    rows, D, ld = c.p["rows"], c.p["D"], c.p["D"] + c.p["pad"]
    bx, bo = strided(dev, x, ld, c.dtype), Buf(dev, D, "f32")
    st = call("cogs_mean_rows", DT[c.dtype], bx.ptr, ld, rows, D, bo.ptr)
    assert st == OK
    clean(c.id, (bx,), (bo,))
    ref = R.mean_rows64(x)
    if c.p["exact"]:
        assert bo.bits().tobytes() == _bits(ref.astype(F32), "f32").tobytes(), f"{c.id}: not the exact mean"
    else:
        yard(c, bo.vals(), S.means_plain(x), ref, np.abs(x).astype(np.float64).mean(axis=0))
    reach(c)


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_mean_rows_status(dev, dtype):
    bx, bo = Buf(dev, 24, dtype, np.ones(24, F32)), Buf(dev, 8, "f32")
    assert call("cogs_mean_rows", DT[dtype], bx.ptr, 6, 4, 6, bo.ptr) == E_INVALID and bo.untouched()
    assert call("cogs_mean_rows", DT[dtype], bx.ptr, 8, 0, 8, bo.ptr) == E_INVALID and bo.untouched()
    REACHED.add(("cogs_mean_rows", "status D % 4 != 0")), REACHED.add(("cogs_mean_rows", "status rows = 0"))


# ------------------------------------------------------------------------------------------------ cosine
COSINE = S.cosine_cells()


@pytest.mark.parametrize("ci", range(len(COSINE)), ids=ids(COSINE))
def test_cosine_cell(dev, ci):
    """a . b_i / max(|a| |b_i|, 1e-8): absolute error against the yardstick; a zero vector gives exactly 0"""
    c = COSINE[ci]
    a, b = S.build_cosine(c)
    ba, bb, bo = Buf(dev, a.size, "f32", a), Buf(dev, b.size, "f32", b), Buf(dev, c.p["n"], "f32")
    st = call("cogs_cosine", ba.ptr, bb.ptr, c.p["n"], c.p["D"], bo.ptr)
    assert st == OK
    clean(c.id, (ba, bb), (bo,))
    got, ref = bo.vals(), R.cosine64(a, b)
    zero = ref == 0
    assert np.all(np.isfinite(got)) and np.all(got[zero] == 0), f"{c.id}: a zero vector must give 0, got {got[zero]}"
    if c.p["zero"] == "a":
        assert np.all(zero)
    elif c.p["zero"] == "b":
        assert zero[3 % c.p["n"]]
    if np.any(~zero):
        yard(c, got[~zero], S.cosine_plain(a, b)[~zero], ref[~zero], 1.0)
    reach(c)


# ------------------------------------------------------------------------------------------------ pack_rows
PACK = S.pack_cells()


@pytest.mark.parametrize("ci", range(len(PACK)), ids=ids(PACK))
def test_pack_rows_cell(dev, ci):
    """converted values are round_bf16 or the exact widening bit for bit, the padding columns +0.0; the output was NaN tracer"""
    c = PACK[ci]
    x = S.build_pack(c)
    rows, ci_, co = c.p["rows"], c.p["cols_in"], c.p["cols_out"]
    ld_in, ld_out = (ci_ + 3) // 4 * 4 + c.p["pad_in"], co + c.p["pad_out"]
    bx, bo = strided(dev, x, ld_in, c.p["din"]), Buf(dev, rows * ld_out, c.p["dout"])
    st = call("cogs_pack_rows", DT[c.p["din"]], DT[c.p["dout"]], bx.ptr, ld_in, bo.ptr, ld_out, rows, ci_, co)
    assert st == OK
    clean(c.id, (bx,), (bo,))
    got = bo.bits().reshape(rows, ld_out)
    want = _bits(R.pack_rows(x, co, c.p["dout"] == "bf16"), c.p["dout"]).reshape(rows, co)
    assert np.all(want[:, ci_:] == 0)
    bad = R.mismatch(got[:, :co], want)
    assert bad.size == 0, f"{c.id}: {len(bad)} elements differ, first (row, column) {bad[:5].tolist()}"
    assert np.all(got[:, co:] == ITEM[c.p["dout"]][2]), f"{c.id}: the gap behind cols_out was written"
    reach(c)


def test_pack_rows_status(dev):
    bx, bo = Buf(dev, 64, "f32", np.ones(64, F32)), Buf(dev, 64, "bf16")
    for label, args in (("cols_out % 4 != 0", (1, 0, 8, 8, 2, 5, 6)), ("cols_in > cols_out", (1, 0, 12, 8, 2, 12, 8)),
                        ("ld_in % 4 != 0", (1, 0, 6, 8, 2, 5, 8)), ("ld_out % 4 != 0", (1, 0, 8, 10, 2, 5, 8)),
                        ("unknown dtype", (7, 0, 8, 8, 2, 5, 8))):
        di, do, ld_in, ld_out, rows, ci_, co = args
        assert call("cogs_pack_rows", di, do, bx.ptr, ld_in, bo.ptr, ld_out, rows, ci_, co) == E_INVALID, label
        assert bo.untouched(), label
        REACHED.add(("cogs_pack_rows", "status " + label))


# ------------------------------------------------------------------------------------------------ k-means
def _ws(dev, T, PD, K, short=0):
    n = C.c_size_t()
    assert _L().lib.cogs_kmeans_workspace_bytes(T, PD, K, C.byref(n)) == OK
    return Buf(dev, n.value - short, "u8")


def _sqdist(dev, dtype, bx, T, PD, K, centres=None, rows=None, ws=None):
    ws = ws or _ws(dev, T, PD, K)
    bc = Buf(dev, centres.size, "f32", centres) if centres is not None else None
    br = Buf(dev, rows.size, "i32", rows) if rows is not None else None
    bd = Buf(dev, T * K, "f32")
    st = call("cogs_kmeans_sqdist", DT[dtype], bx.ptr, T, PD, bc.ptr if bc else None, br.ptr if br else None, K, bd.ptr, ws.ptr, ws.n)
    clean("sqdist", (bx, bc, br), (bd, ws))
    return st, bd


SQDIST = S.sqdist_cells()


@pytest.mark.parametrize("ci", range(len(SQDIST)), ids=ids(SQDIST))
def test_kmeans_sqdist_cell(dev, ci):
    """exact cells: integer features, every distance an integer below 2^24, bit equality, a row's distance to itself 0.
    numeric cells: relative error against the documented scheme in its plain form. Every cell at the automatic row-group count
    and at km_row_groups 1, 2, 3: bit-equal, the sums within a row do not depend on the grouping"""
    c = SQDIST[ci]
    L = _L()
    x, cen, rows = S.build_sqdist(c)
    T, PD, K = c.p["T"], c.p["PD"], c.p["K"]
    bx = Buf(dev, x.size, c.dtype, x)
    ws = _ws(dev, T, PD, K)
    kw = dict(rows=rows) if rows is not None else dict(centres=cen)
    st, bd = _sqdist(dev, c.dtype, bx, T, PD, K, ws=ws, **kw)
    assert st == OK
    auto = bd.bits().copy()
    for g in (1, 2, 3):
        with L.debug_switch("km_row_groups", g):
            st, bg = _sqdist(dev, c.dtype, bx, T, PD, K, ws=ws, **kw)
        assert st == OK and bg.bits().tobytes() == auto.tobytes(), f"{c.id}: km_row_groups {g} differs from the automatic grouping"
    got = bd.vals().reshape(T, K)
    ref = R.sqdist64(x, cen)
    if c.p["exact"]:
        assert float(ref.max()) < 2 ** 24
        bad = np.argwhere(got != ref.astype(F32))
        assert bad.size == 0, f"{c.id}: {len(bad)} distances differ, first (row, centre) {bad[:5].tolist()}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"
        if rows is not None:
            assert np.all(got[rows, np.arange(K)] == 0)
    else:
        yard(c, got, R.sqdist_scheme32(x, cen), ref, ref)
    reach(c)


def test_kmeans_sqdist_status(dev):
    T, K = 4, 3
    x = np.ones((T, 16), F32)
    bx = Buf(dev, x.size, "f32", x)
    rows = np.array([0, 1, 2], np.int32)
    st, bd = _sqdist(dev, "f32", bx, T, 12, K, rows=rows)
    assert st == E_INVALID and bd.untouched()
    # a shape whose stated need is a multiple of the 256-byte round-up, so that one byte less is less than the need
    T, PD, K = S.tight_ws_shape()
    rows = (np.arange(K) % T).astype(np.int32)
    xx = np.ones((T, PD), F32)
    bxx = Buf(dev, xx.size, "f32", xx)
    full = _ws(dev, T, PD, K)
    assert full.n == S.kmeans_ws_bytes(T, PD, K)
    st, bd = _sqdist(dev, "f32", bxx, T, PD, K, rows=rows, ws=_ws(dev, T, PD, K, short=1))
    assert st == E_WORKSPACE and bd.untouched()
    st, bd = _sqdist(dev, "f32", bxx, T, PD, K, ws=full)
    assert st == E_INVALID and bd.untouched() and full.untouched()
    for label in ("PD % 8 != 0", "workspace one byte short", "both centre sources null"):
        REACHED.add(("cogs_kmeans_sqdist", "status " + label))


ASSIGN = S.assign_cells()


def _lloyd_once(dev, c, bx, bts, cen, cts, alpha):
    T, K, PD = c.p["T"], c.p["K"], c.p["PD"]
    bc, bct, ba = Buf(dev, cen.size, "f32", cen), Buf(dev, K, "f32", cts), Buf(dev, T, "i64")
    ws = _ws(dev, T, PD, K)
    pool = [p % T for p in S.POOL]
    arr = (C.c_int32 * len(pool))(*pool)
    it, used, ex = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    st = call("cogs_kmeans_lloyd", DT[c.dtype], bx.ptr, bts.ptr, T, PD, K, alpha, 1, 0.0, C.cast(arr, C.c_void_p), len(pool), bc.ptr, bct.ptr,
              ba.ptr, C.byref(it), C.byref(used), C.byref(ex), ws.ptr, ws.n)
    clean(c.id, (bx, bts), (bc, bct, ba, ws))
    return st, bc, bct, ba, (it.value, used.value, ex.value), pool, ws


@pytest.mark.parametrize("ci", range(len(ASSIGN)), ids=ids(ASSIGN))
def test_kmeans_assign_cell(dev, ci):
    """cogs_kmeans_assign and the reduce_assign_kernel of cogs_kmeans_lloyd(max_iter = 1) against torch's fp32 operations one by
    one, fed with the kernel's own dist2 bits; counts = bincount; the Lloyd step's centres and centre times bit for bit"""
    c = ASSIGN[ci]
    x, ts, cen, cts, pair = S.build_assign(c)
    T, K, PD, alpha = c.p["T"], c.p["K"], c.p["PD"], c.p["alpha"]
    bx, bts = Buf(dev, x.size, c.dtype, x), Buf(dev, T, "f32", ts)
    st, bd = _sqdist(dev, c.dtype, bx, T, PD, K, centres=cen)
    assert st == OK
    d2 = bd.freeze().vals().reshape(T, K)
    assert np.array_equal(d2, R.sqdist64(x, cen).astype(F32))
    want, fin = R.assign_fp32(d2, ts, cts, alpha)
    if pair is not None:
        assert fin[S.TIE_ROW, pair[0]] == fin[S.TIE_ROW, pair[1]] == 0 and want[S.TIE_ROW] == pair[0]
    if c.p["kind"] in ("nf0", "both0"):
        assert np.all(d2 == d2[:, :1])
    bct, ba, bn = Buf(dev, K, "f32", cts), Buf(dev, T, "i64"), Buf(dev, K, "i32")
    st = call("cogs_kmeans_assign", bd.ptr, bts.ptr, bct.ptr, T, K, alpha, ba.ptr, bn.ptr)
    assert st == OK
    clean(c.id, (bd, bts, bct), (ba, bn))
    got = ba.bits()
    bad = R.mismatch(got, want).ravel()
    assert bad.size == 0, f"{c.id}: cogs_kmeans_assign differs on rows {bad[:8].tolist()}: {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}"
    assert np.array_equal(bn.bits(), np.bincount(want, minlength=K))
    REACHED.add(("cogs_kmeans_assign", c.label))
    st, bc, bct2, ba2, (it, used, ex), pool, _ = _lloyd_once(dev, c, bx, bts, cen, cts, alpha)
    assert st == OK
    got = ba2.bits()
    bad = R.mismatch(got, want).ravel()
    assert bad.size == 0, f"{c.id}: reduce_assign_kernel differs on rows {bad[:8].tolist()}: {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}"
    empty = [k for k in range(K) if not np.any(want == k)]
    reseed = np.zeros(K, np.int64)
    reseed[empty] = pool[:len(empty)]
    nc, nct, _ = R.update_ref(x, ts, want, K, reseed, cen, cts)
    assert (it, used, ex) == (1, len(empty), 0), (c.id, it, used, ex)
    assert bc.bits().tobytes() == _bits(nc, "f32").tobytes(), f"{c.id}: the updated centres differ"
    assert bct2.bits().tobytes() == _bits(nct, "f32").tobytes(), f"{c.id}: the updated centre times differ"
    REACHED.add(("cogs_kmeans_lloyd", c.label))
    for p in c.paths:
        REACHED.add(("reduce_assign_kernel", p)), REACHED.add(("assign_kernel", p))


@pytest.mark.parametrize("what", ["nan row", "nan alpha"])
def test_kmeans_assign_all_nan_row(dev, what):
    """a dist2 row of NaN in a cell whose centre times are all equal: min / max of the row are NaN, `max > min` is false, both
    normalised distances are 0 for every cluster and the first one wins -- cluster 0, as in torch. alpha = NaN makes EVERY final
    distance NaN: a first-minimum scan finds nothing and stays at cluster 0"""
    c = next(c for c in ASSIGN if c.p["kind"] == "nt0" and c.p["K"] == 64)
    x, ts, cen, cts, _ = S.build_assign(c)
    T, K = c.p["T"], c.p["K"]
    d2 = R.sqdist64(x, cen).astype(F32)
    alpha = 2.0
    if what == "nan row":
        d2[7] = np.nan
    else:
        alpha, cts = float("nan"), (cts + np.arange(K)).astype(F32)
    want, fin = R.assign_fp32(d2, ts, cts, alpha)
    assert want[7] == 0 and (what == "nan row" or (np.all(np.isnan(fin)) and np.all(want == 0)))
    assert what == "nan alpha" or np.any(want != 0)
    bd, bts, bct, ba, bn = Buf(dev, d2.size, "f32", d2), Buf(dev, T, "f32", ts), Buf(dev, K, "f32", cts), Buf(dev, T, "i64"), Buf(dev, K, "i32")
    assert call("cogs_kmeans_assign", bd.ptr, bts.ptr, bct.ptr, T, K, alpha, ba.ptr, bn.ptr) == OK
    clean(what, (bd, bts, bct), (ba, bn))
    assert R.mismatch(ba.bits(), want).size == 0 and np.array_equal(bn.bits(), np.bincount(want, minlength=K))
    REACHED.add(("cogs_kmeans_assign", "all-NaN row: " + what))


def test_kmeans_margins_near_tie(dev):
    """one planted near-tie: at least one row below 1e-3, the minimum within a factor of two of the reference's"""
    x, ts, cen, cts = S.build_margin()
    T, PD, K = x.shape[0], x.shape[1], cen.shape[0]
    c = S.Cell("cogs_kmeans_margins", "near-tie", dict(T=T, K=K, PD=PD), (), 0, "f32")
    bx, bts = Buf(dev, x.size, "f32", x), Buf(dev, T, "f32", ts)
    st, bd = _sqdist(dev, "f32", bx, T, PD, K, centres=cen)
    d2 = bd.vals().reshape(T, K)
    want, _ = R.assign_fp32(d2, ts, cts, 2.0)
    st, _, _, ba, (it, _, _), _, ws = _lloyd_once(dev, c, bx, bts, cen, cts, 2.0)
    assert st == OK and it == 1 and np.array_equal(ba.bits(), want)
    m, n = C.c_float(-1), C.c_int32(-1)
    assert call("cogs_kmeans_margins", T, PD, K, ws.ptr, ws.n, C.byref(m), C.byref(n)) == OK
    ref = [R.margin64(d2, ts, cts, 2.0, t) for t in range(T)]
    print(f"margins: device min {m.value:.3e} rows below {n.value}; reference min {min(ref):.3e} rows below {sum(r < 1e-3 for r in ref)}")
    assert ref[5] == min(ref) < 1e-3
    assert n.value >= 1 and min(ref) / 2 <= m.value <= min(ref) * 2
    REACHED.add(("cogs_kmeans_margins", "near-tie"))


UPDATE = S.update_cells()


def _update(dev, c, x, ts, assign, reseed, old_c, old_ct, PD=None, short=0):
    T, K = c.p["T"], c.p["K"]
    PD = PD or c.p["PD"]
    bx, bts, ba, br = Buf(dev, x.size, c.dtype, x), Buf(dev, T, "f32", ts), Buf(dev, T, "i64", assign), Buf(dev, K, "i32", reseed)
    bc, bct, bs = Buf(dev, old_c.size, "f32", old_c), Buf(dev, K, "f32", old_ct), Buf(dev, 1, "f32")
    ws = _ws(dev, T, PD, K, short=short)
    st = call("cogs_kmeans_update", DT[c.dtype], bx.ptr, bts.ptr, T, PD, K, ba.ptr, br.ptr, bc.ptr, bct.ptr, bs.ptr, ws.ptr, ws.n)
    clean(c.id, (bx, bts, ba, br), (bc, bct, bs, ws))
    return st, bc, bct, bs


@pytest.mark.parametrize("ci", range(len(UPDATE)), ids=ids(UPDATE))
def test_kmeans_update_cell(dev, ci):
    """integer features: centres = fp32(sum) / fp32(n) bit for bit, the reseed row for an empty cluster; centre times = the
    sequential fp32 sum in ascending member order / n bit for bit; the shift against the yardstick"""
    c = UPDATE[ci]
    x, ts, assign, reseed, old_c, old_ct = S.build_update(c)
    K = c.p["K"]
    assert assign.min() >= 0 and assign.max() < K and np.bincount(assign, minlength=K).tolist() == c.p["counts"]
    st, bc, bct, bs = _update(dev, c, x, ts, assign, reseed, old_c, old_ct)
    assert st == OK
    nc, nct, shift = R.update_ref(x, ts, assign, K, reseed, old_c, old_ct)
    bad = R.mismatch(bc.bits().reshape(nc.shape), _bits(nc, "f32"))
    assert bad.size == 0, f"{c.id}: {len(bad)} centre elements differ, first (cluster, column) {bad[:5].tolist()}, counts {c.p['counts']}"
    assert bct.bits().tobytes() == _bits(nct, "f32").tobytes(), f"{c.id}: centre times {bct.vals()} want {nct}"
    plain = (torch.norm(torch.from_numpy(nc - old_c), p=2, dim=1).sum() + torch.norm(torch.from_numpy(nct - old_ct), p=2)).item()
    yard(c, bs.vals(), np.array([plain]), np.array([shift]), np.array([shift]), what=" shift")
    reach(c)


def test_kmeans_update_status(dev):
    c = S.Cell("cogs_kmeans_update", "status", dict(T=4, PD=16, K=2, counts=[2, 2]), (), 3, "f32")
    x, ts, assign, reseed, old_c, old_ct = S.build_update(c)
    st, bc, bct, bs = _update(dev, c, x, ts, assign, reseed, old_c, old_ct, PD=12)
    assert st == E_INVALID and bc.untouched() and bct.untouched() and bs.untouched()
    T, PD, K = S.tight_ws_shape()
    c = S.Cell("cogs_kmeans_update", "status", dict(T=T, PD=PD, K=K, counts=np.bincount(np.arange(T) % K, minlength=K).tolist()), (), 3, "f32")
    x, ts, assign, reseed, old_c, old_ct = S.build_update(c)
    st, bc, bct, bs = _update(dev, c, x, ts, assign, reseed, old_c, old_ct, short=1)
    assert st == E_WORKSPACE and bc.untouched() and bct.untouched() and bs.untouched()
    REACHED.add(("cogs_kmeans_update", "status PD % 8 != 0")), REACHED.add(("cogs_kmeans_update", "status workspace short"))


KPP = S.kpp_cells()


@pytest.mark.parametrize("ci", range(len(KPP)), ids=ids(KPP))
def test_kmeans_pp_cell(dev, ci):
    """the whole seeding in one call against the draw-by-draw reference on the kernel's own distances (cogs_kmeans_sqdist with
    centre_rows, folded with min): the same rows; an exact tie goes to the lower row; all rows on the first centre set the flag"""
    c = KPP[ci]
    x, first, q = S.build_kpp(c)
    T, K, PD = c.p["T"], c.p["K"], c.p["PD"]
    bx = Buf(dev, x.size, c.dtype, x)

    def dist(rows):
        st, bd = _sqdist(dev, c.dtype, bx, T, PD, len(rows), rows=rows)
        assert st == OK
        return bd.vals().reshape(T, len(rows))
    want, zero, gaps, holders = S.kpp_reference(x, first, q, K, dist)
    assert all(g > 1e-5 for g in gaps), (c.id, gaps)
    bq, bi, bf, bn = Buf(dev, q.size, "f32", q), Buf(dev, K, "i32"), Buf(dev, 1, "i32"), Buf(dev, T, "f32")
    ws = _ws(dev, T, PD, 1)
    st = call("cogs_kmeans_pp", DT[c.dtype], bx.ptr, T, PD, K, first, bq.ptr, bi.ptr, bf.ptr, bn.ptr, ws.ptr, ws.n)
    assert st == OK
    clean(c.id, (bx, bq), (bi, bf, bn, ws))
    got = bi.bits()
    assert int(bf.bits()[0]) == int(zero), (c.id, bf.bits(), zero)
    assert got[:len(want)].tolist() == want, f"{c.id}: rows {got.tolist()} want {want} (gaps {gaps})"
    if c.p["kind"] == "tie":
        assert holders[0] == list(S.KPP_TIE) and want[1] == S.KPP_TIE[0]
    if c.p["kind"] == "zero":
        assert zero
    reach(c)


# ------------------------------------------------------------------------------------------------ coverage
def test_zz_required_coverage(dev):
    """every (kernel, path) pair the cells are there for was reached; the pairs the issue names are among them"""
    required = {(c.kernel, p) for c in S.all_cells() if c.kernel != "kmeans_assign" for p in c.paths}
    for c in S.assign_cells():
        required |= {("cogs_kmeans_assign", c.label), ("cogs_kmeans_lloyd", c.label)}
        required |= {(k, p) for k in ("assign_kernel", "reduce_assign_kernel") for p in c.paths}
    named = []
    for k in ("cogs_layernorm", "cogs_rmsnorm", "cogs_ln_merge"):
        named += [(k, f"CPL{i}") for i in (1, 2, 3, 4, 8)] + [(k, "last chunk group partly filled"), (k, "last chunk group full")]
        named += [(k, "status " + s) for s in ("H % 8 != 0", "H > 4096", "rows = 0")]
    named += [("cogs_ln_merge", f"group {g}") for g in (1, 3, 4)] + [("cogs_ln_finalize", f"tiles {t}") for t in (1, 2, 18, 56)]
    named += [("cogs_ln_finalize", "second workgroup"), ("cogs_ln_finalize", "status H % 64 != 0")]
    named += [("cogs_pixdiff_mask", p) for p in ("four-chunk loop", "single-chunk loop only", "four-chunk loop with a ragged end", "minor None",
                                                  "minor zeros", "minor frame0", "minor middle", "minor last", "minor quiet", "min_tokens 0",
                                                  "min_tokens 1", "min_tokens 3", "min_tokens P+2", "P > 256", "sum / E against sum * (1 / E)",
                                                  "status E % 8 != 0", "status t = 0")]
    named += [("cogs_frame_mean_to_slot0", p) for p in ("second column trip", "one column trip", "0 frames", "1 frames",
                                                         "several non-adjacent frames", "exact", "numeric", "status D % 4 != 0")]
    named += [("cogs_gather_rows", p) for p in ("second chunk trip", "one chunk trip", "null table B", "two tables", "status D % 8 != 0")]
    named += [("cogs_mean_rows", p) for p in ("rows < 8", "rows == 8", "second row trip", "ldx != D", "last block has col >= D", "full blocks",
                                               "status D % 4 != 0", "status rows = 0")]
    named += [("cogs_cosine", p) for p in ("D < 64", "D == 64", "D % 64 != 0", "many trips", "all-zero a", "one all-zero b row")]
    named += [("cogs_pack_rows", p) for p in ("scalar tail", "no scalar tail", "zero padding groups", "second grid trip", "ld_out padded",
                                               "f32 to bf16", "bf16 to bf16", "f32 to f32", "bf16 to f32", "status cols_out % 4 != 0",
                                               "status cols_in > cols_out", "status ld_in % 4 != 0", "status ld_out % 4 != 0",
                                               "status unknown dtype")]
    named += [("cogs_kmeans_sqdist", p) for p in ("K % 4 != 0 (padded)", "second launch (k0 > 0)", "kc loop second trip", "last slice partly filled",
                                                   "eight-in-flight loop", "two row groups", "row group length % 8 != 0", "t + 8 prefetch",
                                                   "centres from rows", "centres from fp32", "exact", "numeric", "status PD % 8 != 0",
                                                   "status workspace one byte short", "status both centre sources null")]
    for k in ("assign_kernel", "reduce_assign_kernel"):
        named += [(k, p) for p in ("tie-lanes", "tie-same-lane", "nf0", "nt0", "both0", "alpha 0", "alpha 2", "K > 64 (second cluster per lane)",
                                   "T > 256 (second workgroup)", "K == 1")]
    named += [("cogs_kmeans_assign", "all-NaN row: nan row"), ("cogs_kmeans_assign", "all-NaN row: nan alpha"), ("cogs_kmeans_margins", "near-tie")]
    named += [("cogs_kmeans_update", f"member count {n}") for n in (0, 1, 2, 3, 4, 5, 8, 9)]
    named += [("cogs_kmeans_update", p) for p in ("PD crosses a 2048-column block", "PD one full block", "PD one partly filled block", "PD three blocks",
                                                   "members_kernel second thread trip", "members_slow_kernel", "status PD % 8 != 0",
                                                   "status workspace short")]
    named += [("cogs_kmeans_pp", p) for p in ("plain", "tie", "zero", "thread-stride second trip", "K 1", "K 2", "K 6", "two slices", "one slice")]
    required |= set(named)
    missing = sorted(r for r in required if r not in REACHED)
    assert not missing, f"not reached: {missing}"
    print("worst cell per kernel and dtype: kernel worst, yardstick worst there, ratio")
    for (k, dt), (a, b, r) in sorted(TABLE.items()):
        print(f"    {k:32s} {dt:5s} {a:10.3e} {b:10.3e} {r:7.3f}")
