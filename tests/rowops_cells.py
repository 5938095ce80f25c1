"""The cells of tests/test_gpu_rowops_conformance.py: for every kernel a list of Cell(kernel, label, p, paths, seed) and a
builder that turns a cell into its inputs (numpy, fp32 values; bf16 cells hold bf16-representable values). The path
labels say which branch of the launch code a shape is there for; they are derived from the launch code of the .hip file
named next to each list and collected by test_zz_required_coverage. tests/test_rowops_reference.py holds the builders to
their promises (exactness of the exact cells, the midpoint cap, the k-means++ margins) without a GPU.

The yardsticks (plain fp32 implementations: torch on the CPU for norms, means and cosine, sequential numpy loops for sums)
are here too, because both test files need them; torch is imported only inside them."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import rowops_reference as R

F32 = np.float32
EPS = 1e-6


@dataclass
class Cell:
    kernel: str
    label: str
    p: dict
    paths: tuple
    seed: int = 0
    dtype: str = "f32"

    @property
    def bf16(self):
        return self.dtype == "bf16"

    @property
    def id(self):
        return f"{self.kernel}-{self.label}-{self.dtype}".replace(" ", "_")


def _q(x, bf16):
    """fp32 values, bf16-representable for a bf16 cell"""
    return R.round_bf16(x) if bf16 else np.asarray(x, F32)


DTYPES = ("f32", "bf16")

# ------------------------------------------------------------------------------------------------ norms (csrc/norm.hip)
# launch_norm / launch_ln_merge: nch = H / 8 chunks of 8 elements, cpl = ceil(nch / 64) chunks per lane, instantiations
# CPL 1, 2, 3, 4 and 8 (cpl 5..8); cpl > 8, i.e. H > 4096, is refused. One wave per row, 4 rows per workgroup.
NORM_H = [8, 504, 512, 520, 1024, 1032, 1152, 1536, 1544, 2048, 2056, 3584, 4096]
NORM_ROWS = [1, 3, 4, 5, 37]


def norm_inst(H):
    cpl = (H // 8 + 63) // 64
    return cpl if cpl <= 4 else 8


def _norm_paths(H, rows):
    nch = H // 8
    out = [f"CPL{norm_inst(H)}", "last chunk group full" if nch % 64 == 0 else "last chunk group partly filled",
           "rows % 4 == 0" if rows % 4 == 0 else "last workgroup partly filled"]
    if rows > 4:
        out.append("more than one workgroup")
    return tuple(out)


def norm_cells():
    cells = []
    for kernel in ("cogs_layernorm", "cogs_rmsnorm"):
        for i, H in enumerate(NORM_H):
            for j, dt in enumerate(DTYPES):
                rows = NORM_ROWS[(i + 2 * j + (kernel == "cogs_rmsnorm")) % 5]
                cells.append(Cell(kernel, f"H{H} rows{rows}", dict(H=H, rows=rows), _norm_paths(H, rows), 1000 + i, dt))
    merge = [(8, 1, 1), (504, 3, 4), (520, 4, 5), (1152, 1, 5), (1544, 3, 1), (2056, 4, 4), (4096, 4, 1), (1032, 3, 5), (512, 1, 4)]
    for i, (H, group, out_rows) in enumerate(merge):
        for dt in DTYPES:
            cells.append(Cell("cogs_ln_merge", f"H{H} group{group} out{out_rows}", dict(H=H, group=group, out_rows=out_rows),
                              _norm_paths(H, out_rows) + (f"group {group}",), 1100 + i, dt))
    return cells


def build_norm(c: Cell):
    """x with a row mean of 3 standard deviations (1 for RMSNorm). LayerNorm: gamma around 0.5 and |beta| in [2.5, 3.5], so
    that gamma xhat and beta never cancel: where they do, the output is far smaller than its unit |gamma xhat| + |beta|, its
    bf16 steps are far finer than the fp32 bound, and such elements alone push a bf16 cell over the 1 % cap (the share
    grows like the logarithm of 1 / delta); a unit near zero would also let one chance element decide an fp32 cell. A
    bf16 output is still held to delta in absolute terms, whatever beta adds to it. RMSNorm: gamma around 1"""
    rng = np.random.default_rng(c.seed)
    H = c.p["H"]
    rows = c.p["rows"] if "rows" in c.p else c.p["out_rows"] * c.p["group"]
    rms = c.kernel == "cogs_rmsnorm"
    x = _q(rng.normal(1.0 if rms else 3.0, 1.0, (rows, H)), c.bf16)
    gamma = _q((1.0 if rms else 0.5) * (1.0 + 0.25 * rng.normal(size=H)), c.bf16)
    beta = _q(rng.choice([-1.0, 1.0], H) * rng.uniform(2.5, 3.5, H), c.bf16)
    return x, gamma, beta


def norm_reference(c: Cell, x, gamma, beta):
    """-> (ref fp64, unit)"""
    if c.kernel == "cogs_layernorm":
        return R.layernorm64(x, gamma, beta, EPS)
    if c.kernel == "cogs_rmsnorm":
        _, y, unit = R.rmsnorm64(x, gamma, EPS)
        return y, unit
    _, y, unit = R.ln_merge64(x, gamma, beta, c.p["group"], EPS)
    return y, unit


def norm_plain(c: Cell, x, gamma, beta):
    """torch on the CPU in fp32, as the modules being replaced state the operation"""
    import torch
    import torch.nn.functional as F
    xt, g, b = (torch.from_numpy(np.ascontiguousarray(a, F32)) for a in (x, gamma, beta))
    if c.kernel == "cogs_rmsnorm":
        return (g * (xt * torch.rsqrt(xt.pow(2).mean(-1, keepdim=True) + EPS))).numpy()
    y = F.layer_norm(xt, (xt.shape[1],), g, b, EPS)
    if c.kernel == "cogs_ln_merge":
        y = y.view(c.p["out_rows"], c.p["group"], -1).mean(dim=1)
    return y.numpy()


def norm_delta(c: Cell, x, gamma, beta):
    """the fp32 bound of the matching fp32 cell, in the cell's unit: FACTOR * the plain implementation's worst"""
    ref, unit = norm_reference(c, x, gamma, beta)
    _, y, _ = R.yardstick_ratio(ref, norm_plain(c, x, gamma, beta), ref, unit)
    return R.FACTOR * y


# ln_finalize_kernel: one thread per row, 256 per workgroup; tiles = H / 64 pairs per row
FIN = [(1, 1), (2, 255), (18, 256), (56, 257), (1, 257), (2, 256), (18, 1), (56, 255)]
FIN_RATIOS = (0.0, 3.0, 30.0)


def finalize_cells():
    return [Cell("cogs_ln_finalize", f"tiles{t} rows{r}", dict(tiles=t, rows=r, H=64 * t),
                 (f"tiles {t}", "one workgroup" if r <= 256 else "second workgroup", "full workgroup" if r % 256 == 0 else "partly filled workgroup"),
                 1200 + i) for i, (t, r) in enumerate(FIN)]


def build_finalize(c: Cell):
    """partial (sum, sum of squares) of rows whose mean / std is 0, 3 or 30 (row % 3), per 64-column tile, as fp32"""
    rng = np.random.default_rng(c.seed)
    rows, tiles, H = c.p["rows"], c.p["tiles"], c.p["H"]
    ratio = np.array(FIN_RATIOS)[np.arange(rows) % 3]
    x = rng.normal(size=(rows, H)) + ratio[:, None]
    xt = x.reshape(rows, tiles, 64)
    return np.stack([xt.sum(axis=2), (xt * xt).sum(axis=2)], axis=2).astype(F32)


# ------------------------------------------------------------------------------------------------ keep-mask (csrc/compress.hip)
# pixdiff_kernel: one wave per (frame, token); nch = E / 8 chunks; the four-chunk loop runs while ch + 192 < nch (a lane
# takes it from nch >= 193 + lane), the single-chunk loop takes the rest. mask_fix_kernel: one workgroup of 256 per frame.
PIX = [  # E, (t, P), min_tokens (None: P + 2), minor, thr
    (8, (1, 5), 0, None, 0.1), (512, (2, 1), 1, "zeros", 0.1), (520, (3, 7), 3, "frame0", 0.1), (2048, (6, 20), None, "middle", 0.1),
    (2056, (5, 257), 1, "last", 0.1), (2352, (6, 20), 3, "quiet", 0.1), (4104, (3, 7), 0, None, 2.5), (8, (6, 20), 1, "zeros", 0.1),
    (512, (3, 7), None, "last", 2.5), (520, (5, 257), 3, "middle", 2.5), (2048, (2, 1), 0, "frame0", 0.1), (2056, (1, 5), None, None, 0.1),
    (2352, (6, 20), 1, None, 0.1), (4104, (5, 257), 0, "quiet", 0.1), (2352, (3, 7), 1, None, "discriminate"),
    (520, (3, 7), 0, "zeros", "discriminate"), (4104, (2, 1), 3, None, 0.1), (8, (2, 1), None, None, 0.1),
    # sizes outside the list above at which the bf16 chain can tell the two mean forms apart (none of the listed sizes can)
    (504, (3, 7), 1, None, "discriminate"), (3584, (3, 7), 0, "zeros", "discriminate"),
]


def find_discriminating(E, bf16):
    """a row sum (in units of 2^-7) and a threshold on which `sum / E` and `sum * (1 / E)` give different masks"""
    u = np.arange(1, 128 * E)
    s = (u * R.PIX_UNIT).astype(F32)
    vd = R._rnd((R._rnd((s / F32(E)).astype(F32), bf16) * F32(255)).astype(F32), bf16)
    vm = R._rnd((R._rnd((s * (F32(1) / F32(E))).astype(F32), bf16) * F32(255)).astype(F32), bf16)
    hit = np.flatnonzero(vd != vm)
    if hit.size == 0:
        return None
    i = int(hit[0])
    return int(u[i]), float(min(vd[i], vm[i]))


def pix_cells():
    cells = []
    for i, (E, (t, P), mt, minor, thr) in enumerate(PIX):
        for dt in DTYPES:
            extra = None
            if thr == "discriminate":
                found = find_discriminating(E, dt == "bf16")
                if found is None:
                    continue                                             # this dtype cannot tell the two forms apart at this E
                extra, th = found
            else:
                th = thr
            nch = E // 8
            paths = ["four-chunk loop" if nch >= 193 else "single-chunk loop only", f"minor {minor}",
                     "min_tokens " + ("P+2" if mt is None else str(mt)), "frame 0 only" if t == 1 else "difference frames",
                     "P > 256" if P > 256 else "P <= 256"]
            if nch >= 193 and (nch - 193) % 256 < 255 and nch % 64:
                paths.append("four-chunk loop with a ragged end")
            if extra is not None:
                paths.append("sum / E against sum * (1 / E)")
            cells.append(Cell("cogs_pixdiff_mask", f"E{E} t{t} P{P} mt{'P+2' if mt is None else mt} minor-{minor} thr{thr}",
                              dict(E=E, t=t, P=P, min_tokens=P + 2 if mt is None else mt, minor=minor, thr=th, extra=extra), tuple(paths),
                              1300 + i, dt))
    return cells


def _row_with_sum(rng, prev, units):
    """cur = prev + d with sum |d| = units, every |d_i| <= 128 and every step towards zero, so |cur| <= 128 (1.0) like prev"""
    E = prev.size
    base, rem = divmod(int(units), E)
    assert base + 1 <= 128
    mag = np.full(E, base, np.int64)
    mag[rng.permutation(E)[:rem]] += 1
    sign = np.where(prev > 0, -1, np.where(prev < 0, 1, rng.choice([-1, 1], E)))
    return prev + sign * mag


def build_pix(c: Cell):
    """-> (pix in units of 2^-7 [t * P, E] int, minor uint8 [t] or None, planted {row: units}). Frame 0 random in [-32, 32];
    frame f >= 1 is mixed (rows either side of the boundary), quiet (all below) or busy (all above), in turn; the rows at
    the END of frame 1 carry the boundary sums b - 2, b - 1, b, b + 1 of the division chain (as many as the frame has rows;
    a one-row frame takes one of them by the cell's seed) and, in a discriminating cell, the sum the two mean forms split on"""
    rng = np.random.default_rng(c.seed)
    E, t, P, thr = c.p["E"], c.p["t"], c.p["P"], c.p["thr"]
    b = R.pixdiff_boundary(E, thr, c.bf16)
    pix = np.zeros((t, P, E), np.int64)
    pix[0] = rng.integers(-32, 33, (P, E))
    plant = [u for u in (b - 2, b - 1, b, b + 1) if u >= 0]
    if c.p["extra"] is not None:
        plant = [c.p["extra"]] + plant
    if P < len(plant):
        plant = [plant[(c.seed + k) % len(plant)] for k in range(P)]
    planted = {}
    quiet_frame = 2 if t > 2 else 1
    for f in range(1, t):
        kind = ("mixed", "quiet", "busy")[(f - 1) % 3]
        if c.p["minor"] == "quiet" and f == quiet_frame:
            kind = "quiet"
        for j in range(P):
            if f == 1 and j >= P - len(plant) and kind == "mixed":
                units = plant[j - (P - len(plant))]
                planted[f * P + j] = units
            elif kind == "quiet" or (kind == "mixed" and rng.random() < 0.5):
                units = int(rng.integers(0, b))
            else:
                units = int(rng.integers(b, min(3 * b + 3, 128 * E)))
            pix[f, j] = _row_with_sum(rng, pix[f - 1, j], units)
    kind = c.p["minor"]
    minor = None
    if kind is not None:
        minor = np.zeros(t, np.uint8)
        if kind != "zeros":
            minor[{"frame0": 0, "middle": t // 2, "last": t - 1, "quiet": quiet_frame if t > 1 else 0}[kind]] = 1
    return pix.reshape(t * P, E), minor, planted


# ------------------------------------------------------------------------------------------------ frame mean / gather / mean / cosine
# frame_mean_kernel: one workgroup per listed frame, thread d = 4 tid, column loop d += 1024
FRAME_TOTAL = 5
FMEAN = [  # D, P, frames, exact
    (4, 1, [2], True), (252, 2, [0, 2, 4], True), (1024, 64, [0, 2, 4], True), (1028, 2, [2], True), (3584, 64, [4, 0], True),
    (1028, 1, [], True), (4, 7, [0, 2, 4], False), (252, 64, [2], False), (1024, 7, [2], False), (1028, 7, [0, 2, 4], False),
    (3584, 2, [0, 2, 4], False), (252, 1, [0, 2, 4], False), (3584, 7, [2], False), (4, 64, [], False),
]


def fmean_cells():
    cells = []
    for i, (D, P, frames, exact) in enumerate(FMEAN):
        for dt in DTYPES:
            paths = ("second column trip" if D > 1024 else "one column trip", "whole workgroup" if D % 1024 == 0 else "partly filled trip",
                     f"{len(frames)} frames" if len(frames) < 2 else "several non-adjacent frames", f"P {P}", "exact" if exact else "numeric")
            cells.append(Cell("cogs_frame_mean_to_slot0", f"D{D} P{P} frames{len(frames)} {'exact' if exact else 'numeric'}",
                              dict(D=D, P=P, frames=frames, exact=exact), paths, 1400 + i, dt))
    return cells


def build_fmean(c: Cell):
    """exact: integers in [-3, 3] and P a power of two: |column sum| <= 192 < 256, so the mean m / P is exact in bf16 and in
    fp32 whatever the order. numeric: normal data around 2; the last token of every frame is 2^-9 of that size, or the
    column sums of bf16 values would sit on so coarse a grid that the mean of 2 or 7 of them is an exact bf16 midpoint in
    several per cent of the columns (and the cap on excepted elements could not hold)"""
    rng = np.random.default_rng(c.seed)
    P = c.p["P"]
    n = FRAME_TOTAL * P
    if c.p["exact"]:
        return rng.integers(-3, 4, (n, c.p["D"])).astype(F32)
    x = rng.normal(2.0, 1.0, (n, c.p["D"]))
    if P > 1:
        x[P - 1::P] *= 2.0 ** -9
    return _q(x, c.bf16)


# gather_rows_kernel: one wave per output row, 16-byte chunks (8 bf16 / 4 fp32), chunk loop ch += 64
GATHER = [(8, 1), (256, 3), (512, 4), (520, 5), (3584, 130), (8, 130), (256, 5), (512, 1), (520, 3), (3584, 4)]
GATHER_A, GATHER_B = 6, 3
GATHER_PATTERN = [0, GATHER_A - 1, -1, -GATHER_B, 0, 2, -2, GATHER_A - 1, 3, -1]


def gather_cells():
    cells = []
    for i, (D, rows) in enumerate(GATHER):
        for j, dt in enumerate(DTYPES):
            null_b = (i + j) % 3 == 2
            nch = D // (8 if dt == "bf16" else 4)
            paths = ("second chunk trip" if nch > 64 else "one chunk trip", "null table B" if null_b else "two tables",
                     "rows % 4 == 0" if rows % 4 == 0 else "last workgroup partly filled")
            cells.append(Cell("cogs_gather_rows", f"D{D} rows{rows}{' nullB' if null_b else ''}", dict(D=D, rows=rows, null_b=null_b),
                              paths, 1500 + i, dt))
    return cells


def build_gather(c: Cell):
    rng = np.random.default_rng(c.seed)
    D, rows = c.p["D"], c.p["rows"]
    ta = _q(rng.normal(size=(GATHER_A, D)), c.bf16)
    tb = _q(rng.normal(size=(GATHER_B, D)), c.bf16)
    first = [0, GATHER_A - 1, -1, -GATHER_B]                             # both ends of both tables, then the pattern with its repeats
    first = first[c.seed % 4:] + first[:c.seed % 4]
    idx = np.array((first + [GATHER_PATTERN[(c.seed + k) % len(GATHER_PATTERN)] for k in range(rows)])[:rows], np.int64)
    if c.p["null_b"]:
        idx = np.where(idx < 0, GATHER_A + idx, idx)                      # -1 -> the last row of A, -3 -> row 3
    return ta, tb, idx


# mean_rows_kernel: workgroup = 32 column groups of 4 x 8 row lanes, row loop r += 8, grid = ceil(D / 4 / 32)
MEANROWS = [  # D, rows, ldx - D, exact
    (4, 1, 0, True), (124, 8, 4, True), (128, 8, 0, True), (132, 1, 4, True), (3584, 8, 4, True),
    (4, 7, 4, False), (124, 9, 0, False), (128, 333, 4, False), (132, 7, 0, False), (3584, 9, 0, False), (132, 333, 4, False),
    (124, 333, 0, False), (4, 9, 0, False), (128, 7, 4, False),
]


def meanrows_cells():
    cells = []
    for i, (D, rows, pad, exact) in enumerate(MEANROWS):
        for dt in DTYPES:
            paths = ("rows < 8" if rows < 8 else ("rows == 8" if rows == 8 else "second row trip"), "ldx != D" if pad else "ldx == D",
                     "last block has col >= D" if (D // 4) % 32 else "full blocks", "exact" if exact else "numeric")
            cells.append(Cell("cogs_mean_rows", f"D{D} rows{rows} pad{pad} {'exact' if exact else 'numeric'}",
                              dict(D=D, rows=rows, pad=pad, exact=exact), paths, 1600 + i, dt))
    return cells


def build_meanrows(c: Cell):
    """exact: integers in [-8, 8], rows 1 or 8 (a power of two, so the 1 / rows factor is exact): |sum| <= 64"""
    rng = np.random.default_rng(c.seed)
    if c.p["exact"]:
        return rng.integers(-8, 9, (c.p["rows"], c.p["D"])).astype(F32)
    return _q(rng.normal(2.0, 1.0, (c.p["rows"], c.p["D"])), c.bf16)


# cosine_kernel: one wave per b row, element loop d += 64
COSINE = [(1, 1, None), (1, 6, "b"), (63, 1, None), (63, 6, "b"), (64, 1, None), (64, 6, "a"), (65, 1, "a"), (65, 6, "b"),
          (3584, 1, None), (3584, 6, "b")]


def cosine_cells():
    return [Cell("cogs_cosine", f"D{D} n{n} zero-{z}", dict(D=D, n=n, zero=z),
                 ("D < 64" if D < 64 else ("D == 64" if D == 64 else "D % 64 != 0" if D % 64 else "many trips"), f"n {n}",
                  {None: "no zero vector", "a": "all-zero a", "b": "one all-zero b row"}[z]), 1700 + i) for i, (D, n, z) in enumerate(COSINE)]


def build_cosine(c: Cell):
    rng = np.random.default_rng(c.seed)
    a = rng.normal(size=c.p["D"]).astype(F32)
    b = (0.6 * a[None, :] + rng.normal(size=(c.p["n"], c.p["D"]))).astype(F32)
    if c.p["zero"] == "a":
        a[:] = 0
    if c.p["zero"] == "b":
        b[3 % c.p["n"]] = 0
    return a, b


def means_plain(x, axis=0):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, F32)).mean(dim=axis).numpy()


def cosine_plain(a, b):
    import torch
    import torch.nn.functional as F
    return F.cosine_similarity(torch.from_numpy(a)[None, :], torch.from_numpy(b), dim=1, eps=1e-8).numpy()


# ------------------------------------------------------------------------------------------------ pack_rows (csrc/vision_misc.hip)
# pack_rows_kernel: one thread per 4 output columns, grid = min(4096, ceil(groups / 256)), grid-stride loop; a group with
# c + 3 >= cols_in takes the scalar tail
PACK_SHAPES = [(588, 640), (586, 588), (1, 4), (640, 640), (5, 8)]
PACK_PAIRS = [("f32", "bf16"), ("bf16", "bf16"), ("f32", "f32"), ("bf16", "f32")]


def pack_cells():
    cells = []
    k = 0
    for si, (ci, co) in enumerate(PACK_SHAPES):
        for pi, (di, do) in enumerate(PACK_PAIRS):
            rows = [1, 3, 300][(si + pi) % 3]
            pad_in = 8 if (si + pi) % 2 else 0
            paths = ["scalar tail" if ci % 4 else "no scalar tail", "zero padding groups" if co - ci >= 4 else "no whole padding group",
                     f"{di} to {do}", "ld_in padded" if pad_in else "ld_in tight", "one grid trip"]
            cells.append(Cell("cogs_pack_rows", f"{ci}to{co} rows{rows} {di}-{do} ldpad{pad_in}",
                              dict(cols_in=ci, cols_out=co, rows=rows, pad_in=pad_in, pad_out=0, din=di, dout=do), tuple(paths), 1800 + k, di))
            k += 1
    # rows * cols_out / 4 = 2100 * 512 = 1 075 200 > 4096 * 256 = 1 048 576 threads: the grid-stride loop takes a second trip
    cells.append(Cell("cogs_pack_rows", "2045to2048 rows2100 f32-bf16 second grid trip",
                      dict(cols_in=2045, cols_out=2048, rows=2100, pad_in=0, pad_out=0, din="f32", dout="bf16"),
                      ("second grid trip", "scalar tail", "f32 to bf16"), 1890, "f32"))
    cells.append(Cell("cogs_pack_rows", "586to588 rows3 bf16-bf16 ld_out padded",
                      dict(cols_in=586, cols_out=588, rows=3, pad_in=8, pad_out=4, din="bf16", dout="bf16"),
                      ("ld_out padded", "scalar tail", "bf16 to bf16"), 1891, "bf16"))
    return cells


def build_pack(c: Cell):
    """normal data with bf16 rounding midpoints (both parities), values one fp32 ulp either side of a midpoint, signed zeros,
    infinities and the largest finite values sprinkled in"""
    rng = np.random.default_rng(c.seed)
    rows, ci = c.p["rows"], c.p["cols_in"]
    x = rng.normal(size=(rows, ci)).astype(F32)
    special = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000,
                        0x7F7FFFFF, 0x7F7F7FFF, 0xBF818000, 0x3F7FFFFF], np.uint32).view(F32)
    flat = x.reshape(-1)
    pos = rng.permutation(flat.size)[:min(flat.size, 4 * special.size)]
    flat[pos] = special[np.arange(pos.size) % special.size]
    return _q(x, c.p["din"] == "bf16")


# ------------------------------------------------------------------------------------------------ k-means (csrc/kmeans.hip)
# sqdist_kernel: grid (slices of 512 columns, row groups); LDS centres padded to a multiple of 4; one launch per 32 centres
# (k0 = 0, 32, 64); a wave takes rows t, t + 4 of its group per step and prefetches t + 8. launch_sqdist picks the row
# groups (never fewer than 16 rows each), km_row_groups overrides the count before that clamp.
# reduce_row: kp = next power of two >= min(K, 64) lanes per slice group, G = 256 / kp groups; the eight-in-flight loop runs
# while sl + 7 G < nslices; the kc loop takes 64 centres at a time.
SQDIST = [(1, 8, 1), (3, 504, 3), (4, 512, 4), (5, 520, 5), (8, 2568, 31), (9, 8, 32), (33, 504, 33), (40, 512, 64), (1, 520, 65),
          (3, 2568, 70), (4, 8, 70), (5, 504, 1), (8, 512, 3), (9, 520, 4), (33, 2568, 5), (40, 8, 31), (40, 2568, 32), (33, 520, 33),
          (9, 512, 64), (8, 504, 65)]
SQDIST_LONG = [(9, 15368, 64), (9, 115208, 5)]


def _sqdist_paths(T, PD, K, src):
    ns = (PD + 511) // 512
    kp = 1
    while kp < min(K, 64):
        kp <<= 1
    G = 256 // kp
    out = [f"centres from {src}", "K % 4 != 0 (padded)" if K % 4 else "K % 4 == 0",
           "second launch (k0 > 0)" if K > 32 else "one launch", "kc loop second trip" if K > 64 else "one kc trip",
           "last slice partly filled" if PD % 512 else "full slices", "eight-in-flight loop" if ns > 7 * G else "tail loop only"]
    if T >= 32:
        out.append("two row groups")
    if T % 8 not in (0,) or (T >= 32 and ((T + 1) // 2) % 8):
        out.append("row group length % 8 != 0")
    if T > 8:
        out.append("t + 8 prefetch")
    return tuple(out)


def sqdist_cells():
    cells = []
    for i, (T, PD, K) in enumerate(SQDIST + SQDIST_LONG):
        for j, dt in enumerate(DTYPES):
            for src in ("rows", "fp32"):
                if (T, PD, K) in SQDIST_LONG and (j + (src == "rows")) % 2:
                    continue                                             # the long cells: one source per dtype
                cells.append(Cell("cogs_kmeans_sqdist", f"T{T} PD{PD} K{K} {src} exact", dict(T=T, PD=PD, K=K, src=src, exact=True),
                                  _sqdist_paths(T, PD, K, src) + ("exact",), 2000 + i, dt))
    for i, (T, PD, K) in enumerate([(40, 2568, 5), (33, 520, 33)]):
        for dt in DTYPES:
            cells.append(Cell("cogs_kmeans_sqdist", f"T{T} PD{PD} K{K} fp32 numeric", dict(T=T, PD=PD, K=K, src="fp32", exact=False),
                              _sqdist_paths(T, PD, K, "fp32") + ("numeric",), 2100 + i, dt))
    return cells


def build_sqdist(c: Cell):
    """-> (x [T, PD], centres fp32 [K, PD], centre_rows int32 [K] or None). exact: integers in [-4, 4], every squared
    difference <= 64 and every distance <= 64 PD < 2^24. numeric: rows around K random centres"""
    rng = np.random.default_rng(c.seed)
    T, PD, K = c.p["T"], c.p["PD"], c.p["K"]
    if c.p["exact"]:
        x = rng.integers(-4, 5, (T, PD)).astype(F32)
        if c.p["src"] == "rows":
            rows = rng.permutation(max(T, K))[:K] % T                   # repeats when K > T
            return x, x[rows].copy(), rows.astype(np.int32)
        return x, rng.integers(-4, 5, (K, PD)).astype(F32), None
    cent = (3.0 * rng.normal(size=(K, PD))).astype(F32)
    x = _q(cent[rng.integers(0, K, T)] + 0.3 * rng.normal(size=(T, PD)), c.bf16)
    return x, cent, None


# assignment: assign_kernel (one thread per row, 256 per workgroup) and reduce_assign_kernel (one workgroup per row; lane k % 64
# owns cluster k, so clusters 64 apart meet in one lane and neighbours in different lanes)
ASSIGN = [(1, 1, 2, "plain"), (40, 2, 0, "plain"), (255, 5, 2, "tie-lanes"), (256, 63, 2, "plain"), (257, 64, 0, "tie-lanes"),
          (40, 65, 2, "tie-same-lane"), (255, 70, 2, "tie-same-lane"), (256, 5, 2, "nf0"), (257, 2, 0, "nt0"), (1, 70, 0, "plain"),
          (40, 64, 2, "nt0"), (256, 1, 0, "plain"), (257, 63, 2, "nf0"), (255, 65, 0, "tie-same-lane"), (40, 5, 2, "both0"),
          (256, 2, 2, "tie-lanes")]
ASSIGN_PD = 16


def assign_cells():
    cells = []
    for i, (T, K, alpha, kind) in enumerate(ASSIGN):
        paths = (kind, f"alpha {alpha}", "K > 64 (second cluster per lane)" if K > 64 else "K <= 64",
                 "T > 256 (second workgroup)" if T > 256 else "T <= 256", "K == 1" if K == 1 else "K > 1")
        cells.append(Cell("kmeans_assign", f"T{T} K{K} alpha{alpha} {kind}", dict(T=T, K=K, alpha=float(alpha), kind=kind, PD=ASSIGN_PD),
                          paths, 2200 + i, DTYPES[i % 2]))
    return cells


TIE_ROW = 0


def build_assign(c: Cell):
    """-> (x ints [T, PD], ts [T], centres fp32 ints [K, PD], cts [K], tied pair or None). Integer features (exact distances,
    exact cluster sums); time stamps 0.25 + 0.5 t, centre times at non-dyadic offsets. Tie cells copy centre k1 (features and
    time) to k2 and put row TIE_ROW exactly on it, so both reach final distance 0 there"""
    rng = np.random.default_rng(c.seed)
    T, K, PD, kind = c.p["T"], c.p["K"], c.p["PD"], c.p["kind"]
    x = rng.integers(-4, 5, (T, PD)).astype(F32)
    ts = (0.25 + 0.5 * np.arange(T)).astype(F32)
    cen = rng.integers(-4, 5, (K, PD)).astype(F32)
    cts = (rng.uniform(0, 0.5 * T + 1, K) + 0.37).astype(F32)
    pair = None
    if kind in ("tie-lanes", "tie-same-lane"):
        pair = (K - 2, K - 1) if kind == "tie-lanes" else (K - 65, K - 1)
        if kind == "tie-lanes" and K >= 5:
            pair = (1, 2)
        cen[pair[1]] = cen[pair[0]]
        cts[pair[0]] = cts[pair[1]] = ts[TIE_ROW]
        x[TIE_ROW] = cen[pair[0]]
    if kind in ("nf0", "both0"):
        cen[:] = cen[0]
    if kind in ("nt0", "both0"):
        cts[:] = cts[0]
    return x, ts, cen, cts, pair


POOL = [(7 * i + 3) for i in range(128)]


def build_margin():
    """one planted near-tie: well separated centres, all centre times equal, row 5 on the line between centres 0 and 1 a
    fraction 1e-4 off their midpoint -> its two nearest feature distances differ by a few 1e-4 relative"""
    rng = np.random.default_rng(2290)
    T, K, PD = 40, 3, 16
    x = rng.normal(size=(T, PD)).astype(F32)
    cen = (2.0 * rng.normal(size=(K, PD))).astype(F32)
    x[5] = (0.5 * (cen[0] + cen[1]) + 1e-4 * (cen[1] - cen[0])).astype(F32)
    ts = (0.25 + 0.5 * np.arange(T)).astype(F32)
    cts = np.full(K, 4.37, F32)
    return x, ts, cen, cts


# update: members_kernel (one workgroup of min(1024, T rounded up to 64) threads, thread loop t += nt), members_slow_kernel above
# 16384 rows, update_kernel (grid (ceil(PD / 2048), K), four members at a time), update_final_kernel
UPDATE_COUNTS = [0, 1, 2, 3, 4, 5, 8, 9]
UPDATE = [(1, 8, 2), (64, 2040, 9), (65, 2048, 9), (1025, 2056, 9), (64, 4104, 9), (65, 8, 9), (1025, 2048, 9), (1, 2040, 2)]
UPDATE_SLOW = (16385, 8, 3)


def update_counts(T, K, seed):
    if K == 2:
        base = [1, 0]
    elif K == 3:
        base = [0, 5, T - 5]
    else:
        base = UPDATE_COUNTS + [T - sum(UPDATE_COUNTS)]
    r = seed % K
    return base[r:] + base[:r]


def update_cells():
    cells = []
    for i, (T, PD, K) in enumerate(UPDATE + [UPDATE_SLOW]):
        dt = DTYPES[(i + 1) % 2]
        counts = update_counts(T, K, 2300 + i)
        paths = [f"member count {n}" for n in sorted(set(counts)) if n < 10] + [
            {2040: "PD one partly filled block", 2048: "PD one full block", 2056: "PD crosses a 2048-column block", 4104: "PD three blocks",
             8: "PD 8"}[PD],
            "members_slow_kernel" if T > 16384 else ("members_kernel second thread trip" if T > 1024 else "members_kernel one trip")]
        cells.append(Cell("cogs_kmeans_update", f"T{T} PD{PD} K{K}", dict(T=T, PD=PD, K=K, counts=counts), tuple(paths), 2300 + i, dt))
    return cells


def build_update(c: Cell):
    """-> (x ints in [-4, 4], ts, assign int64 (all inside [0, K)), reseed int32 [K], old centres, old centre times).
    Column sums of at most 16385 members of magnitude <= 4 stay below 2^17: exact in fp32"""
    rng = np.random.default_rng(c.seed)
    T, PD, K = c.p["T"], c.p["PD"], c.p["K"]
    x = rng.integers(-4, 5, (T, PD)).astype(F32)
    ts = (0.3 + 0.7 * np.arange(T)).astype(F32)
    assign = rng.permutation(np.repeat(np.arange(K), c.p["counts"])).astype(np.int64)
    reseed = rng.integers(0, T, K).astype(np.int32)
    old_c = rng.integers(-4, 5, (K, PD)).astype(F32)
    old_ct = rng.uniform(0, T, K).astype(F32)
    return x, ts, assign, reseed, old_c, old_ct


# k-means++: reduce_min_kernel (one wave per row, 4 per workgroup), kpp_select_kernel (one workgroup, thread loop t += 256, waves of
# 64, first maximum: lower row on equal ratios)
KPP = [(1, 1, 8, "plain"), (2, 2, 8, "plain"), (255, 6, 520, "plain"), (256, 2, 8, "plain"), (257, 6, 8, "plain"), (600, 6, 520, "plain"),
       (600, 2, 520, "tie"), (257, 6, 520, "tie"), (2, 2, 8, "zero"), (1, 2, 8, "zero"), (255, 1, 520, "plain"), (256, 6, 520, "plain")]
KPP_TIE = (10, 138)          # thread 10 of wave 0 and thread 138 of wave 2


def kpp_cells():
    cells = []
    for i, (T, K, PD, kind) in enumerate(KPP):
        paths = (kind, "T <= 256" if T <= 256 else "thread-stride second trip", f"K {K}", "two slices" if PD > 512 else "one slice",
                 "partly filled wave" if T % 64 else "full waves")
        cells.append(Cell("cogs_kmeans_pp", f"T{T} K{K} PD{PD} {kind}", dict(T=T, K=K, PD=PD, kind=kind), paths, 2400 + i, DTYPES[i % 2]))
    return cells


def build_kpp(c: Cell):
    """-> (x ints [T, PD], first row, q fp32 [K - 1, T] from a seeded numpy exponential). tie: rows KPP_TIE are duplicates with
    the same small q in step 0; zero: every row equals row 0"""
    rng = np.random.default_rng(c.seed)
    T, K, PD, kind = c.p["T"], c.p["K"], c.p["PD"], c.p["kind"]
    x = rng.integers(-4, 5, (T, PD)).astype(F32)
    first = int(rng.integers(0, T))
    q = rng.exponential(size=(max(K - 1, 1), T)).astype(F32)[:K - 1]
    if kind == "zero":
        x[:] = x[0]
    if kind == "tie":
        a, b = KPP_TIE
        x[b] = x[a]
        q[0, a] = q[0, b] = F32(1e-4)
        if first in KPP_TIE:
            first = 0
    return x, first, q


def kpp_reference(x, first, q, K, dist=None):
    """the whole seeding -> (rows [K], zero flag, smallest gap over the steps, best-ratio holders per step). dist(rows) gives the
    squared distances [T, len(rows)] to feature rows (default: exact fp64, right for integer features)"""
    dist = dist or (lambda rows: R.sqdist64(x, x[rows]).astype(F32))
    idx, gaps, holders = [first], [], []
    for m in range(1, K):
        n2 = dist(np.array(idx, np.int32)).min(axis=1)
        row, zero, gap, hold = R.kpp_select(n2, q[m - 1])
        if zero:
            return idx, True, gaps, holders
        idx.append(row)
        gaps.append(gap)
        holders.append(hold)
    return idx, False, gaps, holders


def kmeans_ws_bytes(T, PD, K):
    """the workspace layout stated above cogs_k_kmeans_ws in csrc/kmeans.hip, in bytes before the 256-byte round-up"""
    ns, nblk = (PD + 511) // 512, (PD + 2047) // 2048
    return (max(ns * T * K, nblk * K) + (K + 1) + T + 2 * K + T * K + K + 8 + 4096) * 4


def tight_ws_shape():
    """the first (T, PD, K) whose stated need is a multiple of the 256-byte round-up of cogs_kmeans_workspace_bytes: one byte
    less than the reported size is then less than the need"""
    for T in range(2, 12):
        for K in range(1, T + 1):
            for PD in range(8, 4096, 8):
                if kmeans_ws_bytes(T, PD, K) % 256 == 0:
                    return T, PD, K
    raise AssertionError("no tight shape")


def status_codes():
    """{name: value} of csrc/status.h"""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cogstream_amd", "csrc", "status.h")
    with open(path) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+COGS_(\w+)\s+\(?(-?\d+)\)?", f.read())}


ALL = None


def all_cells():
    global ALL
    if ALL is None:
        ALL = (norm_cells() + finalize_cells() + pix_cells() + fmean_cells() + gather_cells() + meanrows_cells() + cosine_cells() +
               pack_cells() + sqdist_cells() + assign_cells() + update_cells() + kpp_cells())
    return ALL
