"""The rows of tests/test_gpu_sample_conformance.py, built from numpy alone so that tests/test_sample_reference.py can hold
every one of them to the reference's conditions without a GPU (top-p margin >= 100 x the cumulative sum's error bound,
<= 1 % of the Philox draws inside the score margin). A row that misses the margin is rebuilt from the next generator seed
HERE (`_settle`), never skipped there.

Winners are planted, not random: distinct values above a background in [-14, -8], at index 0, n - 1, the first index of the
last non-empty slice and both sides of several seams of the slice path (chunk = ceil(n / 64))."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import sample_reference as R

SLICES, KMAX, SLICE_MAX = 64, 64, 4096


def expected_path(n: int, top_k: int) -> int:
    return 1 if 0 < top_k <= KMAX and SLICES * top_k <= n <= SLICES * SLICE_MAX else 2


@dataclass
class Cell:
    label: str
    n: int
    top_k: int
    top_p: float
    temperature: float
    logits: np.ndarray                       # fp32 [n], before the allowed-id mask
    allowed: Optional[np.ndarray] = None     # ids cogs_logits_process keeps (everything else -inf) before sampling
    check: str = "exact"                     # "exact": ids / order / probs / token; "limit": the stated limits only
    kept_cap: Optional[int] = None           # None: room for every survivor
    tags: tuple = ()
    path: int = field(init=False)

    def __post_init__(self):
        self.path = expected_path(self.n, self.top_k)

    def row(self) -> np.ndarray:
        """what cogs_sample reads"""
        return R.penalty_mask_temperature(self.logits, None, 1.0, self.allowed, 1.0) if self.allowed is not None else self.logits

    def warp(self) -> R.Warped:
        return R.warp(self.row(), self.temperature, self.top_k, self.top_p)


def seam_positions(n: int) -> list:
    chunk = -(-n // SLICES)
    last_first = ((n - 1) // chunk) * chunk
    pos = [0, n - 1, last_first]
    for s in (1, 2, 31, 32, 63, 17):
        pos += [s * chunk - 1, s * chunk]
    out = []
    for p in pos:
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


def planted(n: int, w: int, seed: int, positions=None, step=None, top=4.0, flat_bg=None) -> np.ndarray:
    """w distinct winners (top, top - step', ...; step' jittered so that no two gaps are equal) over the background"""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-14.0, -8.0, n) if flat_bg is None else np.full(n, flat_bg)).astype(np.float32)
    w = min(w, n)
    step = min(0.37, 10.0 / max(w, 1)) if step is None else step
    vals = top - step * (np.arange(w) + rng.uniform(0.0, 0.6, w))
    pos = list(seam_positions(n) if positions is None else positions)[:w]
    free = np.setdiff1d(np.arange(n), pos)
    pos += rng.choice(free, w - len(pos), replace=False).tolist() if w > len(pos) else []
    pos = np.asarray(pos)[rng.permutation(w)]              # which winner sits on which seam changes with the seed
    x[pos] = vals.astype(np.float32)
    return x


def margin_ok(c: Cell) -> bool:
    w = c.warp()
    return w.margin >= R.MARGIN_FACTOR * R.cum_err(w.m0, c.path)


def _settle(make, seed: int) -> Cell:
    for s in range(seed, seed + 64):
        c = make(s)
        if margin_ok(c):
            return c
    raise AssertionError(f"no generator seed in [{seed}, {seed + 64}) gives {c.label} its top-p margin")


TOP_PS = (1.0, 0.8, 0.3, 1e-6, 0.0)
TEMPS = (1.0, 0.7, 1.3)


def _next_below(x: float, ulps: int = 1) -> np.float32:
    b = np.array([x], np.float32).view(np.int32)
    b = b - ulps if x > 0 else b + ulps
    return b.view(np.float32)[0]


def _cut_top_p(row, temperature, top_k, removed_lo: int) -> float:
    """top_p whose cut removes `removed_lo` entries and sits halfway to removing one more (from the fp64 reference)"""
    w = R.warp(row, temperature, top_k, 1.0)
    asc = w.probs[::-1]
    cum = np.cumsum(asc)
    lim = cum[removed_lo - 1] + 0.5 * asc[removed_lo]
    return float(1.0 - lim)


@functools.lru_cache(maxsize=None)
def cells() -> tuple:
    out = []
    seed = [1000]

    def add(label, n, top_k, top_p, temp, make_logits, **kw):
        seed[0] += 100
        out.append(_settle(lambda s: Cell(label, n, top_k, top_p, temp, make_logits(s), **kw), seed[0]))

    # ---- (top_k, n) grid, both paths: every top_p, the temperatures in turn
    grid = [(1, 64), (1, 65), (20, 1280), (20, 1281), (20, 1343), (20, 4097), (20, 152064), (64, 4096), (64, 4159),
            (20, 262144),
            (0, 1), (0, 2), (0, 1023), (0, 1024), (0, 1025), (0, 152064), (20, 1279), (64, 4095), (65, 8192), (20, 262145),
            (2000, 1500), (300, 152064)]
    for gi, (k, n) in enumerate(grid):
        w = max(k + 4, 24) if k <= 300 else 24
        for pi, tp in enumerate(TOP_PS):
            t = TEMPS[(gi + pi) % 3]
            add(f"grid k{k} n{n} p{tp:g} t{t:g}", n, k, tp, t, lambda s, n=n, w=w: planted(n, w, s), tags=("grid", (k, n), tp, t))
    for t in TEMPS:
        add(f"temperature k20 n4097 t{t:g}", 4097, 20, 0.8, t, lambda s: planted(4097, 24, s), tags=("temperature", t))

    # ---- prefilter bounds of the merge kernel (n 4096: chunk 64)
    add("prefilter one-slice", 4096, 20, 0.8, 1.0, lambda s: planted(4096, 24, s, positions=list(range(320, 344))), tags=("prefilter", "kth"))
    add("prefilter slice-maxima", 4096, 20, 0.8, 1.0,
        lambda s: planted(4096, 20, s, positions=[64 * b + (7 * b) % 64 for b in range(3, 63, 3)], flat_bg=-10.0), tags=("prefilter", "maxima"))

    # ---- masked rows
    def allowed_ids(n, cnt, s):                              # three planted winners and cnt - 3 others
        first = seam_positions(n)[:3]
        rest = np.random.default_rng(s).choice(np.setdiff1d(np.arange(n), first), cnt - 3, replace=False)
        return np.concatenate([first, rest]).astype(np.int32)
    for k, n in ((20, 4096), (20, 1279), (0, 4096)):
        for cnt in (6, 256):
            seed[0] += 100
            out.append(_settle(lambda s, k=k, n=n, cnt=cnt: Cell(f"masked k{k} n{n} allowed{cnt}", n, k, 1.0 if cnt == 6 else 0.8, 0.7,
                                                                planted(n, 24, s, step=0.3), allowed=allowed_ids(n, cnt, s),
                                                                tags=("masked", cnt)), seed[0]))
        out.append(Cell(f"all -inf k{k} n{n}", n, k, 0.8, 1.0, np.full(n, -np.inf, np.float32), tags=("all-inf",)))

    # ---- ties of the k-th value (all kept, as in HF), spread so that no slice holds more than k of them
    def tied_row(n, k, t, s, value=-7.0, shift=0.0):         # winners end above -6.5, the background starts at -8
        x = planted(n, k - 1, s)
        x[x > -7.5] += np.float32(shift)
        rng = np.random.default_rng(s + 7)
        free = np.flatnonzero(x < -7.5)
        x[rng.choice(free, t, replace=False)] = np.float32(value)
        return x
    for k, n in ((20, 4096), (20, 1279)):
        for t in (2, 5, 40):
            add(f"topk ties t{t} k{k} n{n}", n, k, 1.0, 1.0, lambda s, k=k, n=n, t=t: tied_row(n, k, t, s), tags=("topk-ties", t))

    def zero_row(n, k, s):
        x = tied_row(n, k, 1, s, value=0.0, shift=7.0)       # every winner above zero
        rng = np.random.default_rng(s + 9)
        free = np.flatnonzero(x < -7.5)
        x[rng.choice(free, 3, replace=False)] = np.float32(-0.0)
        return x
    for k, n in ((20, 4096), (20, 1279)):
        add(f"signed zero k{k} n{n}", n, k, 1.0, 0.7, lambda s, k=k, n=n: zero_row(n, k, s), tags=("signed-zero",))

    # ---- order contract: a top-p cut inside a block of 12 ties that reaches past rank k, spread over many slices
    def block_row(n, above, t, s):
        x = planted(n, above, s, step=0.2)
        rng = np.random.default_rng(s + 3)
        slices = rng.choice(np.arange(2, 62), t, replace=False)
        chunk = -(-n // SLICES)
        x[slices * chunk + rng.integers(1, chunk - 1, t)] = np.float32(x.max() - 2.5)
        return x
    for k, n in ((14, 4096),):
        seed[0] += 100
        for s in range(seed[0], seed[0] + 64):
            row = block_row(n, 8, 12, s)
            c = Cell(f"topp cut in tie block k{k} n{n}", n, k, _cut_top_p(row, 1.0, k, 3), 1.0, row, tags=("tie-block",))
            if margin_ok(c):
                break
        out.append(c)

    # ---- stated limits of the slice path
    def crowd_row(n, k, s, ties, per_slice_all):
        x = planted(n, k - 1, s)
        kth = np.float32(-7.0)
        chunk = -(-n // SLICES)
        if per_slice_all:
            x[5 * chunk + 3 + 2 * np.arange(ties)] = kth           # all in slice 5
        else:
            rng = np.random.default_rng(s)
            per = -(-ties // 60)
            idx = np.concatenate([(b + 2) * chunk + 5 + rng.choice(chunk - 10, per, replace=False) for b in range(60)])[:ties]
            x[idx] = kth
        return x
    out.append(Cell("limit: > k ties in one slice", 4096, 20, 1.0, 1.0, crowd_row(4096, 20, 77, 30, True), check="limit", tags=("limit", "slice")))
    out.append(Cell("limit: > 1024 kept", 65536, 64, 1.0, 1.0, crowd_row(65536, 64, 78, 1100, False), check="limit", tags=("limit", "kept")))

    # ---- kept_cap below the survivor count
    add("kept_cap 3 k20 n4096", 4096, 20, 1.0, 1.0, lambda s: planted(4096, 24, s), kept_cap=3, tags=("kept-cap",))
    add("kept_cap 3 k0 n1025", 1025, 0, 0.8, 1.0, lambda s: planted(1025, 24, s), kept_cap=3, tags=("kept-cap",))

    # ---- radix seams (k-th and (k+1)-th value one ulp apart in the lowest key byte), on both paths
    def ulp_row(n, k, s):
        x = planted(n, k - 1, s)
        kth = np.array([0x3f9e4c80], np.int32).view(np.float32)[0]      # 1.2367..., low key byte 0x80
        x[x > -7.5] += np.float32(12.0)                      # every winner above the pair
        rng = np.random.default_rng(s + 1)
        a, b = rng.choice(np.flatnonzero(x < -7.5), 2, replace=False)
        x[a], x[b] = kth, _next_below(kth)
        return x
    add("radix seam top-k k65 n8192", 8192, 65, 1.0, 1.0, lambda s: ulp_row(8192, 65, s), tags=("radix", "topk"))
    add("ulp seam top-k k20 n4097", 4097, 20, 1.0, 1.0, lambda s: ulp_row(4097, 20, s), tags=("radix", "topk"))

    # top-p boundary probabilities that differ only in their last digit: two scores 2 ulp apart in [2, 4) under a maximum
    # on the same grid (v - max exact), the cut between them
    def pseam_row(n, s):
        x = planted(n, 6, s, top=3.5, step=0.25)
        rng = np.random.default_rng(s + 2)
        a, b = rng.choice(np.flatnonzero(x < -7.0), 2, replace=False)
        lo = np.float32(2.03125)
        x[a], x[b] = lo, _next_below(lo, -2)
        return x
    for n in (1025, 152064):
        seed[0] += 100
        for s in range(seed[0], seed[0] + 64):
            row = pseam_row(n, s)
            c = Cell(f"radix seam top-p n{n}", n, 0, _cut_top_p(row, 1.0, 0, n - 7), 1.0, row, tags=("radix", "topp"))
            if margin_ok(c):
                break
        out.append(c)

    # ---- whole-row path: ties at the top-p boundary all stay
    for k, n in ((0, 1025), (65, 8192)):
        seed[0] += 100
        for s in range(seed[0], seed[0] + 64):
            row = block_row(n, 8, 5, s)
            w0 = R.warp(row, 1.0, k, 1.0)
            c = Cell(f"topp boundary ties k{k} n{n}", n, k, _cut_top_p(row, 1.0, k, w0.m0 - 8 - 3), 1.0, row, tags=("topp-ties",))
            if margin_ok(c):
                break
        out.append(c)

    # ---- one row on both paths: (64, n) slices, (65, n) whole row with one more survivor
    seed[0] += 100
    both = planted(4160, 70, seed[0])
    out.append(Cell("both paths k64 n4160", 4160, 64, 1.0, 1.0, both, tags=("both", 64)))
    out.append(Cell("both paths k65 n4160", 4160, 65, 1.0, 1.0, both, tags=("both", 65)))
    return tuple(out)


# ---- Philox rows: per path one peaked row and one flat over about 15 survivors
@functools.lru_cache(maxsize=None)
def philox_cells() -> tuple:
    out = []
    for k in (20, 0):
        out.append(_settle(lambda s, k=k: Cell(f"philox peaked k{k}", 4096, k, 0.8, 1.0, planted(4096, 24, s, step=1.0), tags=("philox", "peaked")), 5000 + k))

        def flat(s):
            x = planted(4096, 24, s, step=1.0)
            idx = np.argsort(-x)[:15]
            x[idx] = (4.0 - 0.013 * np.arange(15) * (1 + 0.1 * np.random.default_rng(s).uniform(size=15))).astype(np.float32)
            return x
        out.append(_settle(lambda s, k=k: Cell(f"philox flat k{k}", 4096, k, 0.95, 1.0, flat(s), tags=("philox", "flat")), 6000 + k))
    return tuple(out)


def philox_pairs() -> list:
    """256 (seed, offset) pairs: seeds with bits above 32, offsets around 2^32 and at 2^40, consecutive offsets"""
    seeds = [1, 99, (1 << 32) + 5, (1 << 63) + 12345, 0xDEADBEEFCAFEF00D, (7 << 40) + 3]
    offs = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 40]
    pairs = [(s, o) for s in seeds for o in offs]
    pairs += [(0x123456789ABCDEF, o) for o in range(1000, 1000 + 110)]
    pairs += [((5 << 32) + 1, (1 << 32) + o) for o in range(110)]
    return pairs[:256]


def philox_expect(c: Cell, pairs):
    """-> (tokens, safe mask) of the reference for every pair"""
    w = c.warp()
    ids, probs, D = (w.ids, w.probs, w.D) if c.path == 1 else (w.ids_all, w.probs_all, w.D_all)
    toks, safe = [], []
    for s, o in pairs:
        q = R.device_draw(s, o, ids)
        toks.append(R.pick(ids, probs, q)[0])
        safe.append(R.draw_is_safe(D, len(ids), c.path, probs, q, device=True))
    return np.asarray(toks), np.asarray(safe)


def handed_draws(c: Cell, start: int):
    """fp32 Exponential(1) draws for the whole row from the first generator seed >= start whose best / second-best gap is
    safe -> (draws, token)"""
    w = c.warp()
    ids, probs, D = (w.ids, w.probs, w.D) if c.path == 1 else (w.ids_all, w.probs_all, w.D_all)
    for s in range(start, start + 64):
        q = np.random.default_rng(s).exponential(1.0, c.n).astype(np.float32)
        if ids.size == 0:
            return q, 0
        if R.draw_is_safe(D, len(ids), c.path, probs, q[ids].astype(np.float64), device=False):
            return q, R.pick(ids, probs, q[ids].astype(np.float64))[0]
    raise AssertionError(c.label)
