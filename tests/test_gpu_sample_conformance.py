"""cogs_sample (both paths), cogs_argmax, cogs_topk and cogs_logits_process against the numpy reference of
tests/sample_reference.py, on the rows of tests/sample_cells.py (held to the reference's margins on the CPU by
tests/test_sample_reference.py): slice / tie / mask edges of the token selection.

Conventions. Every call goes through ctypes and the test owns every buffer: out_token, kept_idx, kept_prob, n_kept, the
workspace and the logits row each sit inside a tracer-filled allocation with tracer elements before and after. The row's
tracer is a finite 3.39e38, so a read past n wins every selection and fails the cell. Every cell asserts the status and
cogs_debug_get("sample_last_path"), records (path, label) in REACHED, and checks that all guards kept their bits and the
logits are unchanged; test_zz_required_coverage asserts the required list. Survivors, their order (path 1) or set (path 2),
the probabilities (per element against the derived bound) and the token for handed-over draws are compared with the
reference; selections and the logits processors bit for bit."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest
import torch

import sample_cells as S
import sample_reference as R

pytestmark = pytest.mark.gpu

GUARD = 256                    # tracer elements on each side of every buffer
TRACER_F = 3.39e38
TRACER_I = 0x5A5A5A5A
OK, E_INVALID, E_WORKSPACE = 0, -1, -4

REACHED = set()
WORST = {1: 0.0, 2: 0.0}

GRID = {1: [(1, 64), (1, 65), (20, 1280), (20, 1281), (20, 1343), (20, 4097), (20, 152064), (64, 4096), (64, 4159), (20, 262144)],
        2: [(0, 1), (0, 2), (0, 1023), (0, 1024), (0, 1025), (0, 152064), (20, 1279), (64, 4095), (65, 8192), (20, 262145),
            (2000, 1500), (300, 152064)]}


def _L():
    from cogstream_amd import _lib
    return _lib


class Guarded:
    """n elements with GUARD tracer elements before and after; the payload is tracer-filled too until written"""

    def __init__(self, dev, n: int, dtype, data=None):
        self.n, self.dtype = n, dtype
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        if dtype == torch.float32:
            self.buf.fill_(TRACER_F)
        elif dtype == torch.uint8:
            self.buf.fill_(0x5A)
        elif dtype == torch.int64:
            self.buf.fill_(TRACER_I * (1 << 32) + TRACER_I)
        else:
            self.buf.fill_(TRACER_I)
        self.view = self.buf[GUARD:GUARD + n]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)).to(dev))
        self.before = self.buf.cpu().numpy().copy()

    @property
    def ptr(self):
        return self.view.data_ptr() if self.n > 0 else self.buf.data_ptr() + GUARD * self.buf.element_size()

    def host(self) -> np.ndarray:
        return self.buf.cpu().numpy()[GUARD:GUARD + self.n]

    def guards_intact(self) -> bool:
        now = self.buf.cpu().numpy()
        return now[:GUARD].tobytes() == self.before[:GUARD].tobytes() and now[GUARD + self.n:].tobytes() == self.before[GUARD + self.n:].tobytes()

    def untouched(self, lo: int = 0) -> bool:
        """guards intact and the payload from element lo on still what it was at construction"""
        return self.guards_intact() and self.host()[lo:].tobytes() == self.before[GUARD + lo:GUARD + self.n].tobytes()


class Sampler:
    """one guarded set of cogs_sample buffers around a row"""

    def __init__(self, dev, row: np.ndarray, cap: int, logits: Guarded = None):
        L = _L()
        self.L, self.dev, self.n, self.cap = L, dev, row.size, cap
        self.row = np.ascontiguousarray(row, np.float32)
        self.logits = logits if logits is not None else Guarded(dev, row.size, torch.float32, self.row)
        self.out = Guarded(dev, 1, torch.int64)
        self.kidx = Guarded(dev, cap, torch.int32)
        self.kprob = Guarded(dev, cap, torch.float32)
        self.nkept = Guarded(dev, 1, torch.int32)
        self.ws = Guarded(dev, int(L.lib.cogs_sample_workspace_bytes()), torch.uint8)
        self.draws = None

    def call(self, top_k, top_p, temperature, *, draws=None, seed=0, offset=0, n=None, kept=True, ws=True, **ptrs):
        if draws is not None:
            self.draws = Guarded(self.dev, self.n, torch.float32, draws)
        a = dict(logits=self.logits.ptr, out=self.out.ptr, kidx=self.kidx.ptr if kept else None, kprob=self.kprob.ptr if kept else None,
                 nkept=self.nkept.ptr if kept else None, cap=self.cap if kept else 0, ws=self.ws.ptr if ws else None)
        a.update(ptrs)
        st = self.L.lib.cogs_sample(self.L.current_stream(), a["logits"], self.n if n is None else n, float(temperature), int(top_k),
                                    float(top_p), self.draws.ptr if draws is not None else None, int(seed), int(offset), a["out"],
                                    a["kidx"], a["kprob"], a["nkept"], a["cap"], a["ws"])
        torch.cuda.synchronize()
        return st

    @property
    def path(self):
        return self.L.debug_get("sample_last_path")

    def assert_clean(self, label):
        for name in ("logits", "out", "kidx", "kprob", "nkept", "ws", "draws"):
            g = getattr(self, name)
            assert g is None or g.guards_intact(), f"{label}: a write outside {name}"
        assert self.logits.host().tobytes() == self.row.tobytes(), f"{label}: the logits changed"

    def assert_nothing_written(self, label):
        self.assert_clean(label)
        for name in ("out", "kidx", "kprob", "nkept", "ws"):
            assert getattr(self, name).untouched(), f"{label}: {name} was written"

    def result(self):
        nk = int(self.nkept.host()[0])
        w = max(0, min(nk, self.cap))
        return int(self.out.host()[0]), nk, self.kidx.host()[:w].astype(np.int64), self.kprob.host()[:w].copy()


def _masked_logits(dev, c: S.Cell) -> Guarded:
    """the cell's row through cogs_logits_process with its allowed ids, bit for bit the reference's; guarded"""
    L = _L()
    g = Guarded(dev, c.n, torch.float32, c.logits)
    al = Guarded(dev, c.allowed.size, torch.int32, c.allowed)
    st = L.lib.cogs_logits_process(L.current_stream(), g.ptr, c.n, None, 0, 1.0, al.ptr, c.allowed.size, 1.0, None)
    torch.cuda.synchronize()
    assert st == OK and g.guards_intact() and al.untouched()
    assert g.host().tobytes() == c.row().tobytes(), f"{c.label}: the masked row differs from the reference"
    g.before = g.buf.cpu().numpy().copy()
    return g


def _reference(c: S.Cell):
    w = c.warp()
    return (w, w.ids, w.probs, w.D) if c.path == 1 else (w, w.ids_all, w.probs_all, w.D_all)


def _compare(c, ids, probs, D, got_ids, got_probs, ordered, m=None):
    bad, worst = R.compare_kept(ids, probs, D, len(ids) if m is None else m, c.path, got_ids, got_probs, ordered)
    if math.isfinite(worst):
        WORST[c.path] = max(WORST[c.path], worst)
    print(f"{c.label}: path {c.path}, kept {len(ids)}, worst observed / bound {worst:.3f}")
    assert not bad, f"{c.label}: {bad}"


CELLS = S.cells()


@pytest.mark.parametrize("ci", range(len(CELLS)), ids=[c.label.replace(" ", "_") for c in CELLS])
def test_sample_cell(dev, ci):
    """one row of tests/sample_cells.py: status, path, survivors (order on path 1, set on path 2), probabilities, the token for
    handed-over draws, n_kept against kept_cap, guards"""
    c = CELLS[ci]
    w, ids, probs, D = _reference(c)
    q, want_tok = S.handed_draws(c, 100 + ci)
    cap = c.kept_cap if c.kept_cap is not None else (1024 + 8 if c.check == "limit" else len(ids) + 8)
    s = Sampler(dev, c.row(), cap, logits=_masked_logits(dev, c) if c.allowed is not None else None)
    st = s.call(c.top_k, c.top_p, c.temperature, draws=q)
    assert st == OK, (c.label, st)
    assert s.path == c.path == S.expected_path(c.n, c.top_k), (c.label, s.path)
    s.assert_clean(c.label)
    tok, nk, got_ids, got_probs = s.result()
    if c.check == "limit":
        # stated limits of the slice path (include/cogs.h): everything strictly above the k-th value, nothing below it,
        # at least top_k entries, at most 1024
        assert c.top_k <= nk <= 1024 and len(set(got_ids.tolist())) == nk, (c.label, nk)
        assert set(w.topk_above.tolist()) <= set(got_ids.tolist()), c.label
        assert set(got_ids.tolist()) <= set(w.topk_above.tolist()) | set(w.topk_tied.tolist()), c.label
        assert np.array_equal(got_ids[:len(w.topk_above)], ids[:len(w.topk_above)]) and tok in got_ids.tolist()
        assert abs(float(got_probs.astype(np.float64).sum()) - 1.0) < 1e-4
    elif len(ids) == 0:
        assert (tok, nk) == (0, 0), (c.label, tok, nk)
        assert s.kidx.untouched() and s.kprob.untouched()
    elif c.kept_cap is not None:
        assert nk == len(ids) > cap, (c.label, nk)                       # the full count; only kept_cap entries written
        assert s.kidx.guards_intact() and s.kprob.guards_intact()
        if c.path == 1:
            _compare(c, ids[:cap], probs[:cap], D[:cap], got_ids, got_probs, True, m=len(ids))
        else:
            pos = {int(i): j for j, i in enumerate(ids)}
            assert len(set(got_ids.tolist())) == cap and all(int(i) in pos for i in got_ids), (c.label, got_ids)
            sel = np.array([pos[int(i)] for i in got_ids])
            bad, _ = R.compare_kept(ids[sel], probs[sel], D[sel], len(ids), 2, got_ids, got_probs, True)
            assert not bad, (c.label, bad)
        assert tok == want_tok
    else:
        assert nk == len(ids), f"{c.label}: n_kept {nk}, reference {len(ids)} (HF {w.hf_count}); kept {got_ids[:40].tolist()} want {ids[:40].tolist()}"
        _compare(c, ids, probs, D, got_ids, got_probs, ordered=c.path == 1)
        assert not R.compare_token(tok, want_tok), (c.label, tok, want_tok)
        assert s.kidx.untouched(nk) and s.kprob.untouched(nk), f"{c.label}: entries past n_kept written"
        if c.path == 1:
            assert nk == w.hf_count
    if c.tags[0] == "tie-block":
        # the order was undefined before the ranked placement: the same call again gives the same bits
        first = s.kidx.host().tobytes(), s.kprob.host().tobytes(), tok
        for _ in range(3):
            assert s.call(c.top_k, c.top_p, c.temperature, draws=q) == OK
            assert (s.kidx.host().tobytes(), s.kprob.host().tobytes(), s.result()[0]) == first, c.label
    # without the report buffers the token is the same
    s2 = Sampler(dev, c.row(), 1, logits=s.logits)
    assert s2.call(c.top_k, c.top_p, c.temperature, draws=q, kept=False) == OK
    assert int(s2.out.host()[0]) == tok and s2.kidx.untouched() and s2.nkept.untouched()
    s2.assert_clean(c.label)
    REACHED.add((c.path, c.label))


def test_both_paths_on_one_row(dev):
    """the same tie-free row: (64, n) takes the slices, (65, n) the whole row and keeps one more; both agree with the reference
    (test_sample_cell), the shared 64 candidates are the same ids and, renormalised, the same probabilities"""
    a = next(c for c in CELLS if c.label == "both paths k64 n4160")
    b = next(c for c in CELLS if c.label == "both paths k65 n4160")
    res = {}
    for c in (a, b):
        s = Sampler(dev, c.row(), 80)
        assert s.call(c.top_k, c.top_p, c.temperature, seed=3, offset=4) == OK and s.path == c.path
        s.assert_clean(c.label)
        _, nk, ids, pr = s.result()
        res[c.path] = dict(zip(ids.tolist(), pr.astype(np.float64).tolist()))
        assert nk == c.top_k
    extra = set(res[2]) - set(res[1])
    assert set(res[1]) <= set(res[2]) and len(extra) == 1
    scale = 1.0 - res[2][extra.pop()]
    wa = a.warp()
    tol = dict(zip(wa.ids.tolist(), (R.prob_tol(wa.probs, wa.D, 64, 1) + R.prob_tol(wa.probs, wa.D, 65, 2) + 2 * R.U * wa.probs).tolist()))
    for i, p in res[1].items():
        assert abs(res[2][i] / scale - p) <= tol[i], (i, p, res[2][i] / scale)
    REACHED.add((1, "both")), REACHED.add((2, "both"))


PHILOX = S.philox_cells()


@pytest.mark.parametrize("ci", range(len(PHILOX)), ids=[c.label.replace(" ", "_") for c in PHILOX])
def test_philox_keying(dev, ci):
    """256 (seed, offset) pairs per row: the token is pick(ids, p, device_draw(seed, offset, ids)) of the reference -- counter
    (i, offset lo, offset hi, 0), key (seed lo, seed hi) -- except for the pairs the reference lists as inside the score
    margin (<= 1 %, tests/test_sample_reference.py). The same rows distinguish a swapped seed / offset and an offset lowered
    by 2^32, so a kernel that drops a high word fails."""
    c = PHILOX[ci]
    pairs = S.philox_pairs()
    want, safe = S.philox_expect(c, pairs)
    assert np.count_nonzero(~safe) <= 0.01 * len(pairs)
    swapped = S.philox_expect(c, [(o, s_) for s_, o in pairs])[0]
    high = [i for i, (_, o) in enumerate(pairs) if o >= 1 << 32]
    lowered = S.philox_expect(c, [(pairs[i][0], pairs[i][1] - (1 << 32)) for i in high])[0]
    assert np.any(swapped != want) and np.any(lowered != want[high]), "the row cannot tell the high words apart"
    s = Sampler(dev, c.row(), 1)
    toks = Guarded(dev, len(pairs), torch.int64)
    for i, (seed, off) in enumerate(pairs):
        st = s.L.lib.cogs_sample(s.L.current_stream(), s.logits.ptr, c.n, c.temperature, c.top_k, c.top_p, None, seed, off,
                                 toks.ptr + 8 * i, None, None, None, 0, s.ws.ptr)
        assert st == OK
    torch.cuda.synchronize()
    assert s.path == c.path
    s.assert_clean(c.label)
    assert toks.guards_intact() and s.out.untouched()
    got = toks.host()
    miss = [(pairs[i], int(got[i]), int(want[i])) for i in np.flatnonzero(safe) if got[i] != want[i]]
    assert not miss, f"{c.label}: {len(miss)} of {int(safe.sum())} tokens differ, first (pair, device, reference): {miss[:5]}"
    REACHED.add((c.path, "philox " + c.tags[1]))


def test_status_codes(dev):
    """invalid arguments return COGS_E_INVALID, the slice path without a workspace COGS_E_WORKSPACE; nothing is written and the
    path report does not change"""
    fast = next(c for c in CELLS if c.tags[:3] == ("grid", (20, 4097), 0.8))
    full = next(c for c in CELLS if c.tags[:3] == ("grid", (0, 1025), 0.8))
    for c, other in ((fast, full), (full, fast)):
        so = Sampler(dev, other.row(), 64)
        assert so.call(other.top_k, other.top_p, other.temperature) == OK and so.path == other.path
        s = Sampler(dev, c.row(), 64)
        bad = [("n = 0", dict(n=0)), ("n < 0", dict(n=-5)), ("temperature 0", dict(temperature=0.0)),
               ("temperature < 0", dict(temperature=-1.0)), ("temperature NaN", dict(temperature=float("nan"))),
               ("top_k < 0", dict(top_k=-1)), ("kept_idx without kept_prob", dict(kprob=None)),
               ("kept_idx without n_kept", dict(nkept=None)), ("kept_idx without kept_cap", dict(cap=0))]
        for label, kw in bad:
            args = dict(top_k=c.top_k, top_p=c.top_p, temperature=c.temperature)
            args.update({k: kw.pop(k) for k in list(kw) if k in args})
            assert s.call(args["top_k"], args["top_p"], args["temperature"], **kw) == E_INVALID, (c.label, label)
            assert s.path == other.path, (c.label, label, "the report changed")
            s.assert_nothing_written(f"{c.label}: {label}")
        if c.path == 1:
            assert s.call(c.top_k, c.top_p, c.temperature, ws=False) == E_WORKSPACE
            assert s.path == other.path
            s.assert_nothing_written(f"{c.label}: no workspace")
        else:
            assert s.call(c.top_k, c.top_p, c.temperature, ws=False) == OK and s.path == 2      # the whole-row path needs none
        REACHED.add((c.path, "status"))


# ------------------------------------------------------------------------------------------------ argmax / topk / processors
def _bg(n, seed):
    return np.random.default_rng(seed).uniform(-9.0, -1.0, n).astype(np.float32)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 16383, 16384, 16385, 152064])
def test_argmax_first_maximum(dev, n):
    """cogs_argmax = the FIRST maximum under IEEE ==: planted at 0, n - 1 and both sides of the 256- (thread) and 16384-
    (64 blocks x 256 threads) strides; duplicates, +0 / -0 as a tied maximum, a row of -inf"""
    L = _L()
    rows = []
    spots = [p for p in (0, n - 1, 255, 256, 16383, 16384, 2 * 16384 - 1, 2 * 16384) if 0 <= p < n]
    for p in dict.fromkeys(spots):
        x = _bg(n, p)
        x[p] = 3.0
        rows.append(x)
    pairs = [(a, b) for a, b in ((255, 256), (16383, 16384), (0, n - 1), (256, 16384), (16384, 32768 + 255), (n // 2, n - 1)) if a < b < n]
    for a, b in pairs:
        for first in (a, b):
            x = _bg(n, a + b)
            x[[a, b]] = 3.0
            rows.append(x)
            z = np.full(n, -2.0, np.float32)                            # +0 and -0 tie for the maximum, in both orders
            z[first] = 0.0
            z[a + b - first] = -0.0
            rows.append(z)
    rows.append(np.full(n, -np.inf, np.float32))
    rows.append(np.full(n, 1.5, np.float32))
    for x in rows:
        g, out, ws = Guarded(dev, n, torch.float32, x), Guarded(dev, 1, torch.int64), Guarded(dev, 128, torch.float32)
        st = L.lib.cogs_argmax(L.current_stream(), g.ptr, n, out.ptr, ws.ptr)
        torch.cuda.synchronize()
        assert st == OK and int(out.host()[0]) == R.argmax_first(x), (n, int(out.host()[0]), R.argmax_first(x))
        assert g.untouched() and out.guards_intact() and ws.guards_intact()
    out = Guarded(dev, 1, torch.int64)
    assert L.lib.cogs_argmax(L.current_stream(), g.ptr, 0, out.ptr, ws.ptr) == E_INVALID and out.untouched()


@pytest.mark.parametrize("n,k", [(1, 1), (1023, 20), (1024, 20), (1025, 1024), (152064, 1), (152064, 20), (152064, 1024)])
def test_topk_stable_order(dev, n, k):
    """cogs_topk bit for bit: descending, equal values (IEEE ==, so +0 with -0) by ascending index, (-inf, -1) past the finite
    entries; k of 0 and 1025 are refused with the outputs untouched"""
    L = _L()
    rng = np.random.default_rng(n * 31 + k)
    rows = [rng.normal(0, 3, n).astype(np.float32)]
    x = rng.normal(0, 3, n).astype(np.float32)                          # planted ties inside and across the k boundary
    t = rng.choice(n, min(n, 12), replace=False)
    x[t[:6]] = 20.0
    x[t[6:]] = np.sort(x)[::-1][min(k, n) - 1]
    x[t[:2]] = [0.0, -0.0] if n > 2 else x[t[:2]]
    rows.append(x)
    z = np.full(n, -2.0, np.float32)                                    # signed zeros tie
    z[rng.choice(n, min(n, 8), replace=False)] = np.where(np.arange(min(n, 8)) % 2 == 0, 0.0, -0.0)
    rows.append(z)
    f = np.full(n, -np.inf, np.float32)                                 # fewer than k finite entries
    few = rng.choice(n, min(n, max(k // 2, 1)) if k > 1 else 0, replace=False)
    f[few] = rng.normal(0, 1, few.size)
    rows.append(f)
    for ri, x in enumerate(rows):
        g, ws = Guarded(dev, n, torch.float32, x), Guarded(dev, n, torch.float32)
        tv, ti = Guarded(dev, k, torch.float32), Guarded(dev, k, torch.int32)
        st = L.lib.cogs_topk(L.current_stream(), g.ptr, n, k, tv.ptr, ti.ptr, ws.ptr)
        torch.cuda.synchronize()
        val, idx = R.topk_stable(x, k)
        assert st == OK and ti.host().tolist() == idx.tolist(), (n, k, ri, ti.host()[:30], idx[:30])
        assert tv.host().tobytes() == val.tobytes(), (n, k, ri)
        assert g.untouched() and ws.guards_intact() and tv.guards_intact() and ti.guards_intact()
    for bad_k in (0, 1025):
        tv, ti, ws = Guarded(dev, 1025, torch.float32), Guarded(dev, 1025, torch.int32), Guarded(dev, n, torch.float32)
        assert L.lib.cogs_topk(L.current_stream(), g.ptr, n, bad_k, tv.ptr, ti.ptr, ws.ptr) == E_INVALID
        torch.cuda.synchronize()
        assert tv.untouched() and ti.untouched() and ws.untouched() and g.untouched()


def _process(dev, x, prev, pen, allowed, temp):
    L = _L()
    n_prev = 0 if prev is None else len(prev)
    n_al = 0 if allowed is None else len(allowed)
    g = Guarded(dev, x.size, torch.float32, x)
    pv = Guarded(dev, n_prev, torch.int64, np.asarray(prev, np.int64)) if n_prev else None
    al = Guarded(dev, n_al, torch.int32, np.asarray(allowed, np.int32)) if n_al else None
    tmp = Guarded(dev, max(n_prev, 1), torch.float32)
    st = L.lib.cogs_logits_process(L.current_stream(), g.ptr, x.size, pv.ptr if pv else None, n_prev, float(pen),
                                   al.ptr if al else None, n_al, float(temp), tmp.ptr)
    torch.cuda.synchronize()
    assert g.guards_intact() and tmp.guards_intact() and (pv is None or pv.untouched()) and (al is None or al.untouched())
    return st, g


@pytest.mark.parametrize("n_prev", [0, 1, 1023, 1024, 1025, 5000])
def test_logits_process_bit_for_bit(dev, n_prev):
    """repetition penalty (every id of the history once, whatever its multiplicity; positive, negative, +0, -0 and -inf
    logits), then the allowed-id mask (duplicates, ids also in the history), then the temperature: each one fp32 IEEE
    operation, so the row equals the reference bit for bit; tmp and the row are guarded"""
    n = 8192
    rng = np.random.default_rng(n_prev)
    x = rng.normal(0, 4, n).astype(np.float32)
    special = np.array([0, 1, 2, 3, n - 1, 1024, 1025])
    x[special] = [0.0, -0.0, -np.inf, 2.5, -2.5, -0.0, 0.0]
    prev = None
    if n_prev:
        prev = rng.integers(0, n, n_prev)
        m = min(n_prev, special.size)
        prev[:m] = special[:m]
        if n_prev > 16:
            prev[-8:] = prev[:8]                                        # duplicates, also of the special ids
            prev[n_prev // 2] = prev[n_prev // 2 - 1]
    for n_al in (0, 1, 6, 256):
        allowed = None
        if n_al:
            allowed = rng.choice(n, n_al, replace=False)
            if n_al >= 6:
                allowed[:3] = special[:3]                               # ids also in the history
                allowed[-1] = allowed[0]                                # a duplicate
            if n_prev and n_al == 1:
                allowed[0] = prev[0]
        for pen, temp in ((1.3, 0.7), (1.05, 1.0), (0.8, 1.3)):
            st, g = _process(dev, x, prev, pen, allowed, temp)
            want = R.penalty_mask_temperature(x, prev, pen, allowed, temp)
            got = g.host()
            assert st == OK and got.tobytes() == want.tobytes(), (n_prev, n_al, pen, temp, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:10])
    if n_prev:
        st, g = _process(dev, x, prev, 1.0, None, 1.0)                  # penalty 1.0 with a history: nothing changes
        assert st == OK and g.untouched()
    st, g = _process(dev, x, prev, 1.3, np.arange(257), 0.7)            # more than 256 allowed ids
    assert st == E_INVALID and g.untouched()


def test_zz_required_coverage(dev):
    """every cell the file is there for was reached, on the path it was written for"""
    labels = {c.label: c for c in CELLS}
    for path, grid in GRID.items():
        for k, n in grid:
            for tp in S.TOP_PS:
                hit = [c for c in CELLS if c.tags[:3] == ("grid", (k, n), tp)]
                assert len(hit) == 1 and hit[0].path == path == S.expected_path(n, k), (path, k, n, tp)
        assert {c.tags[3] for c in CELLS if c.tags[0] == "grid" and c.path == path} == set(S.TEMPS)
    required = [(c.path, c.label) for c in CELLS]
    for path in (1, 2):
        required += [(path, "both"), (path, "status"), (path, "philox peaked"), (path, "philox flat")]
        for tag in ("masked", "all-inf", "topk-ties", "signed-zero", "kept-cap", "radix"):
            assert any(c.path == path and c.tags[0] == tag for c in CELLS), (path, tag)
    assert {c.tags[1] for c in CELLS if c.tags[0] == "topk-ties" and c.path == 1} == {2, 5, 40}
    assert {c.tags[1] for c in CELLS if c.tags[0] == "masked" and c.path == 1} == {6, 256}
    assert {c.tags[1] for c in CELLS if c.tags[0] == "prefilter" and c.path == 1} == {"kth", "maxima"}
    assert {c.tags[1] for c in CELLS if c.tags[0] == "limit" and c.path == 1} == {"slice", "kept"}
    assert any(c.tags[0] == "tie-block" and c.path == 1 for c in CELLS) and any(c.tags[0] == "topp-ties" and c.path == 2 for c in CELLS)
    assert {c.tags[1] for c in CELLS if c.tags[0] == "radix" and c.path == 2} == {"topk", "topp"}
    assert labels and len(required) == len(set(required))
    missing = [r for r in required if r not in REACHED]
    assert not missing, f"not reached: {missing}"
    print(f"worst observed / bound of the kept probabilities: path 1 {WORST[1]:.3f}, path 2 {WORST[2]:.3f}")
    assert 0.0 < WORST[1] <= 1.0 and 0.0 < WORST[2] <= 1.0
