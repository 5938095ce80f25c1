"""The sampling reference (tests/sample_reference.py) and the rows of the GPU conformance file (tests/sample_cells.py), held
to account without a GPU: the reference reproduces the transformers fixture and the published Philox vectors, the
comparison the GPU tests use rejects the errors it is there to catch, and every GPU row has the top-p margin / draw margin
the reference needs to have ONE right answer."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import sample_cells as S
import sample_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling.npz")


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.mark.parametrize("ci", range(7))
def test_reference_reproduces_transformers_fixture(fixture, ci):
    """all seven cases: the processors bit for bit, the survivor set exactly, the probabilities within the derived bound of
    the fixture's fp32 softmax, and all 16 seeds' multinomial draws from the CPU generator's exponentials"""
    g = fixture
    top_k, top_p, temp, rep = g[f"s{ci}_params"].tolist()
    after = R.penalty_mask_temperature(g[f"s{ci}_logits"], g[f"s{ci}_prev"] if rep != 1.0 else None, rep, None, 1.0)
    assert after.tobytes() == g[f"s{ci}_after_penalty"].tobytes()
    w = R.warp(after, temp, int(top_k), top_p)
    assert w.tie_free or ci == 2, "only the tied case has equal scores at a boundary"
    assert np.sort(np.concatenate([w.topk_above, w.topk_tied])).tolist() == np.sort(g[f"s{ci}_kept_after_topk"]).tolist() or int(top_k) == 0
    order = np.argsort(w.ids)
    assert w.ids[order].tolist() == g[f"s{ci}_kept"].tolist()
    assert w.hf_count == len(g[f"s{ci}_kept"])
    tol = R.prob_tol(w.probs, w.D, len(w.ids), 1)[order]
    err = np.abs(g[f"s{ci}_probs"].astype(np.float64) - w.probs[order])
    assert np.all(err <= tol), (ci, float((err / tol).max()))
    for seed, want in enumerate(g[f"s{ci}_draws"].tolist()):
        q = torch.empty(after.size).exponential_(1, generator=torch.Generator().manual_seed(1000 + seed)).numpy()
        assert R.pick(w.ids, w.probs, q[w.ids].astype(np.float64))[0] == want, (ci, seed)


def test_philox_known_answer_vectors():
    """Philox4x32-10, the three published vectors of the Random123 distribution (kat_vectors), all ten rounds"""
    assert R.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    ones = 0xFFFFFFFF
    assert R.philox4x32_10((ones,) * 4, (ones,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    # the sampler's keying: counter (i, offset lo, offset hi, 0), key (seed lo, seed hi), first word, vectorised over i
    seed, off = 0x299F31D0A4093822, 0x13198A2E85A308D3
    assert int(R.device_word(seed, off, np.array([0x243F6A88]))[0]) == R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0), (0xA4093822, 0x299F31D0))[0]
    words = R.device_word(seed, off, np.arange(5))
    assert [int(x) for x in words] == [R.philox4x32_10((i, 0x85A308D3, 0x13198A2E, 0), (0xA4093822, 0x299F31D0))[0] for i in range(5)]
    q = R.device_draw(7, 1 << 32, np.arange(4096))
    assert q.dtype == np.float64 and np.all(q >= 0) and np.all(np.isfinite(q)) and abs(q.mean() - 1.0) < 0.1


def test_selection_references():
    x = np.array([1.0, -0.0, 3.0, 0.0, 3.0, -np.inf], np.float32)
    assert R.argmax_first(x) == 2
    assert R.argmax_first(np.array([-1.0, -0.0, 0.0], np.float32)) == 1 and R.argmax_first(np.array([-1.0, 0.0, -0.0], np.float32)) == 1
    assert R.argmax_first(np.full(5, -np.inf, np.float32)) == 0
    val, idx = R.topk_stable(x, 7)
    assert idx.tolist() == [2, 4, 0, 1, 3, -1, -1]
    assert val.tobytes() == np.array([3.0, 3.0, 1.0, -0.0, 0.0, -np.inf, -np.inf], np.float32).tobytes()
    y = R.penalty_mask_temperature(np.array([2.0, -2.0, 0.0, -0.0, -np.inf, 5.0], np.float32), [0, 1, 1, 2, 3, 4], 2.0, [0, 1, 2, 3, 4], 0.5)
    assert y.tobytes() == np.array([2.0, -8.0, 0.0, -0.0, -np.inf, -np.inf], np.float32).tobytes()


def test_warp_tie_rules():
    """signed zero at the top-k boundary, the two top-p contracts on a tied boundary, the all -inf row"""
    x = np.full(64, -5.0, np.float32)
    x[[3, 9]] = [2.0, 1.0]
    x[[20, 40]] = 0.0
    x[[10, 50]] = -0.0
    w = R.warp(x, 1.0, 3, 1.0)
    assert w.topk_above.tolist() == [3, 9] and w.topk_tied.tolist() == [10, 20, 40, 50] and w.ids.tolist() == [3, 9, 10, 20, 40, 50]
    p = R.warp(x, 1.0, 3, 1.0).probs
    lim = p[5] + p[4] + 0.5 * p[3]                         # removes two of the four zeros and half of a third
    w = R.warp(x, 1.0, 3, 1.0 - lim)
    assert w.ids.tolist() == [3, 9, 10, 20] and w.hf_count == 4 and w.ids_all.tolist() == [3, 9, 10, 20, 40, 50]
    assert w.topp_above.tolist() == [3, 9] and w.topp_tied.tolist() == [10, 20, 40, 50] and not w.tie_free
    assert abs(w.margin - 0.5 * p[3]) < 1e-7 and abs(w.probs.sum() - 1) < 1e-12 and abs(w.probs_all.sum() - 1) < 1e-12
    w = R.warp(np.full(8, -np.inf, np.float32), 1.0, 3, 0.8)
    assert w.ids.size == 0 and w.hf_count == 0
    w = R.warp(x, 1.0, 0, 0.0)
    assert w.ids.tolist() == [3]


def test_checker_rejects_what_it_is_there_to_catch():
    """the comparison of the GPU tests fails on: a survivor swapped for its tied neighbour where the contract fixes the
    order, a probability 8 ulps off on a small entry, a token equal to the runner-up"""
    c = next(c for c in S.cells() if c.tags[:1] == ("tie-block",))
    w = c.warp()
    got_p = w.probs.astype(np.float32)
    assert R.compare_kept(w.ids, w.probs, w.D, len(w.ids), 1, w.ids, got_p, ordered=True)[0] == []
    dropped = np.setdiff1d(w.topp_tied, w.ids)             # the tied ids the positional cut removed
    assert dropped.size == 3
    swapped = w.ids.copy()
    swapped[-1] = dropped[0]                               # same score, same probability, the higher id
    assert R.compare_kept(w.ids, w.probs, w.D, len(w.ids), 1, swapped, got_p, ordered=True)[0]
    assert R.compare_kept(w.ids, w.probs, w.D, len(w.ids), 2, swapped, got_p, ordered=False)[0]
    two = w.ids.copy()
    two[[8, 9]] = two[[9, 8]]                              # two tied survivors in the wrong order
    assert R.compare_kept(w.ids, w.probs, w.D, len(w.ids), 1, two, got_p, ordered=True)[0]
    assert R.compare_kept(w.ids, w.probs, w.D, len(w.ids), 2, two, got_p, ordered=False)[0] == []
    # 8 ulps on the smallest probability of the survivors. The bound is about (D + ln m + m + 4) u on path 1 and
    # (D + ln m + 7) u on path 2, and 8 ulps are between 8 u and 16 u of the value (16 u just above a power of two): a row
    # of few survivors whose smallest probability sits just above a power of two, so that both paths' bounds are below it
    for path in (1, 2):
        for t in np.arange(-3.0, -2.0, 1.0 / 128):
            x = np.full(64, -30.0, np.float32)
            x[[5, 17, 40]] = [4.0, 2.0, t]
            w = R.warp(x, 1.0, 3, 1.0)
            got_p = w.probs.astype(np.float32)
            if np.frexp(got_p[2])[0] < 0.55:
                break
        assert got_p[2] < 1e-2 * got_p[0] and np.frexp(got_p[2])[0] < 0.55
        assert R.compare_kept(w.ids, w.probs, w.D, 3, path, w.ids, got_p, ordered=path == 1)[0] == []
        for d in (8, -8):
            off = got_p.copy()
            off[2:3] = (off[2:3].view(np.int32) + d).view(np.float32)
            bad, worst = R.compare_kept(w.ids, w.probs, w.D, 3, path, w.ids, off, ordered=path == 1)
            assert bad and 1.0 < worst < 2.0, (path, worst)
        assert abs(float(off[2]) - float(got_p[2])) < 1e-8 * got_p[0], "a norm over the row would not have noticed"
        nan = got_p.copy()
        nan[1] = np.nan
        assert R.compare_kept(w.ids, w.probs, w.D, 3, path, w.ids, nan, ordered=path == 1)[0]
    c = next(c for c in S.cells() if c.tags[:3] == ("grid", (20, 4097), 1.0))
    w = c.warp()
    # the runner-up
    q, tok = S.handed_draws(c, 1)
    _, _, b, s = R.pick(w.ids, w.probs, q[w.ids].astype(np.float64))
    assert int(w.ids[b]) == tok and R.compare_token(tok, tok) == [] and R.compare_token(int(w.ids[s]), tok)


def test_every_gpu_row_has_its_margin():
    """exact cells: the top-p cut is at least 100 cumulative-sum error bounds away from every cumulative sum it compares, so
    fp32 and fp64 cut at the same place; the path is what the cell was written for"""
    cells = S.cells() + S.philox_cells()
    assert len({c.label for c in cells}) == len(cells)
    for c in cells:
        assert c.path == S.expected_path(c.n, c.top_k)
        if c.check != "exact":
            continue
        w = c.warp()
        assert w.margin >= R.MARGIN_FACTOR * R.cum_err(w.m0, c.path), (c.label, w.margin)
        if c.tags[0] not in ("tie-block", "topp-ties"):
            assert w.tie_free, c.label
    # the cells are what their names say
    by = {c.label: c for c in cells}
    w = by["topp cut in tie block k14 n4096"].warp()
    assert len(w.topk_above) == 8 and len(w.topk_tied) == 12 and w.hf_count == 17 and len(w.ids_all) == 20
    chunk = 4096 // 64
    assert len({int(i) // chunk for i in w.topk_tied}) >= 10, "the tied block is spread over many slices"
    for lab in ("topp boundary ties k0 n1025", "topp boundary ties k65 n8192"):
        w = by[lab].warp()
        assert w.hf_count == 11 and len(w.ids_all) == 13 and len(w.topp_tied) == 5
    for t in (2, 5, 40):
        c = by[f"topk ties t{t} k20 n4096"]
        w = c.warp()
        per_slice = np.bincount(w.topk_tied // 64, minlength=64)
        assert len(w.topk_tied) == t and len(w.topk_above) == 19 and per_slice.max() <= 20 - 1 and len(w.ids) == 19 + t
        assert len(by[f"topk ties t{t} k20 n1279"].warp().ids) == 19 + t
    for lab in ("signed zero k20 n4096", "signed zero k20 n1279"):
        c = by[lab]
        w = c.warp()
        z = c.logits[w.topk_tied]
        assert len(z) == 4 and np.all(z == 0) and np.signbit(z).sum() == 3 and len(w.ids) == 23
    c = by["prefilter one-slice"]
    assert {int(i) // 64 for i in np.concatenate([c.warp().topk_above, c.warp().topk_tied])} == {5}
    c = by["prefilter slice-maxima"]
    top = np.concatenate([c.warp().topk_above, c.warp().topk_tied])
    assert len({int(i) // 64 for i in top}) == 20 and np.unique(np.delete(c.logits, top)).size == 1
    for lab in ("radix seam top-k k65 n8192", "ulp seam top-k k20 n4097"):
        c = by[lab]
        v = np.sort(c.logits)[::-1]
        a, b = v[c.top_k - 1:c.top_k + 1].view(np.uint32)
        assert a - b == 1 and a >> 8 == b >> 8
    for lab in ("radix seam top-p n1025", "radix seam top-p n152064"):
        c = by[lab]
        w = c.warp()
        lo = np.sort(c.logits)[::-1][6:8].view(np.uint32)
        assert len(w.ids) == 7 and lo[0] - lo[1] == 2, "the cut falls between two scores 2 ulps apart"
    w = by["limit: > k ties in one slice"].warp()
    assert len({int(i) // 64 for i in w.topk_tied}) == 1 and len(w.topk_tied) == 30
    w = by["limit: > 1024 kept"].warp()
    assert len(w.ids) > 1024
    a, b = by["both paths k64 n4160"], by["both paths k65 n4160"]
    assert a.path == 1 and b.path == 2 and a.logits is b.logits and b.warp().ids[:64].tolist() == a.warp().ids.tolist() and len(b.warp().ids) == 65


def test_philox_rows_leave_out_at_most_one_percent():
    """which (row, seed, offset) draws the device comparison leaves out is decided here, from the reference: those whose
    best / second-best score gap is inside the derived error of p / q on the device. At most 1 % per row; and the rows see
    the high words of seed and offset (swapping the two, or taking 2^32 off an offset, changes tokens)"""
    pairs = S.philox_pairs()
    assert len(pairs) == 256 and len(set(pairs)) == 256
    assert any(s >> 32 for s, _ in pairs) and {0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 40} <= {o for _, o in pairs}
    assert sum(1 for (s0, o0), (s1, o1) in zip(pairs, pairs[1:]) if s0 == s1 and o1 == o0 + 1) >= 100
    cells = S.philox_cells()
    assert sorted((c.path, c.tags[1]) for c in cells) == [(1, "flat"), (1, "peaked"), (2, "flat"), (2, "peaked")]
    for c in cells:
        w = c.warp()
        assert w.tie_free
        if c.tags[1] == "flat":
            assert 12 <= len(w.ids) <= 18, (c.label, len(w.ids))
        toks, safe = S.philox_expect(c, pairs)
        assert np.count_nonzero(~safe) <= 0.01 * len(pairs), (c.label, int(np.count_nonzero(~safe)))
        swapped = S.philox_expect(c, [(o, s) for s, o in pairs])[0]
        high = [i for i, (_, o) in enumerate(pairs) if o >= 1 << 32]
        lowered = S.philox_expect(c, [(pairs[i][0], pairs[i][1] - (1 << 32)) for i in high])[0]
        if c.tags[1] == "flat":
            assert np.count_nonzero(swapped != toks) > 64 and np.count_nonzero(lowered != toks[high]) > len(high) // 4, c.label
        assert len(set(toks.tolist())) >= (8 if c.tags[1] == "flat" else 2)


def test_score_margin_near_u_equal_one():
    """-logf against -log where u -> 1: the smallest nonzero draw is 2^-24 and the absolute 2^-26 allowance is a quarter of
    it, so such a draw is never called safe on a near tie; a draw of exactly 0 (u == 1) gives an infinite score on both
    sides and wins by the lower id"""
    assert R.device_draw(0, 0, np.array([0]))[0] > 0
    q = np.array([2.0 ** -24, 2.0 ** -24 * 1.2], np.float64)
    assert not R.draw_is_safe(np.zeros(2), 2, 1, np.array([0.5, 0.5]), q, device=True)
    assert R.draw_is_safe(np.zeros(2), 2, 1, np.array([0.5, 0.5]), q, device=False)
    tok, gap, _, _ = R.pick(np.array([7, 3]), np.array([0.1, 0.9]), np.array([0.0, 0.0]))
    assert tok == 3 and gap == 0.0
