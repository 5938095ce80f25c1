"""The references of tests/rowops_reference.py and the cells of tests/rowops_cells.py, held to account without a GPU: the
references agree with torch on the CPU and with the oracle on generic cells, round_bf16 is torch's conversion, every exact
cell meets its exactness condition, every capped cell meets its cap with the reference alone, every k-means++ cell has its
ratio margin, and the comparisons the GPU file uses reject the errors they are there to catch (and accept the clean result)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import rowops_cells as S
import rowops_reference as R

F32 = np.float32


def _pick(cells, **kw):
    return [c for c in cells if all(getattr(c, k, None) == v or c.p.get(k) == v for k, v in kw.items())]


# ------------------------------------------------------------------------------------------------ bf16
def test_round_bf16_equals_torch_conversion():
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 1 << 32, 400000, dtype=np.uint64).astype(np.uint32)
    mid = (bits[:50000] & 0xFFFF0000) | 0x8000                                     # exact midpoints, both parities
    den = rng.integers(0, 1 << 23, 50000, dtype=np.uint64).astype(np.uint32) | (bits[:50000] & 0x80000000)      # denormals
    special = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0, 0x80000000,
                        0x00008000, 0x00007FFF, 0x00018000, 0x3F808000, 0x3F818000], np.uint32)
    x = np.concatenate([bits, mid, mid + 1, mid - 1, den, special]).view(F32)
    got = R.round_bf16(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert got[~nan].tobytes() == want[~nan].tobytes()
    assert np.all((got.view(np.uint32) & 0xFFFF) == 0)
    assert R.from_bf16_bits(R.bf16_bits(got[~nan])).tobytes() == got[~nan].tobytes()


def test_nearest_bf16_in_fp64():
    rng = np.random.default_rng(2)
    ref = np.concatenate([rng.normal(size=20000) * 10.0 ** rng.integers(-30, 30, 20000), [0.0, 1.0, -1.0, 1e-40, -3e-39]])
    main, other, near = R.nearest_bf16(ref, 0.0)
    assert np.all(np.abs(main - ref) <= np.abs(other - ref))
    assert main.astype(F32).tobytes() == R.round_bf16(main.astype(F32)).tobytes() and np.all(main.astype(F32) == main)
    far = np.abs(np.abs(main - ref) - np.abs(other - ref)) > 1e-6 * np.abs(ref)
    assert np.array_equal(main[far], R.round_bf16(ref.astype(F32))[far].astype(np.float64))
    # exact midpoints go to the even neighbour and count as near for any delta
    lo = R.round_bf16(rng.normal(size=1000).astype(F32)).astype(np.float64)
    hi = R.bf16_bracket(lo * (1 + 1e-9))[1]
    m, o, n = R.nearest_bf16(0.5 * (lo + hi), 0.0)
    assert np.all(n) and np.all((R.bf16_bits(m.astype(F32)) & 1) == 0) and np.all((R.bf16_bits(o.astype(F32)) & 1) == 1)


# ------------------------------------------------------------------------------------------------ cross-checks
@pytest.mark.parametrize("c", [c for c in S.norm_cells() if not c.bf16 and c.p["H"] in (8, 520, 1152, 4096)], ids=lambda c: c.id)
def test_norm_references_agree_with_torch(c):
    x, gamma, beta = S.build_norm(c)
    ref, unit = S.norm_reference(c, x, gamma, beta)
    k, y, _ = R.yardstick_ratio(S.norm_plain(c, x, gamma, beta), ref, ref, unit)
    assert k < 1e-5, (c.id, k)
    y64 = torch.nn.functional.layer_norm(torch.from_numpy(x).double(), (x.shape[1],), torch.from_numpy(gamma).double(),
                                         torch.from_numpy(beta).double(), S.EPS).numpy()
    if c.kernel == "cogs_layernorm":
        assert np.max(np.abs(y64 - ref)) < 1e-12


def test_ln_finalize_reference_is_the_layernorm_statistics():
    c = S.finalize_cells()[3]
    part = S.build_finalize(c)
    ab = R.ln_finalize64(part, c.p["H"], S.EPS)
    rng = np.random.default_rng(c.seed)
    ratio = np.array(S.FIN_RATIOS)[np.arange(c.p["rows"]) % 3]
    x = rng.normal(size=(c.p["rows"], c.p["H"])) + ratio[:, None]
    rstd = 1.0 / np.sqrt(x.var(axis=1) + S.EPS)
    ok = ratio < 30           # at mean / std 30 the fp32 partials themselves move the variance by more than this check allows
    assert np.allclose(ab[ok, 0], rstd[ok], rtol=2e-5) and np.allclose(ab[ok, 1], (-rstd * x.mean(axis=1))[ok], rtol=2e-5, atol=1e-6)


def test_mean_and_cosine_references_agree_with_torch():
    for c in [S.meanrows_cells()[14], S.meanrows_cells()[20]]:
        x = S.build_meanrows(c)
        assert np.allclose(R.mean_rows64(x), S.means_plain(x), rtol=1e-5, atol=1e-6)
        assert np.allclose(R.seq_sum32(x) / x.shape[0], R.mean_rows64(x), rtol=1e-4, atol=1e-5)
    for c in S.fmean_cells()[12:16]:
        x = S.build_fmean(c)
        for f, m in R.frame_mean64(x, c.p["P"], c.p["frames"]).items():
            assert np.allclose(m, S.means_plain(x[f * c.p["P"]:(f + 1) * c.p["P"]]), rtol=1e-5, atol=1e-6)
    for c in S.cosine_cells():
        a, b = S.build_cosine(c)
        assert np.allclose(R.cosine64(a, b), S.cosine_plain(a, b), atol=1e-6)
        if c.p["zero"] == "a":
            assert np.all(R.cosine64(a, b) == 0)


@pytest.mark.parametrize("c", [c for c in S.pix_cells() if not c.bf16 and c.p["extra"] is None and c.p["t"] * c.p["P"] < 200], ids=lambda c: c.id)
def test_mask_reference_agrees_with_the_oracle_in_fp32(c):
    """torch on the CPU in fp32 divides the exact sum by E: the division chain, element for element, with both fixes"""
    from oracle.compress import compression_mask
    pix, minor, _ = S.build_pix(c)
    t, P, E = c.p["t"], c.p["P"], c.p["E"]
    want = compression_mask(torch.from_numpy((pix * R.PIX_UNIT).astype(F32)), torch.tensor([[t, P, 1]]), torch.tensor([1]), ["video"],
                            threshold=c.p["thr"], min_tokens=c.p["min_tokens"],
                            minor_frame_indices=np.flatnonzero(minor).tolist() if minor is not None else None).numpy().astype(np.uint8)
    got = R.pixdiff_mask(pix, t, P, E, c.p["thr"], c.p["min_tokens"], minor, False, mean_by="div")
    assert np.array_equal(got, want), np.flatnonzero(got != want)


def test_kmeans_step_agrees_with_the_oracle(monkeypatch):
    """one assignment and one update of oracle/kmeans.py (exact_distances=True) with its random choices pinned"""
    import oracle.kmeans as ok
    c = S.assign_cells()[2]                                    # T 255, K 5, a tie between clusters 1 and 2
    x, ts, cen, cts, pair = S.build_assign(c)
    T, K = c.p["T"], c.p["K"]
    # the oracle starts from feature ROWS: take rows as centres instead of the cell's free centres
    rows = [S.TIE_ROW, 9, 9, 33, 120]                          # clusters 1 and 2 coincide
    cen, cts = x[rows].copy(), ts[rows].copy()
    draws = iter(rows + [p % T for p in S.POOL])

    class Pinned:
        @staticmethod
        def randint(a, b):
            return next(draws)
    monkeypatch.setattr(ok, "random", Pinned)
    monkeypatch.setattr(torch, "multinomial", lambda p, n: torch.tensor([next(draws)]))
    cf, ct, assign = ok.kmeans_with_time_min_max(torch.from_numpy(x).view(T, 1, -1), torch.from_numpy(ts), K, alpha=2, max_iteration=1,
                                                 exact_distances=True)
    d2 = R.sqdist64(x, cen).astype(F32)
    want, _ = R.assign_fp32(d2, ts, cts, 2.0)
    assert np.array_equal(want, assign.numpy())
    assert not np.any(want == 2) and np.any(want == 1)         # the tie went to the lower cluster, cluster 2 is empty
    empty = [k for k in range(K) if not np.any(want == k)]
    reseed = np.zeros(K, np.int64)
    reseed[empty] = [p % T for p in S.POOL][:len(empty)]
    nc, nct, _ = R.update_ref(x, ts, want, K, reseed, cen, cts)
    assert nc.tobytes() == cf.reshape(K, -1).numpy().tobytes()           # exact sums, one division: bit for bit
    assert np.allclose(nct, ct.numpy(), rtol=1e-6)                       # torch sums the time stamps in another order
    assert np.allclose(R.sqdist_scheme32(x, cen), d2)


# ------------------------------------------------------------------------------------------------ self-checks
def test_status_numbers_come_from_the_header():
    assert S.status_codes() == dict(OK=0, E_INVALID=-1, E_HIP=-2, E_UNSUPPORTED=-3, E_WORKSPACE=-4)


def test_cells_cover_every_listed_value():
    n = S.norm_cells()
    for k in ("cogs_layernorm", "cogs_rmsnorm"):
        for dt in S.DTYPES:
            assert {c.p["H"] for c in n if c.kernel == k and c.dtype == dt} == set(S.NORM_H)
        assert {c.p["rows"] for c in n if c.kernel == k} == set(S.NORM_ROWS)
    assert {S.norm_inst(H) for H in S.NORM_H} == {1, 2, 3, 4, 8}
    m = [c for c in n if c.kernel == "cogs_ln_merge"]
    assert {c.p["group"] for c in m} == {1, 3, 4} and {c.p["out_rows"] for c in m} == {1, 4, 5} and {S.norm_inst(c.p["H"]) for c in m} == {1, 2, 3, 4, 8}
    f = S.finalize_cells()
    assert {c.p["tiles"] for c in f} == {1, 2, 18, 56} and {c.p["rows"] for c in f} == {1, 255, 256, 257}
    p = S.pix_cells()
    assert {c.p["E"] for c in p} >= {8, 512, 520, 2048, 2056, 2352, 4104}
    assert {(c.p["t"], c.p["P"]) for c in p} == {(1, 5), (2, 1), (3, 7), (6, 20), (5, 257)}
    assert {c.p["minor"] for c in p} == {None, "zeros", "frame0", "middle", "last", "quiet"}
    assert {c.p["min_tokens"] - c.p["P"] for c in p if c.p["min_tokens"] > 3} == {2} and {0, 1, 3} <= {c.p["min_tokens"] for c in p}
    for dt in S.DTYPES:
        assert sum(c.p["extra"] is not None for c in p if c.dtype == dt) >= 2
    fm = S.fmean_cells()
    assert {c.p["D"] for c in fm} == {4, 252, 1024, 1028, 3584} and {c.p["P"] for c in fm} == {1, 2, 7, 64}
    g = S.gather_cells()
    assert {c.p["D"] for c in g} == {8, 256, 512, 520, 3584} and {c.p["rows"] for c in g} == {1, 3, 4, 5, 130}
    mr = S.meanrows_cells()
    assert {c.p["D"] for c in mr} == {4, 124, 128, 132, 3584} and {c.p["rows"] for c in mr} == {1, 7, 8, 9, 333} and {c.p["pad"] for c in mr} == {0, 4}
    co = S.cosine_cells()
    assert {c.p["D"] for c in co} == {1, 63, 64, 65, 3584} and {c.p["n"] for c in co} == {1, 6}
    pk = S.pack_cells()
    assert {(c.p["cols_in"], c.p["cols_out"]) for c in pk} >= set(S.PACK_SHAPES) and {(c.p["din"], c.p["dout"]) for c in pk} == set(S.PACK_PAIRS)
    assert {c.p["rows"] for c in pk} >= {1, 3, 300} and any(c.p["rows"] * c.p["cols_out"] // 4 > 4096 * 256 for c in pk)
    sq = [c for c in S.sqdist_cells() if c.p["exact"]]
    for key, vals in (("T", {1, 3, 4, 5, 8, 9, 33, 40}), ("PD", {8, 504, 512, 520, 2568}), ("K", {1, 3, 4, 5, 31, 32, 33, 64, 65, 70})):
        for v in vals:
            assert len({(c.p["T"], c.p["PD"], c.p["K"]) for c in sq if c.p[key] == v}) >= 2, (key, v)
    assert {(c.p["T"], c.p["PD"], c.p["K"]) for c in sq} >= set(S.SQDIST_LONG)
    a = S.assign_cells()
    for key, vals in (("K", {1, 2, 5, 63, 64, 65, 70}), ("T", {1, 40, 255, 256, 257})):
        assert all(sum(c.p[key] == v for c in a) >= 2 for v in vals)
    u = S.update_cells()
    assert {c.p["PD"] for c in u} == {8, 2040, 2048, 2056, 4104} and {c.p["T"] for c in u} == {1, 64, 65, 1025, 16385}
    assert any(set(S.UPDATE_COUNTS) <= set(c.p["counts"]) for c in u)
    k = S.kpp_cells()
    assert {c.p["T"] for c in k} == {1, 2, 255, 256, 257, 600} and {c.p["K"] for c in k} == {1, 2, 6} and {c.p["PD"] for c in k} == {8, 520}
    assert len({c.id for c in S.all_cells()}) == len(S.all_cells())


@pytest.mark.parametrize("c", S.pix_cells(), ids=lambda c: c.id)
def test_mask_cells_are_exact_and_planted_by_the_scan(c):
    """pixel values are multiples of 2^-7 in [-1, 1]; every difference is exact in bf16; every row sum is below 2^13 (2^20 units,
    so any partial sum is exact in fp32). The planted sums come from scanning the chain: the largest that is dropped, the
    smallest that is kept, one step either side"""
    pix, minor, planted = S.build_pix(c)
    t, P, E = c.p["t"], c.p["P"], c.p["E"]
    assert np.abs(pix).max() <= 128
    v = (pix * R.PIX_UNIT).astype(F32)
    assert R.round_bf16(v).tobytes() == v.tobytes()
    p3 = pix.reshape(t, P, E)
    if t > 1:
        d = p3[1:] - p3[:-1]
        dv = (d * R.PIX_UNIT).astype(F32)
        assert R.round_bf16(dv).tobytes() == dv.tobytes()
        assert np.abs(d).sum(axis=2).max() < 1 << 20
    b = R.pixdiff_boundary(E, c.p["thr"], c.bf16)
    assert b >= 1 and not R.pixdiff_chain(b - 1, E, c.p["thr"], c.bf16) and R.pixdiff_chain(b, E, c.p["thr"], c.bf16)
    if t > 1:
        sums = np.abs(p3[1:] - p3[:-1]).sum(axis=2).reshape(-1)
        for row, units in planted.items():
            assert sums[row - P] == units
        want = {u for u in (b - 2, b - 1, b, b + 1) if u >= 0}
        if P >= 5:
            assert want <= set(planted.values())
        else:
            assert set(planted.values()) & want or c.p["extra"] is not None
    if c.p["extra"] is not None:
        u = c.p["extra"]
        assert u in planted.values()
        assert R.pixdiff_chain(u, E, c.p["thr"], c.bf16, "div") != R.pixdiff_chain(u, E, c.p["thr"], c.bf16, "mul")
    if c.p["minor"] == "quiet" and t > 1:
        f = int(np.flatnonzero(minor)[0])
        raw = R.pixdiff_mask(pix, t, P, E, c.p["thr"], 0, None, c.bf16).reshape(t, P)
        assert raw[f].sum() < c.p["min_tokens"] or c.p["min_tokens"] == 0


def test_exact_cells_meet_their_exactness_condition():
    """the largest possible partial sum stays below 2^24 units of the grid the values sit on"""
    for c in S.fmean_cells():
        if c.p["exact"]:
            x, P = S.build_fmean(c), c.p["P"]
            assert P & (P - 1) == 0 and np.all(x == np.round(x)) and np.abs(x).max() * P < 256
    for c in S.meanrows_cells():
        if c.p["exact"]:
            x, n = S.build_meanrows(c), c.p["rows"]
            assert n & (n - 1) == 0 and np.all(x == np.round(x)) and np.abs(x).max() * n < 1 << 24
    for c in S.sqdist_cells():
        if c.p["exact"]:
            x, cen, _ = S.build_sqdist(c)
            assert np.all(x == np.round(x)) and np.all(cen == np.round(cen))
            assert (np.abs(x).max() + np.abs(cen).max()) ** 2 * c.p["PD"] < 1 << 24
    for c in S.assign_cells():
        x, ts, cen, cts, _ = S.build_assign(c)
        assert np.all(x == np.round(x)) and np.all(cen == np.round(cen)) and 64 * c.p["PD"] < 1 << 24 and 4 * c.p["T"] < 1 << 24
    for c in S.update_cells():
        x = S.build_update(c)[0]
        assert np.all(x == np.round(x)) and np.abs(x).max() * c.p["T"] < 1 << 24
    for c in S.kpp_cells():
        x = S.build_kpp(c)[0]
        assert np.all(x == np.round(x)) and 64 * c.p["PD"] < 1 << 24


@pytest.mark.parametrize("c", [c for c in S.norm_cells() if c.bf16], ids=lambda c: c.id)
def test_capped_cells_meet_their_cap_with_the_reference_alone(c):
    """the bf16 nearest to the reference passes its own cell, and at most 1 % of the cell lies within delta of a midpoint"""
    x, gamma, beta = S.build_norm(c)
    ref, unit = S.norm_reference(c, x, gamma, beta)
    delta = S.norm_delta(c, x, gamma, beta)
    assert delta < 1e-4
    if c.kernel == "cogs_layernorm":
        bad, share = R.check_nearest_bf16(R.nearest_bf16(ref, 0.0)[0], ref, delta * unit)
    elif c.kernel == "cogs_rmsnorm":
        inner = R.rmsnorm64(x, gamma, S.EPS)[0]
        got = R.round_bf16((gamma[None, :].astype(np.float64) * R.nearest_bf16(inner, 0.0)[0]).astype(F32))
        bad, share = R.check_rmsnorm_bf16(got, x, gamma, S.EPS, delta)
    else:
        rows = R.nearest_bf16(R.layernorm64(x, gamma, beta, S.EPS)[0], 0.0)[0]
        got = R.nearest_bf16(rows.reshape(-1, c.p["group"], rows.shape[1]).mean(axis=1), 0.0)[0]
        bad, share = R.check_ln_merge_bf16(got, x, gamma, beta, c.p["group"], S.EPS, delta)
    assert not bad and share <= 0.01, (c.id, bad, share)


@pytest.mark.parametrize("c", [c for c in S.fmean_cells() if c.bf16 and not c.p["exact"]], ids=lambda c: c.id)
def test_frame_mean_cap(c):
    x = S.build_fmean(c)
    for f, mean in R.frame_mean64(x, c.p["P"], c.p["frames"]).items():
        bad, share = R.check_nearest_bf16(R.nearest_bf16(mean, 0.0)[0], mean, 2.0 * np.spacing(np.abs(mean).astype(F32)).astype(np.float64))
        assert not bad and share <= 0.01


@pytest.mark.parametrize("c", S.kpp_cells(), ids=lambda c: c.id)
def test_kpp_cells_have_their_ratio_margin(c):
    x, first, q = S.build_kpp(c)
    idx, zero, gaps, holders = S.kpp_reference(x, first, q, c.p["K"])
    assert all(g > 1e-5 for g in gaps), gaps
    assert zero == (c.p["kind"] == "zero")
    if c.p["kind"] == "tie":
        a, b = S.KPP_TIE
        assert holders[0] == [a, b] and idx[1] == a and a // 64 != b // 64 and a % 256 != b % 256
        assert all(len(h) == 1 for h in holders[1:])
    else:
        assert all(len(h) == 1 for h in holders)
    if not zero:
        assert len(idx) == c.p["K"]


def test_workspace_formula_has_a_tight_shape():
    T, PD, K = S.tight_ws_shape()
    assert S.kmeans_ws_bytes(T, PD, K) % 256 == 0 and PD % 8 == 0 and 1 <= K <= T


def test_tie_and_degenerate_assign_cells():
    for c in S.assign_cells():
        x, ts, cen, cts, pair = S.build_assign(c)
        d2 = R.sqdist64(x, cen).astype(F32)
        a, fin = R.assign_fp32(d2, ts, cts, c.p["alpha"])
        kind = c.p["kind"]
        if pair is not None:
            assert fin[S.TIE_ROW, pair[0]] == fin[S.TIE_ROW, pair[1]] == 0 and a[S.TIE_ROW] == pair[0]
            assert (pair[1] - pair[0]) % 64 == 0 if kind == "tie-same-lane" else (pair[1] - pair[0]) % 64 != 0
        if kind == "both0":
            assert np.all(fin == 0) and np.all(a == 0)
        if kind == "nf0":
            assert np.all(d2 == d2[:, :1])
        if kind == "nt0":
            assert np.all(cts == cts[0])
    # a NaN row with equal centre times: both normalised distances are 0, cluster 0; alpha = NaN: no final distance compares, cluster 0
    c = next(c for c in S.assign_cells() if c.p["kind"] == "nt0" and c.p["K"] == 64)
    x, ts, cen, cts, _ = S.build_assign(c)
    d2 = R.sqdist64(x, cen).astype(F32)
    assert np.any(R.assign_fp32(d2, ts, cts, 2.0)[0] != 0)
    d2[7] = np.nan
    assert R.assign_fp32(d2, ts, cts, 2.0)[0][7] == 0
    assert np.all(R.assign_fp32(d2, ts, cts + np.arange(64, dtype=F32), float("nan"))[0] == 0)
    x, ts, cen, cts = S.build_margin()
    d2 = R.sqdist64(x, cen).astype(F32)
    m = [R.margin64(d2, ts, cts, 2.0, t) for t in range(x.shape[0])]
    assert m[5] == min(m) and 0 < m[5] < 1e-3 and sorted(m)[1] > 1e-3


# ------------------------------------------------------------------------------------------------ mutation checks
def test_mutation_one_element_of_the_last_chunk_left_unnormalised():
    for c in (_pick(S.norm_cells(), kernel="cogs_layernorm", dtype="f32", H=520)[0], _pick(S.norm_cells(), kernel="cogs_layernorm", dtype="bf16", H=520)[0]):
        x, gamma, beta = S.build_norm(c)
        ref, unit = S.norm_reference(c, x, gamma, beta)
        plain = S.norm_plain(c, x, gamma, beta)
        clean = plain if not c.bf16 else R.nearest_bf16(ref, 0.0)[0].astype(F32)
        bad = clean.copy()
        bad[-1, -3] = x[-1, -3]                                          # one element of chunk 64, the only chunk of the last group
        if not c.bf16:
            assert R.yardstick_ratio(clean, plain, ref, unit)[2] <= R.FACTOR
            assert R.yardstick_ratio(bad, plain, ref, unit)[2] > R.FACTOR
        else:
            d = S.norm_delta(c, x, gamma, beta) * unit
            assert not R.check_nearest_bf16(clean, ref, d)[0] and R.check_nearest_bf16(bad, ref, d)[0]


def test_mutation_missing_inner_rounding_in_rmsnorm():
    c = _pick(S.norm_cells(), kernel="cogs_rmsnorm", dtype="bf16", H=1152)[0]
    x, gamma, beta = S.build_norm(c)
    inner = R.rmsnorm64(x, gamma, S.EPS)[0]
    delta = S.norm_delta(c, x, gamma, beta)
    two = R.round_bf16((gamma[None, :].astype(np.float64) * R.nearest_bf16(inner, 0.0)[0]).astype(F32))
    one = R.round_bf16((gamma[None, :].astype(np.float64) * inner).astype(F32))              # gamma * (x rstd) rounded once
    assert np.mean(one != two) > 0.01
    assert not R.check_rmsnorm_bf16(two, x, gamma, S.EPS, delta)[0]
    assert R.check_rmsnorm_bf16(one, x, gamma, S.EPS, delta)[0]


def test_mutation_mask_bit_flipped_on_a_threshold_row():
    c = _pick(S.pix_cells(), dtype="bf16", E=2352, minor=None, min_tokens=1)[0]
    pix, minor, planted = S.build_pix(c)
    ref = R.pixdiff_mask(pix, c.p["t"], c.p["P"], c.p["E"], c.p["thr"], c.p["min_tokens"], minor, True)
    assert R.mismatch(ref.copy(), ref).size == 0
    for row in planted:
        got = ref.copy()
        got[row] ^= 1
        assert R.mismatch(got, ref).tolist() == [[row]]


def test_mutation_padding_left_as_tracer():
    c = _pick(S.pack_cells(), cols_in=588, cols_out=640, dout="bf16")[0]
    x = S.build_pack(c)
    want = R.bf16_bits(R.pack_rows(x, 640, True))
    assert R.mismatch(want.copy(), want).size == 0
    got = want.copy()
    got[0, 639] = 0x7FC5
    assert R.mismatch(got, want).tolist() == [[0, 639]]
    got = want.copy()
    got[:, 588:] = 0x8000                                                # -0.0 is not +0.0 either
    assert len(R.mismatch(got, want)) == x.shape[0] * 52


def test_mutation_one_member_dropped_from_a_cluster_mean():
    c = S.update_cells()[1]
    x, ts, assign, reseed, old_c, old_ct = S.build_update(c)
    K = c.p["K"]
    nc, nct, shift = R.update_ref(x, ts, assign, K, reseed, old_c, old_ct)
    assert R.mismatch(nc.copy(), nc).size == 0
    for k, n in enumerate(c.p["counts"]):
        if n >= 2:
            bc, bct, _ = R.update_ref(x, ts, assign, K, reseed, old_c, old_ct, drop=(k, n - 1))
            assert len(R.mismatch(bc, nc)) > 0 and set(R.mismatch(bc, nc)[:, 0].tolist()) == {k}
            assert R.mismatch(bct, nct).tolist() == [[k]]


def test_mutation_second_of_two_tied_clusters_chosen():
    for c in (S.assign_cells()[2], S.assign_cells()[5]):
        x, ts, cen, cts, pair = S.build_assign(c)
        want, _ = R.assign_fp32(R.sqdist64(x, cen).astype(F32), ts, cts, c.p["alpha"])
        assert R.mismatch(want.copy(), want).size == 0
        got = want.copy()
        got[S.TIE_ROW] = pair[1]
        assert R.mismatch(got, want).tolist() == [[S.TIE_ROW]]
