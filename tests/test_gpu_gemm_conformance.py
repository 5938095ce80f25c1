"""cogs_gemm conformance: every kernel body x epilogue x shape edge x layout against an fp64 reference of the same
operation, element by element (tests/gemm_reference.py holds the reference and the derivation of the tolerance).

Each cell forces its body with debug switches only, asserts which body ran (cogs_debug_get("gemm_last_body"): 1 128x128,
2 256x128 persistent ring, 3 K-tile ping-pong, 4 whole-line ping-pong, 5 ping-pong + ring split, 6 GEMV), and records the
(body, epilogue) pair it reached; the last test asserts that a required list of pairs was reached, so a dispatcher change
that reroutes a cell fails here instead of passing on other evidence. Every output buffer is a view into a larger buffer
filled with a finite tracer pattern, compared bit for bit afterwards (finite, like the attention guard tests: a NaN
tracer would depend on NaN semantics that the -fno-honor-nans builds do not keep): the elements outside the output must
keep their bits."""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import pytest
import torch

import gemm_reference as R
import gemv_reference as G

BF16, F32 = torch.bfloat16, torch.float32
TRACE16, TRACE32 = 0x7F7F, 0x7F7F7F7F        # bf16 3.39e38 / fp32 3.39e38: finite, far outside any result
HD_VIT, HD_QWEN = 72, 128

# masks of csrc/gemm_epilogue.h (mirrored to name what a cell reached)
EPI_BIAS, EPI_RES, EPI_ROPE, EPI_GELU_TANH, EPI_GELU_ERF, EPI_SWIGLU, EPI_F32OUT = 1, 2, 4, 8, 16, 32, 64
EPI_ROWSTAT, EPI_LNFOLD, EPI_HM = 1024, 2048, 4096
SPECIALISED = {
    0: "plain", EPI_BIAS: "bias", EPI_RES: "res", EPI_BIAS | EPI_RES: "bias+res", EPI_BIAS | EPI_ROPE: "bias+rope",
    EPI_BIAS | EPI_GELU_TANH: "bias+gelu_tanh", EPI_BIAS | EPI_GELU_ERF: "bias+gelu_erf", EPI_SWIGLU: "swiglu",
    EPI_F32OUT: "f32out", EPI_BIAS | EPI_ROWSTAT: "bias+rowstat", EPI_BIAS | EPI_RES | EPI_ROWSTAT: "bias+res+rowstat",
    EPI_BIAS | EPI_LNFOLD: "lnfold", EPI_BIAS | EPI_ROPE | EPI_LNFOLD: "lnfold+rope",
    EPI_BIAS | EPI_GELU_TANH | EPI_LNFOLD: "lnfold+gelu_tanh", EPI_BIAS | EPI_ROPE | EPI_HM: "bias+rope+hm",
    EPI_BIAS | EPI_ROPE | EPI_LNFOLD | EPI_HM: "lnfold+rope+hm",
}

# (body, what) pairs the cells below reached; test_zz_required_coverage checks them against REQUIRED
REACHED: set = set()
REQUIRED = (
    [(b, e) for b in (1, 2, 4, 5, 6) for e in ("bias+res", "bias+res in place", "bias+rope", "bias+gelu_tanh", "generic")]
    + [(2, "ring > 256 tiles"), (2, "ring > 256 tiles swiglu"), (2, "swiglu"), (2, "bias+rope sep_sin > 256 tiles"),
       (3, "bias+rope lut"), (3, "bias+res"),
       (4, "tall"), (4, "bias+rowstat"), (4, "bias+res+rowstat"), (4, "lnfold"), (4, "lnfold+rope"), (4, "lnfold+gelu_tanh"),
       (4, "bias+rope+hm"), (4, "lnfold+rope+hm"), (4, "swiglu"),
       (5, "bias+res+rowstat"), (5, "lnfold+rope+hm"), (5, "bias+rope sep_sin"), (5, "lnfold"),
       (1, "ldc%8==4"), (2, "ldc%8==4"), (4, "ldc%8==4"), (5, "ldc%8==4"), (6, "ldc%8==4")]
    + [(b, "exact " + e) for b in (1, 2, 4) for e in ("plain", "bias", "res", "bias+res", "f32out", "bias+rope+hm", "rope swap")]
    + [(b, SPECIALISED[m]) for b in (1, 2) for m in SPECIALISED]
    + [(b, e + q) for b in (1, 2, 4, 5) for e in ("bias+rope", "bias+rope sep_sin", "lnfold+rope", "bias+rope+hm", "lnfold+rope+hm")
       for q in (" q_scale on a tile boundary", " q_scale straddling a tile")]
    + [(3, e + q) for e in ("bias+rope lut", "lnfold+rope lut") for q in (" q_scale on a tile boundary", " q_scale straddling a tile")]
    + [(6, e) for e in ("plain", "bias", "res", "bias+rope", "bias+rope sep_sin", "bias+gelu_tanh", "bias+gelu_erf", "swiglu",
                        "f32out", "gemv small_n", "gemv big_n", "gemv dot2=0")]
)


def _L():
    from cogstream_amd import _lib
    return _lib


def epi_mask(*, bias, res, rope, act, out_f32, stats, ln, hm) -> int:
    """cogs_epi_mask of include/cogs.h's descriptor (csrc/gemm_epilogue.h), or -1 for EPI_GENERIC"""
    m = (EPI_ROWSTAT if stats else 0) | (EPI_LNFOLD | EPI_BIAS if ln else 0) | (EPI_BIAS if bias else 0)
    m |= (EPI_RES if res else 0) | (EPI_ROPE if rope else 0) | (EPI_F32OUT if out_f32 else 0) | (EPI_HM if hm else 0)
    m |= {R.ACT_NONE: 0, R.ACT_GELU_TANH: EPI_GELU_TANH, R.ACT_GELU_ERF: EPI_GELU_ERF, R.ACT_SWIGLU: EPI_SWIGLU}[act]
    return m if m in SPECIALISED else -1


@contextlib.contextmanager
def switches(**kw):
    L = _L()
    kw.setdefault("gemm_co_streams", 1)        # cogs_gemm always plans for one stream (CogsGemm::co_streams); pinned so that an override left set cannot reroute a cell
    with contextlib.ExitStack() as st:
        for k, v in kw.items():
            st.enter_context(L.debug_switch(k, v))
        yield


# ----------------------------------------------------------------------------------------------------------- data
_cache: dict = {}


def _operands(dev, M, N, K, dtype, exact, seed):
    """A [M, K], W [N, K] (bf16 / fp32, device) and their fp64 product and bound; the last few are cached (the large
    shapes serve several epilogues)"""
    key = (M, N, K, dtype, exact, seed)
    if key in _cache:
        return _cache[key]
    if len(_cache) >= 3:
        _cache.pop(next(iter(_cache)))
    g = torch.Generator(device=dev).manual_seed(seed)
    if exact:
        # small integers: every product sum, bias and residual is exact in fp32 and in bf16 (|y| < 256)
        a = torch.randint(-2, 3, (M, K), generator=g, device=dev).to(dtype)
        keep = torch.rand(N, K, generator=g, device=dev) < min(1.0, 24.0 / K)
        w = (torch.randint(-1, 2, (N, K), generator=g, device=dev) * keep).to(dtype)
    else:
        a = (torch.randn(M, K, generator=g, device=dev) * 0.7 + 0.1).to(dtype)
        w = (torch.randn(N, K, generator=g, device=dev) / math.sqrt(K)).to(dtype)
    acc, bound = R.product_and_bound(a, w)
    _cache[key] = (a, w, acc, bound, g)
    return _cache[key]


def _filled(n, dtype, dev):
    if dtype == F32:
        return torch.full((n,), TRACE32, dtype=torch.int32, device=dev).view(F32)
    return torch.full((n,), TRACE16, dtype=torch.int16, device=dev).view(dtype)


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


def _rope_tables(dev, g, M, hd, form):
    """(cos, sin) fp64 [M, hd/2] for the reference and the kernel's arguments"""
    if form in ("swap", "swap_sep"):
        # cos = 0, sin = +-1: the rotation is an exact signed swap of the pair, so a wrong pairing or another row's factors
        # give wrong bits
        cos = torch.zeros(M, hd // 2, device=dev)
        sin = torch.randint(0, 2, (M, hd // 2), generator=g, device=dev).float() * 2 - 1
        lut = rowpos = None
    elif form == "lut":
        nf, maxpos = hd // 4, 45
        inv = 1.0 / (10000.0 ** (torch.arange(nf, dtype=torch.float32, device=dev) / nf))
        ang = torch.arange(maxpos, dtype=torch.float32, device=dev)[:, None] * inv[None, :]
        lut = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
        hpos = torch.randint(0, 23, (M,), generator=g, device=dev)
        wpos = torch.randint(0, maxpos, (M,), generator=g, device=dev)
        rowpos = (hpos | (wpos << 16)).to(torch.int32)
        tab = torch.cat([lut[hpos], lut[wpos]], 1)
        cos, sin = tab[..., 0].contiguous(), tab[..., 1].contiguous()
    else:
        ang = torch.rand(M, hd // 2, generator=g, device=dev) * 6.0
        cos, sin = ang.cos(), ang.sin()
        lut = rowpos = None
    kw = {}
    if form in ("sep", "swap_sep"):
        kw["rope_cos"], kw["rope_sin"] = cos.contiguous(), sin.contiguous()
    else:
        kw["rope_cos"], kw["rope_sin"] = torch.stack([cos, sin], -1).contiguous(), None
    if form == "lut":
        kw["rope_lut"], kw["rope_rowpos"] = lut, rowpos
    return cos, sin, kw


# ----------------------------------------------------------------------------------------------------------- one cell
def run_cell(dev, body, M, N, K, *, dtype=BF16, bias=False, res=None, act=R.ACT_NONE, out_f32=False, rope=None,
             hd=HD_VIT, rope_cols=None, ln=False, stats=False, hm=False, lda_pad=0, ldc_pad=0, c_off=0, ldr_pad=0,
             exact=False, seed=1, tags=(), also_wgs0=False, q_cols=0, **sw):
    """One GEMM through the C ABI with the given epilogue and layout; asserts the body, the values of every output element
    against fp64, the CPU fp64 spot check of a few rows, and the guard bands. res: None | "sep" | "inplace".
    rope: None | "inter" | "sep" | "lut" | "swap" | "swap_sep". q_cols > 0: through cogs_gemm_fused, with the model's q_scale for
    head_dim hd on the columns below it. Returns the output [M, N or N/2] (fp32 / bf16)."""
    L = _L()
    a, w, acc, bound, g = _operands(dev, M, N, K, dtype, exact, seed)
    swiglu = act == R.ACT_SWIGLU
    ocols = N // 2 if swiglu else N
    odt = F32 if (out_f32 or dtype == F32) else dtype
    d = L.GemmDesc()
    d.dtype = L.dtype_code(dtype)
    d.M, d.N, d.K, d.act, d.out_f32 = M, N, K, act, int(out_f32)
    keep = []                                                             # device buffers the descriptor points into
    # A: optionally a column view of a wider buffer (lda > K)
    if lda_pad:
        abuf = torch.zeros(M, K + lda_pad, dtype=dtype, device=dev)
        abuf[:, :K] = a
        a_in = abuf[:, :K]
    else:
        a_in = a
    d.A, d.lda, d.W, d.ldw = a_in.data_ptr(), a_in.stride(0), w.data_ptr(), w.stride(0)
    bias_t = col_c = rstd = None
    if bias:
        bias_t = (torch.randint(-3, 4, (N,), generator=g, device=dev) if exact else torch.randn(N, generator=g, device=dev)).to(dtype)
        d.bias = bias_t.data_ptr()
    if ln:
        rstd = torch.rand(M, generator=g, device=dev) * 1.5 + 0.5
        ln_ab = torch.stack([rstd, torch.full_like(rstd, 1e30)], 1).contiguous()        # [r][1] is not read
        col_c = torch.randn(N, generator=g, device=dev)
        keep += [ln_ab, col_c]
        d.ln_ab, d.col_c = ln_ab.data_ptr(), col_c.data_ptr()
    # C: row-major view into a buffer with one guard row above and below, ldc = ocols + ldc_pad, first column c_off; or
    # head-major [3][heads][hm_rows][hd] with hm_rows = M + 40, inside a buffer with 64 guard elements on each side
    hm_rows = M + 40
    if hm:
        hm_cols = N // 3
        heads = hm_cols // hd
        cbuf = _filled(64 + N * hm_rows + 64, odt, dev)
        d.C, d.ldc, d.hm_rows, d.hm_cols = cbuf[64:].data_ptr(), N, hm_rows, hm_cols
        inside = torch.zeros(cbuf.numel(), dtype=torch.bool, device=dev)
        inside[64:64 + N * hm_rows].view(3, heads, hm_rows, hd)[:, :, :M] = True
        out_view = lambda: cbuf[64:64 + N * hm_rows].view(3, heads, hm_rows, hd)[:, :, :M].permute(2, 0, 1, 3).reshape(M, N)
    else:
        ldc = ocols + ldc_pad
        assert c_off <= ldc_pad
        cbuf = _filled(64 + M * ldc + ldc + 64, odt, dev)
        cview = cbuf[64 + c_off:].as_strided((M, ocols), (ldc, 1))
        d.C, d.ldc = cview.data_ptr(), ldc
        inside = torch.zeros(cbuf.numel(), dtype=torch.bool, device=dev)
        inside[64 + c_off:].as_strided((M, ocols), (ldc, 1)).fill_(True)
        out_view = lambda: cview
    guard_before = _bits(cbuf)[~inside].clone()
    res_t = None
    if res is not None:
        res_t = (torch.randint(-4, 5, (M, N), generator=g, device=dev) if exact else torch.randn(M, N, generator=g, device=dev)).to(dtype)
        if res == "inplace":
            assert not hm and odt == dtype
            cview.copy_(res_t)
            d.residual, d.ldr = cview.data_ptr(), d.ldc
        else:
            ldr = N + ldr_pad
            rbuf = torch.zeros(M * ldr + 8, dtype=dtype, device=dev)
            rview = rbuf[4 if ldr_pad % 8 == 4 else 0:].as_strided((M, N), (ldr, 1))
            rview.copy_(res_t)
            keep.append(rbuf)
            d.residual, d.ldr = rview.data_ptr(), ldr
    cos = sin = None
    if rope is not None:
        rope_cols = rope_cols if rope_cols is not None else 2 * N // 3
        cos, sin, rkw = _rope_tables(dev, g, M, hd, rope)
        keep += [t for t in rkw.values() if t is not None]
        d.rope_cos, d.rope_sin = rkw["rope_cos"].data_ptr(), L.ptr(rkw["rope_sin"])
        d.rope_cols, d.head_dim = rope_cols, hd
        if "rope_lut" in rkw:
            d.rope_lut, d.rope_rowpos, d.rope_maxpos = rkw["rope_lut"].data_ptr(), rkw["rope_rowpos"].data_ptr(), rkw["rope_lut"].shape[0]
    elif hm:
        d.head_dim = hd
    sbuf = None
    if stats:
        sbuf = _filled((M + 8) * (N // 64) * 2, F32, dev)
        d.row_stats = sbuf.data_ptr()
    q_scale = G.model_q_scale(hd) if q_cols else None
    fused = L.GemmFusedArgs()
    if q_cols:
        fused.q_scale, fused.q_cols = q_scale, q_cols

    def launch():
        if q_cols:
            return L.lib.cogs_gemm_fused(L.current_stream(), C.byref(d), C.byref(fused))
        return L.lib.cogs_gemm(L.current_stream(), C.byref(d))

    with switches(**sw):
        L.debug_set("gemm_choice", 0)
        st = launch()
        got_body = L.debug_get("gemm_last_body")
        torch.cuda.synchronize()
    mask = epi_mask(bias=bias, res=res is not None, rope=rope is not None, act=act, out_f32=out_f32, stats=stats, ln=ln, hm=hm)
    what = (f"body {body} M={M} N={N} K={K} {str(dtype)[6:]} mask {SPECIALISED.get(mask, 'generic')} rope={rope} "
            f"q_cols={q_cols} res={res} lda_pad={lda_pad} ldc_pad={ldc_pad} c_off={c_off} ldr_pad={ldr_pad} {sw}")
    assert st == L.OK, (what, st)
    assert got_body == body, f"{what}: ran body {got_body}"
    out = out_view().clone()
    # values: fp64 reference on the device
    rope_ref = R.Rope(cos, sin, d.rope_cols, hd) if rope is not None else None
    ref, tol = R.epilogue(acc, bound, bias=bias_t, rstd=rstd, col_c=col_c, rope=rope_ref, q_scale=q_scale, q_cols=q_cols, act=act,
                          residual=res_t, out_f32=out_f32, out_dtype=odt)
    if exact:
        bad = out.double() != ref
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ from the exact result"
    else:
        R.assert_within(out, ref, tol, what)
    # the yardstick itself: a CPU fp64 recomputation of a few rows on a few aligned column groups
    _cpu_spot_check(out, a, w, rows=sorted({0, M - 1, M // 2, (7 * M) // 9}), N=N, bias=bias_t, rstd=rstd, col_c=col_c,
                    rope=rope_ref, q_scale=q_scale, q_cols=q_cols, act=act, residual=res_t, out_f32=out_f32, odt=odt, what=what)
    # guard bands: nothing outside the output changed
    after = _bits(cbuf)[~inside]
    assert torch.equal(after, guard_before), f"{what}: {int((after != guard_before).sum())} elements written outside C"
    if stats:
        sv = sbuf.view(M + 8, N // 64, 2)
        sref, stol = R.row_stats_reference(out)
        R.assert_within(sv[:M], sref, stol, what + " row_stats")
        assert torch.equal(_bits(sv[M:]), torch.full_like(_bits(sv[M:]), TRACE32)), f"{what}: row_stats written past row M"
    if also_wgs0:
        # the persistent walk (a workgroup's second and later tiles, the K-slab ring across tile boundaries) against one
        # tile per workgroup: the same tile arithmetic, so the same bits
        cbuf2 = cbuf.clone()
        if res == "inplace":
            cview.copy_(res_t)
        with switches(gemm_wgs=0, **sw):
            assert launch() == L.OK
            assert L.debug_get("gemm_last_body") == body
        torch.cuda.synchronize()
        assert torch.equal(_bits(cbuf), _bits(cbuf2)), f"{what}: persistent walk != one tile per workgroup"
    del keep
    label = "generic" if mask < 0 else SPECIALISED[mask]
    if rope == "sep":
        label += " sep_sin"
    if rope == "lut":
        label += " lut"
    if q_cols:
        label += " q_scale on a tile boundary" if q_cols % 64 == 0 else " q_scale straddling a tile"
    reached = {label}
    if res == "inplace":
        reached.add(label + " in place")
    if exact:
        reached.add("exact " + ("rope swap" if rope in ("swap", "swap_sep") and not hm else label))
    if not hm and odt == BF16 and d.ldc % 8 == 4:
        reached.add("ldc%8==4")
    if body == 2 and M >= 512 and sw.get("gemm_wgs", 256) > 0 and ((M + 255) // 256) * ((N + 127) // 128) > 256:
        reached |= {"ring > 256 tiles", f"ring > 256 tiles {'swiglu' if swiglu else ''}".strip(), label + " > 256 tiles"}
    if body == 4 and sw.get("gemm_tall", 1) and K >= 128 and N > 256 and 0 < N % 256 <= 128:
        reached.add("tall")
    reached |= set(tags)
    REACHED.update((body, r) for r in reached)
    return out


def _cpu_spot_check(out, a, w, *, rows, N, bias, rstd, col_c, rope, act, residual, out_f32, odt, what, q_scale=None, q_cols=0):
    gen = torch.Generator().manual_seed(N)
    groups = sorted({0, N // 4 - 1, (N // 2) // 4, N // 4 - 1 if N >= 8 else 0,
                     *torch.randint(0, N // 4, (6,), generator=gen).tolist(), *[min(c // 4, N // 4 - 1) for c in (124, 128, 252, 256)],
                     *([min(max(q_cols // 4 + k, 0), N // 4 - 1) for k in (-1, 0)] if q_cols else [])})
    cols = torch.tensor([4 * gi + j for gi in groups for j in range(4)])
    r = torch.tensor(rows)
    ac = a[r].cpu().double()
    wc = w[cols.to(w.device)].cpu().double()
    K = a.shape[1]
    acc = ac @ wc.t()
    bound = (ac.abs() @ wc.abs().t()) * (K * 2.0 ** -23)
    rope_c = None
    if rope is not None:
        rope_c = R.Rope(rope.cos[r.to(rope.cos.device)].cpu(), rope.sin[r.to(rope.sin.device)].cpu(), rope.cols, rope.head_dim)
    ref, tol = R.epilogue(acc, bound, cols=cols, bias=None if bias is None else bias.cpu(),
                          rstd=None if rstd is None else rstd[r.to(rstd.device)].cpu(),
                          col_c=None if col_c is None else col_c.cpu(), rope=rope_c, q_scale=q_scale, q_cols=q_cols, act=act,
                          residual=None if residual is None else residual[r.to(residual.device)][:, cols.to(residual.device)].cpu(),
                          out_f32=out_f32, out_dtype=odt)
    ocols = cols[0::2] // 2 if act == R.ACT_SWIGLU else cols
    got = out[r.to(out.device)][:, ocols.to(out.device)].cpu()
    R.assert_within(got, ref, tol, what + " (CPU fp64 spot check)")


# ----------------------------------------------------------------------------------------------------------- the checker (CPU)
def test_checker_rejects_a_few_ulp_error_on_a_small_element():
    """the per-element band accepts an fp32-accumulated, bf16-rounded result and rejects one small-magnitude element moved
    by three output ulps -- which the suite's max-normalised rel_err (< 1.2e-2) lets through"""
    from conftest import rel_err
    torch.manual_seed(0)
    M, N, K = 64, 96, 128
    a = torch.randn(M, K).bfloat16()
    w = (torch.randn(N, K) / math.sqrt(K)).bfloat16()
    b = torch.randn(N).bfloat16()
    r = (torch.randn(M, N) * 4).bfloat16()
    acc, bound = R.product_and_bound(a, w)
    ang = torch.rand(M, 8) * 6
    rope = R.Rope(ang.cos().double(), ang.sin().double(), 32, 16)
    for kw in (dict(bias=b, residual=r), dict(bias=b, rope=rope), dict(bias=b, act=R.ACT_GELU_TANH),
               dict(act=R.ACT_SWIGLU), dict(rstd=torch.rand(M) + 0.5, col_c=torch.randn(N), rope=rope)):
        ref, tol = R.epilogue(acc, bound, **kw)
        # a correct kernel: fp32 accumulation, epilogue in fp32, one rounding to bf16
        y32, _ = R.epilogue((a.float() @ w.float().t()).double(), torch.zeros_like(acc), **kw)
        good = y32.float().bfloat16()
        R.assert_within(good, ref, tol, "correct result")
        # the smallest element whose magnitude is still in the bulk: move it three bf16 ulps
        mag = ref.abs()
        i = int(torch.argmin(torch.where(mag > 0.05, mag, torch.full_like(mag, 1e9))))
        bad = good.clone().view(-1)
        bad.view(torch.int16)[i] += 3
        bad = bad.view_as(good)
        assert R.violations(bad, ref, tol).sum() == 1, kw.keys()
        with pytest.raises(AssertionError):
            R.assert_within(bad, ref, tol, "perturbed")
        assert rel_err(bad.float(), ref) < 1.2e-2        # what the max-normalised criterion would have accepted
    nan = good.clone()
    nan[3, 5] = float("nan")
    assert R.violations(nan, ref, tol).sum() == 1


def test_rotary_reference_is_the_packed_rotate_half():
    """the reference's pair layout: packed columns (2i, 2i+1) = rotate_half's (i, i + hd/2), factors of pair i"""
    torch.manual_seed(1)
    M, hd = 5, 8
    y = torch.randn(M, 2 * hd, dtype=torch.float64)
    ang = torch.rand(M, hd // 2, dtype=torch.float64) * 6
    ref, _ = R.epilogue(y, torch.zeros_like(y), rope=R.Rope(ang.cos(), ang.sin(), hd, hd))
    perm = torch.arange(hd).view(2, hd // 2).t().reshape(-1)            # packed column -> rotate_half index
    x = torch.empty(M, hd, dtype=torch.float64)
    x[:, perm] = y[:, :hd]
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)
    want = x * cos + torch.cat([-x[:, hd // 2:], x[:, :hd // 2]], -1) * sin
    assert torch.allclose(ref[:, :hd], want[:, perm], rtol=0, atol=1e-12)
    assert torch.equal(ref[:, hd:], y[:, hd:])                           # columns >= rope_cols untouched


# ----------------------------------------------------------------------------------------------------------- bodies 1 / 2
SPEC_KW = {
    "plain": {}, "bias": dict(bias=True), "res": dict(res="sep"), "bias+res": dict(bias=True, res="sep"),
    "bias+rope": dict(bias=True, rope="inter"), "bias+gelu_tanh": dict(bias=True, act=R.ACT_GELU_TANH),
    "bias+gelu_erf": dict(bias=True, act=R.ACT_GELU_ERF), "swiglu": dict(act=R.ACT_SWIGLU), "f32out": dict(out_f32=True),
    "bias+rowstat": dict(bias=True, stats=True), "bias+res+rowstat": dict(bias=True, res="sep", stats=True),
    "lnfold": dict(ln=True), "lnfold+rope": dict(ln=True, rope="inter"), "lnfold+gelu_tanh": dict(ln=True, act=R.ACT_GELU_TANH),
    "bias+rope+hm": dict(bias=True, rope="inter", hm=True), "lnfold+rope+hm": dict(ln=True, rope="inter", hm=True),
}
GENERIC_KW = {
    "gelu_tanh, no bias": dict(act=R.ACT_GELU_TANH),
    "bias, fp32 out": dict(bias=True, out_f32=True),
    "bias + residual + gelu": dict(bias=True, res="sep", act=R.ACT_GELU_TANH),
    "rotary, no bias": dict(rope="sep"),
    "head-major, no rotary": dict(bias=True, hm=True),
    "residual in place + gelu_erf": dict(bias=True, res="inplace", act=R.ACT_GELU_ERF),
    "bias + rotary + residual, fp32 out": dict(bias=True, rope="inter", res="sep", out_f32=True),
}
N_VIT = 3 * 2 * HD_VIT          # 432: q | k | v of two heads (N % 256 = 176, N % 64 = 48)


@pytest.mark.gpu
@pytest.mark.parametrize("body,M,sw", [(1, 257, {}), (1, 1025, dict(gemm_small=1)), (2, 777, {}), (2, 1023, {})])
@pytest.mark.parametrize("epi", list(SPEC_KW))
def test_every_specialised_epilogue_on_the_128_and_ring_bodies(dev, body, M, sw, epi):
    kw = dict(SPEC_KW[epi])
    N = 1152 if (kw.get("stats") or kw.get("hm")) else N_VIT
    if kw.get("hm"):
        N, kw["hd"] = 3 * 384, 64       # hm_cols 384 = 6 heads of 64 (a multiple of 64: the lean store path)
        kw["rope_cols"] = 768
    run_cell(dev, body, M, N, 192, **kw, **sw)


@pytest.mark.gpu
@pytest.mark.parametrize("body,M,sw", [(1, 300, {}), (2, 600, {}), (4, 1100, dict(gemm_split=0)), (3, 1100, dict(gemm_split=0, gemm_pp64=0))])
@pytest.mark.parametrize("combo", list(GENERIC_KW))
def test_generic_epilogue_combinations(dev, body, M, sw, combo):
    kw = dict(GENERIC_KW[combo])
    N = 1152
    if kw.get("hm"):
        kw["hd"] = 64
    elif kw.get("rope"):
        kw["rope_cols"] = 720           # 10 heads of 72
    run_cell(dev, body, M, N, 128, **kw, **sw)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [2, 63, 64, 65, 255, 256, 257, 383, 384, 385, 511])
@pytest.mark.parametrize("N", [132, 256, 260, 384, 508])
def test_128x128_body_row_and_column_edges(dev, M, N):
    run_cell(dev, 1, M, N, 64 if M % 2 else 320, bias=True, res="sep", seed=M + N)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [512, 513, 767, 1023])
@pytest.mark.parametrize("N,K", [(132, 64), (1028, 192), (1140, 128), (1276, 320)])
def test_ring_body_row_and_column_edges(dev, M, N, K):
    run_cell(dev, 2, M, N, K, bias=True, res="sep", seed=M + N)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("body,M,sw", [(1, 385, {}), (2, 513, {}), (2, 1025, {})])
def test_layouts_lda_ldc_ldr_views(dev, dtype, body, M, sw):
    """A as a column view (lda > K); C and the residual as views with ldc / ldr > N, C starting 8 bytes into a 16-byte
    line (ldc = 4 mod 8 for bf16: the kernels must take their per-wave paths); the residual aliasing C"""
    if dtype == F32 and M == 1025:
        sw = {}
    N, K = 1152, 128
    run_cell(dev, body, M, N, K, dtype=dtype, bias=True, res="sep", lda_pad=64, ldc_pad=12, c_off=4, ldr_pad=4, **sw)
    run_cell(dev, body, M, N, K, dtype=dtype, bias=True, res="sep", ldc_pad=8, ldr_pad=8, **sw)
    run_cell(dev, body, M, N, K, dtype=dtype, bias=True, res="inplace", ldc_pad=4, **sw)
    run_cell(dev, body, M, N, K, dtype=dtype, bias=True, res="inplace", **sw)
    run_cell(dev, body, M, N, K, dtype=dtype, bias=True, act=R.ACT_GELU_TANH, ldc_pad=4, c_off=4, **sw)
    run_cell(dev, body, M, N, K, dtype=dtype, bias=True, rope="inter", rope_cols=720, ldc_pad=4, **sw)


@pytest.mark.gpu
@pytest.mark.parametrize("body,M,sw", [(1, 257, {}), (2, 513, {}), (4, 1025, dict(gemm_split=0))])
@pytest.mark.parametrize("epi", ["plain", "bias", "res", "bias+res", "f32out", "bias+rope+hm", "rope swap", "rope swap sep"])
def test_exact_integer_cells(dev, body, M, sw, epi):
    kw = {"plain": {}, "bias": dict(bias=True), "res": dict(res="sep"), "bias+res": dict(bias=True, res="sep"),
          "f32out": dict(out_f32=True), "bias+rope+hm": dict(bias=True, rope="swap", hm=True, hd=64, rope_cols=768),
          "rope swap": dict(bias=True, rope="swap"), "rope swap sep": dict(bias=True, rope="swap_sep")}[epi]
    N = 1152
    if epi.startswith("rope swap"):
        kw["hd"], kw["rope_cols"] = HD_VIT, 720
    run_cell(dev, body, M, N, 256, exact=True, **kw, **sw)


@pytest.mark.gpu
def test_fp32_inputs_on_the_128_and_ring_bodies(dev):
    for body, M in ((1, 65), (1, 511), (2, 512), (2, 1300)):
        for kw in (dict(bias=True, res="sep"), dict(bias=True, act=R.ACT_GELU_ERF), dict(bias=True, rope="sep"),
                   dict(act=R.ACT_SWIGLU), dict(bias=True, res="inplace", ldc_pad=4)):
            run_cell(dev, body, M, N_VIT, 96, dtype=F32, **kw)


# ----------------------------------------------------------------------------------------------------------- ping-pong bodies
@pytest.mark.gpu
@pytest.mark.parametrize("M", [1024, 1025, 1151, 2049])
@pytest.mark.parametrize("N,K", [(1024, 128), (1152, 192), (1156, 320), (1276, 128), (1144, 1152), (2304, 128)])
def test_whole_line_body_edges(dev, M, N, K):
    """tall tiles (N % 256 = 128), a ragged block of 132 / 252 columns, N just inside the 112 % padding rule, odd slab
    counts (K = 192 / 320)"""
    run_cell(dev, 4, M, N, K, bias=True, res="sep", seed=M + N + K, gemm_split=0)


@pytest.mark.gpu
@pytest.mark.parametrize("epi", list(SPEC_KW))
def test_every_specialised_epilogue_on_the_whole_line_body(dev, epi):
    kw = dict(SPEC_KW[epi])
    N = 1152
    if kw.get("hm"):
        kw["hd"], kw["rope_cols"] = 64, 768
    elif kw.get("rope"):
        kw["rope_cols"] = 720
    run_cell(dev, 4, 1300, N, 192, **kw, gemm_split=0)
    if epi in ("bias+res", "bias+rope", "bias+res+rowstat", "lnfold+rope+hm"):
        run_cell(dev, 4, 2048, 1536, 128, **kw, gemm_split=0)          # full tiles: the lean pair epilogue everywhere


@pytest.mark.gpu
def test_whole_line_body_in_place_and_strided(dev):
    run_cell(dev, 4, 1300, 1152, 192, bias=True, res="inplace", gemm_split=0)
    run_cell(dev, 4, 2048, 1536, 128, bias=True, res="inplace", gemm_split=0)
    run_cell(dev, 4, 2048, 1536, 128, bias=True, res="sep", lda_pad=64, ldc_pad=4, ldr_pad=4, gemm_split=0)
    run_cell(dev, 4, 2048, 1536, 128, bias=True, res="inplace", ldc_pad=4, c_off=4, gemm_split=0)
    run_cell(dev, 4, 1300, 1152, 192, bias=True, act=R.ACT_GELU_TANH, ldc_pad=8, c_off=8, gemm_split=0)
    run_cell(dev, 4, 1300, 1152, 192, bias=True, rope="sep", rope_cols=720, gemm_split=0)
    run_cell(dev, 4, 1300, 1152, 4352, bias=True, res="inplace", stats=True, gemm_split=0)      # the fc2 shape: K = 4352
    run_cell(dev, 2, 777, 1152, 4352, bias=True, res="inplace", stats=True)


@pytest.mark.gpu
def test_k_tile_body_and_the_rotary_lut(dev):
    run_cell(dev, 3, 1024, 1152, 64, bias=True, res="sep", gemm_split=0)                 # K = 64: one slab, no pp64
    run_cell(dev, 3, 1500, 1512, 128, bias=True, rope="lut", hd=HD_VIT, rope_cols=1008, gemm_split=0, gemm_pp64=0)
    run_cell(dev, 3, 2048, 3 * 1152, 128, bias=True, rope="lut", hd=HD_VIT, rope_cols=2304, gemm_split=0, gemm_pp64=0)
    run_cell(dev, 3, 2048, 3 * 1152, 128, ln=True, rope="lut", hd=HD_VIT, rope_cols=2304, gemm_split=0, gemm_pp64=0)
    for q_cols in (1152, 2 * HD_VIT):          # the pre-scaled Q block: 18 whole 64-column tiles, and two heads (tile 128 .. 192 straddles)
        run_cell(dev, 3, 2048, 3 * 1152, 128, bias=True, rope="lut", hd=HD_VIT, rope_cols=2304, q_cols=q_cols, gemm_split=0, gemm_pp64=0)
        run_cell(dev, 3, 2048, 3 * 1152, 128, ln=True, rope="lut", hd=HD_VIT, rope_cols=2304, q_cols=q_cols, gemm_split=0, gemm_pp64=0)
    for kw in (dict(bias=True, res="sep"), dict(bias=True, res="inplace"), dict(act=R.ACT_SWIGLU),
               dict(bias=True, act=R.ACT_GELU_ERF), dict(bias=True, res="sep", stats=True)):
        run_cell(dev, 3, 1300, 1152, 192, **kw, gemm_split=0, gemm_pp64=0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(14824, 1152, 1152), (6400, 3456, 1152)])
def test_split_body(dev, M, N, K):
    """the round-aligned split: leading row blocks on the whole-line kernel, the rest on the ring kernel with every row
    operand advanced by rows_main (rope_cos / rope_sin / ln_ab / row_stats / residual / head-major C)"""
    rc = 720 if N == 1152 else 2304
    hm_kw = dict(hd=64, rope_cols=N // 3 * 2) if N == 1152 else dict(hd=HD_VIT, rope_cols=2304)
    cells = [dict(bias=True, res="sep"), dict(bias=True, res="inplace"), dict(bias=True, res="sep", stats=True),
             dict(bias=True, res="inplace", stats=True, ldc_pad=4), dict(bias=True, act=R.ACT_GELU_TANH),
             dict(act=R.ACT_GELU_TANH), dict(bias=True, rope="sep", rope_cols=rc), dict(bias=True, rope="inter", rope_cols=rc),
             dict(ln=True, rope="inter", hm=True, **hm_kw), dict(bias=True, rope="swap_sep", hm=True, **hm_kw),
             dict(ln=True), dict(ln=True, act=R.ACT_GELU_TANH), dict(ln=True, rope="sep", rope_cols=rc)]
    if N == 3456:
        cells = cells[6:10]
        # q_scale (cogs_gemm_fused) on the encoder's own QKV shape: the Q block of 16 heads of 72 ends on a 64-column tile
        # boundary (1152); two heads (144) end inside the tile 128 .. 192, which must leave the lean path
        for q_cols in (1152, 2 * HD_VIT):
            cells += [dict(bias=True, rope="inter", rope_cols=rc, hd=HD_VIT, q_cols=q_cols),
                      dict(bias=True, rope="sep", rope_cols=rc, hd=HD_VIT, q_cols=q_cols),
                      dict(ln=True, rope="inter", rope_cols=rc, hd=HD_VIT, q_cols=q_cols),
                      dict(bias=True, rope="inter", hm=True, q_cols=q_cols, **hm_kw),
                      dict(ln=True, rope="inter", hm=True, q_cols=q_cols, **hm_kw)]
    for kw in cells:
        run_cell(dev, 5, M, N, K, **kw)


# ----------------------------------------------------------------------------------------------------------- q_scale, M > 1
@pytest.mark.gpu
@pytest.mark.parametrize("body,M,sw", [(1, 257, {}), (2, 777, {}), (4, 1300, dict(gemm_split=0))])
@pytest.mark.parametrize("q_cols", [576, 144])
def test_q_scale_on_the_prompt_bodies(dev, body, M, sw, q_cols):
    """the Q pre-scale of the rotary epilogues (five places in csrc/gemm_epilogue.h) through cogs_gemm_fused, at the factor the
    model passes for head_dim 72: q_cols = 576 (8 heads) ends on a 64-column tile boundary, q_cols = 144 (2 heads) inside the
    tile 128 .. 192, which has to leave the lean path. Row-major with both table forms and with the LN fold; head-major (the
    encoder's own QKV GEMM: 3 blocks of 8 heads of 72) with bias and with the LN fold"""
    for kw in (dict(bias=True, rope="inter"), dict(bias=True, rope="sep"), dict(ln=True, rope="inter")):
        run_cell(dev, body, M, 1152, 192, hd=HD_VIT, rope_cols=720, q_cols=q_cols, **kw, **sw)
    for kw in (dict(bias=True), dict(ln=True)):
        run_cell(dev, body, M, 3 * 576, 192, rope="inter", hm=True, hd=HD_VIT, rope_cols=1152, q_cols=q_cols, **kw, **sw)


# ----------------------------------------------------------------------------------------------------------- Qwen2 prompts
@pytest.mark.gpu
def test_qwen2_prompt_shapes_on_the_ring(dev):
    """the persistent ring walk past 256 tiles (gate/up SwiGLU at 777 rows: 4 x 296 tiles), the QKV GEMM with its separate
    rope_sin table and the o / down projections with the residual in place"""
    hd = HD_QWEN
    run_cell(dev, 2, 777, 37888, 3584, act=R.ACT_SWIGLU, also_wgs0=True)
    for M in (513, 1023):
        run_cell(dev, 2, M, 4608, 3584, bias=True, rope="sep", hd=hd, rope_cols=4096)
        run_cell(dev, 2, M, 3584, 3584, res="inplace")
    run_cell(dev, 2, 1792, 4608, 3584, bias=True, rope="sep", hd=hd, rope_cols=4096)      # by the few-tile cost model
    run_cell(dev, 2, 2047, 4608, 3584, bias=True, rope="sep", hd=hd, rope_cols=4096, also_wgs0=True, gemm_pingpong=0)
    run_cell(dev, 2, 777, 3584, 18944, res="inplace")


# ----------------------------------------------------------------------------------------------------------- GEMV
@pytest.mark.gpu
@pytest.mark.parametrize("N", [132, 16380, 16384, 16388])
@pytest.mark.parametrize("dot2", [1, 0])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_gemv_edges(dev, N, dot2, dtype):
    kw = dict(gemv_dot2=dot2)
    tags = ("gemv small_n" if N // 16 < 1024 else "gemv big_n",) + (("gemv dot2=0",) if dot2 == 0 else ())
    run_cell(dev, 6, 1, N, 256, dtype=dtype, bias=True, res="sep", ldc_pad=4 if N % 8 == 0 else 0, tags=tags, **kw)
    run_cell(dev, 6, 1, N, 256, dtype=dtype, bias=True, res="inplace", tags=tags, **kw)
    run_cell(dev, 6, 1, N, 256, dtype=dtype, act=R.ACT_SWIGLU, tags=tags, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("epi", ["plain", "bias", "res", "bias+res", "bias+res in place", "bias+rope", "bias+rope sep",
                                 "bias+gelu_tanh", "bias+gelu_erf", "swiglu", "f32out", "generic gelu", "generic f32 res"])
def test_gemv_epilogues_at_the_lm_head_width(dev, epi):
    kw = {"plain": {}, "bias": dict(bias=True), "res": dict(res="sep"), "bias+res": dict(bias=True, res="sep"),
          "bias+res in place": dict(bias=True, res="inplace"), "bias+rope": dict(bias=True, rope="inter"),
          "bias+rope sep": dict(bias=True, rope="sep"), "bias+gelu_tanh": dict(bias=True, act=R.ACT_GELU_TANH),
          "bias+gelu_erf": dict(bias=True, act=R.ACT_GELU_ERF), "swiglu": dict(act=R.ACT_SWIGLU), "f32out": dict(out_f32=True),
          "generic gelu": dict(act=R.ACT_GELU_TANH), "generic f32 res": dict(bias=True, res="sep", out_f32=True)}[epi]
    if "rope" in kw:
        kw.update(hd=HD_QWEN, rope_cols=4096)
    run_cell(dev, 6, 1, 152064, 512, **kw)


# ----------------------------------------------------------------------------------------------------------- status contract
@pytest.mark.gpu
def test_rejected_descriptors_return_their_status_and_leave_c_alone(dev):
    """every combination include/cogs.h declares unsupported or invalid, on valid allocations: the host returns the
    documented status before any launch and C keeps its bits"""
    L = _L()
    M, N, K = 300, 1152, 128
    g = torch.Generator(device=dev).manual_seed(3)
    a = torch.randn(M, K, generator=g, device=dev).bfloat16()
    w = torch.randn(N, K, generator=g, device=dev).bfloat16()
    a32 = a.float()
    w32 = w.float()
    out = _filled(M * N + 64, BF16, dev)
    res = torch.randn(M, N, generator=g, device=dev).bfloat16()
    bias = torch.randn(N, generator=g, device=dev).bfloat16()
    ln_ab = torch.ones(M, 2, device=dev)
    col_c = torch.zeros(N, device=dev)
    stats = torch.zeros(M, N // 64, 2, device=dev)
    tab = torch.zeros(M, 36, 2, device=dev)
    before = _bits(out).clone()

    def desc(**kw):
        d = L.GemmDesc()
        d.dtype = L.DT_BF16
        d.A, d.lda, d.W, d.ldw, d.C, d.ldc = a.data_ptr(), K, w.data_ptr(), K, out.data_ptr(), N
        d.M, d.N, d.K = M, N, K
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    LN = dict(ln_ab=ln_ab.data_ptr(), col_c=col_c.data_ptr())
    UNS, INV = L.E_UNSUPPORTED, L.E_INVALID
    cases = [
        ("ln_ab + residual", UNS, desc(**LN, residual=res.data_ptr(), ldr=N)),
        ("ln_ab + GELU_ERF", UNS, desc(**LN, act=L.ACT_GELU_ERF)),
        ("ln_ab + SwiGLU", UNS, desc(**LN, act=L.ACT_SWIGLU)),
        ("ln_ab + fp32 output", UNS, desc(**LN, out_f32=1)),
        ("ln_ab + bias", INV, desc(**LN, bias=bias.data_ptr())),
        ("ln_ab, M = 1", UNS, desc(**LN, M=1)),
        ("ln_ab without col_c", INV, desc(ln_ab=ln_ab.data_ptr())),
        ("row_stats without bias", UNS, desc(row_stats=stats.data_ptr())),
        ("row_stats + GELU_TANH", UNS, desc(row_stats=stats.data_ptr(), bias=bias.data_ptr(), act=L.ACT_GELU_TANH)),
        ("row_stats + fp32 output", UNS, desc(row_stats=stats.data_ptr(), bias=bias.data_ptr(), out_f32=1)),
        ("row_stats, M = 1", UNS, desc(row_stats=stats.data_ptr(), bias=bias.data_ptr(), M=1)),
        ("row_stats, N % 64", INV, desc(row_stats=stats.data_ptr(), bias=bias.data_ptr(), N=N - 4)),
        ("head-major + GELU", INV, desc(hm_rows=M, hm_cols=N // 2, head_dim=64, bias=bias.data_ptr(), act=L.ACT_GELU_TANH)),
        ("head-major + residual", INV, desc(hm_rows=M, hm_cols=N // 2, head_dim=64, residual=res.data_ptr(), ldr=N)),
        ("head-major, hm_rows < M", INV, desc(hm_rows=M - 1, hm_cols=N // 2, head_dim=64)),
        ("head-major, head_dim % 8", INV, desc(hm_rows=M, hm_cols=N // 2, head_dim=36)),
        ("head-major, M = 1", UNS, desc(hm_rows=M, hm_cols=N // 2, head_dim=64, M=1)),
        ("head-major, fp32", UNS, desc(hm_rows=M, hm_cols=N // 2, head_dim=64, dtype=L.DT_F32, A=a32.data_ptr(), W=w32.data_ptr())),
        ("K % 64 (bf16)", INV, desc(K=96)),
        ("K % 32 (fp32)", INV, desc(dtype=L.DT_F32, A=a32.data_ptr(), W=w32.data_ptr(), K=80, lda=K, ldw=K)),
        ("N % 4", INV, desc(N=N - 2)),
        ("M = 0", INV, desc(M=0)),
        ("lda not 16-byte", INV, desc(lda=K + 4, M=200)),
        ("SwiGLU + bias", INV, desc(act=L.ACT_SWIGLU, bias=bias.data_ptr())),
        ("SwiGLU + residual", INV, desc(act=L.ACT_SWIGLU, residual=res.data_ptr(), ldr=N)),
        ("SwiGLU + bias, M = 1", INV, desc(act=L.ACT_SWIGLU, bias=bias.data_ptr(), M=1)),
        ("rope, rope_cols % head_dim", INV, desc(rope_cos=tab.data_ptr(), rope_cols=100, head_dim=72, bias=bias.data_ptr())),
        ("rope, head_dim % 4", INV, desc(rope_cos=tab.data_ptr(), rope_cols=140, head_dim=70, bias=bias.data_ptr())),
    ]
    for name, want, d in cases:
        got = L.lib.cogs_gemm(L.current_stream(), C.byref(d))
        assert got == want, (name, got, want)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), before)
    assert torch.equal(stats, torch.zeros_like(stats))


# ----------------------------------------------------------------------------------------------------------- coverage
@pytest.mark.gpu
def test_zz_required_coverage(dev):
    """the cells above reached every required (body, epilogue) pair -- a dispatcher change that reroutes a cell to another
    body fails its own assertion, and one that makes a whole class of cells unreachable fails here"""
    missing = [p for p in REQUIRED if p not in REACHED]
    assert not missing, f"not reached: {missing}"
