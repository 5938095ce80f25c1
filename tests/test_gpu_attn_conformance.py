"""cogs_attention conformance: every attention kernel and variant against an fp64 reference of the same operation, element
by element (tests/attn_reference.py holds the reference and the derivation of the tolerance).

Each cell forces its kernel and variant with debug switches only, asserts which kernel ran (cogs_debug_get
"attn_last_kernel": 1 general MFMA, 2 ViT unpipelined, 3 / 8 ViT pipelined token- / head-major, 4 single-token decode +
combine, 5 prompt LDS-DMA, 7 row-wise; "attn_vit_last_end" for the ViT ends) and records the (kernel, variant) pair it
reached; test_zz_required_coverage asserts a required list of pairs.

Most cells run on EXACT data (attn_reference.exact_kv / exact_q): integer scores aimed at the row's seams (diagonal key,
first masked key, first / last key of the segment and the first of the next, keys 63 / 64 of a tile, the last key of a
ragged tile or split), so that the output must equal the fp64 value rounded once. Before trusting such a cell, the cell
recomputes the reference with each seam moved (mask +-1, segment ends +-1, the last key counted twice, a query head read
from the neighbouring kv head) and asserts that every row the move changes leaves the band: data too weak to carry a seam
fails its own test instead of passing the kernel. Random-data cells at moderate lengths use the derived bound.

Guard bands in every cell: O is a view with ldo > hq*head_dim inside one tracer-filled buffer with tracer rows before and
after; Q, K and V have tracer columns and tracer rows behind their last row; the split-KV workspace is tracer-filled. The
tracer is finite (bf16 / fp32 3.39e38: -fno-honor-nans builds do not keep NaN semantics), so a key read past its range gets
an infinite score and fails the band, and everything outside O's [q_len) x [hq*head_dim) must keep its bits."""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import pytest
import torch

import attn_reference as R

BF16, F32 = torch.bfloat16, torch.float32
TRACE16, TRACE32 = 0x7F7F, 0x7F7F7F7F
GUARD_ROWS = 5
LN2_F32 = R.f32(math.log(2.0))

REACHED: set = set()
VIT_ENDS = {193: 41, 256: 42, 257: 51, 320: 52, 321: 61, 384: 62, 385: 71, 448: 72}
PROMPT_VARIANTS = {"<1,2>": {}}
REQUIRED = (
    [(5, f"{v} hf={hf}") for v in PROMPT_VARIANTS for hf in (0, 1)]
    + [(5, "varlen"), (5, "q_pos0 < 128 new rows"), (5, "15395")]
    + [(4, f"r{r} combine32={c}") for r in (1, 2, 7, 16) for c in (0, 1)] + [(4, "empty splits")]
    + [(1, f"hd{hd} nq{nq} {'pre' if pre else 'classic'} {mode}") for hd in (72, 128) for nq in (1, 2) for pre in (0, 1)
       for mode in ("seg", "causal") + (() if pre else ("bias",))]
    + [(1, f"gqa_pack r{r}") for r in (1, 2, 7, 16)] + [(1, f"split combine32={c}") for c in (0, 1)]
    + [(3, "runtime end"), (8, "runtime end"), (2, "ldk!=ldv"), (2, "attn_vit=1")]
    + [(3, f"end {e}") for e in VIT_ENDS.values()] + [(8, f"end {e}") for e in VIT_ENDS.values()]
    + [(k, f"heads {h}") for k in (3, 8) for h in (1, 8, 16)]
    + [(7, f"{t} hd{hd}") for t in ("bf16", "f32") for hd in (64, 72, 128, 256)]
    + [(7, "bf16 hd64 natural"), (7, "bf16 hd256 natural")]
)


def _L():
    from cogstream_amd import _lib
    return _lib


@contextlib.contextmanager
def switches(**kw):
    L = _L()
    with contextlib.ExitStack() as st:
        for k, v in kw.items():
            st.enter_context(L.debug_switch(k, v))
        yield


def _filled(shape, dtype, dev):
    if dtype == F32:
        return torch.full(shape, TRACE32, dtype=torch.int32, device=dev).view(F32)
    return torch.full(shape, TRACE16, dtype=torch.int16, device=dev).view(dtype)


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


# ----------------------------------------------------------------------------------------------------------- one launch
def launch(dev, q, k, v, *, hq, hkv, hd, dtype=BF16, cu=None, causal=False, q_pos0=0, row_lo=None, row_hi=None,
           bias=0.0, scale=None, prescaled=False, nsplit=1, force_rowwise=False, head_major=False, ldv_pad=0,
           ws_bytes=None, kv_len=None):
    """cogs_attention on guarded copies of q / k / v (host tensors of the exact values). Returns (status, O [Lq, hq*hd]
    on the host in fp32, guards-intact flag, the whole O buffer's bits)"""
    L = _L()
    Lq, Lk = q.shape[0], k.shape[0]
    kv_len = Lk if kv_len is None else kv_len
    d = L.AttnDesc()
    keep = []
    if head_major:
        hs = (Lq + GUARD_ROWS) * hd
        bufs = []
        for t, h in ((q, hq), (k, hkv), (v, hkv)):
            b = _filled((h * hs,), dtype, dev)
            b.view(h, Lq + GUARD_ROWS, hd)[:, :Lq] = t.view(Lq, h, hd).permute(1, 0, 2).to(dev, dtype)
            bufs.append(b)
        keep += bufs
        d.Q, d.K, d.V = (b.data_ptr() for b in bufs)
        d.ldq = d.ldk = d.ldv = hd
        d.head_stride = hs
    else:
        ldq, ldk = hq * hd + 8, hkv * hd + 8
        ldv = ldk + ldv_pad
        bq, bk, bv = _filled((Lq + GUARD_ROWS, ldq), dtype, dev), _filled((Lk + GUARD_ROWS, ldk), dtype, dev), \
            _filled((Lk + GUARD_ROWS, ldv), dtype, dev)
        bq[:Lq, :hq * hd] = q.to(dev, dtype)
        bk[:Lk, :hkv * hd] = k.to(dev, dtype)
        bv[:Lk, :hkv * hd] = v.to(dev, dtype)
        keep += [bq, bk, bv]
        d.Q, d.K, d.V = bq.data_ptr(), bk.data_ptr(), bv.data_ptr()
        d.ldq, d.ldk, d.ldv = ldq, ldk, ldv
    ldo = hq * hd + 8
    obuf = _filled(((GUARD_ROWS + Lq + GUARD_ROWS) * ldo,), dtype, dev)
    before = _bits(obuf).clone()
    d.O, d.ldo = obuf.data_ptr() + GUARD_ROWS * ldo * obuf.element_size(), ldo
    d.dtype = L.dtype_code(dtype)
    cu_d = None
    if cu is not None:
        cu_d = torch.tensor(list(cu), dtype=torch.int32, device=dev)
        d.cu_seqlens, d.nseg = cu_d.data_ptr(), len(cu) - 1
        d.max_seqlen = max(b - a for a, b in zip(cu[:-1], cu[1:]))
    else:
        d.nseg = 1
    if row_lo is not None:
        lo_d, hi_d = row_lo.to(dev, torch.int32), row_hi.to(dev, torch.int32)
        keep += [lo_d, hi_d]
        d.row_lo, d.row_hi, d.bias = lo_d.data_ptr(), hi_d.data_ptr(), bias
    d.q_len, d.kv_len, d.hq, d.hkv, d.head_dim = Lq, kv_len, hq, hkv, hd
    d.scale = scale if scale is not None else LN2_F32
    d.causal, d.q_pos0, d.force_rowwise, d.q_prescaled = int(causal), q_pos0, int(force_rowwise), int(prescaled)
    d.nsplit = nsplit
    ws = None
    if nsplit > 1:
        need = nsplit * Lq * hq * (hd + 2) * 4
        ws = _filled((need // 4,), F32, dev)
        d.ws, d.ws_bytes = ws.data_ptr(), need if ws_bytes is None else ws_bytes
    st = L.lib.cogs_attention(L.current_stream(), C.byref(d))
    torch.cuda.synchronize()
    full = obuf.view(-1, ldo)
    out = full[GUARD_ROWS:GUARD_ROWS + Lq, :hq * hd].float().cpu()
    inside = torch.zeros_like(before, dtype=torch.bool).view(-1, ldo)
    inside[GUARD_ROWS:GUARD_ROWS + Lq, :hq * hd] = True
    inside = inside.view(-1)
    guards_ok = bool(torch.equal(_bits(obuf)[~inside], before[~inside]))
    return st, out, guards_ok, _bits(obuf).clone(), before


# ----------------------------------------------------------------------------------------------------------- data
def seam_targets(Lq, Lk, *, cu=None, causal=False, q_pos0=0, extra=(), row_extra=None, gen=None):
    """targets [Lq, T] and offsets g for exact_q: the seams of every row (see the module docstring)"""
    qs, ks, ke = R._segments(Lq, cu, Lk)
    i = torch.arange(Lq)
    cols, gs = [], []

    def add(key, g):
        cols.append(key.clamp(0, Lk - 1))
        gs.append(torch.full((Lq,), g, dtype=torch.long))

    if causal:
        diag = ks + (i - qs) + q_pos0
        add(diag.clamp(max=Lk - 1), 0)
        add(diag + 1, 0)                                   # the first masked key: must stay out
        tile = ks + ((diag - ks) // 64) * 64
        add(tile, 1)                                       # first key of the diagonal's tile
        add(tile - 1, 0)                                   # last key of the tile before
    add(ks, 1)                                             # the segment's first key
    add(ke - 1, 0)                                         # its last key
    add(ke, 2)                                             # the next segment's first key
    for key in extra:
        add(torch.full((Lq,), int(key)), 0)
    if row_extra is not None:                             # per-row seams [Lq, X] (the bias range ends)
        for c in range(row_extra.shape[1]):
            add(row_extra[:, c].long(), 0)
    r = torch.randint(0, 1 << 30, (Lq,), generator=gen)
    add(ks + r % (ke - ks).clamp(min=1), int(r[0] % 7))   # one random key of the segment, random offset
    return torch.stack(cols, 1), torch.stack(gs, 1)


def random_qkv(Lq, Lk, hq, hkv, hd, gen, prescaled):
    q = torch.randn(Lq, hq * hd, generator=gen)
    q *= (R.LOG2E_F32 / math.sqrt(hd)) if prescaled else 1.0
    k = torch.randn(Lk, hkv * hd, generator=gen)
    v = torch.randn(Lk, hkv * hd, generator=gen)
    return q, k, v


# ----------------------------------------------------------------------------------------------------------- one cell
def run_cell(dev, kernel, variant, *, hq, hkv, hd, q_len, kv_len=None, cu=None, causal=False, q_pos0=0, bias_mode=False,
             prescaled=False, nsplit=1, dtype=BF16, data="exact", force_rowwise=False, head_major=False, ldv_pad=0,
             sw=None, vit_end=None, rows=None, seed=0, extra_seams=(), key_len=None, tags=()):
    L = _L()
    Lk = key_len if key_len is not None else (kv_len if kv_len is not None else (q_len if cu is None else cu[-1]))
    kv = kv_len if kv_len is not None else Lk
    gen = torch.Generator().manual_seed(seed + 7919 * q_len + 31 * Lk + hq)
    row_lo = row_hi = None
    bias = 0.0
    if bias_mode:
        # the eager encoder form: every row sees all keys, a same-block bias on [row_lo, row_hi); +2 log2 units (exact)
        blk = 64
        row_lo = (torch.arange(q_len) // blk) * blk
        row_hi = (row_lo + blk).clamp(max=Lk)
        bias = 2 * LN2_F32
    if data == "exact":
        k, v = R.exact_kv(Lk, hkv, hd, gen)
        row_extra = torch.stack([row_lo - 1, row_lo, row_hi - 1, row_hi], 1) if bias_mode else None
        tg, gg = seam_targets(q_len, kv, cu=cu, causal=causal, q_pos0=q_pos0, extra=extra_seams, row_extra=row_extra,
                              gen=gen)
        q = R.exact_q(tg, gg, hq, hkv, hd)
        scale = LN2_F32
    else:
        q, k, v = random_qkv(q_len, Lk, hq, hkv, hd, gen, prescaled)
        scale = R.f32(1.0 / math.sqrt(hd))
    qx = q.to(dtype).float()
    kx, vx = k.to(dtype).float(), v.to(dtype).float()
    with switches(**(sw or {})):
        st, out, guards_ok, _, _ = launch(dev, qx, kx, vx, hq=hq, hkv=hkv, hd=hd, dtype=dtype, cu=cu, causal=causal,
                                          q_pos0=q_pos0, row_lo=row_lo, row_hi=row_hi, bias=bias, scale=scale,
                                          prescaled=prescaled, nsplit=nsplit, force_rowwise=force_rowwise,
                                          head_major=head_major, ldv_pad=ldv_pad, kv_len=kv)
        ran = L.debug_get("attn_last_kernel")
        end = L.debug_get("attn_vit_last_end")
    what = f"kernel {kernel} {variant} hq {hq}/{hkv} hd {hd} q_len {q_len} kv {kv} cu {cu} causal {causal} q_pos0 {q_pos0}"
    assert st == 0, (what, st)
    assert ran == kernel, (what, ran)
    if vit_end is not None:
        assert end == vit_end, (what, end)
    assert guards_ok, what + ": bits outside O changed"
    rowwise = kernel == 7
    bound = "rowwise" if rowwise else ("exact" if data == "exact" else "mfma")
    kw = dict(hq=hq, hkv=hkv, hd=hd, scale_log2=R.scale_log2_of(scale, prescaled), cu=cu, causal=causal, q_pos0=q_pos0,
              row_lo=row_lo, row_hi=row_hi, bias_log2=R.f32(R.f32(bias) * R.f32(R.LOG2E_F32)) if bias_mode else 0.0,
              kv_len=kv, rows=rows, sum_in_v=(hd % 16 != 0 and not rowwise), out_dtype=dtype, nsplit=nsplit)
    qd, kd, vd = qx.to(dev), kx.to(dev), vx.to(dev)
    ref, tol = R.reference(qd, kd, vd, bound=bound, **kw)
    got = out if rows is None else out[rows]
    R.assert_within(got, ref, tol, what)
    if data == "exact" and not rowwise:
        # exactness premise: live keys x |v| <= 8 x the 2^10 spread of live p (offsets g, deferred or bf16 reference) < 2^24
        assert R.live_counts(qd, kd, hq, hkv, hd, rows if rows is not None else torch.arange(q_len)) < 2048, what
        prove_seams(qd, kd, vd, ref, tol, kw, what)
    REACHED.add((kernel, variant))
    REACHED.update((kernel, t) for t in tags)
    return out


def prove_seams(q, k, v, ref, tol, kw, what):
    """the test of the test: every seam moved by one key changes some rows, and every row it changes leaves the band"""
    moves = []
    if kw["causal"]:
        moves += [("mask -1", dict(q_pos0=kw["q_pos0"] - 1), 0.9), ("mask +1", dict(q_pos0=kw["q_pos0"] + 1), 0.0)]
    if kw["cu"] is not None and len(kw["cu"]) > 2:
        cu = list(kw["cu"])
        for dlt in (-1, 1):
            cu_k = [cu[0]] + [c + dlt for c in cu[1:-1]] + [cu[-1]]
            moves.append((f"segment ends {dlt:+d}", dict(cu_k=cu_k), 0.0))
    elif kw["kv_len"] > 1 and not kw["causal"]:
        moves.append(("key range end -1", dict(kv_len=kw["kv_len"] - 1), 0.9))
    moves.append(("last key counted twice", dict(dup_last=True), None))     # (no change on one-key rows)
    if kw["row_lo"] is not None:
        for dlt in (-1, 1):
            moves.append((f"bias range {dlt:+d}", dict(row_lo=kw["row_lo"] + dlt, row_hi=kw["row_hi"] + dlt), 0.9))
    if kw["hkv"] > 1:
        gsz = kw["hq"] // kw["hkv"]
        moves.append(("head 0 on kv head 1", dict(kv_head=[1] + [h // gsz for h in range(1, kw["hq"])]), 0.0))
    for name, change, min_frac in moves:
        p_kw = dict(kw, **change)
        ref_p, _ = R.reference(q, k, v, bound=None, **p_kw)
        changed = ((ref_p - ref).abs() > 1e-30).any(1)
        decisive = R.violations(ref_p, ref, tol).any(1)
        if min_frac is None:
            min_frac = 0.0
        else:
            assert bool(changed.any()), f"{what}: seam '{name}' changes no row"
        assert bool((decisive | ~changed).all()), \
            f"{what}: seam '{name}' changes {int(changed.sum())} rows, only {int((decisive & changed).sum())} decisively"
        assert float(changed.double().mean()) >= min_frac, (what, name, float(changed.double().mean()))


# ----------------------------------------------------------------------------------------------------------- CPU: the reference and the checker
def _sdpa_restatement(q, k, v, hq, hkv, hd, scale_log2, cu=None, causal=False, q_pos0=0, lo=None, hi=None, bias_log2=0.0):
    """the same operation through torch's fp64 scaled_dot_product_attention on the CPU, masks built explicitly"""
    F = torch.nn.functional
    Lq, Lk = q.shape[0], k.shape[0]
    qh = q.double().view(Lq, hq, hd).transpose(0, 1)
    kh = k.double().view(Lk, hkv, hd).transpose(0, 1).repeat_interleave(hq // hkv, 0)
    vh = v.double().view(Lk, hkv, hd).transpose(0, 1).repeat_interleave(hq // hkv, 0)
    i, j = torch.arange(Lq)[:, None], torch.arange(Lk)[None, :]
    allow = torch.ones(Lq, Lk, dtype=torch.bool)
    if cu is not None:
        cu_t = torch.tensor(cu)
        allow &= torch.bucketize(i, cu_t[1:], right=True) == torch.bucketize(j, cu_t[1:], right=True)
        start = cu_t[torch.bucketize(i, cu_t[1:], right=True)]
    else:
        start = torch.zeros_like(i)
    if causal:
        allow &= (j - start) <= (i - start) + q_pos0
    bias = torch.zeros(Lq, Lk, dtype=torch.float64)
    if lo is not None:
        bias += ((j >= lo[:, None]) & (j < hi[:, None])).double() * bias_log2 * math.log(2.0)
    mask = bias.masked_fill(~allow, float("-inf"))
    out = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, scale=scale_log2 * math.log(2.0))
    return out.transpose(0, 1).reshape(Lq, hq * hd)


@pytest.mark.parametrize("case", ["gqa", "segments", "causal q_pos0", "bias", "segments causal"])
def test_reference_agrees_with_sdpa_restatement(case):
    torch.manual_seed(3)
    hq, hkv, hd, Lq = 6, 2, 16, 40
    kw = {}
    Lk = Lq
    if case == "causal q_pos0":
        Lk, kw = 57, dict(causal=True, q_pos0=17)
    elif case == "segments":
        kw = dict(cu=[0, 7, 8, 30, 40])
    elif case == "segments causal":
        kw = dict(cu=[0, 13, 40], causal=True)
    elif case == "bias":
        lo = (torch.arange(Lq) // 8) * 8
        kw = dict(row_lo=lo, row_hi=lo + 8, bias_log2=1.5)
    q, k, v = torch.randn(Lq, hq * hd), torch.randn(Lk, hkv * hd), torch.randn(Lk, hkv * hd)
    ref, _ = R.reference(q, k, v, hq=hq, hkv=hkv, hd=hd, scale_log2=0.3, bound=None, **kw)
    want = _sdpa_restatement(q, k, v, hq, hkv, hd, 0.3, cu=kw.get("cu"), causal=kw.get("causal", False),
                             q_pos0=kw.get("q_pos0", 0), lo=kw.get("row_lo"), hi=kw.get("row_hi"),
                             bias_log2=kw.get("bias_log2", 0.0))
    assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
    # chunking over rows and a row subset give the same values
    sub, _ = R.reference(q, k, v, hq=hq, hkv=hkv, hd=hd, scale_log2=0.3, bound=None, rows=torch.tensor([3, 17, 39]), chunk=2, **kw)
    assert torch.allclose(sub, ref[[3, 17, 39]], rtol=1e-14, atol=1e-14)


def test_classic_scale_ln2_is_exact_in_log2_units():
    """fp32(ln 2) * fp32(log2 e) rounds to 1.0f: the classic path computes the exact cells exactly too"""
    import numpy as np
    assert np.float32(np.log(2.0)) * np.float32(R.LOG2E_F32) == np.float32(1.0)
    assert R.scale_log2_of(LN2_F32, False) == 1.0
    assert R.f32(R.f32(2 * LN2_F32) * R.f32(R.LOG2E_F32)) == 2.0


def _emulate(q, k, v, hq, hkv, hd, *, causal, q_pos0, sum_in_v, score_err):
    """CPU emulation of the modelled error sources of the log2-domain kernels: scores perturbed by +-score_err (worst
    case: alternating signs), exp2 in fp32, P rounded to bf16 for the PV product, l from the unrounded (hd % 16 == 0)
    or the rounded P (SUM_IN_V), fp32 sums, o * fp32(1 / l), one rounding to bf16"""
    Lq, Lk = q.shape[0], k.shape[0]
    out = torch.zeros(Lq, hq * hd)
    gsz = hq // hkv
    for h in range(hq):
        kh, vh = k[:, (h // gsz) * hd:(h // gsz + 1) * hd], v[:, (h // gsz) * hd:(h // gsz + 1) * hd]
        s = (q[:, h * hd:(h + 1) * hd].double() @ kh.double().t())
        s = s + score_err * torch.where((torch.arange(Lk)[None, :] + torch.arange(Lq)[:, None]) % 2 == 0, 1.0, -1.0)
        s = s.float()
        if causal:
            s = s.masked_fill(torch.arange(Lk)[None, :] > torch.arange(Lq)[:, None] + q_pos0, float("-inf"))
        m = s.amax(1, keepdim=True)
        p = torch.exp2(s - m)
        pb = p.bfloat16().float()
        l = (pb if sum_in_v else p).sum(1, keepdim=True)
        o = pb @ vh.float()
        out[:, h * hd:(h + 1) * hd] = (o * (1.0 / l)).bfloat16().float()
    return out


@pytest.mark.parametrize("hd", [72, 128])
def test_band_contains_the_emulated_kernel_errors(hd):
    torch.manual_seed(hd)
    hq, hkv, Lq, Lk = 4, 2, 48, 300
    q = (torch.randn(Lq, hq * hd) * (R.LOG2E_F32 / math.sqrt(hd)) * 3).bfloat16().float()
    k, v = torch.randn(Lk, hkv * hd).bfloat16().float(), torch.randn(Lk, hkv * hd).bfloat16().float()
    kw = dict(hq=hq, hkv=hkv, hd=hd, scale_log2=1.0, causal=True, q_pos0=Lk - Lq, sum_in_v=hd % 16 != 0)
    ref, tol = R.reference(q, k, v, bound="mfma", **kw)
    # the worst-case score error the bound allows for the largest score magnitudes of these rows
    a_max = max(float((q[:, h * hd:(h + 1) * hd].abs().double() @ k[:, (h // 2) * hd:(h // 2 + 1) * hd].abs().double().t()).max())
                for h in range(hq))
    err = (hd + 8) * 2.0 ** -23 * a_max
    emu = _emulate(q, k, v, hq, hkv, hd, causal=True, q_pos0=Lk - Lq, sum_in_v=hd % 16 != 0, score_err=err)
    R.assert_within(emu, ref, tol, "emulated kernel")
    assert float((emu.double() - ref).abs().max()) > 0          # the emulation is not exact: the band is being used


def test_checker_rejects_a_one_key_mask_error_on_exact_data():
    hq, hkv, hd, Lq = 4, 2, 128, 200
    gen = torch.Generator().manual_seed(1)
    k, v = R.exact_kv(Lq, hkv, hd, gen)
    tg, gg = seam_targets(Lq, Lq, causal=True, gen=gen)
    q = R.exact_q(tg, gg, hq, hkv, hd)
    kw = dict(hq=hq, hkv=hkv, hd=hd, scale_log2=1.0, causal=True)
    ref, tol = R.reference(q, k, v, bound="exact", **kw)
    # a correct kernel's result: exact sums, one rounding to bf16
    good = ref.float().bfloat16()
    R.assert_within(good, ref, tol, "exact")
    for q_pos0 in (-1, 1):
        bad, _ = R.reference(q, k, v, bound=None, **dict(kw, q_pos0=q_pos0))
        bad = bad.float().bfloat16()
        rows = R.violations(bad, ref, tol).any(1)
        assert float(rows.double().mean()) > (0.9 if q_pos0 < 0 else 0.5), q_pos0


def test_checker_rejects_a_three_ulp_error_on_a_small_element_of_random_data():
    from conftest import rel_err
    """the band of an element is ~ its own output ulp plus 2^-8 (P|v|) (the bf16 rounding of P, worst case): on rows whose
    softmax is peaked the two are of one size, and a small element moved by three output ulps leaves its band"""
    torch.manual_seed(4)
    hq, hkv, hd, Lq = 4, 2, 128, 256
    q = (torch.randn(Lq, hq * hd) * (3 * R.LOG2E_F32 / math.sqrt(hd))).bfloat16().float()
    k, v = torch.randn(Lq, hkv * hd).bfloat16().float(), torch.randn(Lq, hkv * hd).bfloat16().float()
    ref, tol = R.reference(q, k, v, hq=hq, hkv=hkv, hd=hd, causal=True, bound="mfma")
    good = ref.float().bfloat16()
    R.assert_within(good, ref, tol, "good")
    mag = ref.abs()
    ulp = 2.0 ** (torch.floor(torch.log2(mag.clamp_min(1e-30))) - 7)
    small = (mag > 0.02 * float(mag.max())) & (mag < float(mag.median())) & (3 * ulp - 0.5 * ulp > tol)
    assert int(small.sum()) > 100                          # many small elements where three ulps are decisive
    i = int(torch.argmin(torch.where(small, mag, torch.full_like(mag, 1e9))))
    bad = good.clone().view(-1)
    bad.view(torch.int16)[i] += 3
    bad = bad.view_as(good)
    assert int(R.violations(bad, ref, tol).sum()) == 1
    assert rel_err(bad.float(), ref) < 1.5e-2            # what the max-normalised criterion would have accepted


# ----------------------------------------------------------------------------------------------------------- 5: prompt
PROMPT_LENS = [2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097]


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv", [(28, 4), (4, 2)])
@pytest.mark.parametrize("q_len", PROMPT_LENS)
def test_prompt_kernel_lengths(dev, hq, hkv, q_len):
    if hq == 28 and q_len == 4097:
        q_len = 2049            # (the 28-head form of the longest cell: the same seams, half the reference work)
    run_cell(dev, 5, "<1,2> hf=1" if q_len > 128 else "<1,2> short", hq=hq, hkv=hkv, hd=128, q_len=q_len, causal=True,
             prescaled=True)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(PROMPT_VARIANTS))
@pytest.mark.parametrize("hf", [0, 1])
@pytest.mark.parametrize("q_len,q_pos0", [(129, 0), (257, 64), (1000, 173)])
def test_prompt_kernel_variants(dev, variant, hf, q_len, q_pos0):
    sw = dict(PROMPT_VARIANTS[variant])
    if not hf:
        sw["attn_light_first"] = 1
    run_cell(dev, 5, f"{variant} hf={hf}", hq=4, hkv=2, hd=128, q_len=q_len, kv_len=q_len + q_pos0, causal=True,
             q_pos0=q_pos0, prescaled=True, sw=sw)


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv", [(28, 4), (4, 2)])
@pytest.mark.parametrize("q_len,q_pos0", [(65, 1), (100, 63), (127, 64), (1, 64), (7, 173), (200, 173), (130, 1500)])
def test_prompt_kernel_behind_a_prefix(dev, hq, hkv, q_len, q_pos0):
    if q_len == 1:
        q_len = 2               # one row is the decode shape (gqa_pack): the prompt kernel starts at two
    run_cell(dev, 5, "q_pos0 < 128 new rows" if q_len < 128 else "<1,2> hf=1", hq=hq, hkv=hkv, hd=128, q_len=q_len,
             kv_len=q_len + q_pos0, causal=True, q_pos0=q_pos0, prescaled=True)


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [[1, 63, 64, 65, 128, 129], [129, 1, 64, 128, 65, 63], [257, 128, 1, 300]])
@pytest.mark.parametrize("hq,hkv", [(28, 4), (4, 2)])
def test_prompt_kernel_varlen(dev, lens, hq, hkv):
    cu = [0] + torch.tensor(lens).cumsum(0).tolist()
    run_cell(dev, 5, "varlen", hq=hq, hkv=hkv, hd=128, q_len=cu[-1], cu=cu, causal=True, prescaled=True)


@pytest.mark.gpu
def test_prompt_kernel_random_data(dev):
    run_cell(dev, 5, "<1,2> hf=1", hq=4, hkv=2, hd=128, q_len=700, kv_len=800, causal=True, q_pos0=100, prescaled=True,
             data="random")


@pytest.mark.gpu
def test_prompt_kernel_at_the_cfg2_prompt_length(dev):
    n = 15395
    gen = torch.Generator().manual_seed(15395)
    seam = [0, 1, 63, 64, 127, 128, 129, 8191, 8192, 15263, 15264, n - 2, n - 1]
    rows = torch.tensor(sorted(set(seam + torch.randint(0, n, (200,), generator=gen).tolist())))
    run_cell(dev, 5, "15395", hq=28, hkv=4, hd=128, q_len=n, causal=True, prescaled=True, rows=rows)


# ----------------------------------------------------------------------------------------------------------- 4: decode
@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv", [(4, 4), (4, 2), (28, 4), (16, 1)])
@pytest.mark.parametrize("ctx,nsplit", [(65, 2), (128, 3), (129, 2), (1000, 8), (1000, 128), (4100, 17), (4100, 61)])
@pytest.mark.parametrize("c32", [1, 0])
def test_decode_kernel(dev, hq, hkv, ctx, nsplit, c32):
    nt = (ctx + 63) // 64
    splits = [nt * s // nsplit * 64 for s in range(1, nsplit)]
    tags = ["empty splits"] if nsplit > nt else []
    run_cell(dev, 4, f"r{hq // hkv} combine32={c32}", hq=hq, hkv=hkv, hd=128, q_len=1, key_len=ctx + 3, kv_len=ctx + 3,
             causal=True, q_pos0=ctx - 1, prescaled=True, nsplit=nsplit, sw=dict(attn_combine32=c32),
             extra_seams=[63, 64] + splits[:2] + [s - 1 for s in splits[:2]] + splits[-1:], tags=tags)


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv", [(28, 4), (16, 1)])
def test_decode_kernel_random_data(dev, hq, hkv):
    run_cell(dev, 4, f"r{hq // hkv} combine32=1", hq=hq, hkv=hkv, hd=128, q_len=1, kv_len=900, causal=True, q_pos0=899,
             prescaled=True, nsplit=9, data="random")


# ----------------------------------------------------------------------------------------------------------- 1: general
@pytest.mark.gpu
@pytest.mark.parametrize("hd", [72, 128])
@pytest.mark.parametrize("nq", [1, 2])
@pytest.mark.parametrize("pre,mode", [(0, "seg"), (0, "causal"), (0, "bias"), (1, "seg"), (1, "causal")])  # no pre-scaled bias mode
@pytest.mark.parametrize("data", ["exact", "random"])
def test_general_kernel(dev, hd, nq, pre, mode, data):
    sw = dict(attn_nq=nq, attn_prefill_dma=0)
    hq, hkv = 4, 2                      # GQA keeps hd 72 / pre-scaled / segments off the ViT kernel
    kw = dict(hq=hq, hkv=hkv, hd=hd, prescaled=bool(pre), sw=sw, data=data)
    label = f"hd{hd} nq{nq} {'pre' if pre else 'classic'} {mode}"
    if mode == "seg":
        lens = [1, 63, 64, 65, 128, 129, 200]
        cu = [0] + torch.tensor(lens).cumsum(0).tolist()
        run_cell(dev, 1, label, q_len=cu[-1], cu=cu, **kw)
    elif mode == "causal":
        run_cell(dev, 1, label, q_len=300, kv_len=373, causal=True, q_pos0=73, **kw)
    else:
        run_cell(dev, 1, label, q_len=192, bias_mode=True, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("hq,hkv", [(4, 4), (4, 2), (28, 4), (16, 1)])
@pytest.mark.parametrize("ctx", [1, 33, 63, 64])
def test_general_kernel_short_context_decode(dev, hq, hkv, ctx):
    """the production decode step for contexts <= 64 (one split: gqa_pack on the general kernel)"""
    run_cell(dev, 1, f"gqa_pack r{hq // hkv}", hq=hq, hkv=hkv, hd=128, q_len=1, key_len=ctx + 2, kv_len=ctx + 2,
             causal=True, q_pos0=ctx - 1, prescaled=True, extra_seams=[0, ctx - 1])


@pytest.mark.gpu
@pytest.mark.parametrize("c32", [1, 0])
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("ctx,nsplit", [(300, 3), (1000, 20), (200, 8)])
def test_general_kernel_split_path(dev, c32, pre, ctx, nsplit):
    run_cell(dev, 1, f"split combine32={c32}", hq=28, hkv=4, hd=128, q_len=1, key_len=ctx + 2, kv_len=ctx + 2, causal=True,
             q_pos0=ctx - 1, prescaled=bool(pre), nsplit=nsplit, sw=dict(attn_decode=0, attn_combine32=c32),
             extra_seams=[63, 64, ctx - 1])


# ----------------------------------------------------------------------------------------------------------- 2 / 3 / 8: ViT
VIT_SEGS = [1, 31, 32, 33, 63, 64, 65, 127, 128]


@pytest.mark.gpu
@pytest.mark.parametrize("heads", [1, 8, 16])
@pytest.mark.parametrize("layout", ["token", "head"])
@pytest.mark.parametrize("data", ["exact", "random"])
def test_vit_kernel_runtime_end(dev, heads, layout, data):
    cu = [0] + torch.tensor(VIT_SEGS + [300]).cumsum(0).tolist()
    kernel = 8 if layout == "head" else 3
    run_cell(dev, kernel, "runtime end", hq=heads, hkv=heads, hd=72, q_len=cu[-1], cu=cu, prescaled=True,
             head_major=layout == "head", vit_end=0, data=data, tags=[f"heads {heads}"])


@pytest.mark.gpu
@pytest.mark.parametrize("seg", list(VIT_ENDS))
@pytest.mark.parametrize("layout", ["token", "head"])
def test_vit_kernel_compile_time_ends(dev, seg, layout):
    nseg = 3
    cu = [seg * i for i in range(nseg + 1)]
    kernel = 8 if layout == "head" else 3
    run_cell(dev, kernel, f"end {VIT_ENDS[seg]}", hq=8, hkv=8, hd=72, q_len=cu[-1], cu=cu, prescaled=True,
             head_major=layout == "head", vit_end=VIT_ENDS[seg], sw=dict(attn_uniform_hint=seg))


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["ldk!=ldv", "attn_vit=1"])
def test_vit_unpipelined_kernel(dev, how):
    cu = [0] + torch.tensor(VIT_SEGS + [200]).cumsum(0).tolist()
    kw = dict(ldv_pad=8) if how == "ldk!=ldv" else dict(sw=dict(attn_vit=1))
    run_cell(dev, 2, how, hq=8, hkv=8, hd=72, q_len=cu[-1], cu=cu, prescaled=True, **kw)


# ----------------------------------------------------------------------------------------------------------- 7: row-wise
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("hd", [64, 72, 128, 256])
@pytest.mark.parametrize("mode", ["seg", "causal", "bias"])
def test_rowwise_kernel(dev, dtype, hd, mode):
    dt = BF16 if dtype == "bf16" else F32
    kw = dict(hq=4, hkv=2, hd=hd, dtype=dt, force_rowwise=dtype == "bf16", data="random")
    label = f"{dtype} hd{hd}"
    if mode == "seg":
        cu = [0, 1, 64, 129, 200]
        run_cell(dev, 7, label, q_len=200, cu=cu, **kw)
    elif mode == "causal":
        run_cell(dev, 7, label, q_len=100, kv_len=170, causal=True, q_pos0=70, **kw)
    else:
        run_cell(dev, 7, label, q_len=128, bias_mode=True, **kw)
    if dtype == "bf16" and hd in (64, 256) and mode == "causal":
        kw["force_rowwise"] = False
        run_cell(dev, 7, f"bf16 hd{hd} natural", q_len=100, kv_len=170, causal=True, q_pos0=70, **kw)


# ----------------------------------------------------------------------------------------------------------- status contract
@pytest.mark.gpu
def test_rejected_descriptors_return_their_status_and_leave_o_alone(dev):
    """every attention descriptor the dispatcher refuses, on valid allocations: the documented status comes back before any
    launch and O keeps its bits (test_c_abi_error_behaviour covers the model-level entry points)"""
    L = _L()
    Lq, hq, hkv, hd = 64, 4, 2, 128
    q = torch.randn(Lq, hq * 256, device=dev).bfloat16()
    k = torch.randn(Lq, hkv * 256, device=dev).bfloat16()
    out = _filled((Lq * hq * 256 + 64,), BF16, dev)
    ws = torch.zeros(1 << 20, device=dev)
    cu = torch.tensor([0, 30, 64], dtype=torch.int32, device=dev)
    lo = torch.zeros(Lq, dtype=torch.int32, device=dev)
    before = _bits(out).clone()

    def desc(**kw):
        d = L.AttnDesc()
        d.dtype = L.DT_BF16
        d.Q, d.K, d.V, d.O = q.data_ptr(), k.data_ptr(), k.data_ptr(), out.data_ptr()
        d.ldq, d.ldk, d.ldv, d.ldo = hq * hd, hkv * hd, hkv * hd, hq * hd
        d.q_len, d.kv_len, d.hq, d.hkv, d.head_dim, d.scale, d.nseg, d.nsplit = Lq, Lq, hq, hkv, hd, 0.1, 1, 1
        for kk, vv in kw.items():
            setattr(d, kk, vv)
        return d

    UNS, INV, WS = L.E_UNSUPPORTED, L.E_INVALID, L.E_WORKSPACE
    one = dict(q_len=1, causal=1, q_pos0=Lq - 1, q_prescaled=1)
    cases = [
        ("head_dim % 8", UNS, desc(head_dim=68, ldq=hq * 68, ldk=hkv * 68, ldv=hkv * 68, ldo=hq * 68)),
        ("head_dim > 256", UNS, desc(head_dim=264, ldq=hq * 264, ldk=hkv * 264, ldv=hkv * 264, ldo=hq * 264)),
        ("nsplit > 128", UNS, desc(**one, nsplit=129, ws=ws.data_ptr(), ws_bytes=ws.numel() * 4)),
        ("split with cu_seqlens", UNS, desc(nsplit=2, cu_seqlens=cu.data_ptr(), nseg=2, max_seqlen=34, ws=ws.data_ptr(),
                                             ws_bytes=ws.numel() * 4)),
        ("no workspace", WS, desc(**one, nsplit=4)),
        ("workspace too small", WS, desc(**one, nsplit=4, ws=ws.data_ptr(), ws_bytes=4 * hq * (hd + 2) * 4 - 4)),
        ("head_stride, hd 128", UNS, desc(head_stride=Lq * hd, ldq=hd, ldk=hd, ldv=hd)),
        ("head_stride, causal hd 72", UNS, desc(head_dim=72, hkv=hq, head_stride=Lq * 72, ldq=72, ldk=72, ldv=72,
                                                causal=1, q_prescaled=1, ldo=hq * 72)),
        ("q_prescaled with row_lo", UNS, desc(q_prescaled=1, row_lo=lo.data_ptr(), row_hi=lo.data_ptr())),
        ("ldq % 8", INV, desc(ldq=hq * hd + 4)),
        ("ldk % 8", INV, desc(ldk=hkv * hd + 4, ldv=hkv * hd + 4)),
        ("ldo % 4", INV, desc(ldo=hq * hd + 2)),
        ("ViT shape, ldk % 8", INV, desc(head_dim=72, hkv=hq, cu_seqlens=cu.data_ptr(), nseg=2, max_seqlen=34, q_prescaled=1,
                                          ldq=hq * 72, ldk=hq * 72 + 4, ldv=hq * 72 + 4, ldo=hq * 72)),
        ("ViT head-major, ld != 72", INV, desc(head_dim=72, hkv=hq, cu_seqlens=cu.data_ptr(), nseg=2, max_seqlen=34,
                                                q_prescaled=1, head_stride=Lq * 72, ldq=80, ldk=72, ldv=72, ldo=hq * 72)),
    ]
    for name, want, d in cases:
        got = L.lib.cogs_attention(L.current_stream(), C.byref(d))
        assert got == want, (name, got, want)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), before)


# ----------------------------------------------------------------------------------------------------------- coverage
@pytest.mark.gpu
def test_zz_required_coverage(dev):
    """the cells above reached every required (kernel, variant) pair -- a dispatcher change that reroutes a cell fails its
    own assertion, and one that makes a whole class of cells unreachable fails here"""
    missing = [p for p in REQUIRED if p not in REACHED]
    assert not missing, f"not reached: {missing}"
