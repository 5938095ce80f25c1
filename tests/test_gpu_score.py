"""Teacher-forced scoring on the device: cogs_row_lse (the fold kernel on its own), cogs_lm_score (row blocks x
vocabulary panels behind the lm_head GEMM), Qwen2Engine.score and CogReasoner.forward / forward_train / score_answers,
against fp64 torch and against the fixtures the reference's model object produced (tests/golden/make_golden_score.py).

Tolerances and where they come from:
  * target_logit, max_logit, argmax of cogs_row_lse: exact (they are copies / comparisons of the inputs).
  * lse of cogs_row_lse: the yardstick is torch.logsumexp in fp32 on the CPU for the same rows, both measured against
    fp64; ours may be at most 2 x that error (another summation order in the same precision), with a floor of 4 fp32
    ulps. An "ulp" is the fp32 spacing at max(|lse|, |lse - max|): lse is the fp32 sum max + log(sum exp(x - max)) of an
    exact first term and a rounded second one, so its rounding error scales with the larger of the result and that second
    term (when max ~ -log(...) the result cancels towards 0 and its own spacing says nothing about the terms).
  * fp32 parity mode against fixtures: 1e-4 of the maximum (the project's fp32 bar, tests/test_gpu_golden.py).
  * bf16 against fixtures: test_gpu_golden._as_good_as_reference_bf16 (the reference's own bf16 error, slack 1.5).
  * production size: the per-element bound of tests/gemm_reference.py for an fp32-output GEMM."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def _spacing32(x: torch.Tensor) -> torch.Tensor:
    """fp32 spacing at |x| (fp64 in, fp64 out)"""
    a = x.abs().float().clamp_min(2.0 ** -126)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


class _switches:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from cogstream_amd import _lib as L
        self.cms = [L.debug_switch(k, v) for k, v in self.kw.items()]
        for c in self.cms:
            c.__enter__()

    def __exit__(self, *exc):
        for c in reversed(self.cms):
            c.__exit__(*exc)
        return False


def _check_row_lse(x_cpu: torch.Tensor, targets_cpu, dev, what: str, stride_pad: int = 0):
    """run ops.row_lse on x (fp32 [rows, n], optionally inside a wider buffer) with guard words around every output and
    compare with fp64 / the fp32 CPU yardstick. Returns (result dict, geometry the library reports)."""
    from cogstream_amd import _lib as L
    from cogstream_amd import ops
    rows, n = x_cpu.shape
    if stride_pad:
        wide = torch.full((rows, n + stride_pad), 1e30, dtype=torch.float32)      # a read past column n would win every maximum
        wide[:, :n] = x_cpu
        xd = wide.to(dev)[:, :n]
        assert rows == 1 or not xd.is_contiguous()
    else:
        xd = x_cpu.to(dev)
    G = 8
    guards = {}
    out = {}
    for key, dt, fill in (("lse", torch.float32, 12345.0), ("target_logit", torch.float32, 12345.0),
                          ("max_logit", torch.float32, 12345.0), ("argmax", torch.int64, -7), ("n_bad", torch.int32, -7)):
        m = 1 if key == "n_bad" else rows
        buf = torch.full((m + 2 * G,), fill, dtype=dt, device=dev)
        guards[key] = (buf, fill, m)
        out[key] = buf[G:G + m]
    td = None if targets_cpu is None else targets_cpu.to(dev)
    res = ops.row_lse(xd, td, out=out)
    geo = {k: L.debug_get("lm_score_last_" + k) for k in ("rows", "cols", "split", "chunk")}
    torch.cuda.synchronize()
    for key, (buf, fill, m) in guards.items():
        assert bool((buf[:G] == fill).all()) and bool((buf[G + m:] == fill).all()), f"{what}: guard words of {key} overwritten"
    lse, tl, mx, am = (res[k].cpu() for k in ("lse", "target_logit", "max_logit", "argmax"))
    x64 = x_cpu.double()
    # exact outputs
    assert torch.equal(mx, x_cpu.max(dim=1).values), what
    assert am.tolist() == np.argmax(x_cpu.numpy(), axis=1).tolist(), what          # numpy: first maximum
    t = torch.full((rows,), -100, dtype=torch.int64) if targets_cpu is None else targets_cpu
    valid = (t >= 0) & (t < n)
    want_tl = torch.zeros(rows)
    want_tl[valid] = x_cpu[valid, t[valid]]
    assert torch.equal(tl, want_tl), what
    assert int(res["n_bad"].item()) == int(((~valid) & (t != -100)).sum()), what
    # lse against the fp32 CPU yardstick
    lse64 = torch.logsumexp(x64, dim=1)
    lse32 = torch.logsumexp(x_cpu, dim=1).double()
    fin = torch.isfinite(lse64)
    assert torch.equal(lse[~fin].double(), lse64[~fin]), what                       # -inf rows stay -inf, no NaN
    assert not bool(torch.isnan(lse).any()), what
    unit = _spacing32(torch.maximum(lse64.abs(), (lse64 - x64.max(dim=1).values).abs()))[fin]
    e_ours = (lse.double() - lse64).abs()[fin]
    e_torch = (lse32 - lse64).abs()[fin]
    allowed = torch.maximum(2 * e_torch, 4 * unit)
    print(f"row_lse {what} panel {geo['rows']}x{geo['cols']} split {geo['split']} chunk {geo['chunk']}: lse error ours max "
          f"{float((e_ours / unit).max()):.2f} ulp, torch fp32 CPU max {float((e_torch / unit).max()):.2f} ulp")
    worst = int((e_ours - allowed).argmax())
    assert bool((e_ours <= allowed).all()), (what, worst, float(e_ours[worst]), float(allowed[worst]))
    return res, geo


def _boundary_targets(rows: int, n: int, geo: dict) -> torch.Tensor:
    """targets at column 0, n - 1, on both sides of every panel and column-split boundary, plus one ignored row and one
    out-of-range target (only when there are rows to spare)"""
    cand = {0, n - 1}
    for c0 in range(0, n, geo["cols"]):
        for c in range(c0, min(n, c0 + geo["cols"]), geo["chunk"]):
            cand.update({c, c - 1})
    cand = sorted(c for c in cand if 0 <= c < n)
    t = torch.tensor([cand[i % len(cand)] for i in range(rows)], dtype=torch.int64)
    if rows >= len(cand) + 2:
        t[-1], t[-2] = -100, n + 3
    return t


def _geometry(rows, n, dev):
    from cogstream_amd import _lib as L
    from cogstream_amd import ops
    ops.row_lse(torch.zeros(rows, n, device=dev))
    return {k: L.debug_get("lm_score_last_" + k) for k in ("rows", "cols", "split", "chunk")}


SMALL_N = [4, 60, 64, 68, 252, 256, 260]


@pytest.mark.parametrize("split", [0, 4])
@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65])
def test_row_lse_small_rows_panel_and_split_edges(dev, rows, split):
    """panels forced to 256 columns (n = panel - 4 / panel / panel + 4 among others) and, with split = 4, 64-column
    workgroup chunks: every boundary has a target on both sides; non-contiguous rows"""
    for n in SMALL_N:
        g = torch.Generator().manual_seed(1000 * rows + n)
        x = torch.randn(rows, n, generator=g) * 3
        with _switches(lm_score_cols=256, lm_score_split=split):
            geo = _geometry(rows, n, dev)
            assert geo["cols"] == min(n, 256) and geo["rows"] == rows
            if split:
                assert geo["chunk"] == 64 or n < 256
            _check_row_lse(x, _boundary_targets(rows, n, geo), dev, f"rows {rows} n {n} split {split}", stride_pad=12)


@pytest.mark.parametrize("rows", [1, 2, 65])
@pytest.mark.parametrize("cols", [0, 8192])
def test_row_lse_vocabulary_width(dev, rows, cols):
    """n = 152 064 with few rows: the columns of a panel are split over workgroups (asserted), as one panel and as 19
    panels of 8 192"""
    n = 152064
    g = torch.Generator().manual_seed(rows + cols)
    x = torch.randn(rows, n, generator=g) * 3
    with _switches(lm_score_cols=cols):
        geo = _geometry(rows, n, dev)
        assert geo["split"] > 1, geo                                  # few rows: column split
        assert geo["cols"] == (n if cols == 0 else cols)
        _check_row_lse(x, _boundary_targets(rows, n, geo), dev, f"rows {rows} n {n} cols {cols}")


@pytest.mark.parametrize("rows", [2047, 2048, 2049])
def test_row_lse_row_block_edges(dev, rows):
    """the default row block (2 048) - 1 / + 0 / + 1 with the default 8 192-column panel - 4 / + 0 / + 4; many rows: one
    workgroup per row (asserted)"""
    for n in (60, 8188, 8192, 8196):
        g = torch.Generator().manual_seed(rows + n)
        x = torch.randn(rows, n, generator=g) * 3
        geo = _geometry(rows, n, dev)
        assert geo["rows"] == min(rows, 2048) and geo["split"] == 1, geo
        if rows >= 2048:
            assert geo["cols"] == min(n, 8192)
        _check_row_lse(x, _boundary_targets(rows, n, geo), dev, f"rows {rows} n {n}", stride_pad=4 if n == 8196 else 0)


def test_row_lse_special_values(dev):
    """ties of the maximum across a column-split and a panel boundary (first wins), the maximum in the LAST panel (the
    running sum is rescaled), logits of +-80, a row of -inf with one finite entry, all rows ignored / none ignored, an
    out-of-range target"""
    rows, n = 8, 1024
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, n, generator=g) * 2
    x[0, 127] = x[0, 128] = 9.0                 # tie across a split boundary (chunk 128)
    x[1, 255] = x[1, 256] = 9.0                 # tie across a panel boundary (panel 256)
    x[2, 1000] = 40.0                           # maximum in the last panel
    x[2, 3] = 25.0
    x[3] = torch.where(torch.arange(n) % 2 == 0, torch.tensor(80.0), torch.tensor(-80.0))
    x[4] = float("-inf")
    x[4, 700] = 1.5
    x[5, 0] = x[5, n - 1] = 11.0                # tie of the first and the last column
    x[6] = float("-inf")                        # nothing finite at all: lse -inf, argmax 0 (torch)
    x[7, 512] = -80.0
    with _switches(lm_score_cols=256, lm_score_split=2):
        geo = _geometry(rows, n, dev)
        assert geo["cols"] == 256 and geo["chunk"] == 128 and geo["split"] == 2
        t_mixed = torch.tensor([127, 256, 1000, 1, 700, n - 1, 5, -100])
        res, _ = _check_row_lse(x, t_mixed, dev, "special values")
        assert res["argmax"].tolist()[:6] == [127, 255, 1000, 0, 700, 0]
        assert float(res["lse"][4]) == 1.5 and float(res["lse"][6]) == float("-inf")
        _check_row_lse(x, torch.full((rows,), -100), dev, "all rows ignored")
        _check_row_lse(x, None, dev, "no targets")
        _check_row_lse(x, torch.arange(rows) * 100, dev, "no row ignored")
        res, _ = _check_row_lse(x, torch.tensor([n, -1, 2 ** 40, -100, 0, 1, 2, 3]), dev, "out-of-range targets")
        assert int(res["n_bad"].item()) == 3 and res["target_logit"][:4].tolist() == [0, 0, 0, 0]


def test_row_lse_rejects_unaligned_shapes(dev):
    from cogstream_amd import _lib as L
    from cogstream_amd import ops
    with pytest.raises(L.CogsError):
        ops.row_lse(torch.zeros(2, 6, device=dev))                    # n % 4
    with pytest.raises(L.CogsError):
        ops.row_lse(torch.zeros(2, 10, device=dev)[:, :8])            # row stride % 4


@pytest.mark.parametrize("rows,n,cols", [(3, 152064, 8192), (300, 4096, 1024), (2049, 2052, 0)])
def test_row_lse_same_call_twice_gives_identical_bits(dev, rows, n, cols):
    from cogstream_amd import ops
    x = (torch.randn(rows, n, generator=torch.Generator().manual_seed(n)) * 4).to(dev)
    t = torch.randint(0, n, (rows,), generator=torch.Generator().manual_seed(rows)).to(dev)
    with _switches(lm_score_cols=cols):
        a = ops.row_lse(x, t)
        b = ops.row_lse(x, t)
    for k in ("lse", "target_logit", "max_logit"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.equal(a["argmax"], b["argmax"])


# ---------------------------------------------------------------------------------------------- C ABI

_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "cogs_handle": C.c_void_p, "cogs_stream": C.c_void_p, "cogs_status": C.c_int}


def _bind_from_header(lib, name):
    """argtypes / restype of `name` from its declaration in include/cogs.h (pointers -> void*)"""
    hdr = open(os.path.join(ROOT, "include", "cogs.h")).read()
    m = re.search(r"^(\w+)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.M | re.S)
    assert m, f"{name} is not declared in include/cogs.h"
    args = []
    for p in m.group(2).split(","):
        p = p.strip()
        if "*" in p:
            args.append(C.c_void_p)
        else:
            ty = p.replace("const", "").split()[0]
            args.append(_CTYPES[ty])
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _CTYPES[m.group(1)], args
    return fn


def _lm_head_only(dev, H, V, dtype, lm_head=None):
    """a handle whose LLM table holds nothing but an lm_head (cogs_lm_score reads no other weight)"""
    from cogstream_amd import _lib as L
    lib = C.CDLL(str(L.LIB_PATH))
    h = C.c_void_p()
    create = _bind_from_header(lib, "cogs_create")
    assert create(dev.index or 0, C.byref(h)) == 0
    layers = (L.LlmLayer * 1)()
    w = L.LlmWeights()
    w.dtype = L.dtype_code(dtype)
    w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = H, 512, 1, H // 128, H // 128, 128, V
    w.rms_eps, w.rope_theta = 1e-6, 1e6
    w.lm_head = 0 if lm_head is None else lm_head.data_ptr()
    w.layer = layers
    L.check(L.lib.cogs_llm_load(h, C.byref(w)), "cogs_llm_load")
    return lib, h, (layers, w)


def test_lm_score_abi_status_codes_and_workspace_bound(dev):
    """declarations taken from the header text: S <= 0 and a handle without LLM are COGS_E_INVALID, a short workspace is
    COGS_E_WORKSPACE; at H 3 584 / V 152 064 the workspace stays within 64 MiB + 64 bytes per row"""
    from cogstream_amd import _lib as L
    lib, h, keep = _lm_head_only(dev, 3584, 152064, torch.bfloat16)
    ws_bytes = _bind_from_header(lib, "cogs_lm_score_workspace_bytes")
    score = _bind_from_header(lib, "cogs_lm_score")
    destroy = _bind_from_header(lib, "cogs_destroy")
    n = C.c_size_t()
    sizes = {}
    for S in (1, 4096, 16384):
        assert ws_bytes(h, S, C.byref(n)) == L.OK
        sizes[S] = n.value
        assert n.value <= (64 << 20) + 64 * S, (S, n.value)
    print("cogs_lm_score workspace bytes:", sizes)
    assert ws_bytes(h, 0, C.byref(n)) == L.E_INVALID
    hid = torch.zeros(4, 3584, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(4, device=dev)
    ws = torch.zeros(1024, device=dev, dtype=torch.uint8)
    st = L.current_stream()
    assert score(h, st, hid.data_ptr(), 0, None, lse.data_ptr(), None, None, None, None, ws.data_ptr(), ws.numel()) == L.E_INVALID
    assert score(h, st, hid.data_ptr(), 4, None, lse.data_ptr(), None, None, None, None, ws.data_ptr(), ws.numel()) == L.E_WORKSPACE
    assert score(h, st, hid.data_ptr(), 4, None, lse.data_ptr(), None, None, None, None, None, 1 << 30) == L.E_WORKSPACE
    bare = C.c_void_p()
    assert _bind_from_header(lib, "cogs_create")(dev.index or 0, C.byref(bare)) == 0
    assert ws_bytes(bare, 4, C.byref(n)) == L.E_INVALID
    assert score(bare, st, hid.data_ptr(), 4, None, lse.data_ptr(), None, None, None, None, ws.data_ptr(), ws.numel()) == L.E_INVALID
    row_ws = _bind_from_header(lib, "cogs_row_lse_workspace_bytes")
    row = _bind_from_header(lib, "cogs_row_lse")
    assert row_ws(0, 8, C.byref(n)) == L.E_INVALID
    x = torch.zeros(4, 8, device=dev)
    assert row(st, x.data_ptr(), 4, 8, 8, None, lse.data_ptr(), None, None, None, None, None, 0) == L.E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((lse == 0).all())                                       # nothing ran
    destroy(h)
    destroy(bare)


# ---------------------------------------------------------------------------------------------- engine


def _engine(tag, dtype, dev):
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    g = _load("score.npz")
    lcfg = LlmConfig(**json.loads(str(g[f"{tag}_cfg"])))
    lst = random_llm_state(lcfg, seed=7, std=0.05)
    assert abs(float(sum(v.double().abs().sum() for v in lst.values())) - float(g[f"{tag}_llm_checksum"])) < 1e-6
    return g, Qwen2Engine(lst, lcfg, dtype=dtype, device=dev)


def _shifted(labels: torch.Tensor) -> torch.Tensor:
    t = torch.full_like(labels, -100)
    t[:-1] = labels[1:]
    return t


@pytest.mark.parametrize("tag", ["t", "g"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_engine_score_vs_reference_fixture(dev, tag, dtype):
    """Qwen2Engine.score against what Qwen2ForCausalLM.forward(labels=) of the reference's model object gave
    (score.npz). fp32 parity mode: log-probabilities and loss within 1e-4, argmax equal on every scored row (the
    fixture guarantees a top-1/top-2 margin of 100 x that bar there) and on every other row with that margin. bf16:
    as good as the reference's own bf16 run."""
    from test_gpu_golden import _as_good_as_reference_bf16, _dist
    g, eng = _engine(tag, dtype, dev)
    labels = torch.from_numpy(g[f"{tag}_labels"])
    tgt = _shifted(labels)
    scored = tgt != -100
    res = eng.score(torch.from_numpy(g[f"{tag}_embeds"]).to(dev, dtype), tgt)
    lp, lse, am = res["logprobs"].cpu(), res["lse"].cpu(), res["argmax"].cpu()
    assert bool((lp[~scored] == 0).all())
    loss = float(-lp[scored].double().mean())
    ref32 = {k: torch.from_numpy(g[f"{tag}_{k}_f32"]) for k in ("logprob", "lse", "argmax", "margin")}
    loss32 = float(g[f"{tag}_loss_f32"])
    if dtype == torch.float32:
        for name, got, want in (("logprob", lp, ref32["logprob"]), ("lse", lse, ref32["lse"])):
            m, r = _dist(got, want)
            print(f"score[{tag}] fp32 {name}: max {m:.2e} rms {r:.2e}")
            assert m < 1e-4 and r < 1e-4, (name, m, r)
        print(f"score[{tag}] fp32 loss {loss:.7f} vs {loss32:.7f}")
        assert abs(loss - loss32) < 1e-4 * abs(loss32)
        assert torch.equal(am[scored], ref32["argmax"][scored])
        clear = ref32["margin"] >= float(g["margin_bar"]) * float(g[f"{tag}_maxabs_f32"])
        assert bool(clear[scored].all()) and torch.equal(am[clear], ref32["argmax"][clear])
    else:
        ref16 = torch.from_numpy(g[f"{tag}_logprob_bf16"])
        _as_good_as_reference_bf16(lp[scored], ref16[scored], ref32["logprob"][scored], f"score[{tag}] logprob")
        ref_gap = abs(float(g[f"{tag}_loss_bf16"]) - loss32)
        print(f"score[{tag}] bf16 loss {loss:.5f}; reference bf16 {float(g[f'{tag}_loss_bf16']):.5f}, fp32 {loss32:.5f}")
        assert abs(loss - loss32) <= 1.5 * ref_gap, (loss, loss32, ref_gap)
    with pytest.raises(ValueError):
        bad = tgt.clone()
        bad[3] = eng.cfg.vocab_size
        eng.score(torch.from_numpy(g[f"{tag}_embeds"]).to(dev, dtype), bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_score_agrees_with_generate_and_last_row_logits(dev, dtype):
    """inside the product: (fp32 parity mode) greedy generate n tokens, then score prompt + tokens -> the argmax behind
    every answer position is the generated token. Both precisions: the last row's argmax equals the argmax of the
    logits forward() gives for the same hidden row, for S = 1 (GEMV path) and S > 1; logits() of the last rows agrees with
    forward()'s last-row logits (a 2-row GEMM against the GEMV: summation order only)."""
    g, eng = _engine("t", dtype, dev)
    P = int(g["t_prompt_len"])
    emb = torch.from_numpy(g["t_embeds"]).to(dev, dtype)[:P]
    if dtype == torch.float32:
        n = 6
        toks = eng.generate(emb, max_new_tokens=n, eos_token_id=[], do_sample=False)
        assert len(toks) == n
        tk = torch.tensor(toks, dtype=torch.int64)
        rows = torch.cat([emb, eng.embed_tokens(tk[:-1])], dim=0)
        tgt = torch.cat([torch.full((P - 1,), -100, dtype=torch.int64), tk])
        res = eng.score(rows, tgt)
        assert res["argmax"][P - 1:].tolist() == toks
        assert float(res["logprobs"][P - 1:].max()) < 0 and bool((res["logprobs"][:P - 1] == 0).all())
    for S in (1, 2, P):
        f = eng.forward(emb[:S], None, want_logits=True, want_hidden=True)
        sc = eng.score_hidden(f["hidden"], torch.full((S,), -100, dtype=torch.int64))
        assert int(sc["argmax"][-1]) == int(f["logits"].argmax()), S
        assert float(sc["lse"][-1]) == pytest.approx(float(torch.logsumexp(f["logits"].double(), 0)), rel=1e-5)
        if S > 1:
            k = min(S, 2)
            lg = eng.logits(f["hidden"][-k:])
            assert lg.shape == (k, eng.cfg.vocab_size) and lg.dtype == torch.float32
            assert rel_err(lg[-1], f["logits"]) < 1e-5
            assert sc["argmax"][-k:].tolist() == lg.argmax(dim=1).tolist()
    if dtype == torch.float32:      # the plain decode call (final norm fused into the GEMV) agrees as well
        assert int(eng.score(emb[:1], torch.tensor([-100]))["argmax"][0]) == int(eng.forward(emb[:1], None)["logits"].argmax())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_continuations_scored_against_one_prefilled_prompt(dev, dtype):
    """k continuations against ONE prefilled cache (cache.reset(prompt_len) in between) vs the k concatenations scored
    from scratch. Continuations of >= 2 rows go through the prefill kernels on both sides: rows behind a cache see the
    same GEMM rows and the same keys in the same order, and the two results are bit-identical (asserted). A 1-row
    continuation is the decode GEMV path, whose rounding differs from the prefill GEMMs (llm.PrefixKV.plan): it must
    work, and is held to the fp32 bar in parity mode only."""
    g, eng = _engine("g", dtype, dev)
    P = int(g["g_prompt_len"])
    emb = torch.from_numpy(g["g_embeds"]).to(dev, dtype)
    prompt = emb[:P]
    gen = torch.Generator().manual_seed(3)
    conts = [torch.randint(0, eng.cfg.vocab_size, (n,), generator=gen) for n in (2, 5, 12, 3)]
    cache = eng.new_cache(P + 16)
    eng.forward(prompt[:P - 1], cache, want_logits=False, want_hidden=True)
    for ids in conts + [conts[0][:1]]:
        n = ids.numel()
        rows = torch.cat([prompt[P - 1:], eng.embed_tokens(ids[:-1])], dim=0) if n > 1 else prompt[P - 1:]
        cache.reset(P - 1)
        a = eng.score(rows, ids, cache=cache)
        assert cache.len == P - 1 + n
        full = eng.score(torch.cat([prompt[:P - 1], rows], dim=0), torch.cat([torch.full((P - 1,), -100, dtype=torch.int64), ids]))
        b = {k: v[P - 1:] for k, v in full.items()}
        same = all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                               b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in a)
        d = float((a["logprobs"] - b["logprobs"]).abs().max())
        print(f"shared prefix {dtype} n={n}: bit-identical {same}, max |dlogprob| {d:.2e}")
        if n >= 2:
            assert same, (n, d)
        else:
            assert bool(torch.isfinite(a["logprobs"]).all()) and float(a["logprobs"][0]) < 0
            if dtype == torch.float32:
                assert d <= 1e-4 * float(b["logprobs"].abs().max()), (n, d)
                assert torch.equal(a["argmax"], b["argmax"])


# ---------------------------------------------------------------------------------------------- CogReasoner


def _tiny_model(dev, dtype, attn_mode):
    from test_gpu_golden import _tiny_model as make
    return make(dev, dtype, attn_mode)


@pytest.mark.parametrize("mode", ["eager", "blockdiag"])
@pytest.mark.parametrize("tag", ["a", "c"])
def test_forward_train_end_to_end_vs_reference(dev, mode, tag):
    """CogReasoner.forward_train on the e2e clips (a: 8 frames + history, c: 150 frames with forced event cosines ->
    event compression), token compression on, fp32 parity mode, in both encoder attention modes, against the loss the
    reference's forward_train gave under no_grad (score_e2e.npz): ids, boundary and compacted labels equal, loss and
    per-position log-probabilities within the fp32 bar."""
    from golden.inputs import FORCED_COSINE, e2e_inputs
    from test_gpu_golden import _dist
    from toy_tokenizer import ToyTokenizer
    g = _load("score_e2e.npz")
    k = f"{mode}_{tag}"
    inp = e2e_inputs(tag)
    assert abs(float(inp["pixel_values"].double().abs().sum()) - float(g[f"{k}_pix_checksum"])) < 1e-6
    model = _tiny_model(dev, torch.float32, 1 if mode == "eager" else 0)
    model.cosine_override = FORCED_COSINE if tag == "c" else None
    tok = ToyTokenizer()
    enc = tok(inp["text"])
    random.seed(5)
    torch.manual_seed(5)
    out = model.forward_train(input_ids=enc["input_ids"], attention_mask=enc["attention_mask"],
                              pixel_values=inp["pixel_values"], grid_sizes=inp["grid_sizes"], merge_sizes=inp["merge_sizes"],
                              modals=["video"], tokenizer=tok, hist_qs=inp["hist_qs"], hist_as=inp["hist_as"],
                              current_question=inp["current_question"], all_timestamps=inp["timestamps"],
                              total_image_num=inp["T"], answer=str(g[f"{k}_answer"]), cor=g[f"{k}_cor"].tolist(),
                              if_visual=True, original_text=inp["text"], num_logits_to_keep=1)
    assert torch.equal(model.last_debug["train_input_ids"], torch.from_numpy(g[f"{k}_input_ids"]))
    assert model.last_debug["train_prompt_tokens"] == int(g[f"{k}_prompt_tokens"])
    assert torch.equal(out.labels[0], torch.from_numpy(g[f"{k}_labels"]))
    S = out.labels.shape[1]
    assert out.logits.shape == (1, 1, 512) and out.token_logprobs.shape == (1, S)
    ref_lp = torch.zeros(S, dtype=torch.float64)
    ref_lp[1:] = torch.from_numpy(g[f"{k}_logprob"])[:-1]              # the fixture indexes by row, the product by label position
    m, r = _dist(out.token_logprobs[0], ref_lp)
    print(f"forward_train[{k}] loss {float(out.loss):.7f} vs {float(g[f'{k}_loss']):.7f}; token logprobs max {m:.2e} rms {r:.2e}")
    assert out.loss.dtype == torch.float32 and out.loss.dim() == 0
    assert abs(float(out.loss) - float(g[f"{k}_loss"])) < 1e-4 * float(g[f"{k}_loss"])
    assert m < 1e-4 and r < 1e-4
    assert bool((out.token_logprobs[0].cpu()[out.labels[0] == -100] == 0).all())


def test_forward_text_path_and_score_answers(dev):
    """forward(input_ids=, labels=) without pixels against the reference's text path; __call__ is forward; score_answers
    prefills the multimodal prompt once and ranks the reference's greedy answer (e2e.npz) above the same tokens
    shuffled, with numbers equal to forward(labels=) on prompt + answer."""
    from golden.inputs import e2e_inputs
    from toy_tokenizer import ToyTokenizer
    g, e = _load("score.npz"), _load("e2e.npz")
    model = _tiny_model(dev, torch.float32, 1)
    ids = torch.from_numpy(g["text_input_ids"])[None]
    labels = torch.from_numpy(g["text_labels"])[None]
    out = model(input_ids=ids, attention_mask=torch.ones_like(ids), labels=labels, num_logits_to_keep=2)
    print(f"forward text path: loss {float(out.loss):.7f} vs {float(g['text_loss']):.7f}")
    assert abs(float(out.loss) - float(g["text_loss"])) < 1e-4 * float(g["text_loss"])
    ref_lp = torch.zeros(ids.shape[1], dtype=torch.float64)
    ref_lp[1:] = torch.from_numpy(g["text_logprob"])[:-1]
    assert rel_err(out.token_logprobs[0], ref_lp) < 1e-4
    assert out.logits.shape == (1, 2, 512)
    every = model.forward(input_ids=ids, labels=labels)                # 0 = all rows, as transformers
    assert every.logits.shape == (1, ids.shape[1], 512) and torch.equal(every.logits[0, -2:], out.logits[0])
    lp_from_logits = torch.log_softmax(every.logits[0].double(), -1)[:-1].gather(1, ids[0, 1:, None].to(dev))[:, 0]
    keep = (labels[0, 1:] != -100).to(dev)
    assert rel_err(out.token_logprobs[0, 1:][keep], lp_from_logits[keep]) < 1e-5
    assert torch.isnan(model(input_ids=ids, labels=torch.full_like(labels, -100), num_logits_to_keep=1).loss)

    inp = e2e_inputs("a")
    tok = ToyTokenizer()
    enc = tok(inp["text"])
    random.seed(5)
    torch.manual_seed(5)
    sel = model.qa_selection(current_question=inp["current_question"], hist_qs=inp["hist_qs"], hist_as=inp["hist_as"],
                             tokenizer=tok, original_text=inp["text"], input_ids=enc["input_ids"],
                             attention_mask=enc["attention_mask"], mode="FCC", all_timestamps=inp["timestamps"])
    greedy = e["a_tokens"].tolist()
    perm = torch.randperm(len(greedy), generator=torch.Generator().manual_seed(1)).tolist()
    shuffled = [greedy[i] for i in perm]
    assert shuffled != greedy
    calls = []
    orig = model.encode_images
    model.encode_images = lambda *a, **k: calls.append(1) or orig(*a, **k)
    sc = model.score_answers(pixel_values=inp["pixel_values"], grid_sizes=inp["grid_sizes"], merge_sizes=inp["merge_sizes"],
                             modals=["video"], new_input_ids=sel["new_input_ids"], new_attention_mask=sel["new_attention_mask"],
                             selection_module_output=sel["selection_module_output"], if_visual=sel["if_visual"],
                             total_image_num=inp["T"], answers=[greedy, shuffled, greedy[:1], "A man.", ""])
    model.encode_images = orig
    assert len(calls) == 1                                              # one encode for all candidates
    print("score_answers:", sc)
    assert [s["n_tokens"] for s in sc] == [len(greedy), len(greedy), 1, 6, 0]
    assert sc[0]["sum_logprob"] > sc[1]["sum_logprob"] and sc[0]["mean_logprob"] > sc[1]["mean_logprob"]
    assert sc[4]["sum_logprob"] == 0.0 and sc[4]["mean_logprob"] != sc[4]["mean_logprob"]
    # the same number through forward(labels=) on prompt + answer
    p_ids = sel["new_input_ids"]
    full = torch.cat([p_ids, torch.tensor([greedy])], dim=1)
    lab = torch.cat([torch.full_like(p_ids, -100), torch.tensor([greedy])], dim=1)
    ref = model.forward(input_ids=full, attention_mask=torch.ones_like(full), labels=lab, pixel_values=inp["pixel_values"],
                        grid_sizes=inp["grid_sizes"], merge_sizes=inp["merge_sizes"], modals=["video"],
                        total_image_num=inp["T"], if_visual=sel["if_visual"], num_logits_to_keep=1)
    assert sc[0]["mean_logprob"] == pytest.approx(-float(ref.loss), rel=1e-4)
    assert sc[2]["sum_logprob"] == pytest.approx(float(ref.token_logprobs[0, -len(greedy)]), rel=1e-4)


# ---------------------------------------------------------------------------------------------- production size


def test_lm_score_at_production_size_vs_fp64(dev):
    """H 3 584, V 152 064, S 4 096, bf16 weights drawn on the GPU: cogs_lm_score against fp64 torch in row chunks of
    256. The panel IS the output of an fp32-output bf16 GEMM, so target_logit / max_logit get the per-element band of
    tests/gemm_reference.py (product_and_bound + the fp32 store), lse the row's largest such band (d lse / d logit sums to
    1) plus the fold's own error (4 fp32 ulps, test_row_lse_*), argmax must be equal on every row whose reference
    top-1/top-2 margin exceeds twice the row's band; at most 1 % of the rows may lie below that (asserted, printed).
    Peak device memory during the call rises by no more than workspace + outputs; the many-row walk takes one workgroup
    per row, a 4-row call splits the columns (lm_score_last_split)."""
    from cogstream_amd import _lib as L
    from gemm_reference import epilogue, product_and_bound
    H, V, S = 3584, 152064, 4096
    gen = torch.Generator(device=dev).manual_seed(20260101)
    w = (torch.randn(V, H, device=dev, generator=gen) * 0.02).bfloat16()
    # A trained head puts one token well ahead on most rows; i.i.d. logits would not (the top-1/top-2 gap of 152 064
    # Gaussians is below twice the GEMM band on ~14 % of the rows). So 98 % of the rows carry 7 x the lm_head row of a
    # drawn token on top of unit noise: that token's logit is ~10 against ~6 for the best of the rest (sigma 1.2);
    # every 50th row stays plain noise. The drawn token is the row's target, except on the ignored rows.
    planted = torch.randint(0, V, (S,), device=dev, generator=gen)
    hid = torch.randn(S, H, device=dev, generator=gen)
    keep_plain = torch.arange(S, device=dev) % 50 == 49
    hid = torch.where(keep_plain[:, None], hid, hid + 7.0 * w[planted].float()).bfloat16()
    tgt = planted.clone()
    tgt[::97] = -100
    lib, h, keep = _lm_head_only(dev, H, V, torch.bfloat16, w)
    ws_bytes = _bind_from_header(lib, "cogs_lm_score_workspace_bytes")
    score = _bind_from_header(lib, "cogs_lm_score")
    n = C.c_size_t()
    assert ws_bytes(h, S, C.byref(n)) == 0
    ws = torch.empty(n.value, device=dev, dtype=torch.uint8)
    lse, tl, mx = (torch.empty(S, device=dev) for _ in range(3))
    am = torch.empty(S, device=dev, dtype=torch.int64)
    nbad = torch.empty(1, device=dev, dtype=torch.int32)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    rc = score(h, L.current_stream(), hid.data_ptr(), S, tgt.data_ptr(), lse.data_ptr(), tl.data_ptr(), am.data_ptr(),
               mx.data_ptr(), nbad.data_ptr(), ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    assert rc == 0
    rise = torch.cuda.max_memory_allocated(dev) - before
    print(f"cogs_lm_score S {S}: workspace {n.value / 2**20:.2f} MiB, peak memory rise during the call {rise} bytes")
    assert rise <= n.value + 5 * S * 8                                   # (everything was allocated before: the rise is 0)
    assert L.debug_get("lm_score_last_split") == 1 and L.debug_get("lm_score_last_rows") == 2048
    assert L.debug_get("lm_score_last_cols") == 8192 and L.debug_get("gemm_last_body") != 6
    assert int(nbad.item()) == 0
    w64 = None
    below = 0
    worst = {"tl": 0.0, "mx": 0.0, "lse": 0.0}
    for r0 in range(0, S, 256):
        a = hid[r0:r0 + 256]
        acc, bound = product_and_bound(a, w)                             # fp64 [256, V] on the device
        ref, tol = epilogue(acc, bound, out_f32=True)
        t = tgt[r0:r0 + 256]
        ok = t != -100
        idx = t.clamp_min(0)[:, None]
        e_tl = (tl[r0:r0 + 256].double() - ref.gather(1, idx)[:, 0]).abs()
        band_tl = tol.gather(1, idx)[:, 0]
        assert bool((e_tl[ok] <= band_tl[ok]).all()) and bool((tl[r0:r0 + 256][~ok] == 0).all()), r0
        top2 = ref.topk(2, dim=1)
        band_row = tol.max(dim=1).values
        e_mx = (mx[r0:r0 + 256].double() - top2.values[:, 0]).abs()
        assert bool((e_mx <= band_row).all()), r0
        lse64 = torch.logsumexp(ref, dim=1)
        unit = _spacing32(torch.maximum(lse64.abs(), (lse64 - top2.values[:, 0]).abs()).cpu()).to(dev)
        e_lse = (lse[r0:r0 + 256].double() - lse64).abs()
        assert bool((e_lse <= band_row + 4 * unit).all()), (r0, float((e_lse / (band_row + 4 * unit)).max()))
        clear = (top2.values[:, 0] - top2.values[:, 1]) > 2 * band_row
        below += int((~clear).sum())
        assert torch.equal(am[r0:r0 + 256][clear], top2.indices[:, 0][clear]), r0
        worst["tl"] = max(worst["tl"], float((e_tl[ok] / band_tl[ok]).max()))
        worst["mx"] = max(worst["mx"], float((e_mx / band_row).max()))
        worst["lse"] = max(worst["lse"], float((e_lse / (band_row + 4 * unit)).max()))
        del acc, bound, ref, tol
    print(f"production size: worst error / band: target_logit {worst['tl']:.3f}, max_logit {worst['mx']:.3f}, lse {worst['lse']:.3f}; "
          f"{below} of {S} rows have a top-1/top-2 margin below twice their band (cap {S // 100})")
    assert below <= S // 100
    # few rows: the columns are split over workgroups, same numbers for those rows
    lse4 = torch.empty(4, device=dev)
    am4 = torch.empty(4, device=dev, dtype=torch.int64)
    assert score(h, L.current_stream(), hid.data_ptr(), 4, None, lse4.data_ptr(), None, am4.data_ptr(), None, None,
                 ws.data_ptr(), ws.numel()) == 0
    torch.cuda.synchronize()
    assert L.debug_get("lm_score_last_split") > 1 and L.debug_get("lm_score_last_cols") == V
    assert torch.equal(am4, am[:4]) and float((lse4 - lse[:4]).abs().max()) < 1e-3
    _bind_from_header(lib, "cogs_destroy")(h)
