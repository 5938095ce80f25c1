"""The attention launch plan (csrc/attn_plan.h, cogs_plan_attention / cogs_plan_attention_rows) pinned on the CPU.

tests/golden/attn_plan.json was recorded on an MI355X by tools/record_attn_plan.py at the commit it names, BEFORE the plan
became a function of its own: per cell of the sweep of tests/attn_plan_cells.py, at the shipped switches and with each plan
switch flipped alone, the status cogs_attention / cogs_attention_rows returned and the `attn_last_kernel` /
`attn_vit_last_end` reports behind an accepted call. The plan must give the same for every record. The fields no record
carries (instantiation, grid, derived kernel arguments, combine step, workspace) are asserted for the production shapes
from the constants written in the launchers at that commit."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

import attn_plan_cells as cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cogstream_amd", "csrc")
OK, E_INVALID, E_UNSUPPORTED, E_WORKSPACE = 0, -1, -3, -4      # include/cogs.h
COMBINE_NONE, COMBINE_HEAD, COMBINE_SLICE32 = 0, 1, 2


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    so = tmp_path_factory.mktemp("attn_plan") / "attn_plan_shim.so"
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "attn_plan_shim.cpp"),
                        "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    for f in ("attn_tuning_names", "attn_plan_names", "attn_query_names", "attn_rows_query_names"):
        getattr(lib, f).restype = C.c_char_p
    lib.attn_split_ws_bytes.restype = C.c_longlong
    return lib


def tuning_defaults(shim):
    names = shim.attn_tuning_names().decode().split()
    vals = (C.c_longlong * len(names))()
    shim.attn_tuning_defaults(vals)
    return dict(zip(names, vals))


def _tuning(shim, switches):
    t = tuning_defaults(shim)
    assert set(switches) <= set(t), switches
    t.update(switches)
    return (C.c_longlong * len(t))(*t.values())


def plan(shim, q, rows=False, **switches):
    """the AttnPlan of a query given as a dict of AttnQuery / AttnRowsQuery fields (tests/attn_plan_cells.py::query makes one)"""
    names = (shim.attn_rows_query_names if rows else shim.attn_query_names)().decode().split()
    vals = (C.c_longlong * len(names))(*(int(q[n]) for n in names))
    out_names = shim.attn_plan_names().decode().split()
    out = (C.c_longlong * len(out_names))()
    (shim.plan_attention_rows if rows else shim.plan_attention)(vals, _tuning(shim, switches), out)
    return dict(zip(out_names, out))


def query(**kw):
    """an AttnQuery: the struct's defaults + kw"""
    q = dict(bf16=1, head_dim=0, q_len=0, kv_len=0, hq=1, hkv=1, ldq=0, ldk=0, ldv=0, ldo=0, head_stride=0, has_cu=0, has_row_lo=0,
             has_ws=0, nseg=1, max_seqlen=0, uniform_seqlen=0, causal=0, q_pos0=0, q_prescaled=0, force_rowwise=0, nsplit=1, ws_bytes=0)
    assert set(kw) <= set(q), kw
    q.update(kw)
    return q


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "attn_plan.json")) as f:
        doc = json.load(f)
    assert len(doc["recorded_at_commit"]) == 40
    return doc


def test_tuning_defaults_are_the_shipped_switch_defaults(shim):
    """AttnTuning{} = the defaults of the same switches in csrc/debug.h"""
    text = open(os.path.join(CSRC, "debug.h")).read()
    shipped = {m.group(1): int(m.group(2)) for m in re.finditer(r"X\((\w+), (-?\d+)(?:LL)?,", text)}
    t = tuning_defaults(shim)
    assert len(t) == 9
    for name, value in t.items():
        assert shipped[name] == value, name


def test_fixture_is_the_sweep_of_the_cell_builder():
    doc = fixture()
    assert doc["cells"] == cells.cells() and doc["switches"] == cells.SWITCHED
    assert len(doc["records"]) == len(doc["cells"]) * len(doc["switches"])
    assert [r[:2] for r in doc["records"]] == [[c, s] for c in range(len(doc["cells"])) for s in range(len(doc["switches"]))]
    # every kernel and every status is somewhere in the records
    assert {r[3] for r in doc["records"]} == {0, 1, 2, 3, 4, 5, 7, 8}
    assert {r[2] for r in doc["records"]} == {OK, E_INVALID, E_UNSUPPORTED, E_WORKSPACE}
    assert {r[4] for r in doc["records"]} == {0} | set(cells.VIT_ENDS.values())


def test_plan_reproduces_every_recorded_choice(shim):
    doc = fixture()
    assert len(doc["records"]) >= 300
    for ci, si, status, kernel, vit_end in doc["records"]:
        cell, sw = doc["cells"][ci], doc["switches"][si]
        rows = cell.get("kind") == "rows"
        q = cells.query(cell)
        p = plan(shim, q, rows=rows, **sw)
        what = (cell, sw, p)
        assert p["status"] == status, what
        if status != OK:
            continue
        assert p["kernel"] == kernel and p["vit_end"] == vit_end, what
        # every ws_need against the formulas include/cogs.h documents
        if rows:
            assert p["ws_need"] == (q["nsplit"] + 1) * q["rows"] * q["hq"] * (q["head_dim"] + 2) * 4, what
            assert p["parts"] == q["nsplit"] + 1 and p["grid_x"] == q["nsplit"] * p["ntile"] + q["rows"] and p["grid_y"] == q["hkv"], what
            assert p["ntile"] == -(-q["rows"] * (q["hq"] // q["hkv"]) // 16) and p["rows_slot"] == q["has_slot"], what
        elif p["nsplit"] > 1:
            assert p["nsplit"] == q["nsplit"] and p["ws_need"] == q["nsplit"] * q["q_len"] * q["hq"] * (q["head_dim"] + 2) * 4, what
            assert p["ws_need"] <= q["ws_bytes"], what
        else:
            assert p["ws_need"] == 0 and p["combine"] == COMBINE_NONE, what
        # the fields are consistent with the report
        assert (p["combine"] != COMBINE_NONE) == (rows or p["nsplit"] > 1), what
        if p["combine"] != COMBINE_NONE:
            want = COMBINE_SLICE32 if q["head_dim"] % 32 == 0 and sw.get("attn_combine32", 1) else COMBINE_HEAD
            assert p["combine"] == want and p["combine_z"] == (q["head_dim"] // 32 if want == COMBINE_SLICE32 else 1), what
            assert p["part_ml_off"] * (q["head_dim"] + 2) * 4 == p["ws_need"] * q["head_dim"], what
        assert p["vit_pipe"] == (kernel in (3, 8)) and (p["vit_end"] == 10 * p["vit_r"] + p["vit_nlb"]), what
        if kernel == 1:
            assert p["hd"] == q["head_dim"] and p["nq"] in (1, 2) and p["block_x"] == 1024 // (2 * p["nq"]), what
            assert p["pre"] == q["q_prescaled"], what
        if kernel == 4:
            assert p["gqa_pack"] == 1 and (p["grid_x"], p["grid_y"], p["grid_z"]) == (q["nsplit"], q["hkv"], 1), what
        if kernel == 7:
            assert (p["grid_x"], p["grid_y"], p["grid_z"], p["block_x"]) == (q["q_len"], q["hq"], 1, 64), what


def test_cfg2_prompt_and_decode(shim):
    """Qwen2-7B at cfg2 as capi_llm.hip fills the descriptor: 28 / 4 heads, hd 128, causal, pre-scaled Q, K / V in the cache"""
    hq, hkv, hd, S = 28, 4, 128, 15395
    base = dict(head_dim=hd, hq=hq, hkv=hkv, ldq=(hq + 2 * hkv) * hd, ldk=hkv * hd, ldv=hkv * hd, ldo=hq * hd, causal=1, q_prescaled=1)
    p = plan(shim, query(q_len=S, kv_len=S, **base))
    assert (p["status"], p["kernel"]) == (OK, 5), p
    assert (p["grid_x"], p["grid_y"], p["grid_z"], p["block_x"]) == (121, 28, 1, 256), p
    assert (p["heavy_first"], p["nsplit"], p["gqa_pack"], p["q_prescaled"], p["combine"]) == (1, 1, 0, 1, COMBINE_NONE), p
    # the routing conditions no GPU cell exercises: O rows that are 8- but not 16-byte aligned
    # stay on the general kernel; a prompt behind a cached prefix stays on the prompt kernel whatever its length
    assert plan(shim, query(q_len=S, kv_len=S, **base), attn_light_first=1)["heavy_first"] == 0
    assert plan(shim, query(q_len=S, kv_len=S, **{**base, "ldo": hq * hd + 4}))["kernel"] == 1
    p = plan(shim, query(q_len=5, kv_len=S + 5, q_pos0=S, **base))
    assert (p["kernel"], p["grid_x"], p["heavy_first"]) == (5, 1, 0), p
    # the decode step behind the prompt
    t = _tuning(shim, {})
    ctx = S + 1
    nsplit = shim.attn_nsplit(ctx, t)
    need = shim.attn_split_ws_bytes(nsplit, 1, hq, hd)
    assert nsplit == 61 and need == 61 * 28 * 130 * 4
    dec = query(q_len=1, kv_len=ctx, q_pos0=S, nsplit=nsplit, has_ws=1, ws_bytes=need, **base)
    p = plan(shim, dec)
    assert (p["status"], p["kernel"], p["grid_x"], p["grid_y"], p["grid_z"], p["block_x"]) == (OK, 4, 61, 4, 1, 256), p
    assert (p["kend"], p["gsz"], p["nsplit"], p["gqa_pack"]) == (ctx, 7, 61, 1), p
    assert (p["combine"], p["combine_x"], p["combine_y"], p["combine_z"], p["parts"]) == (COMBINE_SLICE32, 1, 28, 4, 61), p
    assert p["ws_need"] == 61 * 28 * 130 * 4 and p["part_ml_off"] == 61 * 28 * 128, p
    assert plan(shim, {**dec, "ws_bytes": need - 1})["status"] == E_WORKSPACE
    assert plan(shim, {**dec, "q_pos0": -1})["status"] == E_INVALID            # no visible key
    p = plan(shim, dec, attn_decode=0)
    assert (p["kernel"], p["hd"], p["nq"], p["pre"], p["grid_x"], p["grid_y"], p["block_x"]) == (1, 128, 2, 1, 61, 4, 256), p


def test_cfg2_encoder_launch(shim):
    """the encoder's one-video launch at cfg2 as VitRange passes it: 64 frames of 22 x 42 = 924 patches, 16 heads of 72,
    head-major q / k / v behind the QKV GEMM, O rows of the hidden size. 924 rows = 15 key tiles: 4 + ((15 - 4) & 3) = 7 behind the
    four-tile loop, the last tile holds 28 rows = one 32-key block"""
    frames, per, heads = 64, 924, 16
    N = frames * per
    q = query(head_dim=72, q_len=N, kv_len=N, hq=heads, hkv=heads, ldq=72, ldk=72, ldv=72, ldo=heads * 72, head_stride=N * 72,
              has_cu=1, nseg=frames, max_seqlen=per, uniform_seqlen=per, q_prescaled=1)
    p = plan(shim, q)
    assert (p["status"], p["kernel"], p["vit_pipe"], p["vit_r"], p["vit_nlb"], p["vit_end"]) == (OK, 8, 1, 7, 1, 71), p
    assert (p["nqb"], p["grid_x"], p["grid_y"], p["grid_z"], p["block_x"]) == (8, 8 * 8, heads // 8, frames, 256), p
    assert (p["xcd_order"], p["uniform_len"], p["head_stride"], p["early_prefetch"]) == (1, per, N * 72, 0), p
    assert plan(shim, q, attn_vit_len=0)["vit_end"] == 0 and plan(shim, q, attn_vit_early=1)["early_prefetch"] == 1
    tok = {**q, "ldq": 3 * heads * 72, "ldk": 3 * heads * 72, "ldv": 3 * heads * 72, "head_stride": 0}      # gemm_headmajor = 0
    p = plan(shim, tok)
    assert (p["kernel"], p["vit_end"], p["head_stride"]) == (3, 71, 72), p
    # a hint that does not describe the launch is dropped; heads that are no multiple of 8 walk the plain grid
    assert plan(shim, {**q, "uniform_seqlen": per + 1})["uniform_len"] == 0
    p = plan(shim, {**tok, "hq": 12, "hkv": 12, "ldo": 12 * 72})
    assert (p["xcd_order"], p["grid_x"], p["grid_y"], p["grid_z"]) == (0, 8, 12, frames), p
    assert plan(shim, {**q, "nseg": 65536, "q_len": 65536 * per, "kv_len": 65536 * per})["status"] == E_INVALID


def test_rows_step(shim):
    """the multi-row step at Qwen2-7B's heads: grid, partials and combine; and the statuses no GPU cell exercises"""
    q = cells.query(dict(kind="rows", rows=4, hq=28, hkv=4, prefix_len=1024, nsplit=32))
    p = plan(shim, q, rows=True)
    assert (p["status"], p["kernel"], p["gsz"], p["ntile"], p["kend"], p["rows_slot"]) == (OK, 0, 7, 2, 1024, 0), p
    assert (p["grid_x"], p["grid_y"], p["grid_z"], p["block_x"]) == (32 * 2 + 4, 4, 1, 256), p
    assert (p["combine"], p["combine_x"], p["combine_y"], p["combine_z"], p["parts"]) == (COMBINE_SLICE32, 1, 4 * 28, 4, 33), p
    assert p["ws_need"] == 33 * 4 * 28 * 130 * 4 and p["part_ml_off"] == 33 * 4 * 28 * 128, p
    assert plan(shim, q, rows=True, attn_combine32=0)["combine"] == COMBINE_HEAD
    # no query head: the combine has no (row, head) slot -- COGS_E_INVALID, behind the decode-rows checks (an empty buffer is
    # large enough; a head dim the kernel does not have comes first)
    assert plan(shim, {**q, "hq": 0, "ws_bytes": 0}, rows=True)["status"] == E_INVALID
    assert plan(shim, {**q, "hq": 0, "ws_bytes": 0, "head_dim": 72}, rows=True)["status"] == E_UNSUPPORTED
    assert plan(shim, {**q, "hq": 0, "has_ws": 0}, rows=True)["status"] == E_WORKSPACE
    assert plan(shim, {**q, "prefix_len": 0}, rows=True)["status"] == E_INVALID


def test_split_rule(shim):
    """at least 32 splits while a split keeps 64 keys, 256 keys per split beyond that, at most 128 (rows: 127, their tails are
    one more partial)"""
    t = _tuning(shim, {})
    want = {1: 1, 100: 2, 2048: 32, 15360: 60, 15395: 61, 40000: 128}
    assert {c: shim.attn_nsplit(c, t) for c in want} == want
    assert {c: shim.attn_rows_nsplit(c, t) for c in want} == {**want, 40000: 127}
    t = _tuning(shim, {"llm_split_keys": 128})
    assert [shim.attn_nsplit(c, t) for c in want] == [1, 1, 16, 120, 121, 128]
    assert [shim.attn_rows_nsplit(c, t) for c in want] == [1, 1, 16, 120, 121, 127]
    # monotonic in the context: the workspace is sized with the largest
    t = _tuning(shim, {})
    ns = [shim.attn_nsplit(c, t) for c in range(1, 40001, 7)]
    assert ns == sorted(ns)
    assert shim.attn_split_ws_bytes(3, 5, 7, 128) == 3 * 5 * 7 * 130 * 4


def test_plan_header_is_host_only():
    text = open(os.path.join(CSRC, "attn_plan.h")).read()
    assert "hip" not in "".join(l for l in text.splitlines() if l.lstrip().startswith("#include")).lower()


def test_retired_attention_switches_are_unknown_names():
    """attn_prefill_deep and attn_prio selected forms of the prompt kernel that no longer exist: the switch table answers them
    like any other unknown name"""
    from cogstream_amd import _lib as L
    for name in ("attn_prefill_deep", "attn_prio"):
        assert name not in L.debug_list()
        assert L.lib.cogs_debug_set(name.encode(), 1) == L.E_INVALID, name
