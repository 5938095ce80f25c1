"""The GEMM launch plan (csrc/gemm_plan.h, cogs_plan_gemm) pinned on the CPU.

tests/golden/gemm_plan.json was recorded on an MI355X by tools/record_gemm_plan.py at the commit it names, BEFORE the
plan became a function of its own: per cell of the sweep the body `gemm_last_body` reported and the `[gemm choice]` line
(ping-pong tiles, rounds, remainder, mb_main; shapes that are not ping-pong-eligible printed none). The plan must give
the same for every record. The fields no record carries (tall tiles, group size, tiles of a full group, grid) are
asserted for the cfg2 production shapes from the constants written in the code at that commit."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cogstream_amd", "csrc")
EPI = {"none": 0, "bias": 1, "res": 2, "bias_res": 1 | 2, "bias_gelu": 1 | 8, "swiglu": 32}     # csrc/gemm_epi_mask.h
LAUNCH = ("body", "rows", "nbm", "nbn", "ntiles", "group_m", "cf", "tall", "grid", "rope_lut")
VIT = {"patch_embed": (1152, 640), "qkv": (3456, 1152), "out_proj": (1152, 1152), "fc1": (4352, 1152), "fc2": (1152, 4352)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_shim.so"
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "gemm_plan_shim.cpp"),
                        "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    lib.plan_tuning_names.restype = C.c_char_p
    return lib


def tuning_defaults(shim):
    names = shim.plan_tuning_names().decode().split()
    vals = (C.c_longlong * len(names))()
    shim.plan_tuning_defaults(vals)
    return dict(zip(names, vals))


def plan(shim, M, N, K, *, dtype="bf16", epi="bias", force_small=False, rope_lut=False, rope_lut_bytes=0, co_streams=1, **switches):
    t = tuning_defaults(shim)
    assert set(switches) <= set(t), switches
    t.update(switches)
    vals = (C.c_longlong * len(t))(*t.values())
    out = (C.c_int * 27)()
    shim.plan_gemm(int(dtype == "bf16"), M, N, K, EPI[epi] if isinstance(epi, str) else epi, int(force_small), int(rope_lut),
                   rope_lut_bytes, co_streams, vals, out)
    p = dict(zip(("body", "rows_main", "pp_eligible", "tiles", "rounds", "rem", "mb_main"), out[:7]))
    p["main"] = dict(zip(LAUNCH, out[7:17]))
    p["rest"] = dict(zip(LAUNCH, out[17:27]))
    return p


def fixture_records():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plan.json")) as f:
        doc = json.load(f)
    assert len(doc["recorded_at_commit"]) == 40
    return doc["records"]


def test_tuning_defaults_are_the_shipped_switch_defaults(shim):
    """GemmTuning{} = the defaults of the same switches in csrc/debug.h"""
    import re
    text = open(os.path.join(CSRC, "debug.h")).read()
    shipped = {m.group(1): int(m.group(2)) for m in re.finditer(r"X\((\w+), (-?\d+)(?:LL)?,", text)}
    t = tuning_defaults(shim)
    assert len(t) == 13
    for name, value in t.items():
        assert shipped[name] == value, name


def test_plan_reproduces_every_recorded_choice(shim):
    recs = fixture_records()
    assert len(recs) >= 200
    for r in recs:
        p = plan(shim, r["M"], r["N"], r["K"], dtype=r["dtype"], epi=r["epi"], **r["switches"])
        what = (r["name"], r["M"], r["switches"])
        assert p["body"] == r["body"], (what, p)
        if "tiles" in r:
            assert p["pp_eligible"] == 1, what
            assert (p["tiles"], p["rounds"], p["rem"], p["mb_main"]) == (r["tiles"], r["rounds"], r["rem"], r["mb_main"]), (what, p)
        else:
            assert p["pp_eligible"] == 0, (what, p)
        # the stream count as a field of the query is the switch's value by another way
        s = r["switches"]["gemm_co_streams"]
        sw = {k: v for k, v in r["switches"].items() if k != "gemm_co_streams"}
        assert plan(shim, r["M"], r["N"], r["K"], dtype=r["dtype"], epi=r["epi"], co_streams=s, **sw) == p, what
        # launches are consistent with the report
        assert p["main"]["rows"] == p["rows_main"] and p["rows_main"] + p["rest"]["rows"] == r["M"], (what, p)
        assert (p["rest"]["body"] != 0) == (p["body"] == 5), (what, p)
        if p["body"] == 5:
            assert p["main"]["body"] in (3, 4) and p["rest"]["body"] == 2 and p["rest"]["rows"] >= 512, (what, p)
            assert p["rows_main"] == 256 * r["mb_main"], (what, p)
        # the persistent grid: 256 workgroups whenever there are more tiles, else one per tile
        for l in (p["main"], p["rest"]):
            if l["body"] in (2, 3, 4) and not (l["body"] == 4 and r["switches"].get("gemm_even_grid")) and r["switches"].get("gemm_wgs", 256) == 256:
                assert l["grid"] == min(l["ntiles"], 256), (what, l)
            if l["body"] == 1 or (l["body"] == 2 and r["switches"].get("gemm_wgs") == 0):
                assert l["grid"] == l["ntiles"], (what, l)
            if l["body"] == 4 and r["switches"].get("gemm_even_grid") and l["ntiles"] > 256:
                rounds = (l["ntiles"] + 255) // 256
                assert l["grid"] == min(256, ((l["ntiles"] + rounds - 1) // rounds + 7) // 8 * 8), (what, l)


def test_cfg2_production_shapes(shim):
    """M = 59 136 (the whole clip on one stream), default switches: tall tiles for the ragged N = 1152 / 3456 and not for
    4352; groups of 6 row blocks (tall), 3 (tall, <= 6 column blocks and K >= 2048: fc2), 8 (fc1); tiles of a full group;
    256 persistent workgroups"""
    want = {"out_proj": (1, 6, 28, 1078, 4), "qkv": (1, 6, 82, 3157, 4), "fc1": (0, 8, 136, 3927, 4), "fc2": (1, 3, 14, 1078, 5)}
    for name, (tall, group_m, cf, tiles, body) in want.items():
        n, k = VIT[name]
        p = plan(shim, 59136, n, k)
        m = p["main"]
        assert (m["tall"], m["group_m"], m["cf"], p["tiles"], p["body"], m["grid"]) == (tall, group_m, cf, tiles, body, 256), (name, p)
        assert m["body"] == 4 and m["nbn"] == n // 256
    p = plan(shim, 59136, *VIT["fc2"])
    assert p["mb_main"] == 219 and p["rest"]["rows"] == 3072 and p["rest"]["body"] == 2 and p["rest"]["grid"] == 12 * 9, p
    assert p["main"]["ntiles"] == 219 // 3 * 14 and p["main"]["nbm"] == 219, p


def test_rank_share_and_two_stream_choices(shim):
    """one rank's share (M = 6 400, one stream) and the two-stream halves of small clips"""
    got = {name: plan(shim, 6400, *VIT[name]) for name in ("out_proj", "qkv", "fc1", "fc2")}
    assert [got[n]["body"] for n in ("out_proj", "qkv", "fc1", "fc2")] == [2, 5, 4, 2]
    q = got["qkv"]
    assert q["mb_main"] == 18 and q["main"]["grid"] == 246 and q["main"]["ntiles"] == 246 and q["rest"]["rows"] == 1792, q
    assert got["fc1"]["main"]["grid"] == 256 and got["fc1"]["tiles"] == 425
    assert got["out_proj"]["main"]["grid"] == 25 * 9            # ring kernel: 225 tiles, one per workgroup
    for m, bodies in ((3696, [2, 4, 4, 2]), (29568, [4, 4, 4, 4])):
        ps = [plan(shim, m, *VIT[name], co_streams=2) for name in ("out_proj", "qkv", "fc1", "fc2")]
        assert [p["body"] for p in ps] == bodies, (m, ps)
        assert all(p["rest"]["body"] == 0 for p in ps)
    # the switch overrides the caller's count
    assert plan(shim, 3696, *VIT["out_proj"], co_streams=2, gemm_co_streams=1) == plan(shim, 3696, *VIT["out_proj"])


def test_rotary_lut_only_on_the_k_tile_body(shim):
    rope = 1 | 4                                   # EPI_BIAS | EPI_ROPE
    kw = dict(epi=rope, rope_lut=True, rope_lut_bytes=64 * 18 * 8)
    p = plan(shim, 14784, 3456, 1152, **kw)
    assert p["main"]["body"] == 4 and p["main"]["rope_lut"] == 0
    p = plan(shim, 14784, 3456, 1152, gemm_pp64=0, **kw)
    assert p["main"]["body"] == 3 and p["main"]["rope_lut"] == 1 and p["main"]["tall"] == 0
    assert plan(shim, 14784, 3456, 1152, gemm_pp64=0, gemm_rope_lut=0, **kw)["main"]["rope_lut"] == 0
    assert plan(shim, 14784, 3456, 1152, gemm_pp64=0, epi=rope, rope_lut=True, rope_lut_bytes=29 * 1024)["main"]["rope_lut"] == 0
    assert plan(shim, 14784, 3456, 1152, gemm_pp64=0, epi=rope | 2048, rope_lut=True, rope_lut_bytes=4096)["main"]["rope_lut"] == 1
    assert plan(shim, 14784, 3456, 1152, gemm_pp64=0, epi=rope | 4096, rope_lut=True, rope_lut_bytes=4096)["main"]["rope_lut"] == 0


def test_plan_header_is_host_only():
    for name in ("gemm_plan.h", "gemm_epi_mask.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "hip" not in "".join(l for l in text.splitlines() if l.lstrip().startswith("#include")).lower(), name
