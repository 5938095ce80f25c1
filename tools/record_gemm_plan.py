#!/usr/bin/env python3
"""Record which GEMM body (and which ping-pong split) every cell of a fixed shape sweep gets: the fixture behind
tests/test_gemm_plan.py.

    python tools/record_gemm_plan.py --out tests/golden/gemm_plan.json --commit <hash of the commit that ran>

Every cell is one ops.gemm with a cheap epilogue. The sweep runs in a child process with the `gemm_choice` switch on and
its stderr in a file; the record of a cell is the `[gemm choice]` line the library printed for it (shapes that are not
ping-pong-eligible print none) plus `gemm_last_body` after the call. Only the switch table and ops.gemm are used, so the
same script runs on any commit that has them. `--child` runs the sweep alone (for a kernel trace of the same launches).
The sweep has no per-cell time limit (the child is bounded as a whole): start it under `timeout -k 10 <seconds>`.
"""
from __future__ import annotations

import argparse
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

VIT = [("patch_embed", 1152, 640, "bias"), ("qkv", 3456, 1152, "bias"), ("out_proj", 1152, 1152, "bias_res"),
       ("fc1", 4352, 1152, "bias_gelu"), ("fc2", 1152, 4352, "bias_res")]
VIT_M = [59136, 29568, 14784, 7392, 6400, 3696, 3200, 1024, 1023, 600, 511, 100]
QWEN = [("llm_qkv", 4608, 3584, "bias"), ("llm_gate_up", 37888, 3584, "swiglu"), ("llm_down", 3584, 18944, "res")]
SWITCHED = [("gemm_tall", 0), ("gemm_split", 0), ("gemm_pp64", 0), ("gemm_pingpong", 0), ("gemm_small", 1),
            ("gemm_even_grid", 1), ("gemm_pad_pct", 100), ("gemm_group_m", 3), ("gemm_wgs", 0)]


def cells():
    """(name, dtype, M, N, K, epilogue, {switch: value}) in the order they run"""
    out = []
    for streams in (1, 2):
        for m in VIT_M:
            for name, n, k, epi in VIT:
                out.append((name, "bf16", m, n, k, epi, {"gemm_co_streams": streams}))
    for m in (2048, 2100):
        for name, n, k, epi in QWEN:
            out.append((name, "bf16", m, n, k, epi, {"gemm_co_streams": 1}))
    out.append(("fp32_small", "fp32", 600, 1152, 1152, "bias", {"gemm_co_streams": 1}))
    out.append(("fp32_large", "fp32", 3696, 3456, 1152, "bias", {"gemm_co_streams": 1}))
    out.append(("gemv", "bf16", 1, 3584, 3584, "none", {"gemm_co_streams": 1}))
    for sw, val in SWITCHED:
        for m in (14784, 6400):
            for name, n, k, epi in VIT:
                out.append((name, "bf16", m, n, k, epi, {"gemm_co_streams": 1, sw: val}))
    return out


def child():
    import torch
    from cogstream_amd import _lib as L
    from cogstream_amd import ops

    dev = torch.device("cuda")
    L.debug_set("gemm_choice", 1)
    for i, (name, dtype, m, n, k, epi, switches) in enumerate(cells()):
        dt = torch.bfloat16 if dtype == "bf16" else torch.float32
        a = torch.zeros(m, k, device=dev, dtype=dt)
        w = torch.zeros(n, k, device=dev, dtype=dt)
        kw = {}
        if "bias" in epi:
            kw["bias"] = torch.zeros(n, device=dev, dtype=dt)
        if "res" in epi:
            kw["residual"] = torch.zeros(m, n, device=dev, dtype=dt)
        if "gelu" in epi:
            kw["act"] = L.ACT_GELU_TANH
        if epi == "swiglu":
            kw["act"] = L.ACT_SWIGLU
        old = {s: L.debug_get(s) for s in switches}
        for s, v in switches.items():
            L.debug_set(s, v)
        torch.cuda.synchronize()
        sys.stderr.write(f"[cell] {i}\n")
        sys.stderr.flush()
        try:
            ops.gemm(a, w, **kw)
            torch.cuda.synchronize()
            body = L.debug_get("gemm_last_body")
        finally:
            for s, v in old.items():
                L.debug_set(s, v)
        sys.stderr.write(f"[body] {body}\n")
        sys.stderr.flush()
        del a, w, kw


CHOICE = re.compile(r"\[gemm choice\] M=(\d+) N=(\d+) K=(\d+): (\d+) ping-pong tiles \((\d+) rounds \+ (\d+)\), mb_main (-?\d+)")


def parse(text: str):
    got, cur = {}, None
    for line in text.splitlines():
        if line.startswith("[cell] "):
            cur = int(line.split()[1])
            got[cur] = {"choice": []}
        elif cur is not None and line.startswith("[body] "):
            got[cur]["body"] = int(line.split()[1])
            cur = None
        elif cur is not None:
            m = CHOICE.search(line)
            if m:
                got[cur]["choice"].append([int(x) for x in m.groups()])
    records = []
    for i, (name, dtype, m, n, k, epi, switches) in enumerate(cells()):
        g = got.get(i)
        if g is None or "body" not in g:
            raise SystemExit(f"cell {i} ({name} M={m}) left no record")
        if len(g["choice"]) > 1:
            raise SystemExit(f"cell {i} ({name} M={m}) printed {len(g['choice'])} choice lines")
        rec = {"name": name, "dtype": dtype, "M": m, "N": n, "K": k, "epi": epi, "switches": switches, "body": g["body"]}
        if g["choice"]:
            cm, cn, ck, tiles, rounds, rem, mb_main = g["choice"][0]
            assert (cm, cn, ck) == (m, n, k), (i, g["choice"])
            rec.update(tiles=tiles, rounds=rounds, rem=rem, mb_main=mb_main)
        records.append(rec)
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="run the sweep only (records go to stderr)")
    ap.add_argument("--out", default="gemm_plan.json")
    ap.add_argument("--commit", default="unknown", help="hash of the commit whose library ran")
    args = ap.parse_args()
    if args.child:
        child()
        return
    with tempfile.TemporaryDirectory() as tmp:
        log = Path(tmp) / "stderr.txt"
        with open(log, "w") as f:
            subprocess.run([sys.executable, __file__, "--child"], stderr=f, check=True, timeout=900)
        records = parse(log.read_text())
    note = "tools/record_gemm_plan.py on an MI355X: gemm_last_body and the [gemm choice] line of every cell"
    with open(args.out, "w") as f:
        f.write(f'{{\n "recorded_at_commit": {json.dumps(args.commit)},\n "note": {json.dumps(note)},\n "records": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in records))
        f.write("\n ]\n}\n")
    print(f"{len(records)} records -> {args.out}")


if __name__ == "__main__":
    main()
