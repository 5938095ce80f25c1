#!/usr/bin/env python3
"""Record which attention kernel every cell of a fixed descriptor sweep gets: the fixture behind tests/test_attn_plan.py and
tests/test_gpu_attn_plan.py.

    timeout -k 10 600 python tools/record_attn_plan.py --out tests/golden/attn_plan.json --commit <hash of the commit that ran>

The cells are those of tests/attn_plan_cells.py (one place: the tests import the same builder). Every cell is one
cogs_attention / cogs_attention_rows on zero-filled guarded buffers of the cell's size, under the shipped switches and with
each plan switch flipped alone; its record is the returned status and, when the call was accepted, the `attn_last_kernel` /
`attn_vit_last_end` reports behind it (cogs_attention_rows writes neither: its records carry the status alone). Only the
switch table and the two entry points are used, so the same script runs on any commit that has them. One process; it stops
at the first HIP error (the synchronise behind every call raises) and has no time limit of its own: start it under `timeout`.
`--dump DIR` also writes the sha256 of every accepted call's whole O buffer (for comparing two builds of the library)."""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import attn_plan_cells as cells_mod  # noqa: E402


def sweep(dump=None):
    """[cell index, switch index, status, attn_last_kernel, attn_vit_last_end] per call, in the order they run"""
    import contextlib

    import torch
    from cogstream_amd import _lib as L

    dev = torch.device("cuda")
    records, blobs = [], []
    for ci, cell in enumerate(cells_mod.cells()):
        b = cells_mod.Buffers(cell, dev)
        for si, sw in enumerate(cells_mod.SWITCHED):
            with contextlib.ExitStack() as stack:
                for k, v in sw.items():
                    stack.enter_context(L.debug_switch(k, v))
                st, kernel, end = b.call()
            ok = st == L.OK and not b.rows_kind
            records.append([ci, si, st, kernel if ok else 0, end if ok and kernel in (3, 8) else 0])
            if dump is not None and st == L.OK:
                blobs.append(f"{ci} {si} {hashlib.sha256(b.obuf.cpu().numpy().tobytes()).hexdigest()}\n")
        if not b.guards_intact():
            raise SystemExit(f"cell {ci} {cell}: bits outside O changed")
        del b
    if dump is not None:
        Path(dump).mkdir(parents=True, exist_ok=True)
        (Path(dump) / "outputs.sha256").write_text("".join(blobs))
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="attn_plan.json")
    ap.add_argument("--commit", default="unknown", help="hash of the commit whose library ran")
    ap.add_argument("--dump", default=None, help="directory for the sha256 of every accepted call's O buffer")
    args = ap.parse_args()
    records = sweep(args.dump)
    note = ("tools/record_attn_plan.py on an MI355X: per call [cell, switches, status, attn_last_kernel, attn_vit_last_end] "
            "(indices into `cells` and `switches`; the reports are 0 where the call was rejected or writes none)")
    with open(args.out, "w") as f:
        f.write(f'{{\n "recorded_at_commit": {json.dumps(args.commit)},\n "note": {json.dumps(note)},\n')
        f.write(f' "switches": {json.dumps(cells_mod.SWITCHED)},\n "cells": [\n')
        f.write(",\n".join("  " + json.dumps(c) for c in cells_mod.cells()))
        f.write("\n ],\n \"records\": [\n")
        f.write(",\n".join("  " + json.dumps(r) for r in records))
        f.write("\n ]\n}\n")
    print(f"{len(records)} records -> {args.out}")


if __name__ == "__main__":
    main()
