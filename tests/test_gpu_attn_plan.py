"""The built library still routes every cell of tests/golden/attn_plan.json as the commit that recorded it did: the sweep of
tests/attn_plan_cells.py is replayed on the recorder's own buffers (one builder: tools/record_attn_plan.py imports the same)
and the returned status and the `attn_last_kernel` / `attn_vit_last_end` reports are compared per call."""
import contextlib
import json
import os

import pytest

import attn_plan_cells as cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_library_routes_every_recorded_cell_as_recorded():
    import torch
    from cogstream_amd import _lib as L

    with open(os.path.join(ROOT, "tests", "golden", "attn_plan.json")) as f:
        doc = json.load(f)
    assert doc["cells"] == cells.cells() and doc["switches"] == cells.SWITCHED
    records = iter(doc["records"])
    dev = torch.device("cuda")
    for ci, cell in enumerate(doc["cells"]):
        b = cells.Buffers(cell, dev)
        for si, sw in enumerate(doc["switches"]):
            rci, rsi, status, kernel, vit_end = next(records)
            assert (rci, rsi) == (ci, si)
            with contextlib.ExitStack() as stack:
                for k, v in sw.items():
                    stack.enter_context(L.debug_switch(k, v))
                st, ran, end = b.call()
            what = (cell, sw)
            assert st == status, what
            if st == L.OK and not b.rows_kind:
                assert ran == kernel, what
                if kernel in (3, 8):
                    assert end == vit_end, what
        assert b.guards_intact(), cell
    assert next(records, None) is None
