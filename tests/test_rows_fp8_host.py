"""Host side of the e4m3 multi-row decode step, on the built library without a device: the switch and the reporter of
csrc/debug.h and the ABI of cogs_gemm_rows_fp8."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_switch_and_reporter_are_listed():
    from cogstream_amd import _lib as L
    listing = L.debug_list()
    assert re.search(r"^llm_rows_fp8 = [01]: ", listing, re.M)
    assert re.search(r"^llm_last_rows_fp8 \(read only\): ", listing, re.M)


def test_reporter_is_read_only_and_starts_at_zero():
    from cogstream_amd import _lib as L
    import torch
    before = L.debug_get("llm_last_rows_fp8")
    if not torch.cuda.is_available():                      # with a device, GPU tests of the same process may have run a step
        assert before == 0
    assert before in (0, 1)
    assert L.lib.cogs_debug_set(b"llm_last_rows_fp8", 1) == L.E_INVALID
    assert L.lib.cogs_debug_set(b"llm_last_rows_fp8", 0) == L.E_INVALID
    assert L.debug_get("llm_last_rows_fp8") == before


def test_switch_round_trips_and_rejects_other_values():
    from cogstream_amd import _lib as L
    shipped = L.debug_get("llm_rows_fp8")
    assert shipped in (0, 1)
    try:
        for v in (1, 0, 1):
            L.debug_set("llm_rows_fp8", v)
            assert L.debug_get("llm_rows_fp8") == v
        assert L.lib.cogs_debug_set(b"llm_rows_fp8", 2) == L.E_INVALID and L.lib.cogs_debug_set(b"llm_rows_fp8", -1) == L.E_INVALID
        assert L.debug_get("llm_rows_fp8") == 1             # a refused value changes nothing
        with L.debug_switch("llm_rows_fp8", 0):
            assert L.debug_get("llm_rows_fp8") == 0
        assert L.debug_get("llm_rows_fp8") == 1
    finally:
        L.debug_set("llm_rows_fp8", shipped)


def test_gemm_rows_fp8_is_exported_with_the_bound_signature():
    from cogstream_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cogs.h")).read()
    m = re.search(r"cogs_status\s+cogs_gemm_rows_fp8\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/cogs.h does not declare cogs_gemm_rows_fp8"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["cogs_stream stream", "const cogs_gemm_desc* d", "const float* scale", "float q_scale", "int q_cols"]
    assert hasattr(L.lib, "cogs_gemm_rows_fp8")
    res, argtypes = L.SIGNATURES["cogs_gemm_rows_fp8"]
    assert res is C.c_int and argtypes == [C.c_void_p, C.POINTER(L.GemmDesc), C.c_void_p, C.c_float, C.c_int]
    assert L.lib.cogs_gemm_rows_fp8.argtypes == argtypes
    # the bf16 entry point keeps its signature
    assert L.SIGNATURES["cogs_gemm_rows"][1] == [C.c_void_p, C.POINTER(L.GemmDesc), C.c_float, C.c_int]
    # refused before any device work: no descriptor; a descriptor without operands; no scale
    assert L.lib.cogs_gemm_rows_fp8(None, None, None, 0.0, 0) == L.E_INVALID
    d = L.GemmDesc()
    assert L.lib.cogs_gemm_rows_fp8(None, C.byref(d), None, 0.0, 0) == L.E_INVALID


def test_revision_string_stays():
    from cogstream_amd import _lib as L
    assert " 0.4 " in L.lib.cogs_version().decode()
