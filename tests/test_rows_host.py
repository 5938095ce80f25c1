"""Host side of generate(num_return_sequences=N), without a GPU: argument rules, padding, the draw bookkeeping of both
samplers, the torch.multinomial equivalence the host-sampler mode rests on, and the ABI of the new entry points."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_num_return_sequences_argument_rules():
    from cogstream_amd.llm import MAX_RETURN_SEQUENCES, Qwen2Engine, check_num_return_sequences
    assert MAX_RETURN_SEQUENCES == 16
    assert check_num_return_sequences(1, False) == 1 and check_num_return_sequences(16, True) == 16
    with pytest.raises(ValueError, match="Greedy methods without beam search"):
        check_num_return_sequences(2, False)
    for n in (0, 17, -3):
        with pytest.raises(ValueError, match="between 1 and 16"):
            check_num_return_sequences(n, True)
    # generate() applies them before it touches the engine or the embeddings
    with pytest.raises(ValueError, match="Greedy methods"):
        Qwen2Engine.generate(None, None, max_new_tokens=4, num_return_sequences=3)
    with pytest.raises(ValueError, match="between 1 and 16"):
        Qwen2Engine.generate(None, None, max_new_tokens=4, do_sample=True, num_return_sequences=17)


def test_ragged_rows_are_cut_and_padded():
    from cogstream_amd.llm import pad_rows, truncate_at_eos
    rows = truncate_at_eos([[5, 6, 9, 7, 9], [9, 1], [1, 2, 3, 4, 5]], [9, 11])
    assert rows == [[5, 6, 9], [9], [1, 2, 3, 4, 5]]
    assert truncate_at_eos([[1, 2]], []) == [[1, 2]]
    out = pad_rows(rows, 77)
    assert out.dtype == torch.int64 and out.tolist() == [[5, 6, 9, 77, 77], [9, 77, 77, 77, 77], [1, 2, 3, 4, 5]]
    assert pad_rows([[], []], 3).shape == (2, 0)


def test_philox_offsets():
    from cogstream_amd.llm import philox_offset
    assert [philox_offset(s, 1, 0) for s in range(5)] == [0, 1, 2, 3, 4]          # N = 1: the offsets of the single-row loop
    seen = [philox_offset(s, 5, r) for s in range(4) for r in range(5)]
    assert seen == list(range(20))                                                # N rows: no offset twice, none skipped


def test_host_draw_block_shape_and_order():
    from cogstream_amd.llm import host_draw_block
    g = torch.Generator().manual_seed(3)
    blk = host_draw_block(g, 4, 50)
    assert blk.shape == (4, 50) and blk.dtype == torch.float32 and bool((blk > 0).all())
    # row-major: the block is the next 200 draws of the generator, in order
    flat = torch.empty(200).exponential_(1, generator=torch.Generator().manual_seed(3))
    assert torch.equal(blk.reshape(-1), flat)


def test_multinomial_rows_consume_one_row_major_exponential_block():
    """what sampler="host" rests on: torch.multinomial(probs[N, V], 1) on the CPU generator equals argmax(probs / q) with q
    ONE [N, V] Exponential(1) block, and leaves the generator where that block leaves it"""
    from cogstream_amd.llm import host_draw_block
    N, V = 5, 301
    probs = torch.softmax(torch.randn(N, V, generator=torch.Generator().manual_seed(1)) * 2, -1)
    for seed in (0, 1, 2):
        g1, g2 = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        want = torch.multinomial(probs, 1, generator=g1).view(-1)
        q = host_draw_block(g2, N, V)
        assert torch.equal((probs / q).argmax(-1), want)
        assert torch.equal(g1.get_state(), g2.get_state())


_CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float}


def _header_fields(hdr: str, name: str):
    """[(field, ctypes type)] of `typedef struct { ... } name;` as written in the header (pointers -> c_void_p)"""
    body = re.search(r"typedef struct \{((?:[^{}]|\{[^{}]*\})*?)\}\s*" + name + r"\s*;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(?:const\s+)?(\w+)\s*(.*)$", decl, re.S)
        base = m.group(1)
        for item in (x.strip() for x in m.group(2).split(",")):
            if item.startswith("*"):
                out.append((item.lstrip("* "), C.c_void_p))
            else:
                out.append((item, _CTYPE[base]))
    return out


def test_new_abi_resolves_against_the_header():
    from cogstream_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cogs.h")).read()
    for sym in ("cogs_gemm_rows", "cogs_attention_rows", "cogs_llm_decode_rows", "cogs_llm_decode_rows_workspace_bytes"):
        assert re.search(r"\b" + sym + r"\s*\(", hdr), sym
        assert hasattr(L.lib, sym) and sym in L.SIGNATURES
    for cname, cls in (("cogs_kv_rows", L.KVRows), ("cogs_attn_rows_desc", L.AttnRowsDesc), ("cogs_kv", L.KV)):
        assert _header_fields(hdr, cname) == [(n, t) for n, t in cls._fields_], cname
    names = [n for n, _ in L.KVRows._fields_]
    assert names == ["k", "v", "max_len", "prefix_len", "tail_k", "tail_v", "tail_max", "tail_len"]
    # argument lists as declared: (stream, desc*, q_scale, q_cols) and (h, stream, embeds, R, kv*, logits, ws, ws_bytes)
    assert L.SIGNATURES["cogs_gemm_rows"][1][2:] == [C.c_float, C.c_int]
    assert L.SIGNATURES["cogs_llm_decode_rows"][1][3:5] == [C.c_int, C.POINTER(L.KVRows)]
    assert " 0.4 " in L.lib.cogs_version().decode()        # the revision string stays
    # refused before any device work: no descriptor, no handle
    assert L.lib.cogs_gemm_rows(None, None, 0.0, 0) == L.E_INVALID
    assert L.lib.cogs_attention_rows(None, None) == L.E_INVALID
    assert L.lib.cogs_llm_decode_rows(None, None, None, 1, None, None, None, 0) == L.E_INVALID
