"""generate(num_beams=B) on the GPU, layer by layer: the tail indirection of cogs_attention_rows against the fp64 reference of
tests/attn_reference.py and, exactly, against the same call on physically gathered tails; cogs_beam_topk against its CPU
definition (ops.beam_topk_cpu), exactly; the lockstep step with a slot table against the step on gathered tails; and the
host loop of Qwen2Engine.beam_search / generate / CogReasoner.generate on the toy model of tests/test_gpu_rows.py."""
from __future__ import annotations

import ctypes as C
import itertools

import pytest
import torch

import attn_reference as AR
import test_gpu_rows as TR

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
HD = 128
BIG = TR.BIG


def _L():
    from cogstream_amd import _lib
    return _lib


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


# ------------------------------------------------------------------------------ 1. cogs_attention_rows with a slot table
_ROWS, _HEADS, _PREFIX, _TAIL = (1, 3, 16), ((7, 1), (28, 4), (2, 2)), (1, 65), (1, 63, 64, 65)
# rows x tail_len in full; heads and prefix_len follow i + j, which pairs every value of one factor with every value of another
SLOT_CASES = [(_ROWS[i], *_HEADS[(i + j) % 3], _PREFIX[(i + j) % 2], _TAIL[j]) for i in range(3) for j in range(4)]


def test_slot_cases_cover_every_pair():
    cols = [[c[0] for c in SLOT_CASES], [(c[1], c[2]) for c in SLOT_CASES], [c[3] for c in SLOT_CASES], [c[4] for c in SLOT_CASES]]
    for a, b in itertools.combinations(range(4), 2):
        assert len(set(zip(cols[a], cols[b]))) == len(set(cols[a])) * len(set(cols[b])), (a, b)


def _slot_operands(dev, rows, hq, hkv, prefix_len, tail_len, tail_max=72):
    g = torch.Generator(device=dev).manual_seed(rows * 1000 + hq * 10 + prefix_len + tail_len)
    kvd = hkv * HD
    qbuf = torch.randn(rows, hq * HD + 2 * kvd, generator=g, device=dev).to(BF16)
    q = qbuf[:, :hq * HD]
    k = torch.full((prefix_len + 5, kvd), BIG, dtype=BF16, device=dev)
    v = torch.full((prefix_len + 5, kvd), BIG, dtype=BF16, device=dev)
    k[:prefix_len] = torch.randn(prefix_len, kvd, generator=g, device=dev).to(BF16)
    v[:prefix_len] = torch.randn(prefix_len, kvd, generator=g, device=dev).to(BF16)
    tk = torch.full((rows, tail_max, kvd), BIG, dtype=BF16, device=dev)          # unused tail positions: the BIG filler
    tv = torch.full((rows, tail_max, kvd), -BIG, dtype=BF16, device=dev)
    tk[:, :tail_len] = torch.randn(rows, tail_len, kvd, generator=g, device=dev).to(BF16)
    tv[:, :tail_len] = torch.randn(rows, tail_len, kvd, generator=g, device=dev).to(BF16) + \
        torch.arange(rows, device=dev).view(rows, 1, 1).to(BF16)
    slot = torch.full((rows, tail_max), 99, dtype=torch.int32, device=dev)       # entries behind tail_len are never read
    slot[:, :tail_len] = torch.randint(0, rows, (rows, tail_len), generator=g, device=dev).to(torch.int32)
    return q, k, v, tk, tv, slot


@pytest.mark.parametrize("rows,hq,hkv,prefix_len,tail_len", SLOT_CASES)
def test_attention_rows_slot_table(dev, rows, hq, hkv, prefix_len, tail_len):
    from cogstream_amd import ops
    q, k, v, tk, tv, slot = _slot_operands(dev, rows, hq, hkv, prefix_len, tail_len)
    nsplit = TR._nsplit(prefix_len)
    kw = dict(prefix_len=prefix_len, tail_len=tail_len, hq=hq, hkv=hkv, nsplit=nsplit)
    out = ops.attention_rows(q, k, v, tk, tv, tail_slot=slot, **kw)
    # the reference gathers per key ...
    pos = torch.arange(tail_len, device=dev)
    gk, gv = tk.clone(), tv.clone()
    for r in range(rows):
        gk[r, :tail_len] = tk[slot[r, :tail_len].long(), pos]
        gv[r, :tail_len] = tv[slot[r, :tail_len].long(), pos]
    what = f"attention_rows + table rows={rows} hq={hq} hkv={hkv} prefix={prefix_len} tail={tail_len}"
    for r in range(rows):
        kk = torch.cat([k[:prefix_len], gk[r, :tail_len]])
        vv = torch.cat([v[:prefix_len], gv[r, :tail_len]])
        ref, tol = AR.reference(q[r:r + 1], kk, vv, hq=hq, hkv=hkv, hd=HD, scale_log2=1.0, nsplit=nsplit + 1)
        AR.assert_within(out[r:r + 1], ref, tol, f"{what} row {r}")
    # ... and the same call on physically gathered tails, without a table, gives the same bits
    plain = ops.attention_rows(q, k, v, gk, gv, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(plain)), what + ": differs from the call on gathered tails"
    if rows > 1 and tail_len > 1:
        moved = ops.attention_rows(q, k, v, tk, tv, **kw)
        assert not torch.equal(_bits(out), _bits(moved)), what + ": the table made no difference"


def test_attention_rows_slot_table_stride_is_checked(dev):
    from cogstream_amd import ops
    L = _L()
    q, k, v, tk, tv, slot = _slot_operands(dev, 3, 7, 1, 65, 63)
    kw = dict(prefix_len=65, tail_len=63, hq=7, hkv=1, nsplit=TR._nsplit(65))
    with pytest.raises(L.CogsError, match=rf"\({L.E_INVALID}\)"):
        ops.attention_rows(q, k, v, tk, tv, tail_slot=slot[:, :62].contiguous(), **kw)
    ops.attention_rows(q, k, v, tk, tv, tail_slot=slot[:, :63].contiguous(), **kw)      # ld == tail_len is enough
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 2. cogs_beam_topk
TOPK_SHAPES = [(rows, n) for rows in (1, 2, 16) for n in (4, 512, 152064)]
TRACE32 = 0x7F7F7F7F


def _topk_inputs(rows, n, variant, pad):
    """fp32 [rows, n + pad] on the CPU (the scores in the first n columns, a value that would win in the padding) and the addends.
    variant 0: scores and addends are multiples of 1/4 (their sums are exact, so equal sums abound, within and across rows),
    with a planted maximum that occurs twice in row 0 and once in the last row. variant 1: continuous values, the last row
    masked to -inf but for 3 entries, and (rows > 1) the addend -1e9 on row 0."""
    g = torch.Generator().manual_seed(rows * 7 + n + 13 * variant)
    buf = torch.full((rows, n + pad), 3.0e38)
    s = buf[:, :n]
    if variant == 0:
        s.copy_((torch.randn(rows, n, generator=g) * 4).round() / 4)
        add = (torch.randn(rows, generator=g) * 4).round() / 4
        s[0, 1] = s[0, n - 1] = 40.0 - add[0]
        s[rows - 1, 2] = 40.0 - add[rows - 1]
    else:
        s.copy_(torch.randn(rows, n, generator=g) * 3 - 5)
        add = torch.randn(rows, generator=g)
        s[rows - 1].fill_(float("-inf"))
        s[rows - 1, [0, n // 2, n - 1]] = torch.tensor([1.0, 50.0, 1.0])
        if rows > 1:
            add[0] = -1.0e9
    return buf, add


@pytest.mark.parametrize("variant", ["ties", "masked row and -1e9"])
@pytest.mark.parametrize("rows,n", TOPK_SHAPES)
def test_beam_topk_matches_the_cpu_definition_exactly(dev, rows, n, variant):
    from cogstream_amd import ops
    L = _L()
    pad = 4
    buf, add = _topk_inputs(rows, n, 0 if variant == "ties" else 1, pad)
    ks = [k for k in (1, 2, 32) if k <= rows * n]
    dbuf, dadd = buf.to(dev), add.to(dev)
    before = _bits(dbuf).clone()
    for cpu_add, row_add in ((add, dadd), (None, None)):
        want_val, want_row, want_tok = ops.beam_topk_cpu(buf[:, :n], cpu_add, max(ks))    # a total order: the best k are its first k
        for k in ks:
            out = torch.full((3, k + 4), TRACE32, dtype=torch.int32, device=dev)
            nbytes = C.c_size_t()
            L.check(L.lib.cogs_beam_topk_workspace_bytes(rows, n, k, C.byref(nbytes)))
            ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
            L.check(L.lib.cogs_beam_topk(L.current_stream(), dbuf.data_ptr(), rows, n, n + pad, L.ptr(row_add), k, out[0].data_ptr(),
                                         out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws.numel()), "cogs_beam_topk")
            got = out.cpu()
            what = f"beam_topk rows={rows} n={n} k={k} {variant} row_add={row_add is not None}"
            assert bool((got[:, k:] == TRACE32).all()), what + ": wrote behind out[k]"
            assert torch.equal(got[0, :k], _bits(want_val[:k])), (what, got[0, :k].view(F32), want_val[:k])
            assert torch.equal(got[1, :k], want_row[:k]) and torch.equal(got[2, :k], want_tok[:k]), (what, got[1:, :k], want_row[:k], want_tok[:k])
        if row_add is not None:      # the wrapper gives the same
            val, row, tok = ops.beam_topk(dbuf[:, :n], dadd, ks[-1])
            assert torch.equal(_bits(val.cpu()), _bits(want_val[:ks[-1]])) and torch.equal(row.cpu(), want_row[:ks[-1]]) and \
                torch.equal(tok.cpu(), want_tok[:ks[-1]])
    assert torch.equal(_bits(dbuf), before)


def test_beam_topk_status_codes(dev):
    from cogstream_amd import ops
    L = _L()
    with pytest.raises(L.CogsError, match=rf"\({L.E_UNSUPPORTED}\)"):
        ops.beam_topk(torch.zeros(17, 8, device=dev), None, 2)
    with pytest.raises(L.CogsError, match=rf"\({L.E_UNSUPPORTED}\)"):
        ops.beam_topk(torch.zeros(2, 64, device=dev), None, 65)
    with pytest.raises(L.CogsError, match=rf"\({L.E_INVALID}\)"):
        ops.beam_topk(torch.zeros(2, 6, device=dev), None, 2)                # n % 4
    with pytest.raises(L.CogsError, match=rf"\({L.E_INVALID}\)"):
        ops.beam_topk(torch.zeros(1, 8, device=dev), None, 9)                # k > rows * n
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 3. the step
def test_decode_rows_with_a_slot_table_equals_the_step_on_gathered_tails(dev):
    """Prompt of 70 tokens, R = 3, five steps; from the second step on every row continues another row (fixed parents). The
    step that reads the tails through the table and the step on tails gathered with index_select (no table) give identical
    logits bits at every step; a run that ignores the parents does not."""
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    cfg = LlmConfig(**TR.STEP_MODELS["4 heads, 2 kv heads"])
    eng = Qwen2Engine(random_llm_state(cfg, seed=7, std=0.05), cfg, dtype=BF16, device=dev)
    torch.manual_seed(12)
    P, Rn, steps = 70, 3, 5
    parents = [None, [0, 0, 1], [2, 0, 0], [1, 1, 2], [0, 2, 1]]
    prompt = (torch.randn(P, cfg.hidden_size) * 0.5).to(BF16)
    toks = torch.randint(0, 480, (Rn, steps))
    emb = eng.embed_tokens(toks.reshape(-1).to(dev)).view(Rn, steps, cfg.hidden_size)
    cache = eng.new_cache(P + steps + 2)
    eng.forward(prompt.to(dev), cache)
    kv_t, tk_t, tv_t, slot = eng.new_rows_kv(cache, Rn, steps, slots=True)
    kv_g, tk_g, tv_g = eng.new_rows_kv(cache, Rn, steps)
    kv_n, tk_n, tv_n = eng.new_rows_kv(cache, Rn, steps)
    assert slot.shape == (Rn, steps) and slot.dtype == torch.int32
    ident = torch.arange(Rn, dtype=torch.int32, device=dev)
    differs = False
    for s in range(steps):
        e = emb[:, s].contiguous()
        if parents[s] is not None:
            par = torch.tensor(parents[s], device=dev)
            slot = slot.index_select(0, par)
            tk_g[:, :, :s] = tk_g.index_select(1, par)[:, :, :s]
            tv_g[:, :, :s] = tv_g.index_select(1, par)[:, :, :s]
        slot[:, s] = ident
        with_table = eng.decode_rows(e, kv_t, slot)
        gathered = eng.decode_rows(e, kv_g)
        ignored = eng.decode_rows(e, kv_n)
        assert torch.equal(_bits(with_table), _bits(gathered)), s
        differs = differs or not torch.equal(_bits(with_table), _bits(ignored))
    assert differs, "the parents made no difference"
    assert kv_t.tail_len == steps and cache.len == P


# ------------------------------------------------------------------------------------------------- 4. generate
NEW = 12


def _cpu_select(scores, row_add, k):
    from cogstream_amd import ops
    return ops.beam_topk_cpu(scores.cpu(), row_add, k)


def _invariants(seqs, scores, n):
    assert len(seqs) == len(scores) == n
    assert all(scores[i] >= scores[i + 1] for i in range(n - 1)), scores
    assert len({tuple(s) for s in seqs}) == n, "hypotheses must be pairwise different"


@pytest.fixture(scope="module")
def beam_run(dev):
    """(engine, prompt embeddings, the B = 4, N = 4 run without an EOS): computed once, shared, not modified"""
    cfg, eng = TR._engine(dev, BF16)
    emb = TR._prompt(dev, BF16)
    seqs, scores = eng.beam_search(emb, num_beams=4, num_return_sequences=4, max_new_tokens=NEW, eos_token_id=[])
    return cfg, eng, emb, seqs, scores


def test_beam_search_is_deterministic_and_ordered(dev, beam_run):
    cfg, eng, emb, seqs, scores = beam_run
    again = eng.beam_search(emb, num_beams=4, num_return_sequences=4, max_new_tokens=NEW, eos_token_id=[])
    assert again == (seqs, scores)                        # identical sequences and score bits (floats compare exactly)
    _invariants(seqs, scores, 4)
    assert all(len(s) == NEW for s in seqs)
    assert eng.generate(emb, num_beams=4, num_return_sequences=4, max_new_tokens=NEW, eos_token_id=[]) == seqs
    best = eng.generate(emb, num_beams=4, max_new_tokens=NEW, eos_token_id=[])
    assert best == seqs[0] and isinstance(best[0], int)


def test_beam_search_table_gather_and_cpu_selection_agree(dev, beam_run):
    L = _L()
    cfg, eng, emb, seqs, scores = beam_run
    kw = dict(num_beams=4, num_return_sequences=4, max_new_tokens=NEW, eos_token_id=[])
    with L.debug_switch("beam_gather_tails", 1):
        assert eng.beam_search(emb, **kw) == (seqs, scores)
    assert eng.beam_search(emb, select_fn=_cpu_select, **kw) == (seqs, scores)


def test_beam_search_eos_closes_hypotheses_early(dev, beam_run):
    from cogstream_amd.chat import CogReasoner
    L = _L()
    cfg, eng, emb, free, _ = beam_run
    eos = free[0][2]                                      # the best hypothesis now ends with its third token
    kw = dict(num_beams=4, num_return_sequences=4, max_new_tokens=NEW, eos_token_id=[eos])
    seqs, scores = eng.beam_search(emb, **kw)
    _invariants(seqs, scores, 4)
    assert len({len(s) for s in seqs}) > 1 and all(eos not in s[:-1] for s in seqs)
    assert any(s[-1] == eos and len(s) < NEW for s in seqs)
    with L.debug_switch("beam_gather_tails", 1):
        assert eng.beam_search(emb, **kw) == (seqs, scores)
    assert eng.beam_search(emb, select_fn=_cpu_select, **kw) == (seqs, scores)
    # the public surface: padded [N, L], arguments through the generation config or as keywords; the prompt is reused
    ids = torch.randint(0, 480, (1, 40), generator=torch.Generator().manual_seed(2))
    probe = eng.generate(eng.embed_tokens(ids.reshape(-1)), num_beams=4, max_new_tokens=16, eos_token_id=[])
    gen = dict(do_sample=False, eos_token_id=[probe[2]], pad_token_id=498, num_beams=4, num_return_sequences=4)
    model = CogReasoner(None, None, eng, cfg, generation_config=gen)
    model.enable_prefix_cache()
    out, _ = model.generate(new_input_ids=ids, max_new_tokens=16)
    want = eng.generate(eng.embed_tokens(ids.reshape(-1)), num_beams=4, num_return_sequences=4, max_new_tokens=16, eos_token_id=[probe[2]])
    assert out.dtype == torch.int64 and out.shape == (4, max(len(s) for s in want))
    for r in range(4):
        assert out[r, :len(want[r])].tolist() == want[r] and bool((out[r, len(want[r]):] == 498).all())
    again, _ = model.generate(new_input_ids=ids, max_new_tokens=16, num_beams=4, num_return_sequences=2, length_penalty=1.0)
    assert again.shape[0] == 2 and again.dtype == torch.int64
    assert model.prefix_cache_stats()["answer"] == (38, 80)        # second call: all rows but the two that are always prefilled


def test_beam_search_fp32_fallback(dev):
    cfg, eng = TR._engine(dev, F32)
    emb = TR._prompt(dev, F32)
    kw = dict(num_beams=4, num_return_sequences=4, max_new_tokens=8, eos_token_id=[])
    seqs, scores = eng.beam_search(emb, **kw)
    _invariants(seqs, scores, 4)
    assert eng.beam_search(emb, **kw) == (seqs, scores)
    assert eng.beam_search(emb, select_fn=_cpu_select, **kw) == (seqs, scores)
    eos = seqs[0][2]
    short, sc = eng.beam_search(emb, **dict(kw, eos_token_id=[eos]))
    _invariants(short, sc, 4)
    assert all(eos not in s[:-1] for s in short) and any(s[-1] == eos and len(s) < 8 for s in short)


@pytest.mark.parametrize("lp", [1.0, 0.6])
def test_beam_scores_are_the_sequences_log_probabilities(dev, lp):
    """For every returned hypothesis: |returned score - oracle| <= 2 * err_score + floor, where oracle = the length-penalised sum of
    the log-probabilities the CPU oracle (fp32 on the bf16-rounded weights) gives the sequence teacher-forced, err_score = the
    error against that oracle of the existing teacher-forced Qwen2Engine.score on the same sequence, and floor = 2^-8 |oracle| --
    the yardstick form of test_gpu_rows.py::test_decode_rows_step_teacher_forced: both are bf16 paths that differ in summation
    order. A hypothesis assembled from the wrong beam's tokens or scores misses by the size of a token's log-probability."""
    from cogstream_amd.llm import Qwen2Engine
    from cogstream_amd.weights import LlmConfig, random_llm_state
    from oracle import qwen2 as oq
    cfg = LlmConfig(**TR.LLM)
    st = random_llm_state(cfg, seed=7, std=0.05)
    st_r = {k: v.to(BF16).float() for k, v in st.items()}
    eng = Qwen2Engine(st, cfg, dtype=BF16, device=dev)
    okw = dict(heads=cfg.num_attention_heads, kv_heads=cfg.num_key_value_heads, layers=cfg.num_hidden_layers)
    emb = TR._prompt(dev, BF16)
    P = emb.shape[0]
    seqs, scores = eng.beam_search(emb, num_beams=4, num_return_sequences=4, max_new_tokens=NEW, eos_token_id=[], length_penalty=lp)
    for seq, got in zip(seqs, scores):
        n = len(seq)
        ids = torch.tensor(seq, device=dev)
        full = torch.cat([emb, eng.embed_tokens(ids[:-1])]) if n > 1 else emb
        hid, _ = oq.forward(st_r, full.float().cpu(), **okw)
        lps = torch.log_softmax(torch.stack([oq.logits(st_r, hid[P - 1 + i]) for i in range(n)]).double(), -1)
        oracle = float(lps[torch.arange(n), torch.tensor(seq)].sum()) / n ** lp
        targets = torch.cat([torch.full((P - 1,), -100, dtype=torch.int64), torch.tensor(seq, dtype=torch.int64)])
        forced = float(eng.score(full, targets)["logprobs"].double().sum()) / n ** lp
        err_score, floor = abs(forced - oracle), 2.0 ** -8 * abs(oracle)
        print(f"lp {lp}: score {got:.6f} oracle {oracle:.6f} teacher-forced {forced:.6f}: error {abs(got - oracle):.3g}, "
              f"bound 2 * {err_score:.3g} + {floor:.3g}")
        assert abs(got - oracle) <= 2 * err_score + floor, (seq, got, oracle, forced)
