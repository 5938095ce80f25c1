"""Host side of generate(num_beams=B), without a GPU: beam.beam_search against GenerationMixin.generate of the installed
transformers (output for output, on a tiny Qwen2 in fp32 on the CPU), the semantics of the CPU beam_topk that the device
kernel is compared with, the argument rules, and the ABI of the new entry points."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEEDS = (0, 1, 2, 4, 5, 7)
# (num_beams, num_return_sequences, length_penalty, early_stopping, repetition_penalty)
SETTINGS = [(4, 4, 1.0, False, 1.0), (3, 2, 0.6, True, 1.0), (16, 1, 1.0, False, 1.05)]
P_LEN, NEW, EOS, PAD = 9, 10, 127, 126


def _tiny(seed):
    from transformers import Qwen2Config, Qwen2ForCausalLM
    cfg = Qwen2Config(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                      num_key_value_heads=1, vocab_size=128, eos_token_id=EOS, pad_token_id=PAD)
    torch.manual_seed(seed)
    model = Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.normal_(0, 0.2)
    prompt = torch.randint(0, 120, (1, P_LEN), generator=torch.Generator().manual_seed(seed))
    return model, prompt


def _ours(seed, B, N, lp, es, rep):
    """beam.beam_search on the tiny model: the model in fp32 on the full sequences, no cache; the CPU beam_topk"""
    from transformers import RepetitionPenaltyLogitsProcessor
    from cogstream_amd import ops
    from cogstream_amd.beam import beam_search
    model, prompt = _tiny(seed)
    eos = [EOS, int(prompt[0, 3])]
    state = {"seqs": [[]]}
    head = prompt[0].tolist()

    def logprobs(seqs):
        with torch.no_grad():
            logits = model(torch.tensor([head + s for s in seqs])).logits[:, -1].float()
        return torch.log_softmax(logits, -1)

    def step(tokens, parents):
        state["seqs"] = [state["seqs"][p] + [t] for t, p in zip(tokens, parents)]
        return logprobs(state["seqs"])

    def process(scores, t):
        if rep == 1.0:
            return scores
        return RepetitionPenaltyLogitsProcessor(rep)(torch.tensor([head + s for s in state["seqs"]]), scores)

    seqs, scores = beam_search(step, ops.beam_topk, logprobs([[]])[0], num_beams=B, max_new_tokens=NEW, eos_token_id=eos,
                               pad_token_id=PAD, length_penalty=lp, early_stopping=es, num_return_sequences=N, process_fn=process)
    return seqs, scores, model, prompt, eos


@pytest.mark.parametrize("B,N,lp,es,rep", SETTINGS)
@pytest.mark.parametrize("seed", SEEDS)
def test_beam_search_matches_transformers(seed, B, N, lp, es, rep):
    from cogstream_amd.llm import pad_rows
    seqs, scores, model, prompt, eos = _ours(seed, B, N, lp, es, rep)
    with torch.no_grad():
        want = model.generate(prompt, attention_mask=torch.ones_like(prompt), num_beams=B, num_return_sequences=N, length_penalty=lp,
                              early_stopping=es, do_sample=False, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=PAD,
                              repetition_penalty=rep, return_dict_in_generate=True, output_scores=True)
    got = torch.cat([prompt.expand(N, -1), pad_rows(seqs, PAD)], 1)
    assert got.tolist() == want.sequences.tolist(), (seed, B, seqs)
    err = (torch.tensor(scores) - want.sequences_scores).abs().max()
    assert float(err) <= 1e-4, (seed, B, scores, want.sequences_scores.tolist())
    assert all(len(s) <= NEW and all(t not in eos for t in s[:-1]) for s in seqs)


def test_some_case_has_hypotheses_of_different_lengths():
    """EOS handling and padding are exercised by the comparison above: among its cases are returned sets that are ragged"""
    B, N, lp, es, rep = SETTINGS[1]
    ragged = [len({len(s) for s in _ours(seed, B, N, lp, es, rep)[0]}) > 1 for seed in (4, 5, 7)]
    assert any(ragged), ragged


def test_beam_topk_cpu_semantics():
    from cogstream_amd import ops
    inf = float("inf")
    # the same value in two rows and twice in one row: ascending flat index
    s = torch.tensor([[1.0, 5.0, 5.0, -2.0], [5.0, 0.0, 7.0, 5.0]])
    val, row, tok = ops.beam_topk(s, None, 6)
    assert val.tolist() == [7.0, 5.0, 5.0, 5.0, 5.0, 1.0] and val.dtype == torch.float32
    assert row.tolist() == [1, 0, 0, 1, 1, 0] and tok.tolist() == [2, 1, 2, 0, 3, 0] and row.dtype == tok.dtype == torch.int32
    # row_add moves a row as a whole; one fp32 addition
    val, row, tok = ops.beam_topk(s, torch.tensor([0.0, -2.0]), 3)
    assert (val.tolist(), row.tolist(), tok.tolist()) == ([5.0, 5.0, 5.0], [0, 0, 1], [1, 2, 2])
    # -1e9 on a row: it only supplies candidates once the other rows are used up; the sum is the fp32 sum, in which -1e9 absorbs
    # the scores, so that row's candidates are all equal and come in index order
    val, row, tok = ops.beam_topk(s, torch.tensor([-1e9, 0.0]), 6)
    assert row.tolist() == [1, 1, 1, 1, 0, 0] and tok.tolist() == [2, 0, 3, 1, 0, 1]
    assert val[4].item() == val[5].item() == (torch.tensor(5.0) + torch.tensor(-1e9)).item() == -1e9
    # -inf entries rank last, in index order; k = rows * n returns everything
    m = torch.tensor([[-inf, 2.0, -inf, -inf], [-inf, -inf, 3.0, -inf]])
    val, row, tok = ops.beam_topk(m, None, 8)
    assert val.tolist() == [3.0, 2.0] + [-inf] * 6
    assert (row * 4 + tok).tolist() == [6, 1, 0, 2, 3, 4, 5, 7]
    # -0 and +0 are one value
    z = torch.tensor([[-0.0, 0.0, -0.0, 0.0]])
    assert ops.beam_topk(z, None, 4)[2].tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        ops.beam_topk(z, None, 5)
    with pytest.raises(ValueError):
        ops.beam_topk(z, None, 0)


def test_beam_argument_rules():
    from cogstream_amd.beam import candidates_per_step, check_beam_args
    from cogstream_amd.llm import Qwen2Engine, check_num_return_sequences
    assert check_beam_args(2) == 2 and check_beam_args(16, 16, False, 3) == 16
    assert check_num_return_sequences(4, False, 4) == 4 and check_num_return_sequences(1, False, 16) == 1
    assert candidates_per_step(4, 0) == 8 and candidates_per_step(4, 1) == 8 and candidates_per_step(4, 2) == 12
    with pytest.raises(ValueError, match="do_sample"):
        check_beam_args(4, 1, True)
    with pytest.raises(ValueError, match=r"`num_return_sequences` \(5\) has to be smaller or equal to `num_beams` \(4\)"):
        check_beam_args(4, 5)
    with pytest.raises(ValueError, match="smaller or equal to `num_beams`"):
        check_num_return_sequences(5, False, 4)
    for b in (17, 0, -2):
        with pytest.raises(ValueError, match="num_beams has to be between 1 and 16"):
            check_beam_args(b)
    with pytest.raises(ValueError, match="candidates per step"):
        check_beam_args(16, 1, False, 4)
    # the two-argument form is what it was
    with pytest.raises(ValueError, match=r"Greedy methods without beam search do not support `num_return_sequences` different "
                                         r"than 1 \(got 2\)\."):
        check_num_return_sequences(2, False)
    # generate() applies the rules before it touches the engine or the embeddings
    with pytest.raises(ValueError, match="do_sample"):
        Qwen2Engine.generate(None, None, max_new_tokens=4, num_beams=4, do_sample=True)
    with pytest.raises(ValueError, match="smaller or equal to `num_beams`"):
        Qwen2Engine.generate(None, None, max_new_tokens=4, num_beams=2, num_return_sequences=3)
    with pytest.raises(ValueError, match="between 1 and 16"):
        Qwen2Engine.generate(None, None, max_new_tokens=4, num_beams=17)
    with pytest.raises(ValueError, match="Greedy methods"):
        Qwen2Engine.generate(None, None, max_new_tokens=4, num_beams=1, num_return_sequences=3)


def test_beam_abi_resolves_against_the_header():
    from cogstream_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cogs.h")).read()
    for sym in ("cogs_beam_topk", "cogs_beam_topk_workspace_bytes", "cogs_llm_decode_rows_slots", "cogs_sub_rows"):
        assert re.search(r"\b" + sym + r"\s*\(", hdr), sym
        assert hasattr(L.lib, sym) and sym in L.SIGNATURES
    names = [n for n, _ in L.AttnRowsDesc._fields_]
    assert names[-2:] == ["tail_slot", "tail_slot_ld"] and names[-3] == "ws_bytes"       # appended at the end
    assert L.AttnRowsDesc().tail_slot is None and L.AttnRowsDesc().tail_slot_ld == 0     # zero = off
    assert L.debug_get("beam_gather_tails") == 0
    # refused before any device work
    n = C.c_size_t()
    assert L.lib.cogs_beam_topk_workspace_bytes(1, 8, 1, None) == L.E_INVALID
    assert L.lib.cogs_beam_topk_workspace_bytes(16, 152064, 32, C.byref(n)) == L.OK and n.value > 0
    for rows, cols, k, want in ((0, 8, 1, L.E_INVALID), (17, 8, 1, L.E_UNSUPPORTED), (1, 6, 1, L.E_INVALID), (1, 8, 9, L.E_INVALID),
                                (2, 64, 65, L.E_UNSUPPORTED), (1, 8, 0, L.E_INVALID)):
        assert L.lib.cogs_beam_topk_workspace_bytes(rows, cols, k, C.byref(n)) == want, (rows, cols, k)
    assert L.lib.cogs_beam_topk(None, None, 1, 8, 8, None, 1, None, None, None, None, 0) == L.E_INVALID
    assert L.lib.cogs_llm_decode_rows_slots(None, None, None, 1, None, None, None, None, 0) == L.E_INVALID
