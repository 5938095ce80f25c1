"""Beam search for one prompt, host side: GenerationMixin.generate(num_beams=B, do_sample=False) behind
model/cogreasoner_chat.py:802-807, written against the model through two callables so that it runs on any engine (and on the
CPU, where tests/test_beam_host.py compares it with the installed transformers output for output).

The bookkeeping follows GenerationMixin._beam_search of the transformers installed at build time (5.x: the vectorised
form with running beams / finished beams / an early-stop heuristic; the reference pins 4.46.3 with the BeamSearchScorer
heap -- DESIGN.md §4.7 lists where the two can differ), for batch size 1, in fp32 as there:

  * running beam scores start as [0, -1e9, ...]: step 0 selects from the single prefill row;
  * per step K = max(2, 1 + number of EOS ids) * B candidates are taken from scores[b] + running_score[b], best first;
  * a candidate "hits" when its token is an EOS id or it is the max_new_tokens-th token; the first B candidates that do not hit
    are the next running beams; a hit at rank < B becomes a finished hypothesis with score value / length ** length_penalty
    (length = generated tokens including this one), a hit at rank >= B is dropped;
  * the B best finished hypotheses are kept; the loop ends when the best running score, length-penalised with the current
    length (early_stopping=False) or max_new_tokens ("never", length_penalty > 0), cannot beat the worst of B finished ones, or
    (early_stopping=True) as soon as B hypotheses are finished, or when every candidate of a step hit.

This module imports no GPU code."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch

NEG = -1.0e9          # GenerationMixin's "minus infinity" for beam scores (fp32: absorbs any log-probability sum)
MAX_BEAMS = 16        # rows of one lockstep decode step
MAX_CANDIDATES = 64   # cogs_beam_topk's k


def candidates_per_step(num_beams: int, n_eos: int) -> int:
    """beams_to_keep of GenerationMixin._beam_search"""
    return max(2, 1 + int(n_eos)) * int(num_beams)


def check_beam_args(num_beams: int, num_return_sequences: int = 1, do_sample: bool = False, n_eos: int = 1) -> int:
    """the argument rules of generate(num_beams=B > 1); the messages are GenerationConfig.validate's where it has one"""
    B, n = int(num_beams), int(num_return_sequences)
    if B < 2 or B > MAX_BEAMS:
        raise ValueError(f"num_beams has to be between 1 and {MAX_BEAMS}, but is {B}")
    if do_sample:
        raise ValueError("beam sampling (`num_beams` > 1 with `do_sample=True`) is not supported: use `do_sample=False`")
    if n < 1:
        raise ValueError(f"num_return_sequences has to be between 1 and {MAX_BEAMS}, but is {n}")
    if n > B:
        raise ValueError(f"`num_return_sequences` ({n}) has to be smaller or equal to `num_beams` ({B}).")
    if candidates_per_step(B, n_eos) > MAX_CANDIDATES:
        raise ValueError(f"num_beams {B} with {n_eos} EOS ids needs {candidates_per_step(B, n_eos)} candidates per step; "
                         f"at most {MAX_CANDIDATES} are selected")
    return B


def _order_desc(x: torch.Tensor) -> List[int]:
    """indices of x in descending order, equal values by ascending index"""
    return torch.sort(-x, stable=True).indices.tolist()


def beam_search(step_fn: Callable, select_fn: Callable, first_logprobs: torch.Tensor, *, num_beams: int, max_new_tokens: int,
                eos_token_id: Sequence[int], pad_token_id: Optional[int] = None, length_penalty: float = 1.0,
                early_stopping=False, num_return_sequences: int = 1,
                process_fn: Optional[Callable] = None) -> Tuple[List[List[int]], List[float]]:
    """-> (the num_return_sequences best hypotheses as lists of NEW token ids, a closing EOS included, best first; their
    scores = sum of log-probabilities / length ** length_penalty).

    first_logprobs  fp32 [V]: log-softmax of the prompt's last-row logits
    step_fn(tokens, parents) -> fp32 [B, V] log-probabilities of the token after `tokens[b]`, where beam b continues beam
                    parents[b] of the previous call (of the prompt, at the first call: parents are all 0 then)
    process_fn(scores [rows, V], t) -> the scores after the logits processors, which HF applies to the log-probabilities; row b
                    belongs to the beam whose last token was tokens[b] of the latest step_fn call (t = 0: one row, the prompt)
    select_fn(scores [rows, V], row_add fp32 [rows] (on the CPU), k) -> (values, rows, tokens): ops.beam_topk
    pad_token_id is accepted for signature parity (the result is ragged; pad_rows / CogReasoner.generate pad it)."""
    B = int(num_beams)
    eos = set(int(e) for e in eos_token_id)
    K = candidates_per_step(B, len(eos))
    lp = float(length_penalty)
    if max_new_tokens <= 0:
        return [[] for _ in range(num_return_sequences)], [0.0] * num_return_sequences
    running_seqs: List[List[int]] = [[] for _ in range(B)]
    running_scores = torch.full((B,), NEG, dtype=torch.float32)
    running_scores[0] = 0.0
    fin_seqs: List[List[int]] = [[] for _ in range(B)]
    fin_scores = torch.full((B,), NEG, dtype=torch.float32)
    fin_done = [False] * B
    unsatisfied = True
    scores = first_logprobs.reshape(1, -1)
    for t in range(max_new_tokens):
        if process_fn is not None:
            scores = process_fn(scores, t)
        if t == 0 and K > scores.shape[1]:         # fewer tokens than candidates: HF's B identical rows, B - 1 of them at -1e9
            scores = scores.expand(B, -1).contiguous()
        rows = scores.shape[0]
        vals, crow, ctok = select_fn(scores, running_scores[:rows], min(K, rows * scores.shape[1]))
        vals = torch.as_tensor(vals, dtype=torch.float32).cpu()          # the one read-back of the step
        crow, ctok = [int(x) for x in crow.tolist()], [int(x) for x in ctok.tolist()]
        n = len(ctok)
        cand_seqs = [running_seqs[crow[i]] + [ctok[i]] for i in range(n)]
        last = t + 1 == max_new_tokens
        hit = torch.tensor([last or ctok[i] in eos for i in range(n)])
        # the running beams of the next step: the best B that did not hit
        run_vals = vals + hit.to(torch.float32) * NEG
        keep = _order_desc(run_vals)[:B]
        # finished hypotheses: hits among the first B candidates, length-penalised
        top = torch.arange(n) < B
        new = vals / ((t + 1) ** lp)
        new = new + (~(hit & top)).to(torch.float32) * NEG
        merged = torch.cat([fin_scores, new])
        merged_seqs = fin_seqs + cand_seqs
        merged_done = fin_done + (hit & top).tolist()
        best = _order_desc(merged)[:B]
        fin_scores = merged[best]
        fin_seqs = [merged_seqs[i] for i in best]
        fin_done = [merged_done[i] for i in best]
        parents = [crow[i] for i in keep]
        tokens = [ctok[i] for i in keep]
        running_seqs = [cand_seqs[i] for i in keep]
        running_scores = run_vals[keep]
        while len(parents) < B:                    # (only when K candidates did not exist: rows * V < B)
            parents.append(parents[-1]); tokens.append(tokens[-1]); running_seqs.append(running_seqs[-1])
            running_scores = torch.cat([running_scores, torch.tensor([NEG])])
        # can a running beam still beat the worst finished hypothesis?
        length = max_new_tokens if (early_stopping == "never" and lp > 0.0) else t + 1
        best_possible = running_scores[0] / (length ** lp)
        worst = torch.where(torch.tensor(fin_done), fin_scores.min(), torch.tensor(NEG))
        unsatisfied = unsatisfied and bool((best_possible > worst).any())
        if not unsatisfied or (all(fin_done) and early_stopping is True) or bool(hit.all()):
            break
        scores = step_fn(tokens, parents)
    N = int(num_return_sequences)
    return [list(s) for s in fin_seqs[:N]], [float(x) for x in fin_scores[:N]]
