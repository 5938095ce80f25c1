"""How the rows of one generate() advance, written once (host code only; llm.py imports this module, never the reverse).

  * History: the token history the logits processors see, whose tail is the generated ids.
  * SingleRow / Lockstep / Replay: the three ways a step is taken. step(tokens, parents, live) -> fp32 logits [rows, vocab] of
    the token after `tokens`; close(n_kept) puts the shared cache back where the caller expects it.
  * sample(): the one token loop of sampling and greedy decoding, N >= 1 rows. Beam search (llm.Qwen2Engine.beam_search)
    drives a rows stepper and a History from beam.beam_search.

The engine is duck-typed -- cfg, dtype, device, forward, embed_tokens, decode_rows, new_rows_kv -- and so is the cache (k, v
[layers, max_len, kv_dim], len, reset): tests/test_decode_host.py runs everything here against a CPU toy."""
from __future__ import annotations

from typing import List, Sequence

import torch

from . import _lib as L
from . import ops


def philox_offset(step: int, n_rows: int, row: int) -> int:
    """sampler="device": the Philox offset of row `row` at step `step` of an n_rows-wide generate (= step at n_rows 1)"""
    return step * n_rows + row


def host_draw_block(generator, n_rows: int, vocab: int) -> torch.Tensor:
    """sampler="host": the ONE [n_rows, vocab] Exponential(1) block torch.multinomial(probs[n_rows, vocab], 1) draws on the CPU
    generator per step, row-major (row r of the block decides row r's token; n_rows 1: GenerationMixin._sample's [vocab] draw,
    transformers 4.46.3 -- the reference's CPU path draws from the global generator)"""
    return torch.empty(n_rows, vocab, dtype=torch.float32).exponential_(1, generator=generator)


def truncate_at_eos(rows: Sequence[Sequence[int]], eos) -> List[List[int]]:
    """every row up to and including its first EOS"""
    eos = set(int(e) for e in eos)
    out = []
    for r in rows:
        hit = next((i for i, t in enumerate(r) if t in eos), None)
        out.append(list(r) if hit is None else list(r[:hit + 1]))
    return out


class History:
    """[rows, n_prompt + max_new] int64 on the device: the prompt ids, then the generated ids. The generated ids ARE the tail of
    the repetition-penalty history: argmax / the sampler write them once, straight into `toks`, and they feed the next
    embedding gather without a host round trip. alloc: torch.zeros where whole rows are copied before they are full (beams)."""

    def __init__(self, engine, rows: int, max_new: int, prompt_ids, repetition_penalty: float, allowed_ids, alloc=torch.empty):
        dev = engine.device
        self.allowed = torch.tensor(list(allowed_ids), dtype=torch.int32, device=dev) if allowed_ids is not None else None
        self.penalty = repetition_penalty
        self.on = repetition_penalty != 1.0 or self.allowed is not None     # the temperature is applied inside cogs_sample
        self.n_prompt = int(prompt_ids.numel()) if prompt_ids is not None else 0
        self.seen = alloc(rows, self.n_prompt + max_new, dtype=torch.int64, device=dev)
        if self.n_prompt:
            self.seen[:, :self.n_prompt] = prompt_ids.reshape(1, -1).to(dev)

    @property
    def toks(self) -> torch.Tensor:
        """the generated block [rows, max_new], a view"""
        return self.seen[:, self.n_prompt:]

    def process(self, logits: torch.Tensor, row: int, t: int) -> None:
        """repetition penalty -> allowed-id mask on `row`'s logits for its t-th generated token, in place"""
        if self.on:
            n = self.n_prompt + t
            prev = self.seen[row, :n] if (n and self.penalty != 1.0) else None
            ops.logits_process(logits, prev, self.penalty, self.allowed, 1.0)

    def reorder(self, parents: torch.Tensor) -> None:
        """row b continues row parents[b] (int64 on the device): the histories follow the beams"""
        self.seen = self.seen.index_select(0, parents)


class SingleRow:
    """one sequence on the cache itself: every step is one forward that appends a row"""
    per_row = False

    def __init__(self, engine, cache, pos_start: int):
        self.engine, self.cache, self.pos_start = engine, cache, pos_start

    def step(self, tokens, parents=None, live=None):
        return self.engine.forward(self.engine.embed_tokens(tokens), self.cache)["logits"].view(1, -1)

    def close(self, n_kept: int):
        # forwards issued past the EOS only wrote KV rows that are dropped again here (nothing to drop when the run was not cut)
        self.cache.reset(min(self.cache.len, self.pos_start + n_kept - 1))


class Lockstep:
    """bf16 / head_dim 128: the rows share the cache's prompt and advance together, one cogs_llm_decode_rows per token, their own
    K / V rows in per-row tails. With `parents` (slots=True) a row's K / V stay in the tail slot that wrote them and the int32
    [rows, t] slot table follows the parents -- or, under the debug switch beam_gather_tails, the tails are copied by parent
    and no table is passed (the two must agree bit for bit)."""
    per_row = False

    def __init__(self, engine, cache, rows: int, max_steps: int, slots: bool = False):
        self.engine, self.cache, self.P, self.t = engine, cache, cache.len, 0
        self.kv, self.tail_k, self.tail_v, *slot = engine.new_rows_kv(cache, rows, max_steps, slots=slots)
        self.slot = slot[0] if slots else None
        self.gather = L.debug_get("beam_gather_tails") != 0
        self.ident = torch.arange(rows, dtype=torch.int32, device=engine.device) if slots else None

    def step(self, tokens, parents=None, live=None):
        t, table = self.t, None
        if parents is not None and self.gather:
            if t:
                self.tail_k[:, :, :t] = self.tail_k[:, parents, :t]
                self.tail_v[:, :, :t] = self.tail_v[:, parents, :t]
        elif parents is not None:
            assert self.slot is not None, "parents need a stepper built with slots=True"
            table = self.slot.index_select(0, parents)
            table[:, t] = self.ident
            self.slot = table
        self.t = t + 1
        return self.engine.decode_rows(self.engine.embed_tokens(tokens.contiguous()), self.kv, table)

    def close(self, n_kept: int = 0):
        self.cache.reset(self.P)


class Replay:
    """any engine: one private K / V copy per row, [rows][layers][max_steps][kv_dim], replayed behind the prompt through the one
    cache -- per stepped row the private rows are copied behind the prompt, the single-row forward appends one more, and that
    one is copied back. With `parents` the copies are gathered first and the rows' logits are copied into one [rows, vocab]
    tensor (the selection reads it whole); without, each row's own logits tensor is handed back, in a list. With `live` only
    those rows are stepped (the other entries of the result are not written)."""
    per_row = True

    def __init__(self, engine, cache, rows: int, max_steps: int):
        self.engine, self.cache, self.P, self.t, self.rows = engine, cache, cache.len, 0, rows
        self.k = torch.empty((rows, cache.k.shape[0], max_steps, cache.k.shape[2]), device=engine.device, dtype=engine.dtype)
        self.v = torch.empty_like(self.k)

    def step(self, tokens, parents=None, live=None):
        eng, cache, P, t = self.engine, self.cache, self.P, self.t
        if parents is not None:
            self.k, self.v = self.k.index_select(0, parents), self.v.index_select(0, parents)
        out = torch.empty(self.rows, eng.cfg.vocab_size, device=eng.device, dtype=torch.float32) if parents is not None else [None] * self.rows
        for r in (range(self.rows) if live is None else live):
            cache.k[:, P:P + t] = self.k[r, :, :t]
            cache.v[:, P:P + t] = self.v[r, :, :t]
            cache.reset(P + t)
            out[r] = eng.forward(eng.embed_tokens(tokens[r:r + 1]), cache)["logits"]
            self.k[r, :, t] = cache.k[:, P + t]
            self.v[r, :, t] = cache.v[:, P + t]
        self.t = t + 1
        return out

    def close(self, n_kept: int = 0):
        self.cache.reset(self.P)


def rows_stepper(engine, cache, rows: int, max_steps: int, slots: bool = False):
    """several rows behind the prompt in `cache`: the multi-row kernels exist for bf16 at head_dim 128"""
    if engine.dtype == torch.bfloat16 and engine.cfg.head_dim == 128:
        return Lockstep(engine, cache, rows, max_steps, slots)
    return Replay(engine, cache, rows, max_steps)


def sample(engine, first: torch.Tensor, cache, pos_start: int, n_rows: int, *, max_new_tokens: int, eos_token_id, ignore_eos,
           do_sample, temperature, top_k, top_p, repetition_penalty, allowed_ids, prompt_ids, generator, sampler,
           seed) -> List[List[int]]:
    """GenerationMixin._sample / _greedy on the n_rows times expanded prompt, without expanding it -> n_rows lists of new ids.
    `first`: the prompt's last-row logits. Every row has the same history then, so they are processed once, in place; N > 1
    rows each draw their first token from a copy. Row r of step s draws with philox_offset(s, N, r) (device sampler) or from
    row r of the step's host_draw_block (host sampler: steps issued past the EOS would advance the CPU generator beyond where
    GenerationMixin stops, so the stop test runs every step; else every 8 steps and at the last). A row that has produced
    an EOS is cut there; in lockstep it keeps being stepped until every row is done (rows do not influence one another), a
    per-row stepper stops stepping it."""
    N, V = n_rows, engine.cfg.vocab_size
    hist = History(engine, N, max_new_tokens, prompt_ids, repetition_penalty, allowed_ids)
    eos = set() if ignore_eos else set(int(e) for e in eos_token_id)
    host = bool(do_sample) and sampler == "host"
    if do_sample and sampler == "device" and seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
    top_p = 1.0 if top_p is None else top_p
    if N > 1 or max_new_tokens > 0:
        hist.process(first, 0, 0)
    if max_new_tokens <= 0:
        return [[] for _ in range(N)]
    stepper = SingleRow(engine, cache, pos_start) if N == 1 else rows_stepper(engine, cache, N, max_new_tokens)
    toks = hist.toks
    check_every = 1 if host else 8
    live = list(range(N))
    logits = rows = None
    draws = lambda: host_draw_block(generator, N, V).to(engine.device, non_blocking=True)  # noqa: E731
    for step in range(max_new_tokens):
        block = draws() if host and N > 1 else None             # N rows: the step's block, ahead of the step's launches
        for r in live:
            if step == 0:
                row = first.clone() if N > 1 else first
            else:
                row = logits[r]
                hist.process(row, r, step)
            if host and N == 1:
                block = draws()                                  # one row: behind the processors
            if do_sample:
                ops.sample(row, top_k or 0, top_p, draws=block[r] if host else None, seed=seed or 0,
                           offset=philox_offset(step, N, r), temperature=temperature, out=toks[r, step:step + 1])
            else:
                ops.argmax(row, out=toks[r, step:step + 1])
        produced = step + 1
        last = produced == max_new_tokens
        if eos and (produced % check_every == 0 or (last and not stepper.per_row)):      # the host only looks at the ids here
            got = toks[:, :produced].tolist()
            done = [any(t in eos for t in row) for row in got]
            if all(done):
                rows = got if type(stepper) is Lockstep else None     # (the others read again below, as their loops always did)
                break
            if stepper.per_row:
                live = [r for r in live if not done[r]]
        if not last:
            logits = stepper.step(toks[:, step], live=live)
    rows = truncate_at_eos(rows if rows is not None else toks[:, :produced].tolist(), eos)
    stepper.close(len(rows[0]))
    return rows
