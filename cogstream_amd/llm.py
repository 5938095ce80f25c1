"""Host mirror of the Qwen2 seams the reference calls (transformers, pinned 4.46.3):
self.get_model()(inputs_embeds=..., attention_mask=...) (model/cogreasoner_chat.py:312-316,322) and
super().generate(inputs_embeds=...) (:802-807), computing through cogs_llm_forward."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib as L
from . import beam as beam_host
from . import decode
from . import ops
from .decode import host_draw_block, philox_offset, truncate_at_eos  # noqa: F401  (tests and callers import them from here)
from .runtime import get_handle
from .weights import LlmConfig, PackedLlm


MAX_RETURN_SEQUENCES = 16      # rows of one lockstep decode step: the 16 activation columns of the MFMA tile


def check_num_return_sequences(n: int, do_sample: bool, num_beams: int = 1) -> int:
    """the argument rules of generate(num_return_sequences=): transformers 4.46.3 refuses several greedy copies, the
    lockstep step has 16 columns; with num_beams > 1 up to num_beams hypotheses may be returned (beam.check_beam_args)"""
    n = int(n)
    if n < 1 or n > MAX_RETURN_SEQUENCES:
        raise ValueError(f"num_return_sequences has to be between 1 and {MAX_RETURN_SEQUENCES}, but is {n}")
    if int(num_beams) > 1:
        beam_host.check_beam_args(num_beams, n, do_sample)
        return n
    if n > 1 and not do_sample:
        raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {n}).")
    return n


def pad_rows(rows: Sequence[Sequence[int]], pad_token_id: int) -> torch.Tensor:
    """ragged token rows -> int64 [N, L] right-padded with pad_token_id (what GenerationMixin returns for finished rows)"""
    width = max((len(r) for r in rows), default=0)
    out = torch.full((len(rows), width), int(pad_token_id), dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(list(r), dtype=torch.int64)
    return out


class KVCache:
    def __init__(self, cfg: LlmConfig, max_len: int, dtype, device):
        kvd = cfg.num_key_value_heads * cfg.head_dim
        self.k = torch.empty(cfg.num_hidden_layers, max_len, kvd, device=device, dtype=dtype)
        self.v = torch.empty_like(self.k)
        self.struct = L.KV(self.k.data_ptr(), self.v.data_ptr(), max_len, 0)

    @property
    def len(self) -> int:
        return self.struct.len

    def reset(self, length: int = 0):
        self.struct.len = length


class PrefixKV:
    """KV rows of the previous prompt, kept so that the next generate() only prefills what differs (SURVEY.md §8f
    rank 3; the reference rebuilds the whole conversation every turn, evaluate/answer_generate.py:130-148).
    The reusable prefix is found by comparing the new input embeddings with the previous ones bit for bit on the
    device: KV row i depends only on rows 0..i and the position i, so every invalidation rule (resized frames, a
    history turn dropped by the selection stage, another question) is covered by that comparison. Only rows that
    were PREFILLED are reused -- rows written by decode steps went through the GEMV kernels."""

    def __init__(self, engine: "Qwen2Engine"):
        self.engine = engine
        self.cache: Optional[KVCache] = None
        self.rows: Optional[torch.Tensor] = None   # [n, H] embeddings whose KV rows 0..n-1 are in `cache`
        self.reused = 0    # rows taken from the cache, summed over calls
        self.seen = 0      # prompt rows, summed over calls

    def plan(self, embeds: torch.Tensor, need: int) -> int:
        """-> number of leading rows of `embeds` whose KV is already in self.cache (at most len(embeds) - 2)"""
        if self.cache is None or self.cache.k.shape[1] < need:
            old = self.cache
            self.cache = self.engine.new_cache(need + need // 2)   # sessions grow: leave room for the next turns
            if old is not None and self.rows is not None:
                n = self.rows.shape[0]
                self.cache.k[:, :n].copy_(old.k[:, :n])
                self.cache.v[:, :n].copy_(old.v[:, :n])
            else:
                self.rows = None
        p = 0
        if self.rows is not None and self.rows.dtype == embeds.dtype:
            # at least 2 rows are always prefilled: a 1-row forward is the decode GEMV, whose rounding differs
            n = min(self.rows.shape[0], embeds.shape[0] - 2)
            if n > 0:
                bits = torch.int16 if embeds.element_size() == 2 else torch.int32
                neq = (self.rows[:n].view(bits) != embeds[:n].view(bits)).any(dim=1)
                idx = torch.arange(n, device=embeds.device)
                p = int(torch.where(neq, idx, torch.full_like(idx, n)).min().item())
        self.seen += embeds.shape[0]
        self.reused += p
        return p

    def drop(self):
        self.rows = None


class Qwen2Engine:
    def __init__(self, state: Dict[str, torch.Tensor], cfg: LlmConfig, dtype=torch.bfloat16, device="cuda",
                 decode_weights: Optional[str] = None):
        """decode_weights="fp8": W8A16 decode -- single-token steps stream e4m3 codes of the linears (half the bytes), every
        other pass reads the dequantised weights through the usual kernels (weights.PackedLlm / fp8_model_state). The
        multi-row step behind num_return_sequences / num_beams (decode_rows) streams the codes too (cogs_gemm_rows_fp8);
        the debug switch llm_rows_fp8 = 0 sends it through the dequantised weights again, with the same logits bits
        """
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.handle = get_handle(self.device)
        self.packed = PackedLlm(state, cfg, dtype, self.device, decode_weights=decode_weights)
        self.decode_weights = self.packed.decode_weights
        self._activate()

    def _load(self):
        L.check(L.lib.cogs_llm_load(self.handle.h, C.byref(self.packed.struct)), "cogs_llm_load")
        if self.packed.fp8_struct is not None:
            L.check(L.lib.cogs_llm_attach_fp8(self.handle.h, C.byref(self.packed.fp8_struct)), "cogs_llm_attach_fp8")

    def _activate(self):
        self.handle.activate("llm", self, self._load)

    def new_cache(self, max_len: int) -> KVCache:
        return KVCache(self.cfg, max_len, self.dtype, self.device)

    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        return ops.gather_rows(self.packed.embed, None, ids.reshape(-1).to(self.device, torch.int64))

    def forward(self, embeds: torch.Tensor, cache: Optional[KVCache] = None, *, want_logits: bool = True,
                want_pooled: bool = False, want_hidden: bool = False):
        """returns dict(logits fp32 [vocab] | pooled fp32 [H] | hidden [S,H])"""
        self._activate()
        embeds = embeds.contiguous()
        S = embeds.shape[0]
        ctx = S + (cache.len if cache is not None else 0)
        nbytes = C.c_size_t()
        L.check(L.lib.cogs_llm_workspace_bytes(self.handle.h, S, ctx, C.byref(nbytes)), "cogs_llm_workspace_bytes")
        ws = self.handle.workspace("llm", nbytes.value)
        out = {}
        logits = torch.empty(self.cfg.vocab_size, device=self.device, dtype=torch.float32) if want_logits else None
        pooled = torch.empty(self.cfg.hidden_size, device=self.device, dtype=torch.float32) if want_pooled else None
        hidden = torch.empty(S, self.cfg.hidden_size, device=self.device, dtype=self.dtype) if want_hidden else None
        L.check(L.lib.cogs_llm_forward(self.handle.h, L.current_stream(), embeds.data_ptr(), S,
                                       C.byref(cache.struct) if cache is not None else None, L.ptr(logits),
                                       L.ptr(pooled), L.ptr(hidden), ws.data_ptr(), ws.numel()), "cogs_llm_forward")
        if want_logits:
            out["logits"] = logits
        if want_pooled:
            out["pooled"] = pooled
        if want_hidden:
            out["hidden"] = hidden
        return out

    def score(self, embeds: torch.Tensor, target_ids: torch.Tensor, *, cache: Optional[KVCache] = None) -> Dict[str, torch.Tensor]:
        """Teacher-forced scoring of S rows: how probable is target_ids[i], the token that FOLLOWS row i (the caller has
        shifted; -100 = ignore, e.g. on a last row without successor). -> dict(logprobs fp32 [S] (0 where ignored), lse
        fp32 [S], argmax int64 [S] = the greedy token after every row), on the device. One forward for the final hidden
        states, then cogs_lm_score: the [S, vocab] logits are never materialised (one panel of at most 64 MiB is).
        With `cache` the rows sit at positions cache.len ..: prefill a prompt once, then score several continuations
        against it with cache.reset(prompt_len) in between. Raises ValueError for a target outside the vocabulary
        (checked once, after everything has been queued). Forward pass only: nothing here is differentiable."""
        S = embeds.shape[0]
        target_ids = target_ids.reshape(-1).to(self.device, torch.int64).contiguous()
        if target_ids.numel() != S:
            raise ValueError(f"{target_ids.numel()} targets for {S} rows")
        hidden = self.forward(embeds, cache, want_hidden=True, want_logits=False)["hidden"]
        return self.score_hidden(hidden, target_ids)

    def score_hidden(self, hidden: torch.Tensor, target_ids: torch.Tensor) -> Dict[str, torch.Tensor]:
        """score() behind the forward: final-norm hidden states [S, H] + shifted targets -> dict(logprobs, lse, argmax)"""
        target_ids = target_ids.reshape(-1).to(self.device, torch.int64).contiguous()
        res = self.lm_score(hidden, target_ids)
        # the one place the log-probability is formed
        logprobs = torch.where(target_ids == -100, torch.zeros_like(res["lse"]), res["target_logit"] - res["lse"])
        n_bad = int(res["n_bad"].item())
        if n_bad:
            raise ValueError(f"{n_bad} target ids outside [0, {self.cfg.vocab_size}) (and not -100)")
        return {"logprobs": logprobs, "lse": res["lse"], "argmax": res["argmax"]}

    def lm_score(self, hidden: torch.Tensor, target_ids: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
        """cogs_lm_score on final-norm hidden states [S, H] -> dict(lse, target_logit, max_logit fp32 [S], argmax int64
        [S], n_bad int32 [1]); no host synchronisation"""
        self._activate()
        hidden = hidden.contiguous()
        assert hidden.dtype == self.dtype and hidden.shape[1] == self.cfg.hidden_size
        S = hidden.shape[0]
        nbytes = C.c_size_t()
        L.check(L.lib.cogs_lm_score_workspace_bytes(self.handle.h, S, C.byref(nbytes)), "cogs_lm_score_workspace_bytes")
        ws = self.handle.workspace("lm_score", nbytes.value)
        f32 = dict(device=self.device, dtype=torch.float32)
        res = {"lse": torch.empty(S, **f32), "target_logit": torch.empty(S, **f32), "max_logit": torch.empty(S, **f32),
               "argmax": torch.empty(S, device=self.device, dtype=torch.int64),
               "n_bad": torch.empty(1, device=self.device, dtype=torch.int32)}
        L.check(L.lib.cogs_lm_score(self.handle.h, L.current_stream(), hidden.data_ptr(), S, L.ptr(target_ids),
                                    L.ptr(res["lse"]), L.ptr(res["target_logit"]), L.ptr(res["argmax"]),
                                    L.ptr(res["max_logit"]), L.ptr(res["n_bad"]), ws.data_ptr(), ws.numel()), "cogs_lm_score")
        return res

    def logits(self, hidden_rows: torch.Tensor) -> torch.Tensor:
        """lm_head on a caller-chosen SMALL set of final-norm hidden rows [R, H] -> fp32 [R, vocab] (cogs_gemm with fp32
        output, the accumulators of forward()'s last-row logits): R * vocab * 4 bytes, 0.6 MB per row at vocab 152 064"""
        self._activate()
        return ops.gemm(hidden_rows.contiguous(), self.packed.lm_head, out_f32=True)

    def forward_segments(self, embeds: torch.Tensor, seg_lens: Sequence[int]) -> torch.Tensor:
        """several independent sequences stored back to back -> mean of the final hidden states of each, fp32
        [nseg, H] (cogs_llm_forward_segments): one var-len prefill instead of one forward per sequence"""
        self._activate()
        embeds = embeds.contiguous()
        S = embeds.shape[0]
        cu = [0]
        for n in seg_lens:
            cu.append(cu[-1] + int(n))
        assert cu[-1] == S and all(int(n) > 0 for n in seg_lens)
        nbytes = C.c_size_t()
        L.check(L.lib.cogs_llm_workspace_bytes(self.handle.h, S, S, C.byref(nbytes)), "cogs_llm_workspace_bytes")
        ws = self.handle.workspace("llm", nbytes.value)
        out = torch.empty(len(seg_lens), self.cfg.hidden_size, device=self.device, dtype=torch.float32)
        cua = (C.c_int32 * len(cu))(*cu)
        L.check(L.lib.cogs_llm_forward_segments(self.handle.h, L.current_stream(), embeds.data_ptr(), S, cua, len(seg_lens),
                                                out.data_ptr(), ws.data_ptr(), ws.numel()), "cogs_llm_forward_segments")
        return out

    def _prefill(self, embeds, max_new_tokens, cache, prefix, prefilled):
        """the prompt pass of generate(): -> (forward result with the prompt's last-row logits, the cache that now holds the
        prompt, position of the first generated token). `prefilled`: the caller has run it; `prefix`: only the rows that
        differ from the previous call's are run; else the whole prompt, into `cache` or a new one"""
        S = embeds.shape[0]
        if prefilled is not None:
            assert cache is not None and prefix is None and cache.len >= S and "logits" in prefilled
            return prefilled, cache, cache.len
        if prefix is not None:
            assert cache is None
            embeds = embeds.contiguous()
            p = prefix.plan(embeds, S + max_new_tokens)
            cache = prefix.cache
            cache.reset(p)
            prefix.rows = None          # not valid while this call is rewriting the cache
            res = self.forward(embeds[p:], cache)
            prefix.rows = embeds        # rows 0..S-1 are prefilled; decode rows behind them are never reused
            return res, cache, S
        if cache is None:
            cache = self.new_cache(S + max_new_tokens)
        pos_start = cache.len + S
        return self.forward(embeds, cache), cache, pos_start

    def generate(self, embeds: torch.Tensor, *, max_new_tokens: int, eos_token_id: Sequence[int] = (),
                 do_sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                 repetition_penalty: float = 1.0, allowed_ids: Optional[Sequence[int]] = None,
                 prompt_ids: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                 sampler: str = "device", seed: Optional[int] = None,
                 cache: Optional[KVCache] = None, ignore_eos: bool = False,
                 prefix: Optional[PrefixKV] = None, prefilled: Optional[dict] = None,
                 stage_times: Optional[dict] = None, num_return_sequences: int = 1,
                 pad_token_id: Optional[int] = None, num_beams: int = 1, length_penalty: float = 1.0,
                 early_stopping=False):
        """GenerationMixin.generate with inputs_embeds: prefill, then one cogs_llm_forward per token (the token loop and the
        ways a row advances are decode.py's: decode.sample, decode.SingleRow / Lockstep / Replay).
        Returns the NEW token ids only. Logits processors run in HF order:
        repetition penalty -> custom (allowed-id mask) -> temperature -> top-k -> top-p.
        `prefix`: reuse the KV rows of the leading embeddings that are unchanged since the previous call.
        `prefilled`: the result of a forward(embeds, cache) the caller has already run into `cache` (bench.py times the
        prefill and the token loop separately this way); the prompt is then not prefilled again.
        Sampling (do_sample): cogs_sample on the device, tokens never visit the host. sampler="device": Philox draws
        keyed by `seed` (default: one draw of the CPU generator) and the step; sampler="host": the CPU generator
        (`generator`, default the global one) makes the [vocab] exponential draws of every step exactly as
        torch.multinomial does in the reference's CPU run, so the sampled ids are the reference's.
        num_return_sequences = N > 1 (sampling only, N <= 16): N continuations of the one prefilled prompt, advanced in
        lockstep by cogs_llm_decode_rows -> a list of N token lists (see decode.sample); pad_token_id is accepted for
        signature parity with GenerationMixin (the lists are ragged; CogReasoner.generate pads).
        num_beams = B > 1 (2 .. 16, no sampling): beam search (see beam_search) -> the best hypothesis as a token list, or,
        for num_return_sequences = N <= B, the N best as a list of lists."""
        if int(num_beams) != 1:
            seqs, _ = Qwen2Engine.beam_search(self, embeds, num_beams=num_beams, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                                              num_return_sequences=num_return_sequences, length_penalty=length_penalty,
                                              early_stopping=early_stopping, do_sample=do_sample,
                                              repetition_penalty=repetition_penalty, allowed_ids=allowed_ids, prompt_ids=prompt_ids,
                                              cache=cache, ignore_eos=ignore_eos, prefix=prefix, prefilled=prefilled)
            return seqs[0] if int(num_return_sequences) == 1 else seqs
        N = check_num_return_sequences(num_return_sequences, do_sample)
        if N > 1:
            stage_times = None             # the split is taken on the single-row path only, as before
        if stage_times is not None:        # bench.py's pipeline split: the prompt pass and the token loop, drained on both sides
            import time
            torch.cuda.synchronize()
            t_start = time.perf_counter()
        res, cache, pos_start = self._prefill(embeds, max_new_tokens, cache, prefix, prefilled)
        if stage_times is not None:
            torch.cuda.synchronize()
            t_loop = time.perf_counter()
            stage_times["answer_prefill"] = stage_times.get("answer_prefill", 0.0) + t_loop - t_start
        rows = decode.sample(self, res["logits"], cache, pos_start, N, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                             ignore_eos=ignore_eos, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
                             repetition_penalty=repetition_penalty, allowed_ids=allowed_ids, prompt_ids=prompt_ids,
                             generator=generator, sampler=sampler, seed=seed)
        if stage_times is not None:
            stage_times["decode"] = stage_times.get("decode", 0.0) + time.perf_counter() - t_loop
        return rows[0] if N == 1 else rows

    def decode_rows(self, embeds: torch.Tensor, kv: "L.KVRows", tail_slot: Optional[torch.Tensor] = None) -> torch.Tensor:
        """cogs_llm_decode_rows: one token per sequence, embeddings [R, H] -> fp32 logits [R, vocab]; advances kv.tail_len.
        tail_slot (cogs_llm_decode_rows_slots): int32 [R, kv.tail_max] on the device, row r reads tail position j from slot
        tail_slot[r, j]; the caller has set tail_slot[r, kv.tail_len] = r"""
        self._activate()
        embeds = embeds.contiguous()
        R = embeds.shape[0]
        nbytes = C.c_size_t()
        L.check(L.lib.cogs_llm_decode_rows_workspace_bytes(self.handle.h, R, kv.prefix_len, C.byref(nbytes)),
                "cogs_llm_decode_rows_workspace_bytes")
        ws = self.handle.workspace("llm_rows", nbytes.value)
        logits = torch.empty(R, self.cfg.vocab_size, device=self.device, dtype=torch.float32)
        if tail_slot is not None:
            assert tail_slot.is_cuda and tail_slot.dtype == torch.int32 and tail_slot.shape == (R, kv.tail_max) and tail_slot.is_contiguous()
            L.check(L.lib.cogs_llm_decode_rows_slots(self.handle.h, L.current_stream(), embeds.data_ptr(), R, C.byref(kv),
                                                     tail_slot.data_ptr(), logits.data_ptr(), ws.data_ptr(), ws.numel()),
                    "cogs_llm_decode_rows_slots")
            return logits
        L.check(L.lib.cogs_llm_decode_rows(self.handle.h, L.current_stream(), embeds.data_ptr(), R, C.byref(kv), logits.data_ptr(),
                                           ws.data_ptr(), ws.numel()), "cogs_llm_decode_rows")
        return logits

    def new_rows_kv(self, cache: KVCache, n_rows: int, tail_max: int, slots: bool = False):
        """the cogs_kv_rows view of `cache` (its first cache.len rows are the shared prompt) + fresh tails for n_rows
        sequences; the tail tensors are returned too (they own the memory). slots: a fourth result, the int32 [n_rows,
        tail_max] slot table of beam search (zeros: every entry names a valid slot)"""
        kvd = self.cfg.num_key_value_heads * self.cfg.head_dim
        tk = torch.empty(self.cfg.num_hidden_layers, n_rows, tail_max, kvd, device=self.device, dtype=self.dtype)
        tv = torch.empty_like(tk)
        kv = L.KVRows(cache.k.data_ptr(), cache.v.data_ptr(), cache.k.shape[1], cache.len, tk.data_ptr(), tv.data_ptr(), tail_max, 0)
        if slots:
            return kv, tk, tv, torch.zeros(n_rows, tail_max, device=self.device, dtype=torch.int32)
        return kv, tk, tv

    def beam_search(self, embeds: torch.Tensor, *, num_beams: int, max_new_tokens: int, eos_token_id: Sequence[int] = (),
                    num_return_sequences: int = 1, length_penalty: float = 1.0, early_stopping=False, do_sample: bool = False,
                    repetition_penalty: float = 1.0, allowed_ids: Optional[Sequence[int]] = None,
                    prompt_ids: Optional[torch.Tensor] = None, cache: Optional[KVCache] = None, ignore_eos: bool = False,
                    prefix: Optional[PrefixKV] = None, prefilled: Optional[dict] = None, pad_token_id: Optional[int] = None,
                    select_fn=None):
        """GenerationMixin.generate(num_beams=B, do_sample=False) on one prefilled prompt -> (the num_return_sequences best
        hypotheses as lists of new token ids, their length-penalised scores); the bookkeeping is beam.beam_search.
        The beams advance on a rows stepper of decode.py (decode.rows_stepper). bf16 / head_dim 128, decode.Lockstep: one
        cogs_llm_decode_rows_slots per step, a beam's K / V rows stay in the tail slot that wrote them and the int32 [B, t] slot
        table follows the beams' parents -- nothing of the KV moves (the debug switch beam_gather_tails = 1 copies the tails by
        parent instead; tests: the two must agree bit for bit). fp32 engines / head_dim != 128, decode.Replay: single-row steps,
        one private K / V copy per beam, gathered by parent. The token histories of the repetition penalty (decode.History) are
        reordered the same way. Then cogs_row_lse + cogs_sub_rows turn the step's logits into log-probabilities in place,
        cogs_logits_process runs per row when a penalty or mask is on (HF applies its processors to the log-probabilities in
        beam search), and cogs_beam_topk selects the candidates with row_add = the beam scores; the candidates' (value, row,
        token) triples are the step's one read-back. The shared cache is left at the prompt length, so a PrefixKV stays valid.
        select_fn: ops.beam_topk."""
        eos = [] if ignore_eos else sorted(set(int(e) for e in eos_token_id))
        B = beam_host.check_beam_args(num_beams, num_return_sequences, do_sample, len(eos))
        N = check_num_return_sequences(num_return_sequences, do_sample, B)
        res, cache, _ = self._prefill(embeds, max_new_tokens, cache, prefix, prefilled)
        V, dev = self.cfg.vocab_size, self.device
        hist = decode.History(self, B, max(max_new_tokens, 1), prompt_ids, repetition_penalty, allowed_ids, alloc=torch.zeros)
        stepper = decode.rows_stepper(self, cache, B, max(max_new_tokens, 1), slots=True)

        def logprobs(logits):                       # fp32 [rows, V] logits -> log-probabilities, in place
            return ops.sub_rows(logits, ops.row_lse(logits)["lse"])

        def process(scores, t):
            if hist.on:
                for r in range(scores.shape[0]):
                    hist.process(scores[r], r, t)
            return scores

        def step(tokens, parents):                  # the histories follow the beams, then the K / V rows do
            par = torch.tensor(parents, dtype=torch.int64, device=dev)
            tok = torch.tensor(tokens, dtype=torch.int64, device=dev)
            hist.reorder(par)
            hist.seen[:, hist.n_prompt + stepper.t] = tok
            return logprobs(stepper.step(tok, par))

        def select(scores, row_add, k):             # the candidates come back in ONE copy: the step's synchronisation
            val, crow, ctok = (select_fn or ops.beam_topk)(scores, row_add, k)
            if val.is_cuda:
                host = torch.stack([val.view(torch.int32), crow, ctok]).cpu()
                val, crow, ctok = host[0].view(torch.float32), host[1], host[2]
            return val, crow, ctok

        try:
            first = logprobs(res["logits"].view(1, V))
            seqs, scores = beam_host.beam_search(step, select, first, num_beams=B, max_new_tokens=max_new_tokens,
                                                 eos_token_id=eos, pad_token_id=pad_token_id, length_penalty=length_penalty,
                                                 early_stopping=early_stopping, num_return_sequences=N, process_fn=process)
        finally:
            stepper.close()
        return seqs, scores
