#!/usr/bin/env python3
"""The beam-search step (cogs_llm_decode_rows_slots behind generate(num_beams=B)) against the plain lockstep step
(cogs_llm_decode_rows) on the same tails, in ONE process on ONE engine (28 layers at Qwen2-7B's dimensions, random bf16
weights), interleaved round by round, HIP events around each timed window (the method of tools/decode_rows_time.py).

    python tools/decode_beam_time.py [--ctx 1024] [--beams 2 4 8 16] [--tails 1 64 512] [--rounds 5] [--steps 6] [--out FILE]

Per B and number of generated tokens t, three steps at tail length t, every one including what its variant does per step:
  plain   decode_rows, every row reads its own tail (no beam search: the yardstick)
  table   slot = slot[parents]; slot[:, t] = arange(B); decode_rows with the table (the slot table holds a random permutation
          of the slots at every position, so every row's tail is scattered over all slots)
  gather  tail_k / tail_v[:, :, :t] = ...[:, parents, :t] (the physical copy the table avoids), then the plain step
and the ratio table / plain per interleaved pair (median, and the pair-to-pair spread min .. max). Then, per B, what the
selection adds to a step: cogs_row_lse + cogs_sub_rows (logits -> log-probabilities), cogs_beam_topk with k = 2B, and the
read-back of the 2B (value, row, token) triples (wall clock: it is the step's synchronisation).
Writes profiles/decode_beam_time.txt (or --out)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cogstream_amd import _lib as L  # noqa: E402
from cogstream_amd import ops  # noqa: E402
from cogstream_amd.llm import Qwen2Engine  # noqa: E402
from cogstream_amd.weights import LlmConfig, random_llm_state  # noqa: E402

BF16 = torch.bfloat16


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--beams", type=int, nargs="*", default=[2, 4, 8, 16])
    ap.add_argument("--tails", type=int, nargs="*", default=[1, 64, 512])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "decode_beam_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_beam_time.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    cfg = LlmConfig(num_hidden_layers=args.layers)
    eng = Qwen2Engine(random_llm_state(cfg, seed=2, device=dev, dtype=BF16), cfg, dtype=BF16, device=dev)
    H, V, nl = cfg.hidden_size, cfg.vocab_size, cfg.num_hidden_layers
    kvd = cfg.num_key_value_heads * cfg.head_dim
    n, ctx = args.steps, args.ctx
    tail_max = max(args.tails) + 8
    lines = [f"# tools/decode_beam_time.py: {nl} layers at H {H} V {V}, bf16, context {ctx}; {args.rounds} interleaved rounds of {n} steps "
             f"per variant, all at one tail length (kv.tail_len is set back before every step)",
             f"# {torch.cuda.get_device_name(0)}; {L.lib.cogs_version().decode()}",
             "# ratio = table step / plain step of the same round (median; spread = min .. max over the rounds' pairs)"]
    print("\n".join(lines), flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    emb = (torch.randn(ctx, H, device=dev, generator=gen) * 0.02).to(BF16)
    cache = eng.new_cache(ctx + 16)
    eng.forward(emb, cache)
    for B in args.beams:
        e = (torch.randn(B, H, device=dev, generator=gen) * 0.02).to(BF16)
        kv, tk, tv, _ = eng.new_rows_kv(cache, B, tail_max, slots=True)
        tk.normal_(0, 0.5)
        tv.normal_(0, 0.5)
        ident = torch.arange(B, dtype=torch.int32, device=dev)
        par = torch.randperm(B, device=dev, generator=gen)
        # a random permutation of the slots at every tail position
        slot0 = torch.stack([torch.randperm(B, device=dev, generator=gen) for _ in range(tail_max)], 1).to(torch.int32).contiguous()
        for t in args.tails:
            state = {"slot": slot0.clone()}

            def plain_step():
                kv.tail_len = t
                return eng.decode_rows(e, kv)

            def table_step():
                kv.tail_len = t
                s = state["slot"].index_select(0, par)
                s[:, t] = ident
                state["slot"] = s
                return eng.decode_rows(e, kv, s)

            def gather_step():
                kv.tail_len = t
                tk[:, :, :t] = tk[:, par, :t]
                tv[:, :, :t] = tv[:, par, :t]
                return eng.decode_rows(e, kv)

            variants = [plain_step, table_step, gather_step]
            for f in variants:
                f()                                                        # warm (workspace, first touch)
            torch.cuda.synchronize()
            ms = [[], [], []]
            for rnd in range(args.rounds):
                order = [0, 1, 2] if rnd % 2 == 0 else [2, 1, 0]
                for i in order:
                    ms[i].append(timed(lambda: [variants[i]() for _ in range(n)]) / n)
            ratios = [b / a for a, b in zip(ms[0], ms[1])]
            copied = 2 * nl * B * t * kvd * 2
            lines.append(f"B {B:2d} t {t:3d}: plain {median(ms[0]):.4f} ms/step | table {median(ms[1]):.4f} | ratio {median(ratios):.4f} "
                         f"(spread {min(ratios):.4f} .. {max(ratios):.4f}) | gather {median(ms[2]):.4f} ms/step "
                         f"({median(ms[2]) / median(ms[0]):.3f} x plain; copies {copied / 1e6:.1f} MB per step)")
            print(lines[-1], flush=True)
        # the selection on its own
        logits = plain_step().clone()
        add = torch.zeros(B, device=dev)
        k = 2 * B
        keep = logits.clone()

        def to_logprobs():
            logits.copy_(keep)
            ops.sub_rows(logits, ops.row_lse(logits)["lse"])

        to_logprobs()
        ops.beam_topk(logits, add, k)
        t_lp = median([timed(lambda: [to_logprobs() for _ in range(8)]) / 8 for _ in range(args.rounds)])
        t_copy = median([timed(lambda: [logits.copy_(keep) for _ in range(8)]) / 8 for _ in range(args.rounds)])
        t_sel = median([timed(lambda: [ops.beam_topk(logits, add, k) for _ in range(8)]) / 8 for _ in range(args.rounds)])
        back = []
        for _ in range(args.rounds * 4):
            val, row, tok = ops.beam_topk(logits, add, k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.stack([val.view(torch.int32), row, tok]).cpu()
            back.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"B {B:2d} selection: row_lse + sub_rows {t_lp - t_copy:.4f} ms | beam_topk k={k} {t_sel:.4f} ms (incl. its workspace "
                     f"allocation) | read-back of {k} triples {median(back):.4f} ms wall (idle stream)")
        print(lines[-1], flush=True)
        del kv, tk, tv
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
