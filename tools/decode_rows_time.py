#!/usr/bin/env python3
"""The lockstep multi-row decode step (cogs_llm_decode_rows, behind generate(num_return_sequences=R)) against R single-row
steps of the untouched single-sequence path, in ONE process on ONE engine (28 layers at Qwen2-7B's dimensions, random bf16
weights), interleaved round by round, HIP events around each timed window (the method of tools/decode_fp8_time.py).

    python tools/decode_rows_time.py [--ctx 1024 15395] [--rows 1 2 4 8 16] [--rounds 5] [--steps 12] [--out FILE]

Per context and R: ms per multi-row step, ms per single-row step, the ratio  step(R) / (R x single step)  -- below 1 is what
sharing the weight stream buys; at or above 1 at R >= 4 the kernel, not the bytes, is the limit -- the GEMM share of the
multi-row step from the library's per-class event profiler, and the ALGORITHMIC bytes a step reads (a formula, not a
counter reading): the weights once (they do not grow
with R) plus the KV cache, whose shared prefix is read once per tile of 16 query columns and kv head
(ceil(R x heads per kv head / 16) times) and whose tails are R private rows per generated token.
Writes profiles/decode_rows_time.txt (or --out)."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cogstream_amd import _lib as L  # noqa: E402
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
    ap.add_argument("--ctx", type=int, nargs="*", default=[1024, 15395])
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 2, 4, 8, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "decode_rows_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_rows_time.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    cfg = LlmConfig(num_hidden_layers=args.layers)
    eng = Qwen2Engine(random_llm_state(cfg, seed=2, device=dev, dtype=BF16), cfg, dtype=BF16, device=dev)
    H, I, V, nl = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
    kvd = cfg.num_key_value_heads * cfg.head_dim
    gsz = cfg.num_attention_heads // cfg.num_key_value_heads
    qd = cfg.num_attention_heads * cfg.head_dim + 2 * kvd
    w_bytes = 2 * ((qd * H + H * cfg.num_attention_heads * cfg.head_dim + 2 * I * H + H * I) * nl + V * H)
    n = args.steps
    lines = [f"# tools/decode_rows_time.py: {nl} layers at H {H} I {I} V {V}, bf16; {args.rounds} interleaved rounds of {n} steps per side; "
             f"weights {w_bytes / 1e9:.2f} GB per step on either side",
             f"# {torch.cuda.get_device_name(0)}; {L.lib.cogs_version().decode()}",
             "# ratio = multi-row step / (R x single-row step); the steps are timed without the sampler (N logits_process + N sample "
             "launches per step in generate(), the same per sequence on either side)",
             "# GB = ALGORITHMIC bytes of a multi-row step (weights once + shared prefix once per 16-column tile and kv head + tails "
             "at mid-run length): a formula, not a counter reading"]
    print("\n".join(lines), flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    for ctx in args.ctx:
        emb = (torch.randn(ctx, H, device=dev, generator=gen) * 0.02).to(BF16)
        cache = eng.new_cache(ctx + n + 16)
        eng.forward(emb, cache)
        for R in args.rows:
            e = (torch.randn(R, H, device=dev, generator=gen) * 0.02).to(BF16)
            e1 = e[:1].contiguous()

            def multi():
                cache.reset(ctx)
                kv, tk, tv = eng.new_rows_kv(cache, R, n + 1)
                eng.decode_rows(e, kv)                                   # warm (workspace, first touch of the tails)
                return timed(lambda: [eng.decode_rows(e, kv) for _ in range(n)]) / n

            def single():
                cache.reset(ctx)
                eng.forward(e1, cache)
                return timed(lambda: [eng.forward(e1, cache) for _ in range(n)]) / n

            multi(), single()
            tm, ts = [], []
            for rnd in range(args.rounds):
                for side in ((0, 1) if rnd % 2 == 0 else (1, 0)):
                    (tm if side == 0 else ts).append(multi() if side == 0 else single())
            # GEMM share of the multi-row step (events around every launch: host gaps are not in it)
            cache.reset(ctx)
            kv, tk, tv = eng.new_rows_kv(cache, R, 5)                   # 1 warm + 4 profiled steps, whatever --steps is
            eng.decode_rows(e, kv)
            torch.cuda.synchronize()
            L.check(L.lib.cogs_profile_begin(eng.handle.h))
            for _ in range(4):
                eng.decode_rows(e, kv)
            ms, cnt = (C.c_float * 4)(), (C.c_int * 4)()
            L.check(L.lib.cogs_profile_end(eng.handle.h, L.current_stream(), ms, cnt))
            cache.reset(ctx)
            tiles = (R * gsz + 15) // 16
            kv_bytes = 2 * nl * kvd * 2 * (ctx * tiles + R * (n // 2 + 1))      # prefix once per tile; tails at mid-run length
            m, s = median(tm), median(ts)
            lines.append(f"context {ctx:5d} R {R:2d}: multi-row {m:.4f} ms/step (min {min(tm):.4f}) | single-row {s:.4f} ms/step x {R} = {s * R:.4f} | "
                         f"ratio {m / (s * R):.3f} | per sequence {m / R:.4f} ms/token | GEMMs {ms[0] / 4:.4f} ms ({w_bytes / (ms[0] / 4) / 1e9:.2f} TB/s "
                         f"on the weights), attention {ms[1] / 4:.4f} ms | algorithmic reads {(w_bytes + kv_bytes) / 1e9:.2f} GB = {w_bytes / 1e9:.2f} weights + "
                         f"{kv_bytes / 1e9:.3f} KV ({tiles} prefix pass{'es' if tiles > 1 else ''})")
            print(lines[-1], flush=True)
        del emb, cache
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
