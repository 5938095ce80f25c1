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
Writes profiles/decode_rows_time.txt (or --out).

    python tools/decode_rows_time.py --fp8 [--ctx ...] [--rows ...] [--rounds 5] [--steps 12] [--out FILE]

The fp8-engine arm (decode_weights="fp8"): the same multi-row step on ONE engine in one process with the debug switch
llm_rows_fp8 alternating 0 (the dequantised bf16 matrices through gemm_rows_kernel: the path before the e4m3 kernel existed)
and 1 (the codes through gemm_rows_fp8_kernel), interleaved pair by pair, sampler excluded; before a shape is timed one step
under either switch is compared bit for bit. Per context and R: every pair, the medians, and whether fp8 won EVERY pair
(the rule for the switch's default). Then per GEMM shape of the model (qkv, o, gate/up, down, lm_head) at M = 4 and
16: ops.gemm_rows against ops.gemm_rows_fp8 over rotating weight copies (more than the 256 MiB Infinity Cache holds), time and
TB/s on the bytes each side actually reads (weights, + 4 bytes of scale per row for fp8).
Writes profiles/decode_rows_fp8_time.txt (or --out)."""
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


def fp8_arm(args, dev):
    from cogstream_amd import ops
    cfg = LlmConfig(num_hidden_layers=args.layers)
    eng = Qwen2Engine(random_llm_state(cfg, seed=2, device=dev, dtype=BF16), cfg, dtype=BF16, device=dev, decode_weights="fp8")
    H, I, V, nl = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
    kvd = cfg.num_key_value_heads * cfg.head_dim
    qd_q = cfg.num_attention_heads * cfg.head_dim
    qd = qd_q + 2 * kvd
    elems = (qd * H + H * qd_q + 2 * I * H + H * I) * nl + V * H
    rows_n = (qd + H + 2 * I + H) * nl + V
    wb = {0: 2 * elems, 1: elems + 4 * rows_n}
    n = args.steps
    lines = [f"# tools/decode_rows_time.py --fp8: {nl} layers at H {H} I {I} V {V}, fp8 engine (bf16 activations); {args.rounds} interleaved "
             f"pairs of {n} steps per side; llm_rows_fp8 = 0 reads {wb[0] / 1e9:.2f} GB of dequantised bf16 weights per step, "
             f"1 reads {wb[1] / 1e9:.2f} GB of e4m3 codes and scales",
             f"# {torch.cuda.get_device_name(0)}; {L.lib.cogs_version().decode()}; shipped llm_rows_fp8 = {L.debug_get('llm_rows_fp8')}",
             "# HIP events around each window of steps; the steps are timed without the sampler; the logits of one step under "
             "either switch are compared bit for bit before a shape is timed"]
    print("\n".join(lines), flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    verdict = True
    for ctx in args.ctx:
        emb = (torch.randn(ctx, H, device=dev, generator=gen) * 0.02).to(BF16)
        cache = eng.new_cache(ctx + n + 16)
        eng.forward(emb, cache)
        for R in args.rows:
            e = (torch.randn(R, H, device=dev, generator=gen) * 0.02).to(BF16)

            def multi(sw, steps=n):
                with L.debug_switch("llm_rows_fp8", sw):
                    cache.reset(ctx)
                    kv, tk, tv = eng.new_rows_kv(cache, R, steps + 1)
                    first = eng.decode_rows(e, kv)                        # warm (workspace, first touch of the tails)
                    assert L.debug_get("llm_last_rows_fp8") == sw
                    if steps == 0:
                        torch.cuda.synchronize()
                        return first
                    return timed(lambda: [eng.decode_rows(e, kv) for _ in range(steps)]) / steps

            same = torch.equal(multi(0, 0).view(torch.int32), multi(1, 0).view(torch.int32))
            multi(0), multi(1)
            t = {0: [], 1: []}
            for rnd in range(args.rounds):
                for sw in ((0, 1) if rnd % 2 == 0 else (1, 0)):
                    t[sw].append(multi(sw))
            # the GEMMs of a step under either switch (events around every launch: host gaps are not in it)
            gm = {}
            for sw in (0, 1):
                with L.debug_switch("llm_rows_fp8", sw):
                    cache.reset(ctx)
                    kv, tk, tv = eng.new_rows_kv(cache, R, 5)             # 1 warm + 4 profiled steps
                    eng.decode_rows(e, kv)
                    torch.cuda.synchronize()
                    L.check(L.lib.cogs_profile_begin(eng.handle.h))
                    for _ in range(4):
                        eng.decode_rows(e, kv)
                    ms, cnt = (C.c_float * 4)(), (C.c_int * 4)()
                    L.check(L.lib.cogs_profile_end(eng.handle.h, L.current_stream(), ms, cnt))
                    gm[sw] = ms[0] / 4
            cache.reset(ctx)
            wins = sum(b < a for a, b in zip(t[0], t[1]))
            if R >= 2 and wins != args.rounds:
                verdict = False
            m0, m1 = median(t[0]), median(t[1])
            pairs = " ".join(f"{a:.4f}/{b:.4f}" for a, b in zip(t[0], t[1]))
            lines.append(f"context {ctx:5d} R {R:2d}: bf16 {m0:.4f} ms/step | fp8 {m1:.4f} ms/step | fp8 / bf16 {m1 / m0:.3f} | fp8 faster in "
                         f"{wins} of {args.rounds} pairs | GEMMs {gm[0]:.4f} ms = {wb[0] / gm[0] / 1e9:.2f} TB/s / {gm[1]:.4f} ms = {wb[1] / gm[1] / 1e9:.2f} TB/s | "
                         f"logits {'bit-identical' if same else 'DIFFER'} | pairs bf16/fp8: {pairs}")
            print(lines[-1], flush=True)
        del emb, cache
    lines.append(f"# rule: llm_rows_fp8 = 1 ships only if fp8 is faster in EVERY pair at R >= 2 at every context: "
                 f"{'met' if verdict else 'NOT met'} in this run")
    print(lines[-1], flush=True)
    # ---- the GEMMs alone, shape by shape: one call per layer's matrix, back to back (the 28 matrices of a shape are more than
    # L2 and the Infinity Cache hold together), on the engine's own codes / dequantised matrices
    pk = eng.packed
    by_ptr = {t.data_ptr(): t for t in pk.keep}
    lines.append(f"# per shape: ops.gemm_rows (dequantised bf16) against ops.gemm_rows_fp8 (codes) over the {nl} layers' matrices, median of "
                 f"{args.rounds} interleaved pairs; TB/s on the weight (+ scale) bytes each side reads. Python + ctypes per call, ~12 us: "
                 "rows below that are the launch floor on both sides")
    shapes = [("qkv", qd, H, "qkv", {}), ("o", H, qd_q, "o", {}), ("gate/up", 2 * I, H, "gu", dict(act=L.ACT_SWIGLU)),
              ("down", H, I, "down", {}), ("lm_head", V, H, None, dict(out_f32=True))]
    for name, N, K, key, kw in shapes:
        if key:
            codes = [pk.fp8_codes[f"layers.{i}.{key}"] for i in range(nl)]
            scales = [pk.fp8_scales[f"layers.{i}.{key}"] for i in range(nl)]
            dense = [by_ptr[getattr(pk.layers[i], key + "_w")] for i in range(nl)]
        else:
            codes, scales, dense = [pk.fp8_codes["lm_head"]] * 4, [pk.fp8_scales["lm_head"]] * 4, [pk.lm_head] * 4
        for M in (4, 16):
            a = (torch.randn(M, K, device=dev, generator=gen) * 0.5).to(BF16)
            o16 = ops.gemm_rows(a, dense[0], **kw)
            o8 = ops.gemm_rows_fp8(a, codes[0], scales[0], **kw)
            same = torch.equal(o16.view(torch.uint8), o8.view(torch.uint8))

            def side(sw):
                if sw == 0:
                    return timed(lambda: [ops.gemm_rows(a, w, out=o16, **kw) for _ in range(4) for w in dense]) / (4 * len(dense))
                return timed(lambda: [ops.gemm_rows_fp8(a, c, sc, out=o8, **kw) for _ in range(4) for c, sc in zip(codes, scales)]) / (4 * len(codes))

            side(0), side(1)
            t = {0: [], 1: []}
            for rnd in range(args.rounds):
                for sw in ((0, 1) if rnd % 2 == 0 else (1, 0)):
                    t[sw].append(side(sw))
            m0, m1 = median(t[0]), median(t[1])
            lines.append(f"  {name:8s} N {N:6d} K {K:5d} M {M:2d}: bf16 {m0 * 1e3:8.2f} us = {2 * N * K / m0 / 1e9:.2f} TB/s | fp8 {m1 * 1e3:8.2f} us = "
                         f"{(N * K + 4 * N) / m1 / 1e9:.2f} TB/s | fp8 / bf16 {m1 / m0:.3f} | outputs {'bit-identical' if same else 'DIFFER'}")
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, nargs="*", default=[1024, 15395])
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 2, 4, 8, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--fp8", action="store_true", help="the fp8-engine arm: llm_rows_fp8 0 / 1 on one engine")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "decode_rows_fp8_time.txt" if args.fp8 else "decode_rows_time.txt")
    if not torch.cuda.is_available():
        sys.exit("decode_rows_time.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    if args.fp8:
        lines = fp8_arm(args, dev)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return 0
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
