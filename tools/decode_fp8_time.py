#!/usr/bin/env python3
"""W8A16 decode against the same model in bf16, in ONE process on ONE engine (28 layers at Qwen2-7B's dimensions, random
weights, decode_weights="fp8"): the debug switch llm_decode_fp8 alternates between the e4m3 GEMVs (1) and the dequantised
bf16 GEMVs (0), pair by pair, HIP events around each timed window (the method of tools/lm_score_time.py).

    python tools/decode_fp8_time.py [--ctx 1024 15395] [--pairs 5] [--ndec 48] [--sweep] [--out FILE]

Per context and side: ms per generated token (greedy token loop, prefill excluded), the GEMV share of a step from the
library's per-class event profiler (cogs_profile_begin / _end: events around every launch, so host gaps are not in it) and
TB/s on the weight bytes that side really reads. Then the time per GEMV shape on both sides (one call per layer's matrix,
28 back to back; every call goes through Python + ctypes, ~12 us, so the qkv / o rows read as that floor on either side).
--sweep: the four kernel variants (gemv_fp8_load x gemv_fp8_deep) on the token loop at the first context.
Exit status 1 when the fp8 side is not faster in every pair."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def gemv_ms_per_step(eng, cache, ctx, e, steps=8):
    """GEMM-class milliseconds of one single-token forward (every GEMM of a decode step is a GEMV), from the profiler"""
    cache.reset(ctx)
    eng.forward(e, cache)
    torch.cuda.synchronize()
    L.check(L.lib.cogs_profile_begin(eng.handle.h))
    for _ in range(steps):
        eng.forward(e, cache)
    ms, n = (C.c_float * 4)(), (C.c_int * 4)()
    L.check(L.lib.cogs_profile_end(eng.handle.h, L.current_stream(), ms, n))
    return ms[0] / steps, n[0] // steps


def token_loop_ms(eng, emb, cache, res, ctx, ndec):
    cache.reset(ctx)
    out = []
    t = timed(lambda: out.extend(eng.generate(emb, max_new_tokens=ndec, ignore_eos=True, cache=cache, prefilled=res)))
    return t / (ndec - 1), out[:6]           # the last token needs no forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, nargs="*", default=[1024, 15395])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--ndec", type=int, default=48)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_fp8_time.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    cfg = LlmConfig(num_hidden_layers=args.layers)
    eng = Qwen2Engine(random_llm_state(cfg, seed=2, device=dev, dtype=BF16), cfg, dtype=BF16, device=dev, decode_weights="fp8")
    H, I, V, nl = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
    qd = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim
    shapes = [("qkv", qd, H), ("o", H, H), ("gate/up", 2 * I, H), ("down", H, I)]
    weights = sum(n * k for _, n, k in shapes) * nl + V * H
    rows = sum(n for _, n, _ in shapes) * nl + V
    assert eng.packed.fp8_bytes == weights
    read = {1: weights + 4 * rows, 0: 2 * weights}                     # bytes a step streams: codes + scales / bf16
    lines = [f"# tools/decode_fp8_time.py: {nl} layers at H {H} I {I} V {V}, bf16 activations, {args.pairs} A/B pairs of {args.ndec} "
             f"tokens, llm_decode_fp8 = 1 (e4m3 codes, {read[1] / 1e9:.2f} GB per token) against 0 (dequantised bf16, {read[0] / 1e9:.2f} GB)",
             f"# {torch.cuda.get_device_name(0)}; {L.lib.cogs_version().decode()}; gemv_fp8_load {L.debug_get('gemv_fp8_load')} "
             f"gemv_fp8_deep {L.debug_get('gemv_fp8_deep')}"]
    print("\n".join(lines), flush=True)
    ok = True
    gen = torch.Generator(device=dev).manual_seed(0)
    first = None
    for ctx in args.ctx:
        emb = (torch.randn(ctx, H, device=dev, generator=gen) * 0.02).to(BF16)
        cache = eng.new_cache(ctx + args.ndec + 16)
        res = eng.forward(emb, cache)
        e1 = emb[:1].contiguous()
        if first is None:
            first = (ctx, emb, cache, res)
        t, gm, toks = {1: [], 0: []}, {1: [], 0: []}, {}
        for sw in (1, 0):                                               # warm both sides
            with L.debug_switch("llm_decode_fp8", sw):
                token_loop_ms(eng, emb, cache, res, ctx, 8)
        for pair in range(args.pairs):
            for sw in ((1, 0) if pair % 2 == 0 else (0, 1)):
                with L.debug_switch("llm_decode_fp8", sw):
                    ms, toks[sw] = token_loop_ms(eng, emb, cache, res, ctx, args.ndec)
                    assert L.debug_get("llm_last_decode_fp8") == sw
                    t[sw].append(ms)
                    gm[sw].append(gemv_ms_per_step(eng, cache, ctx, e1))
            faster = t[1][-1] < t[0][-1]
            ok = ok and faster
            lines.append(f"context {ctx} pair {pair}: fp8 {t[1][-1]:.4f} ms/token, bf16 {t[0][-1]:.4f} ms/token, ratio {t[1][-1] / t[0][-1]:.3f}"
                         f"{'' if faster else '   <-- fp8 NOT faster'}")
            print(lines[-1], flush=True)
        for sw, name in ((1, "fp8 "), (0, "bf16")):
            g = median([x[0] for x in gm[sw]])
            lines.append(f"context {ctx} {name}: median {median(t[sw]):.4f} ms/token (min {min(t[sw]):.4f}) = {1e3 / median(t[sw]):.1f} tok/s; "
                         f"GEMVs {g:.4f} ms per step in {gm[sw][0][1]} launches = {read[sw] / g / 1e9:.2f} TB/s on {read[sw] / 1e9:.2f} GB; first tokens {toks[sw]}")
        r_all, r_gemv = median(t[1]) / median(t[0]), median([x[0] for x in gm[1]]) / median([x[0] for x in gm[0]])
        lines.append(f"context {ctx}: ms/token ratio fp8 / bf16 {r_all:.3f}; GEMV-only ratio {r_gemv:.3f} (bytes: {read[1] / read[0]:.3f})"
                     f"{'  -- above 0.65: see the per-shape table' if r_gemv > 0.65 else ''}")
        print("\n".join(lines[-3:]), flush=True)
        if ctx != first[0]:
            del emb, cache, res
    # per shape, both sides: one call per layer's matrix, back to back (28 matrices of a shape are > L2 + Infinity Cache together)
    pk = eng.packed
    x = {H: (torch.randn(1, H, device=dev, generator=gen) * 0.5).to(BF16), I: (torch.randn(1, I, device=dev, generator=gen) * 0.5).to(BF16)}
    by_ptr = {t.data_ptr(): t for t in pk.keep}
    table = []
    for name, N, K in shapes + [("lm_head", V, H)]:
        key = {"qkv": "qkv", "o": "o", "gate/up": "gu", "down": "down"}.get(name)
        if key:
            codes = [pk.fp8_codes[f"layers.{i}.{key}"] for i in range(nl)]
            scales = [pk.fp8_scales[f"layers.{i}.{key}"] for i in range(nl)]
            dense = [by_ptr[getattr(pk.layers[i], key + "_w")] for i in range(nl)]
        else:
            codes, scales, dense = [pk.fp8_codes["lm_head"]] * 4, [pk.fp8_scales["lm_head"]] * 4, [pk.lm_head] * 4
        kw = dict(act=L.ACT_SWIGLU) if name == "gate/up" else (dict(out_f32=True) if name == "lm_head" else {})
        out8 = ops.gemv_fp8(x[K], codes[0], scales[0], **kw)
        out16 = ops.gemm(x[K], dense[0], **kw)
        same = bool(torch.equal(out8.view(-1), out16.view(-1)))
        t8, t16 = [], []
        for r in range(args.pairs + 1):
            a = timed(lambda: [ops.gemv_fp8(x[K], c, s, out=out8, **kw) for c, s in zip(codes, scales)]) / len(codes)
            b = timed(lambda: [ops.gemm(x[K], w, out=out16, **kw) for w in dense]) / len(dense)
            if r:
                t8.append(a)
                t16.append(b)
        a, b = median(t8), median(t16)
        per = 1 if name == "lm_head" else nl
        table.append(f"{name:8s} N {N:6d} K {K:5d}: fp8 {a * 1e3:7.1f} us {(N * K + 4 * N) / a / 1e9:5.2f} TB/s | bf16 {b * 1e3:7.1f} us "
                     f"{2 * N * K / b / 1e9:5.2f} TB/s | ratio {a / b:.3f} | x{per} = {a * per:.3f} vs {b * per:.3f} ms/token | outputs "
                     f"{'bit-identical' if same else 'differ'}")
    lines.append("per GEMV shape (Python + ctypes per call, ~12 us: rows below that are the launch floor on both sides):")
    lines += table
    print("\n".join(lines[-(len(table) + 1):]), flush=True)
    if args.sweep:
        ctx, emb, cache, res = first
        e1 = emb[:1].contiguous()
        lines.append(f"sweep at context {ctx} (fp8 side only; rows per wave follow gemv_small_n as in the bf16 GEMV): load bytes x depth "
                     "(deep = the bf16 kernel's bytes in flight per lane: R x U = 2 x 7 / 4 x 4 loads of 8 B or 2 x 4 / 4 x 2 of 16 B; else half)")
        combos = [(8, 1), (8, 0), (16, 1), (16, 0)]
        ts = {c: [] for c in combos}
        gs = {c: [] for c in combos}
        for r in range(args.pairs + 1):
            for c in combos:
                with L.debug_switch("gemv_fp8_load", c[0]), L.debug_switch("gemv_fp8_deep", c[1]):
                    ms, _ = token_loop_ms(eng, emb, cache, res, ctx, args.ndec)
                    g = gemv_ms_per_step(eng, cache, ctx, e1)[0]
                if r:
                    ts[c].append(ms)
                    gs[c].append(g)
        for c in combos:
            lines.append(f"  gemv_fp8_load {c[0]:2d} gemv_fp8_deep {c[1]}: median {median(ts[c]):.4f} ms/token (min {min(ts[c]):.4f}); GEMVs "
                         f"{median(gs[c]):.4f} ms per step = {read[1] / median(gs[c]) / 1e9:.2f} TB/s")
        print("\n".join(lines[-(len(combos) + 1):]), flush=True)
    lines.append("fp8 faster in every pair: " + ("yes" if ok else "NO"))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
