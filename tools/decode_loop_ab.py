#!/usr/bin/env python3
"""The host token loops behind Qwen2Engine.generate, for comparing two checkouts of the Python tree on ONE build of the library
(COGS_LIB_PATH): the driver behind profiles/decode_loop_ab.txt. It imports cogstream_amd from the tree it lies in.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/decode_loop_ab.py record OUT.txt
    python tools/decode_loop_ab.py time [--rounds 5]

record: one fixed, seeded script over the toy engines of tests/test_gpu_rows.py (hidden 256, 2 layers, head_dim 128, vocab 512;
bf16 and fp32; a 40-row prompt): N = 1 greedy and sampled, N = 4 sampled, B = 4 beams, with the stop, cache, prefix and sampler
variants listed in record(). OUT.txt gets one line per call: the token lists, the beam score bits, cache.len afterwards, the
sha256 of the CPU generator's state afterwards, the prefix statistics where a prefix is used.
time: ms per generated token of WHOLE generate() calls (HIP events around the call: the host loop is inside) at Qwen2-7B's
dimensions, context 1 024, 32 new tokens, ignore_eos: N = 1 greedy, N = 4 with the device sampler, B = 4 beams.
One process, no time limit of its own: start it under `timeout`."""
import argparse
import hashlib
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cogstream_amd import _lib as L  # noqa: E402
from cogstream_amd.llm import PrefixKV, Qwen2Engine  # noqa: E402
from cogstream_amd.weights import LlmConfig, random_llm_state  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
LLM = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
           vocab_size=512, image_token_index=500, eos_token_id=499)
SAMPLE = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.05)


def record(path):
    dev = torch.device("cuda:0")
    cfg = LlmConfig(**LLM)
    state = random_llm_state(cfg, seed=7, std=0.05)
    engines = {"bf16": Qwen2Engine(state, cfg, dtype=BF16, device=dev), "fp32": Qwen2Engine(state, cfg, dtype=F32, device=dev)}
    rows = torch.randn(52, LLM["hidden_size"], generator=torch.Generator().manual_seed(9)) * 0.5
    ids = torch.randint(0, 480, (1, 40), generator=torch.Generator().manual_seed(2))
    pen = dict(repetition_penalty=1.05, allowed_ids=list(range(7, 400, 2)), prompt_ids=ids)
    lines = []

    def gen_state(g):
        return "-" if g is None else hashlib.sha256(g.get_state().numpy().tobytes()).hexdigest()[:16]

    def call(name, eng="bf16", *, cache=None, emb=None, generator=None, beams=False, **kw):
        e = engines[eng]
        emb = (rows[:40] if emb is None else emb).to(dev, e.dtype)
        cache = e.new_cache(200) if (cache is None and "prefix" not in kw) else cache
        g = torch.Generator().manual_seed(generator) if generator is not None else None
        extra = ""
        if beams:
            out, scores = e.beam_search(emb, cache=cache, **kw)
            extra = " scores=" + ",".join(struct.pack("<f", s).hex() for s in scores)
        else:
            out = e.generate(emb, cache=cache, **({"generator": g} if g is not None else {}), **kw)
        if "prefix" in kw:
            p = kw["prefix"]
            cache, extra = p.cache, extra + f" prefix={p.reused}/{p.seen}"
        lines.append(f"{name}: {out} cache_len={cache.len} gen={gen_state(g)}{extra}")
        return out

    # N = 1 greedy: plain and with penalty + mask; lengths around the 8-step stop test; a stop inside a window and across one
    for tag, kw in (("plain", {}), ("pen", pen)):
        for m in (0, 1, 8, 9, 20):
            free = call(f"greedy_{tag}_m{m}", max_new_tokens=m, eos_token_id=[], **kw)
        for at in (2, 10):
            call(f"greedy_{tag}_eos{at}", max_new_tokens=20, eos_token_id=[free[at]], **kw)
        call(f"greedy_{tag}_ignore_eos", max_new_tokens=20, eos_token_id=[free[2]], ignore_eos=True, **kw)
    cache = engines["bf16"].new_cache(200)
    call("greedy_cache_call1", cache=cache, max_new_tokens=20, eos_token_id=[free[2]], **pen)
    call("greedy_cache_call2", cache=cache, emb=rows[40:52], max_new_tokens=9, eos_token_id=[])
    prefix = PrefixKV(engines["bf16"])
    call("greedy_prefix_call1", prefix=prefix, max_new_tokens=8, eos_token_id=[])
    call("greedy_prefix_call2", prefix=prefix, emb=torch.cat([rows[:30], rows[40:52]]), max_new_tokens=8, eos_token_id=[])
    cache = engines["bf16"].new_cache(200)
    res = engines["bf16"].forward(rows[:40].to(dev, BF16), cache)
    call("greedy_prefilled", cache=cache, prefilled=res, max_new_tokens=8, eos_token_id=[])
    # N = 1 sampled
    call("sample1_device_seed", max_new_tokens=12, eos_token_id=[], seed=5, **SAMPLE)
    call("sample1_device_generator", max_new_tokens=12, eos_token_id=[], generator=4, **SAMPLE)
    free = call("sample1_host", max_new_tokens=12, eos_token_id=[], generator=4, sampler="host", **SAMPLE)
    call("sample1_host_eos", max_new_tokens=12, eos_token_id=[free[2]], generator=4, sampler="host", **SAMPLE)
    # N = 4 sampled
    for eng in ("bf16", "fp32"):
        kw = dict(SAMPLE, eng=eng, num_return_sequences=4, prompt_ids=ids)
        free = call(f"rows_{eng}_device", max_new_tokens=20, eos_token_id=[], seed=3, **kw)
        call(f"rows_{eng}_device_eos", max_new_tokens=20, eos_token_id=[free[0][2]], seed=3, **kw)
        call(f"rows_{eng}_device_generator", max_new_tokens=9, eos_token_id=[], generator=6, **kw)
        free = call(f"rows_{eng}_host", max_new_tokens=12, eos_token_id=[], generator=4, sampler="host", **kw)
        call(f"rows_{eng}_host_eos", max_new_tokens=12, eos_token_id=sorted({r[2] for r in free}), generator=4, sampler="host", **kw)
        for m in (0, 1):
            call(f"rows_{eng}_m{m}", max_new_tokens=m, eos_token_id=[], seed=3, allowed_ids=list(range(7, 400, 2)), **kw)
    # B = 4 beams, the 4 best returned
    for eng in ("bf16", "fp32"):
        kw = dict(eng=eng, beams=True, num_beams=4, num_return_sequences=4, max_new_tokens=12)
        free = call(f"beam_{eng}_free", eos_token_id=[], **kw)
        eos = [free[0][2]]
        call(f"beam_{eng}_eos", eos_token_id=eos, **kw)
        call(f"beam_{eng}_lp06", eos_token_id=eos, length_penalty=0.6, **kw)
        call(f"beam_{eng}_early", eos_token_id=eos, early_stopping=True, **kw)
        call(f"beam_{eng}_never", eos_token_id=eos, early_stopping="never", **kw)
        call(f"beam_{eng}_pen", eos_token_id=eos, **pen, **kw)
        with L.debug_switch("beam_gather_tails", 1):
            call(f"beam_{eng}_gather", eos_token_id=eos, **pen, **kw)
        call(f"beam_{eng}_m1", eos_token_id=eos, **dict(kw, max_new_tokens=1))
    torch.cuda.synchronize()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} calls -> {path}")


def time_generate(rounds):
    dev = torch.device("cuda:0")
    cfg = LlmConfig()
    eng = Qwen2Engine(random_llm_state(cfg, seed=2, device=dev, dtype=BF16), cfg, dtype=BF16, device=dev)
    ctx, new = 1024, 32
    emb = (torch.randn(ctx, cfg.hidden_size, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 0.02).to(BF16)
    cache = eng.new_cache(ctx + new + 16)
    cases = (("greedy_n1", dict()), ("sample_n4", dict(do_sample=True, top_k=20, top_p=0.8, temperature=0.7, seed=1, num_return_sequences=4)),
             ("beams_b4", dict(num_beams=4)))

    def run(kw):
        cache.reset(0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = eng.generate(emb, max_new_tokens=new, ignore_eos=True, cache=cache, **kw)
        e1.record()
        torch.cuda.synchronize()
        assert len(out if isinstance(out[0], int) else out[0]) == new
        return e0.elapsed_time(e1)

    print(f"# {torch.cuda.get_device_name(0)}; {L.lib.cogs_version().decode()}; context {ctx}, {new} new tokens, the prompt pass is inside "
          f"every call; median of {rounds} calls after one warm call", flush=True)
    for name, kw in cases:
        run(kw)
        t = sorted(run(kw) for _ in range(rounds))
        print(f"{name} ms_per_token {t[rounds // 2] / new:.4f} (whole call: median {t[rounds // 2]:.3f} ms, min {t[0]:.3f}, max {t[-1]:.3f})",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["record", "time"])
    ap.add_argument("out", nargs="?")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_loop_ab.py runs on the GPU; there is none here")
    if args.mode == "record":
        if not args.out:
            ap.error("record needs OUT.txt")
        record(args.out)
    else:
        time_generate(args.rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
