#!/usr/bin/env python3
"""Timing of teacher-forced scoring at production width (H 3 584, V 152 064, bf16), in one process, variants interleaved
round by round, HIP events around each call, medians (the method of tools/gemm_ab.py):

    python tools/lm_score_time.py [--S 64 1024 4096] [--rounds 7] [--shapes 2048x8192 1024x16384 1024x8192] [--out FILE]

  (a) cogs_lm_score: lm_head GEMM into an fp32 panel + fold, panel by panel -- per panel shape (rows x columns; the
      library caps a panel at 64 MiB), the first shape being the shipped default;
  (b) the yardstick: the same product as ONE plain cogs_gemm with bf16 output into a materialised [S, V] buffer -- what
      the library could do toward the same end before cogs_lm_score, and the floor of any panel scheme;
  (c) the fold alone (cogs_row_lse on a resident fp32 panel of the variant's shape: fold + final kernel, ten calls per
      timed window), in GB/s of panel bytes; the kernel's own time is in the rocprofv3 kernel trace of this tool.
The ratio (a)/(b) says what the 2 x S x V x 4 bytes of panel traffic cost on top of the GEMM."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cogstream_amd import _lib as L  # noqa: E402
from cogstream_amd import ops  # noqa: E402
from cogstream_amd.llm import Qwen2Engine  # noqa: E402

H, V = 3584, 152064
FOLD_REPS = 10      # (c): calls per timed window, so that the host's per-call work hides behind the queue


class LmHeadOnly(Qwen2Engine):
    """an engine that holds nothing but an lm_head: cogs_lm_score reads no other weight"""

    def __init__(self, lm_head: torch.Tensor):
        import ctypes as C
        from cogstream_amd.runtime import get_handle
        from cogstream_amd.weights import LlmConfig
        self.cfg = LlmConfig(hidden_size=H, vocab_size=V)
        self.dtype, self.device = lm_head.dtype, lm_head.device
        self.handle = get_handle(self.device)
        self._layers = (L.LlmLayer * 1)()
        w = L.LlmWeights()
        w.dtype = L.dtype_code(self.dtype)
        w.hidden, w.inter, w.layers, w.heads, w.kv_heads, w.head_dim, w.vocab = H, 512, 1, H // 128, H // 128, 128, V
        w.rms_eps, w.rope_theta, w.lm_head, w.layer = 1e-6, 1e6, lm_head.data_ptr(), self._layers
        self._w, self._lm_head = w, lm_head
        self.handle.activate("llm", self, lambda: L.check(L.lib.cogs_llm_load(self.handle.h, C.byref(w)), "cogs_llm_load"))

    def _activate(self):
        pass


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", nargs="*", default=["2048x8192", "1024x16384", "1024x8192"])
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    w = (torch.randn(V, H, device=dev, generator=gen) * 0.02).bfloat16()
    eng = LmHeadOnly(w)
    lines = [f"# tools/lm_score_time.py: H {H} V {V} bf16, {args.rounds} interleaved rounds x 2 timed calls, medians (min)",
             f"# {torch.cuda.get_device_name(0)}; {L.lib.cogs_version().decode()}"]
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes]
    for S in args.S:
        hid = torch.randn(S, H, device=dev, generator=gen).bfloat16()
        tgt = torch.randint(0, V, (S,), device=dev, generator=gen)
        full = torch.empty(S, V, device=dev, dtype=torch.bfloat16)
        variants = []
        seen = set()
        for rows, cols in shapes:
            with L.debug_switch("lm_score_rows", rows), L.debug_switch("lm_score_cols", cols):
                eng.lm_score(hid, tgt)
                geo = tuple(L.debug_get("lm_score_last_" + k) for k in ("rows", "cols", "split"))
            if geo not in seen:              # small S clamps several requests to the same panel
                seen.add(geo)
                variants.append((rows, cols, geo))
        panels = {v: torch.randn(v[2][0], v[2][1], device=dev, generator=gen) for v in variants}
        outs = {v: ops.row_lse(panels[v]) for v in variants}        # reused outputs: (c) queues FOLD_REPS calls back to back
        ta = {v: [] for v in variants}
        tc = {v: [] for v in variants}
        tb = []
        for r in range(args.rounds + 1):
            for v in variants:
                rows, cols, geo = v
                with L.debug_switch("lm_score_rows", rows), L.debug_switch("lm_score_cols", cols):
                    for rep in range(3):
                        t = timed(lambda: eng.lm_score(hid, tgt))
                        if r and rep:
                            ta[v].append(t)
                    for rep in range(3):
                        t = timed(lambda: [ops.row_lse(panels[v], out=outs[v]) for _ in range(FOLD_REPS)]) / FOLD_REPS
                        if r and rep:
                            tc[v].append(t)
            for rep in range(3):
                t = timed(lambda: ops.gemm(hid, w, out=full))
                if r and rep:
                    tb.append(t)
        b = median(tb)
        flop = 2.0 * S * V * H
        lines.append(f"S={S}: (b) one bf16-output GEMM into [S, V]: {b:.4f} ms (min {min(tb):.4f})  {flop / b / 1e9:6.0f} TFLOP/s  "
                     f"body {L.debug_get('gemm_last_body')}")
        for v in variants:
            rows, cols, geo = v
            a, c = median(ta[v]), median(tc[v])
            pbytes = geo[0] * geo[1] * 4
            lines.append(f"S={S}: panel {geo[0]}x{geo[1]} ({pbytes / 2**20:.1f} MiB, fold split {geo[2]}): (a) cogs_lm_score {a:.4f} ms "
                         f"(min {min(ta[v]):.4f})  {flop / a / 1e9:6.0f} TFLOP/s  (a)/(b) {a / b:.3f} | (c) fold alone on one resident "
                         f"panel {c * 1e3:.1f} us (min {min(tc[v]) * 1e3:.1f})  {pbytes / c / 1e6:6.0f} GB/s")
        print("\n".join(lines[-(len(variants) + 1):]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
