#!/usr/bin/env python3
"""What e4m3 weights with power-of-two row scales do to the logits: the CPU oracle on weights.fp8_model_state against the
same oracle on the original weights, on the two models of tests/golden/qwen2.npz (their embeddings, every prompt row).
A property of the number format, not of any kernel; reported, not asserted. Runs without a GPU.

    python tools/fp8_quant_shift.py [--dtype bf16|fp32]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cogstream_amd.weights import (LlmConfig, dequantize_fp8_rows, fp8_model_state, quantize_fp8_rows,  # noqa: E402
                                   random_llm_state)
from oracle import qwen2 as oq  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16", help="the engine dtype the weights are rounded to first")
    args = ap.parse_args()
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    g = np.load(os.path.join(ROOT, "tests", "golden", "qwen2.npz"), allow_pickle=False)
    for tag in ("t", "g"):
        cfg = LlmConfig(**json.loads(str(g[f"{tag}_cfg"])))
        st = {k: v.to(dt).float() for k, v in random_llm_state(cfg, seed=7, std=0.05).items()}
        q = fp8_model_state(st)
        emb = torch.from_numpy(g[f"{tag}_embeds"]).float()
        kw = dict(heads=cfg.num_attention_heads, kv_heads=cfg.num_key_value_heads, layers=cfg.num_hidden_layers)
        a = oq.logits(st, oq.forward(st, emb, **kw)[0]).double()
        b = oq.logits(q, oq.forward(q, emb, **kw)[0]).double()
        rms = float(((a - b).pow(2).sum() / a.pow(2).sum()).sqrt())
        cos = float(torch.nn.functional.cosine_similarity(a, b, dim=1).mean())
        cos_min = float(torch.nn.functional.cosine_similarity(a, b, dim=1).min())
        same = float((a.argmax(1) == b.argmax(1)).double().mean())
        w = st["layers.0.mlp.down_proj.weight"]
        per_w = float(((dequantize_fp8_rows(*quantize_fp8_rows(w)) - w).double().pow(2).sum() / w.double().pow(2).sum()).sqrt())
        print(f"qwen2.npz model '{tag}' (hidden {cfg.hidden_size}, {cfg.num_hidden_layers} layers, {emb.shape[0]} rows, weights rounded to "
              f"{args.dtype} first): logits relative RMS {rms:.3e}, cosine mean {cos:.6f} min {cos_min:.6f}, same argmax on "
              f"{same * 100:.1f} % of rows; per-weight relative RMS of one linear {per_w:.3e}")


if __name__ == "__main__":
    main()
