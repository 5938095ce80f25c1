#!/usr/bin/env python3
"""One fixed script over the host drivers, for comparing two builds of the library (COGS_LIB_PATH) launch by launch and byte
by byte: the driver behind profiles/attn_plan_ab.txt section 1.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/attn_plan_driver.py OUT.txt

Seeded tiny models: a ViT (hidden 576, 2 layers, head_dim 72) on three videos of different grids in both attention modes and
on one video of three 224-patch frames (the compile-time ragged end), the projector; a bf16 Qwen2 (hidden 256, 2 layers,
head_dim 128, vocab 512): a prompt with cache, decode steps, rows behind the cached prefix, a prompt without cache, segments,
decode_rows without and with a slot table, generate, one e4m3 decode step, teacher-forced scoring. OUT.txt gets one line per
output tensor: name, shape, bytes, sha256. One process, no time limit of its own: start it under `timeout`."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cogstream_amd import vision as V  # noqa: E402
from cogstream_amd.llm import Qwen2Engine  # noqa: E402
from cogstream_amd.vision import Projector, VisionEncoder  # noqa: E402
from cogstream_amd.weights import LlmConfig, VisionConfig, random_llm_state, random_proj_state, random_vit_state  # noqa: E402

BF16 = torch.bfloat16


def main():
    dev = torch.device("cuda:0")
    outs = []

    def rec(name, t):
        t = t.detach().contiguous().cpu()
        b = t.view(torch.int16 if t.dtype == BF16 else torch.uint8).numpy().tobytes()
        outs.append(f"{name} {tuple(t.shape)} {len(b)} {hashlib.sha256(b).hexdigest()}")

    torch.manual_seed(0)
    vcfg = VisionConfig(hidden_size=576, intermediate_size=200, num_hidden_layers=2, num_attention_heads=8)
    lcfg = LlmConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                     vocab_size=512, image_token_index=500, eos_token_id=499)
    vst = random_vit_state(vcfg, seed=3, std=0.05)
    pst = random_proj_state(vcfg.hidden_size, lcfg.hidden_size, std=0.05)
    lst = random_llm_state(lcfg, seed=7, std=0.05)
    enc = VisionEncoder(vst, vcfg, dtype=BF16, device=dev)
    proj = Projector(pst, dtype=BF16, device=dev)
    eng = Qwen2Engine(lst, lcfg, dtype=BF16, device=dev)

    # ViT: three videos of different grids in both attention modes, then one video of three 224-patch frames
    grid = torch.tensor([[4, 4, 6], [2, 6, 6], [1, 2, 4]])
    merge = torch.tensor([2, 2, 2])
    pix = torch.rand(int(grid.prod(dim=1).sum()), 588) * 2 - 1
    for name, mode in (("blockdiag", V.BLOCK_DIAG), ("eager", V.REF_EAGER_GLOBAL)):
        rec("vit_" + name, enc(pix.to(dev), grid, merge, attn_mode=mode))
    pix1 = torch.rand(3 * 14 * 16, 588) * 2 - 1
    tok1 = enc(pix1.to(dev), torch.tensor([[3, 14, 16]]), torch.tensor([2]))
    rec("vit_uniform224", tok1)
    mm = proj(tok1)                                          # 168 rows of LLM input
    rec("proj", mm)

    # Qwen2: prompt with cache, decode steps, rows behind the cached prefix, prompt without cache, segments
    cache = eng.new_cache(400)
    rec("prefill_logits", eng.forward(mm[:150], cache)["logits"])
    e1 = mm[150:151].contiguous()
    for i in range(3):
        rec(f"decode{i}", eng.forward(e1, cache)["logits"])
    rec("continue5", eng.forward(mm[151:156].contiguous(), cache)["logits"])
    rec("kcache", cache.k[:, :cache.len])
    rec("vcache", cache.v[:, :cache.len])
    rec("nocache", eng.forward(mm[:7].contiguous())["logits"])
    rec("segments", eng.forward_segments(mm[:5].contiguous(), [3, 2]))
    # two lockstep steps of three rows over that cache, without and with a slot table
    e3 = mm[20:23].contiguous()
    for slots in (False, True):
        kv, tk, tv, *table = eng.new_rows_kv(cache, 3, 6, slots=slots)
        for i in range(2):
            if slots:
                table[0][:, kv.tail_len] = torch.arange(3, dtype=torch.int32, device=dev)
                rec(f"rows_slots{i}", eng.decode_rows(e3, kv, table[0]))
            else:
                rec(f"rows{i}", eng.decode_rows(e3, kv))
        rec(f"rows_tk{int(slots)}", tk[:, :, :2])
        rec(f"rows_tv{int(slots)}", tv[:, :, :2])
    # teacher-forced scoring, an e4m3 prompt + decode step, generate
    sc = eng.score(mm[:5].contiguous(), torch.tensor([1, 2, 3, 4, -100]))
    for key in ("lse", "logprobs", "argmax"):
        rec("score_" + key, sc[key])
    eng8 = Qwen2Engine(lst, lcfg, dtype=BF16, device=dev, decode_weights="fp8")
    cache8 = eng8.new_cache(64)
    rec("fp8_prefill", eng8.forward(mm[:9].contiguous(), cache8)["logits"])
    rec("fp8_decode", eng8.forward(e1, cache8)["logits"])
    outs.append(f"generate {eng.generate(mm[:40].contiguous(), max_new_tokens=4, ignore_eos=True)}")
    torch.cuda.synchronize()
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(outs) + "\n")
    print(f"{len(outs)} outputs -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
