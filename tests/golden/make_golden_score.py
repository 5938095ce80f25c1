#!/usr/bin/env python3
"""Fixtures of the teacher-forced scoring path (forward(labels=) / forward_train / Qwen2Engine.score), made by RUNNING
THE REFERENCE's model object on the CPU, like make_golden.py (whose helpers this imports; that file and its fixtures are
not touched). Runs only where the reference checkout exists; data only is committed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_score.py

score.npz        cases "t" / "g" of qwen2.npz's models, fp32 and cast to bf16: inputs_embeds, labels (prompt span -100,
                 answer span, one -100 planted inside the answer), the loss of Qwen2ForCausalLM.forward(labels=), per-row
                 log-probability of the following label / log-sum-exp / argmax / top-1 minus top-2 logit, the logits of the
                 last two rows. Seeds are searched until every SCORED row of the fp32 model has a top-1/top-2 margin of
                 at least 1e-2 of max |logit| -- 100 x the fp32 bar of the tests -- so that the argmax comparison there needs
                 no exclusions; the script refuses to write the file otherwise.
                 Also the text path forward(input_ids=, labels=) of the tiny e2e model ("text_*").
score_e2e.npz    forward_train under no_grad on the e2e clips "a" (8 frames + history) and "c" (150 frames, forced event
                 cosines: event compression), token compression on, in both encoder attention modes ("eager" = the
                 reference's CPU semantics as e2e.npz, "blockdiag" = per-frame attention as e2e_blockdiag.npz): the
                 prepare_inputs(answer=) ids and prompt/answer boundary, the labels after compaction, the loss, the
                 per-position log-probabilities."""
import copy
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402  (puts the repository, tests/ and the reference on sys.path)
from make_golden import LLM, QWEN2_CASES, VIT, build_ref_model, checksum, ref_chat, save  # noqa: E402

from cogstream_amd.weights import (LlmConfig, VisionConfig, random_llm_state, random_proj_state,  # noqa: E402
                                   random_vit_state)
from toy_tokenizer import ToyTokenizer  # noqa: E402
from golden.inputs import FORCED_COSINE, e2e_inputs  # noqa: E402

MARGIN = 1e-2            # of max |logit|: 100 x the fp32 bar (1e-4 of max |logit|) of tests/test_gpu_score.py
ANSWER_TOKENS = {"t": 9, "g": 12}
E2E_ANSWERS = {"a": ("He picks up the red cup.", [1]), "c": ("A person walks through several rooms.", [])}


def row_stats(logits, labels):
    """fp64 on the stored-precision logits: per row i the log-probability of labels[i + 1] (0 where ignored / last
    row), log-sum-exp, argmax, top-1 minus top-2"""
    lg = logits.double()
    lse = torch.logsumexp(lg, dim=-1)
    S = lg.shape[0]
    tgt = torch.full((S,), -100, dtype=torch.long)
    tgt[:-1] = labels[1:]
    scored = tgt != -100
    lp = torch.zeros(S, dtype=torch.float64)
    lp[scored] = lg[scored, tgt[scored]] - lse[scored]
    top2 = lg.topk(2, dim=-1).values
    return lp, lse, lg.argmax(dim=-1), top2[:, 0] - top2[:, 1], scored


def build_case_model(llm):
    lcfg = LlmConfig(**llm)
    lst = random_llm_state(lcfg, seed=7, std=0.05)
    vst = random_vit_state(VisionConfig(**VIT), seed=3, std=0.05)
    pst = random_proj_state(VIT["hidden_size"], llm["hidden_size"], seed=1, std=0.05)
    saved = dict(LLM)
    LLM.clear(); LLM.update(llm)
    try:
        return build_ref_model(vst, pst, lst), lst
    finally:
        LLM.clear(); LLM.update(saved)


def golden_score():
    out = {"transformers_version": np.array(__import__("transformers").__version__), "margin_bar": np.float64(MARGIN)}
    for tag, (llm, P) in QWEN2_CASES.items():
        model, lst = build_case_model(llm)
        A = ANSWER_TOKENS[tag]
        S = P + A
        found = None
        for seed in range(7000 + S, 7000 + S + 400):
            g = torch.Generator().manual_seed(seed)
            embeds = torch.randn(S, llm["hidden_size"], generator=g) * 0.5
            answer = torch.randint(0, llm["vocab_size"], (A,), generator=g)
            labels = torch.cat([torch.full((P,), -100, dtype=torch.long), answer])
            labels[P + A // 2] = -100                       # an ignored position inside the answer
            with torch.no_grad():
                r = model(inputs_embeds=embeds[None], attention_mask=torch.ones(1, S, dtype=torch.long), labels=labels[None])
            lp, lse, am, margin, scored = row_stats(r.logits[0].float(), labels)
            bar = MARGIN * float(r.logits.abs().max())
            if float(margin[scored].min()) >= bar:
                found = seed
                break
        if found is None:
            raise SystemExit(f"case {tag}: no seed gives every scored row a top-1/top-2 margin >= {MARGIN} max|logit|; not saving")
        print(tag, "seed", found, "S", S, "scored rows", int(scored.sum()), "min scored margin / max|logit|",
              float(margin[scored].min()) / float(r.logits.abs().max()))
        out.update({f"{tag}_embeds": embeds, f"{tag}_labels": labels, f"{tag}_seed": np.int64(found),
                    f"{tag}_cfg": np.array(json.dumps(llm)), f"{tag}_llm_checksum": np.float64(checksum(lst)),
                    f"{tag}_prompt_len": np.int64(P)})
        for prec, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            m = copy.deepcopy(model).to(dt).eval()
            with torch.no_grad():
                r = m(inputs_embeds=embeds.to(dt)[None], attention_mask=torch.ones(1, S, dtype=torch.long), labels=labels[None])
            lg = r.logits[0].float()
            lp, lse, am, margin, scored = row_stats(lg, labels)
            # the loss transformers reports must be the mean of the stored log-probabilities (pins the shift / ignore rule)
            assert abs(float(r.loss) + float(lp[scored].mean())) < (1e-5 if dt == torch.float32 else 2e-2), (float(r.loss), float(lp[scored].mean()))
            out.update({f"{tag}_loss_{prec}": np.float64(float(r.loss)), f"{tag}_logprob_{prec}": lp, f"{tag}_lse_{prec}": lse,
                        f"{tag}_argmax_{prec}": am, f"{tag}_margin_{prec}": margin, f"{tag}_last2_{prec}": lg[-2:],
                        f"{tag}_maxabs_{prec}": np.float64(float(lg.abs().max()))})
            print(tag, prec, "loss", float(r.loss))
        assert float(out[f"{tag}_margin_f32"][scored.numpy()].min()) >= MARGIN * float(out[f"{tag}_maxabs_f32"])

    # text path of forward(input_ids=, labels=) on the tiny e2e model
    model, lst = build_case_model(dict(LLM))
    tok = ToyTokenizer()
    prompt = ("<|im_start|>system\nYou are a helpful assistant.<|im_end|>\n<|im_start|>user\nWhat is on the table?<|im_end|>\n"
              "<|im_start|>assistant\n")
    answer = "A red cup.<|im_end|>"
    n_prompt = tok(prompt)["input_ids"].shape[1]
    ids = tok(prompt + answer)["input_ids"]
    labels = ids.clone()
    labels[0, :n_prompt] = -100
    with torch.no_grad():
        r = model(input_ids=ids, attention_mask=torch.ones_like(ids), labels=labels)
    lp, lse, am, margin, scored = row_stats(r.logits[0].float(), labels[0])
    out.update({"text_prompt": np.array(prompt), "text_answer": np.array(answer), "text_input_ids": ids[0], "text_labels": labels[0],
                "text_loss": np.float64(float(r.loss)), "text_logprob": lp, "text_llm_checksum": np.float64(checksum(lst))})
    print("text loss", float(r.loss))
    save("score.npz", **out)


def golden_score_e2e():
    vst = random_vit_state(VisionConfig(**VIT), seed=3, std=0.05)
    pst = random_proj_state(VIT["hidden_size"], LLM["hidden_size"], seed=1, std=0.05)
    lst = random_llm_state(LlmConfig(**LLM), seed=7, std=0.05)
    tok = ToyTokenizer()
    out = {"vit_checksum": np.float64(checksum(vst)), "llm_checksum": np.float64(checksum(lst)),
           "transformers_version": np.array(__import__("transformers").__version__)}
    for mode in ("eager", "blockdiag"):
        model = build_ref_model(vst, pst, lst)
        if mode == "blockdiag":          # per-frame attention through the reference's eager encoder, one frame per call
            venc = model.get_model().get_vision_encoder()
            whole = venc.forward

            def per_frame(pixel_values, grid_sizes, merge_sizes, whole=whole):
                outs, row = [], 0
                for (t, h, w), ms in zip(grid_sizes.tolist(), merge_sizes.tolist()):
                    for _ in range(t):
                        outs.append(whole(pixel_values[row:row + h * w], torch.tensor([[1, h, w]]), torch.tensor([ms])))
                        row += h * w
                return torch.cat(outs, 0)

            venc.forward = per_frame
        for tag, (answer, cor) in E2E_ANSWERS.items():
            inp = e2e_inputs(tag)
            enc = tok(inp["text"])
            cap = {}
            orig_prep, orig_mm = model.prepare_inputs, model.prepare_inputs_labels_for_multimodal
            orig_cos = ref_chat.F.cosine_similarity
            forced = torch.tensor(FORCED_COSINE)

            def wrap_prep(*a, **k):
                r = orig_prep(*a, **k)
                cap["ids"], cap["n_prompt"] = r[0]["input_ids"][0].clone(), int(r[1])
                return r

            def wrap_mm(*a, **k):
                cap["labels_in"] = k["labels"][0].clone()
                r = orig_mm(*a, **k)
                cap["labels_out"], cap["rows"] = r[5][0].clone(), int(r[4].shape[1])
                return r

            def wrap_cos(a, b, dim=1):
                r = orig_cos(a, b, dim=dim)
                return forced.to(r.dtype) if tag == "c" else r

            model.prepare_inputs, model.prepare_inputs_labels_for_multimodal = wrap_prep, wrap_mm
            ref_chat.F.cosine_similarity = wrap_cos
            random.seed(5)
            torch.manual_seed(5)
            try:
                with torch.no_grad():
                    r = model.forward_train(input_ids=enc["input_ids"], attention_mask=enc["attention_mask"],
                                            pixel_values=inp["pixel_values"], grid_sizes=inp["grid_sizes"],
                                            merge_sizes=inp["merge_sizes"], modals=["video"], tokenizer=tok,
                                            hist_qs=inp["hist_qs"], hist_as=inp["hist_as"],
                                            current_question=inp["current_question"], all_timestamps=inp["timestamps"],
                                            total_image_num=inp["T"], answer=answer, cor=cor, if_visual=True,
                                            original_text=inp["text"])
            finally:
                model.prepare_inputs, model.prepare_inputs_labels_for_multimodal = orig_prep, orig_mm
                ref_chat.F.cosine_similarity = orig_cos
            lp, lse, am, margin, scored = row_stats(r.logits[0].float(), cap["labels_out"])
            assert cap["rows"] == cap["labels_out"].numel() == r.logits.shape[1]
            k = f"{mode}_{tag}"
            out.update({f"{k}_answer": np.array(answer), f"{k}_cor": np.array(cor, dtype=np.int64),
                        f"{k}_input_ids": cap["ids"], f"{k}_prompt_tokens": np.int64(cap["n_prompt"]),
                        f"{k}_labels_in": cap["labels_in"], f"{k}_labels": cap["labels_out"],
                        f"{k}_loss": np.float64(float(r.loss)), f"{k}_logprob": lp,
                        f"{k}_pix_checksum": np.float64(inp["pixel_values"].double().abs().sum())})
            print(mode, tag, "prompt+answer ids", cap["ids"].numel(), "boundary", cap["n_prompt"], "rows after compression",
                  cap["rows"], "loss", float(r.loss))
    save("score_e2e.npz", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["score", "score_e2e"]
    if "score" in which:
        golden_score()
    if "score_e2e" in which:
        golden_score_e2e()
