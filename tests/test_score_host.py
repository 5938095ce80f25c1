"""Teacher-forced scoring, host side (no GPU): the fixtures of tests/golden/make_golden_score.py against the fp64
oracle, and the host logic of CogReasoner.forward_train / prepare_inputs(answer=) / label compaction with every device
stage stubbed."""
import json
import os
import types

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LLM = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
           vocab_size=512, image_token_index=258, eos_token_id=257)


def _load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def _shifted(labels: torch.Tensor) -> torch.Tensor:
    t = torch.full_like(labels, -100)
    t[:-1] = labels[1:]
    return t


@pytest.mark.parametrize("tag", ["t", "g"])
def test_fp64_oracle_reproduces_the_scoring_fixture(tag):
    """oracle forward in fp64 -> logits of every row -> log-softmax in fp64 == the reference's fp32 loss / log-probs
    within 1e-5: pins score.npz and its conventions (row i is scored against labels[i + 1], -100 ignored, mean over the
    scored rows)."""
    from cogstream_amd.weights import LlmConfig, random_llm_state
    from oracle import qwen2 as oq
    g = _load("score.npz")
    cfg = json.loads(str(g[f"{tag}_cfg"]))
    lcfg = LlmConfig(**cfg)
    st = random_llm_state(lcfg, seed=7, std=0.05)
    assert abs(float(sum(v.double().abs().sum() for v in st.values())) - float(g[f"{tag}_llm_checksum"])) < 1e-6
    w = {k: v.double() for k, v in st.items()}
    hid = oq.forward(w, torch.from_numpy(g[f"{tag}_embeds"]).double(), heads=lcfg.num_attention_heads,
                     kv_heads=lcfg.num_key_value_heads, layers=lcfg.num_hidden_layers)[0]
    lg = oq.logits(w, hid).double()
    labels = torch.from_numpy(g[f"{tag}_labels"])
    P = int(g[f"{tag}_prompt_len"])
    assert (labels[:P] == -100).all() and int((labels[P:] == -100).sum()) == 1        # one hole inside the answer
    tgt = _shifted(labels)
    scored = tgt != -100
    lse = torch.logsumexp(lg, dim=-1)
    lp = torch.zeros_like(lse)
    lp[scored] = lg[scored, tgt[scored]] - lse[scored]
    ref_lp = torch.from_numpy(g[f"{tag}_logprob_f32"])
    print(f"score[{tag}] oracle vs fixture: logprob max diff {float((lp - ref_lp).abs().max()):.2e}, "
          f"loss {float(-lp[scored].mean()):.7f} vs {float(g[f'{tag}_loss_f32']):.7f}")
    assert float((lp - ref_lp).abs().max()) <= 1e-5 * float(ref_lp.abs().max())
    assert float((lse - torch.from_numpy(g[f"{tag}_lse_f32"])).abs().max()) <= 1e-5 * float(lse.abs().max())
    assert abs(float(-lp[scored].mean()) - float(g[f"{tag}_loss_f32"])) <= 1e-5 * float(g[f"{tag}_loss_f32"])
    assert (ref_lp[~scored] == 0).all()
    # the margins the GPU test's argmax comparison relies on
    assert torch.equal(lg.argmax(-1)[scored], torch.from_numpy(g[f"{tag}_argmax_f32"])[scored])
    assert float(torch.from_numpy(g[f"{tag}_margin_f32"])[scored].min()) >= float(g["margin_bar"]) * float(g[f"{tag}_maxabs_f32"])


def test_fp64_oracle_reproduces_the_text_path_loss():
    from cogstream_amd.weights import LlmConfig, random_llm_state
    from oracle import qwen2 as oq
    from toy_tokenizer import ToyTokenizer
    g = _load("score.npz")
    lcfg = LlmConfig(**LLM)
    w = {k: v.double() for k, v in random_llm_state(lcfg, seed=7, std=0.05).items()}
    tok = ToyTokenizer()
    ids = tok(str(g["text_prompt"]) + str(g["text_answer"]))["input_ids"][0]
    assert torch.equal(ids, torch.from_numpy(g["text_input_ids"]))
    labels = torch.from_numpy(g["text_labels"])
    assert int((labels == -100).sum()) == tok(str(g["text_prompt"]))["input_ids"].shape[1]
    hid = oq.forward(w, w["embed_tokens.weight"][ids], heads=2, kv_heads=1, layers=2)[0]
    lg = oq.logits(w, hid).double()
    tgt = _shifted(labels)
    scored = tgt != -100
    lp = lg[scored, tgt[scored]] - torch.logsumexp(lg[scored], dim=-1)
    assert abs(float(-lp.mean()) - float(g["text_loss"])) <= 1e-5 * float(g["text_loss"])


def _host_model(use_token_compression=True):
    """a CogReasoner whose engines are placeholders: only host logic may run"""
    from cogstream_amd.chat import CogReasoner
    from cogstream_amd.weights import LlmConfig
    fake = types.SimpleNamespace(device=torch.device("cpu"), dtype=torch.float32)
    return CogReasoner(fake, None, None, LlmConfig(**LLM), generation_config=dict(do_sample=False),
                       use_token_compression=use_token_compression)


@pytest.mark.parametrize("mode", ["eager", "blockdiag"])
@pytest.mark.parametrize("tag", ["a", "c"])
def test_forward_train_label_layout_matches_reference(mode, tag, monkeypatch):
    """forward_train builds the selection string from `cor`, prompt + answer through prepare_inputs(answer=), labels =
    -100 on the prompt + the answer ids -- ids, boundary and labels equal what the reference's forward_train built"""
    from golden.inputs import e2e_inputs
    from toy_tokenizer import ToyTokenizer
    g = _load("score_e2e.npz")
    k = f"{mode}_{tag}"
    inp = e2e_inputs(tag)
    model = _host_model()
    seen = {}
    monkeypatch.setattr(model, "forward", lambda **kw: seen.update(kw) or "result")
    tok = ToyTokenizer()
    enc = tok(inp["text"])
    out = model.forward_train(input_ids=enc["input_ids"], attention_mask=enc["attention_mask"], pixel_values="px",
                              grid_sizes="grid", merge_sizes="merge", modals=["video"], tokenizer=tok,
                              hist_qs=inp["hist_qs"], hist_as=inp["hist_as"], current_question=inp["current_question"],
                              all_timestamps=inp["timestamps"], total_image_num=inp["T"], answer=str(g[f"{k}_answer"]),
                              cor=g[f"{k}_cor"].tolist(), if_visual=True, original_text=inp["text"])
    assert out == "result"
    assert torch.equal(seen["input_ids"][0], torch.from_numpy(g[f"{k}_input_ids"]))
    assert torch.equal(seen["labels"][0], torch.from_numpy(g[f"{k}_labels_in"]))
    n = int(g[f"{k}_prompt_tokens"])
    assert model.last_debug["train_prompt_tokens"] == n and (seen["labels"][0, :n] == -100).all()
    assert seen["labels"][0, n:].tolist() == tok(str(g[f"{k}_answer"]))["input_ids"][0].tolist()
    assert seen["pixel_values"] == "px" and seen["total_image_num"] == inp["T"] and seen["if_visual"] is True
    # prepare_inputs(answer=) on its own: (prompt + answer, boundary); without answer the old (prompt, if_visual)
    sel = "[" + ",".join(["yes"] + [str(c) for c in g[f"{k}_cor"].tolist()]) + "]"
    new_inputs, boundary = model.prepare_inputs(sel, original_text=inp["text"], answer=str(g[f"{k}_answer"]))
    assert boundary == n and torch.equal(new_inputs["input_ids"][0], torch.from_numpy(g[f"{k}_input_ids"]))
    plain, vis = model.prepare_inputs(sel, original_text=inp["text"])
    assert vis is True and torch.equal(plain["input_ids"][0], torch.from_numpy(g[f"{k}_input_ids"])[:n])


def test_forward_train_length_assertion():
    """:655 -- a tokenizer for which tokens(prompt + answer) != tokens(prompt) + tokens(answer) must trip the assertion
    instead of scoring misaligned labels"""
    from golden.inputs import e2e_inputs
    from toy_tokenizer import ToyTokenizer

    class Merging(ToyTokenizer):
        def encode(self, text, add_special_tokens=False):
            ids = super().encode(text)
            return ids[:-1] if text.endswith("\nZ") else ids      # "...assistant\n" + "Z" fuses into one token

    inp = e2e_inputs("a")
    model = _host_model()
    model.forward = lambda **kw: pytest.fail("forward must not be reached")
    tok = Merging()
    with pytest.raises(AssertionError):
        model.forward_train(tokenizer=tok, hist_qs=inp["hist_qs"], hist_as=inp["hist_as"],
                            current_question=inp["current_question"], all_timestamps=inp["timestamps"],
                            total_image_num=inp["T"], answer="Z", cor=[0], original_text=inp["text"])


def _stub_device_stages(model, monkeypatch, mask, n_visual):
    from cogstream_amd import chat
    monkeypatch.setattr(model, "encode_images", lambda *a, **k: torch.zeros(n_visual, 4))
    monkeypatch.setattr(model, "select_events_based_on_summary", lambda *a, **k: [])
    monkeypatch.setattr(model, "compress_unimportant_events", lambda mm, *a, **k: mm)
    monkeypatch.setattr(model, "_get_compression_mask", lambda *a, **k: mask)
    monkeypatch.setattr(chat.ops, "gather_rows", lambda a, b, idx, *r, **k: idx.to(torch.float32).reshape(-1, 1))
    model.llm = types.SimpleNamespace(packed=types.SimpleNamespace(embed=None))


@pytest.mark.parametrize("mode,tag", [("eager", "a"), ("eager", "c"), ("blockdiag", "a")])
def test_labels_are_compacted_with_the_ids(mode, tag, monkeypatch):
    """prepare_inputs_labels_for_multimodal(labels=): the labels go through the same text mask as the ids (:461-469);
    the reference's compression mask of the same clip (e2e.npz) gives the reference's compacted labels. labels=None
    still returns today's 2-tuple."""
    from golden.inputs import e2e_inputs
    g, e = _load("score_e2e.npz"), _load("e2e.npz")
    k = f"{mode}_{tag}"
    inp = e2e_inputs(tag)
    mask = torch.from_numpy(e[f"{tag}_mask"])
    ids = torch.from_numpy(g[f"{k}_input_ids"])[None]
    labels = torch.from_numpy(g[f"{k}_labels_in"])[None]
    assert int((ids == 258).sum()) == mask.numel()
    model = _host_model()
    _stub_device_stages(model, monkeypatch, mask, mask.numel())
    args = dict(input_ids=ids, attention_mask=torch.ones_like(ids), pixel_values=torch.zeros(1), grid_sizes=inp["grid_sizes"],
                merge_sizes=inp["merge_sizes"], modals=["video"], total_image_num=inp["T"], if_visual=True)
    got = model.prepare_inputs_labels_for_multimodal(labels=labels, **args)
    assert len(got) == 3
    emb, am, lab = got
    assert torch.equal(lab[0], torch.from_numpy(g[f"{k}_labels"]))
    assert lab.shape == am.shape == (1, emb.shape[1]) and emb.shape[1] == ids.shape[1] - int((~mask).sum())
    # the answer span survives untouched at the end
    n_ans = ids.shape[1] - int(g[f"{k}_prompt_tokens"])
    assert torch.equal(lab[0, -n_ans:], labels[0, -n_ans:])
    two = model.prepare_inputs_labels_for_multimodal(**args)
    assert len(two) == 2 and torch.equal(two[0], emb) and torch.equal(two[1], am)
    # without token compression the labels pass through
    plain = _host_model(use_token_compression=False)
    _stub_device_stages(plain, monkeypatch, mask, mask.numel())
    assert torch.equal(plain.prepare_inputs_labels_for_multimodal(labels=labels, **args)[2], labels)
    # text-only branch
    t3 = model.prepare_inputs_labels_for_multimodal(labels=labels, **dict(args, if_visual=False))
    assert len(t3) == 3 and torch.equal(t3[2], labels)
    assert len(model.prepare_inputs_labels_for_multimodal(**dict(args, if_visual=False))) == 2


def test_compress_visual_tokens_keeps_its_three_tuple():
    model = _host_model()
    ids = torch.tensor([1, 258, 258, 2, 258, 3])
    mask = torch.tensor([True, False, True])
    rows, new_ids, am = model._compress_visual_tokens(mask, ids, torch.ones(6, dtype=torch.long))
    assert rows.tolist() == [0, 2] and new_ids.tolist() == [1, 258, 2, 258, 3] and am.numel() == 5
    out = model._compress_visual_tokens(mask, ids, None, torch.tensor([-100, -100, -100, 7, -100, 9]))
    assert len(out) == 4 and out[3].tolist() == [-100, -100, 7, -100, 9]


def test_forward_semantics_with_a_stubbed_engine(monkeypatch):
    """CogReasoner.forward: labels shifted inside, -100 ignored, mean over the scored rows, nan without any, logits of
    the last num_logits_to_keep rows (0 = all) -- with an engine whose `score_hidden` returns known log-probabilities"""
    model = _host_model()
    S, V = 6, 8
    calls = {}

    class Eng:
        cfg = types.SimpleNamespace(vocab_size=V)

        def embed_tokens(self, ids):
            return torch.zeros(ids.numel(), 4)

        def forward(self, embeds, cache, **kw):
            assert kw == dict(want_hidden=True, want_logits=False) and cache is None
            return {"hidden": torch.arange(embeds.shape[0], dtype=torch.float32)[:, None].repeat(1, 4)}

        def score_hidden(self, hidden, targets):
            calls["targets"] = targets.clone()
            lp = torch.where(targets == -100, torch.zeros(S), -torch.arange(1, S + 1, dtype=torch.float32))
            return {"logprobs": lp, "lse": torch.zeros(S), "argmax": torch.zeros(S, dtype=torch.int64)}

        def logits(self, rows):
            return rows[:, :1].repeat(1, V)

    model.llm = Eng()
    ids = torch.arange(S)[None]
    labels = torch.tensor([[-100, -100, 5, -100, 6, 7]])
    out = model(input_ids=ids, labels=labels, num_logits_to_keep=2)
    assert calls["targets"].tolist() == [-100, 5, -100, 6, 7, -100]
    assert float(out.loss) == pytest.approx((2 + 4 + 5) / 3) and out.loss.dtype == torch.float32
    assert out.token_logprobs.tolist() == [[0, 0, -2, 0, -4, -5]]
    assert torch.equal(out.labels, labels) and out["loss"] is out.loss
    assert out.logits.shape == (1, 2, V) and out.logits[0, :, 0].tolist() == [4, 5]
    assert model.forward(input_ids=ids, labels=labels).logits.shape == (1, S, V)          # 0 = every row, as transformers
    none = model.forward(input_ids=ids, labels=torch.full((1, S), -100), num_logits_to_keep=1)
    assert torch.isnan(none.loss)
    assert model.forward(input_ids=ids, num_logits_to_keep=1).loss is None
    with pytest.raises(NotImplementedError):
        model.forward(input_ids=torch.zeros(2, 3, dtype=torch.long))


def test_result_records_gain_scores_only_with_the_flag(tmp_path, monkeypatch):
    """--score-answers adds answer_logprob / answer_ppl; without it the result JSON is byte-for-byte what it was"""
    import json as js
    import math
    from cogstream_amd import answer_generate as ag
    calls = []

    def fake_infer(conversation, model, processor, max_new_tokens=1024, score_answer=None, **kw):
        calls.append(score_answer)
        if score_answer is not None:
            return "pred", "[yes]", {"sum_logprob": -6.0, "mean_logprob": -2.0, "n_tokens": 3}
        return "pred", "[yes]"

    monkeypatch.setattr(ag, "infer", fake_infer)
    seg = [{"video": None, "timestamps": [0.0], "questions": ["q1", "q2"], "answers": ["a1", "a2"], "relevance": [[], [1]]}]
    base = ag.run_session(None, None, seg)
    want = [{"qa_id": 0, "question": "q1", "answer": "a1", "prediction": "pred", "predicted_coi": [], "predicted_visual": True, "coi": []},
            {"qa_id": 1, "question": "q2", "answer": "a2", "prediction": "pred", "predicted_coi": [0], "predicted_visual": True, "coi": [1]}]
    assert base == want and calls == [None, None]
    p1 = ag.save_to_json("clip", [base], str(tmp_path / "a"))
    p0 = ag.save_to_json("clip", [want], str(tmp_path / "b"))
    assert open(p1, "rb").read() == open(p0, "rb").read()
    scored = ag.run_session(None, None, seg, score_answers=True)
    assert calls[2:] == ["a1", "a2"]
    for rec, old in zip(scored, want):
        assert {k: v for k, v in rec.items() if k not in ("answer_logprob", "answer_ppl")} == old
        assert rec["answer_logprob"] == -6.0 and rec["answer_ppl"] == pytest.approx(math.exp(2.0))
    assert js.loads(js.dumps(scored)) == scored
    src = open(ag.__file__).read()      # the flag exists and is off by default
    assert '"--score-answers"' in src and 'dest="score_answers", action="store_true"' in src


def test_return_labels_stays_unimplemented():
    src = open(os.path.join(os.path.dirname(GOLD), "..", "cogstream_amd", "processing.py")).read()
    assert "return_labels" in src and "NotImplementedError" in src
