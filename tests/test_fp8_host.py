"""Host side of decode_weights="fp8" (cogstream_amd/weights.py): the e4m3fn format, the row quantiser that is the
specification of the device one (csrc/gemv_fp8.hip), and the packing of the quantised model. No GPU."""
from __future__ import annotations

import math

import pytest
import torch


def _formula_table():
    """OCP e4m3fn from the bit fields, written independently of torch's cast: sign, 2^(e-7) (1 + m/8), subnormals
    m/8 * 2^-6, 0x7F / 0xFF NaN; no infinities, largest magnitude 448 (fnuz would have bias 8, one NaN at 0x80 and max 240)"""
    out = []
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = math.nan
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = 2.0 ** (e - 7) * (1.0 + m / 8.0)
        out.append(-v if s else v)
    return torch.tensor(out, dtype=torch.float64)


def _inputs():
    """(name, w [N, K] fp32): Gaussian rows, rows with one outlier, a zero row, rows whose absmax is exactly 2^k * 448"""
    g = torch.Generator().manual_seed(5)
    cases = [("gauss", torch.randn(64, 256, generator=g) * 0.02),
             ("gauss wide", torch.randn(16, 3584, generator=g) * 0.02)]
    w = torch.randn(32, 256, generator=g) * 0.02
    w[torch.arange(32), torch.randint(0, 256, (32,), generator=g)] = torch.randn(32, generator=g).sign() * (1.0 + torch.rand(32, generator=g) * 40)
    cases.append(("outlier", w))
    w = torch.randn(8, 64, generator=g) * 0.02
    w[3] = 0
    cases.append(("zero row", w))
    w = torch.randn(12, 128, generator=g) * 1e-3
    for i, k in enumerate(range(-14, -2)):
        w[i] = w[i].clamp(-2.0 ** k * 100, 2.0 ** k * 100)
        w[i, 7 * i] = 448.0 * 2.0 ** k * (-1 if i % 2 else 1)
    cases.append(("absmax = 2^k * 448", w))
    return cases


def test_decode_table_is_ocp_e4m3fn():
    from cogstream_amd.weights import FP8_MAX, dequantize_fp8_rows, fp8_decode_table
    ref = _formula_table()
    codes = torch.arange(256, dtype=torch.int16).to(torch.uint8).view(256, 1)
    got = dequantize_fp8_rows(codes, torch.ones(256)).double().view(-1)
    tab = fp8_decode_table().double()
    nan = torch.isnan(ref)
    assert nan.nonzero().view(-1).tolist() == [0x7F, 0xFF]
    for t in (got, tab):
        assert torch.equal(torch.isnan(t), nan)
        assert torch.equal(t[~nan], ref[~nan])
    assert float(ref[~nan].max()) == FP8_MAX == 448.0 and float(ref[0x7E]) == 448.0
    assert float(ref[0x80]) == 0.0 and math.copysign(1.0, float(got[0x80])) == -1.0       # 0x80 is -0, not NaN (fnuz)
    assert float(ref[0x01]) == 2.0 ** -9 and float(ref[0x08]) == 2.0 ** -6


@pytest.mark.parametrize("name,w", _inputs(), ids=[n for n, _ in _inputs()])
def test_quantiser_properties(name, w):
    from cogstream_amd.weights import dequantize_fp8_rows, quantize_fp8_rows
    codes, scale = quantize_fp8_rows(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    # a power of two: mantissa exactly 0.5
    m, _ = torch.frexp(scale)
    assert bool((m == 0.5).all())
    tab = _formula_table()
    mag = tab[(codes & 0x7F).long()]
    assert not bool(torch.isnan(mag).any())                                   # no 0x7F / 0xFF
    zero = w.abs().amax(1) == 0
    assert bool((scale[zero] == 1).all()) and bool((codes[zero] == 0).all())
    top = mag.amax(1)[~zero]
    assert bool((top >= 224).all()) and bool((top <= 448).all()), (float(top.min()), float(top.max()))
    if name.startswith("absmax"):
        assert bool((top == 448).all())                                       # exact at the powers of two, not one step up
        assert bool((scale == torch.tensor([2.0 ** k for k in range(-14, -2)])).all())
    # nearest representable: no finite code is closer to w / scale than the chosen one (ties are not exercised)
    finite = tab[~torch.isnan(tab)]
    x = (w.double() / scale.double()[:, None])
    val = tab[codes.long()]
    best = (x.reshape(-1, 1) - finite.view(1, -1)).abs().amin(1).view_as(x)
    assert bool(((x - val).abs() == best).all())
    d = dequantize_fp8_rows(codes, scale)
    assert torch.equal(d.double(), val * scale.double()[:, None])
    assert torch.equal(d.bfloat16().float(), d)                               # bf16-exact
    assert torch.equal(dequantize_fp8_rows(codes, scale, dtype=torch.bfloat16).float(), d)
    # a fixed point: quantising the dequantised matrix gives (codes, scale) back. One exception follows from the scale formula
    # itself and is pinned here too: a row whose largest code ROUNDED DOWN to exactly 224 = 448 / 2 has absmax' / 448 = scale / 2,
    # so the formula now picks scale / 2 and every value of the row takes the code of twice the magnitude -- the same values
    c2, s2 = quantize_fp8_rows(d)
    half = torch.zeros_like(zero)
    half[~zero] = top == 224
    assert torch.equal(s2, torch.where(half, scale / 2, scale))
    assert torch.equal(c2[~half], codes[~half])
    assert torch.equal(tab[c2[half].long()], 2 * tab[codes[half].long()])
    assert torch.equal(dequantize_fp8_rows(c2, s2), d)
    c3, s3 = quantize_fp8_rows(d.bfloat16())                                  # ... from the bf16 copy the engine holds as well
    assert torch.equal(s3, s2) and torch.equal(c3, c2)


def test_prototype_figures():
    """the figures the format was chosen on: 512 x 3584 rows of N(0, 0.02): relative RMS error of a few percent"""
    from cogstream_amd.weights import dequantize_fp8_rows, quantize_fp8_rows
    g = torch.Generator().manual_seed(0)
    w = torch.randn(512, 3584, generator=g) * 0.02
    d = dequantize_fp8_rows(*quantize_fp8_rows(w))
    rms = float(((d - w).double().pow(2).sum() / w.double().pow(2).sum()).sqrt())
    assert 2.0e-2 < rms < 3.2e-2, rms          # 3 mantissa bits: step 2^-3 relative, uniform error -> 2^-3 / sqrt(12) / ~1.4


def _small():
    from cogstream_amd.weights import LlmConfig, random_llm_state
    cfg = LlmConfig(hidden_size=128, intermediate_size=208, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                    vocab_size=96, image_token_index=90, eos_token_id=89)
    return cfg, random_llm_state(cfg, seed=3, std=0.05)


def _packed_reference(st, cfg, dtype):
    """the packing of include/cogs.h applied to per-tensor (codes, scale) pairs"""
    from cogstream_amd.weights import _perm_heads, quantize_fp8_rows
    hd, hq, hkv = cfg.head_dim, cfg.num_attention_heads, cfg.num_key_value_heads
    q = lambda k: quantize_fp8_rows(st[k].to(dtype))
    out = {"lm_head": q("lm_head.weight")}
    for i in range(cfg.num_hidden_layers):
        p = f"layers.{i}."
        a = p + "self_attn."
        (qc, qs), (kc, ks), (vc, vs) = q(a + "q_proj.weight"), q(a + "k_proj.weight"), q(a + "v_proj.weight")
        out[p + "qkv"] = (torch.cat([_perm_heads(qc, hq, hd), _perm_heads(kc, hkv, hd), vc], 0),
                          torch.cat([_perm_heads(qs, hq, hd), _perm_heads(ks, hkv, hd), vs], 0))
        out[p + "o"] = q(a + "o_proj.weight")
        (gc, gs), (uc, us) = q(p + "mlp.gate_proj.weight"), q(p + "mlp.up_proj.weight")
        out[p + "gu"] = (torch.stack([gc, uc], 1).reshape(2 * cfg.intermediate_size, -1), torch.stack([gs, us], 1).reshape(-1))
        out[p + "down"] = q(p + "mlp.down_proj.weight")
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_packed_codes_are_the_packing_of_the_per_tensor_codes(dtype):
    from cogstream_amd.weights import PackedLlm, fp8_model_state
    cfg, st = _small()
    before = {k: v.clone() for k, v in st.items()}
    pk = PackedLlm(st, cfg, dtype=dtype, device="cpu", decode_weights="fp8")
    assert all(torch.equal(st[k], before[k]) for k in st)                     # the caller's tensors are not dequantised in place
    ref = _packed_reference(st, cfg, dtype)
    assert sorted(pk.fp8_codes) == sorted(ref)
    for k, (c, s) in ref.items():
        assert torch.equal(pk.fp8_codes[k], c), k
        assert torch.equal(pk.fp8_scales[k], s), k
    H, I, qd = cfg.hidden_size, cfg.intermediate_size, (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim
    assert pk.fp8_bytes == cfg.vocab_size * H + cfg.num_hidden_layers * (qd * H + H * H + 2 * I * H + H * I)
    # ... and what the M > 1 kernels read is the plain packing of fp8_model_state
    plain = PackedLlm(fp8_model_state(st, dtype=dtype), cfg, dtype=dtype, device="cpu")
    assert plain.fp8_bytes == 0 and plain.fp8_struct is None
    assert len(pk.keep) == len(plain.keep) + 2 * len(ref)
    extra = {id(t) for t in list(pk.fp8_codes.values()) + list(pk.fp8_scales.values())}
    mine = [t for t in pk.keep if id(t) not in extra]
    assert len(mine) == len(plain.keep) and all(torch.equal(a, b) for a, b in zip(mine, plain.keep))
    assert pk.struct.layers == plain.struct.layers and pk.fp8_struct.layers == cfg.num_hidden_layers


def test_merged_lora_is_quantised_after_merging():
    from cogstream_amd.weights import PackedLlm, fp8_model_state, merge_lora, random_lora_state
    cfg, st = _small()
    lora = random_lora_state(cfg, seed=9)
    merged, _ = merge_lora(st, None, lora, cfg)
    pk = PackedLlm(merged, cfg, dtype=torch.bfloat16, device="cpu", decode_weights="fp8")
    ref = _packed_reference(merged, cfg, torch.bfloat16)
    base = _packed_reference(st, cfg, torch.bfloat16)
    assert all(torch.equal(pk.fp8_codes[k], ref[k][0]) and torch.equal(pk.fp8_scales[k], ref[k][1]) for k in ref)
    assert not torch.equal(ref["layers.0.qkv"][0], base["layers.0.qkv"][0])   # the adapter changes the codes
    fs = fp8_model_state(merged)
    assert torch.equal(fs["layers.0.input_layernorm.weight"], merged["layers.0.input_layernorm.weight"])
    assert torch.equal(fs["embed_tokens.weight"], merged["embed_tokens.weight"])
    assert not torch.equal(fs["layers.1.mlp.down_proj.weight"], merged["layers.1.mlp.down_proj.weight"])


def test_construction_rejects_rows_that_are_not_whole_16_byte_chunks():
    from cogstream_amd.weights import LlmConfig, PackedLlm, random_llm_state
    cfg = LlmConfig(hidden_size=128, intermediate_size=200, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                    vocab_size=32, image_token_index=30, eos_token_id=29)
    st = random_llm_state(cfg, seed=1)
    PackedLlm(st, cfg, dtype=torch.float32, device="cpu")                     # fine without the mode
    with pytest.raises(ValueError, match="K % 16"):
        PackedLlm(st, cfg, dtype=torch.float32, device="cpu", decode_weights="fp8")
    with pytest.raises(ValueError, match="decode_weights"):
        PackedLlm(st, cfg, dtype=torch.float32, device="cpu", decode_weights="int4")


def test_abi_revision_and_switches():
    from cogstream_amd import _lib as L
    assert b"0.4" in L.lib.cogs_version()
    assert L.debug_get("llm_decode_fp8") == 1 and L.debug_get("llm_last_decode_fp8") == 0
    for name in ("llm_decode_fp8", "gemv_fp8_load", "gemv_fp8_deep", "llm_last_decode_fp8"):
        assert name in L.debug_list()
    assert L.lib.cogs_debug_set(b"gemv_fp8_load", 12) == L.E_INVALID and L.lib.cogs_debug_set(b"gemv_fp8_deep", 2) == L.E_INVALID
    assert L.lib.cogs_debug_set(b"llm_last_decode_fp8", 1) == L.E_INVALID     # read only
