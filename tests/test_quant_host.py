"""CPU: the host side of the int8 frozen decoder (otter_amd/quant.py) -- the quantiser's definition, the module swap on the tiny MPT and
LLaMA hosts, forward parity with the fake-quantised model (weights overwritten by dequantize(quantize(W))), the error paths.  The fusion
modules' arithmetic comes from tests/_cpu_backend.py, as in tests/test_lora.py; the quantised linears run their documented CPU branch."""
import copy

import pytest
import torch

from oracle import synth
from otter_amd.configuration_otter import OtterConfig
from otter_amd.modeling_otter import OtterForConditionalGeneration
from otter_amd.quant import Int8FrozenLinear, dequantize_weight_int8, quantize_frozen_decoder, quantize_weight_int8
from tests._cpu_backend import oracle_backend


# ---- quantiser ------------------------------------------------------------------------------------------------------------------------

def _weight(n=48, k=64, seed=0):
    return torch.randn(n, k, generator=torch.Generator().manual_seed(seed)) * 0.05


def test_quantiser_range_error_bound_and_row_maximum():
    w = _weight()
    q, s = quantize_weight_int8(w)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and q.shape == w.shape and s.shape == (w.shape[0],)
    assert int(q.abs().max()) <= 127 and int(q.min()) >= -127
    err = (w.double() - q.double() * s.double()[:, None]).abs()
    assert bool((err <= s.double()[:, None] / 2).all())
    # the element of largest magnitude of every row maps to +-127
    idx = w.abs().argmax(dim=1)
    rows = torch.arange(w.shape[0])
    assert torch.equal(q[rows, idx].abs(), torch.full((w.shape[0],), 127, dtype=torch.int8))
    assert torch.equal(torch.sign(q[rows, idx].float()), torch.sign(w[rows, idx]))
    assert torch.equal(s, w.abs().amax(dim=1) / torch.full((w.shape[0],), 127.0))


def test_all_zero_row_gives_zero_and_unit_scale():
    w = _weight()
    w[5] = 0
    q, s = quantize_weight_int8(w)
    assert float(s[5]) == 1.0 and int(q[5].abs().max()) == 0
    assert torch.equal(dequantize_weight_int8(q, s)[5], torch.zeros(w.shape[1]))


def test_ties_round_to_even():
    # scale = 2^-7 exactly (amax = 127 / 128), W = scale * (j + 0.5): every quotient is an exact tie
    scale = 2.0 ** -7
    j = torch.arange(-126, 126, dtype=torch.float32)
    row = torch.cat([scale * (j + 0.5), torch.tensor([127 * scale])])
    q, s = quantize_weight_int8(row[None, :])
    assert float(s[0]) == scale
    want = torch.round(j + 0.5)                      # torch.round is round-half-even
    assert bool(((want % 2) == 0).all())             # ...so every tie lands on an even integer
    assert torch.equal(q[0, :-1].float(), want) and int(q[0, -1]) == 127


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_input_dtypes_of_the_same_values_agree(dtype):
    w = _weight(seed=3).to(dtype)                    # values representable in `dtype`
    q0, s0 = quantize_weight_int8(w.float())
    q1, s1 = quantize_weight_int8(w)
    assert torch.equal(q0, q1) and torch.equal(s0, s1)
    d = dequantize_weight_int8(q1, s1, dtype)
    assert d.dtype == dtype and torch.equal(d, (q1.float() * s1[:, None]).to(dtype))


# ---- module swap ------------------------------------------------------------------------------------------------------------------------

def _cfg(llama=False, lora=None):
    t = synth.TINY
    if llama:
        text_cfg = dict(architectures=["LlamaForCausalLM"], model_type="llama", hidden_size=64, intermediate_size=128, num_hidden_layers=4,
                        num_attention_heads=4, num_key_value_heads=4, vocab_size=t["vocab"], max_position_embeddings=64, rms_norm_eps=1e-6,
                        tie_word_embeddings=False, hidden_act="silu", _name_or_path="llama-tiny")
    else:
        text_cfg = dict(architectures=["MPTForCausalLM"], d_model=t["d_model"], n_heads=t["n_heads"], n_layers=t["n_layers"], expansion_ratio=4,
                        max_seq_len=t["max_seq_len"], vocab_size=t["vocab"], no_bias=True, attn_config=dict(alibi=True, attn_impl="torch"))
    vis_cfg = dict(hidden_size=1024, intermediate_size=t["clip_inter"], num_hidden_layers=1, num_attention_heads=16, image_size=28, patch_size=14,
                   hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=64)
    extra = dict(lora_config=dict(lora)) if lora else {}
    return OtterConfig(vision_config=vis_cfg, text_config=text_cfg, cross_attn_every_n_layers=2, **extra)


def _model(llama=False, lora=None, seed=0):
    torch.manual_seed(seed)
    model = OtterForConditionalGeneration(_cfg(llama, lora)).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():        # away from the initialiser's zeros (gates) and tiny spreads: every block contributes
            if "gate" in n and p.dim() <= 1:
                p.fill_(0.5)
    return model


MPT_NAMES = ("attn.Wqkv", "attn.out_proj", "ffn.up_proj", "ffn.down_proj")
LLAMA_NAMES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


@pytest.mark.parametrize("llama", [False, True])
def test_swap_replaces_exactly_the_frozen_decoder_linears(llama):
    model = _model(llama)
    names = LLAMA_NAMES if llama else MPT_NAMES
    layers = model.lang_encoder._get_decoder_layers()
    shapes = [tuple(getattr_path(l.decoder_layer, n).weight.shape) for l in layers for n in names]
    before_ids = {n: id(m) for n, m in model.named_modules() if not n.startswith("lang_encoder") or "gated_cross_attn_layer" in n}
    wte = model.get_input_embeddings()
    info = model.quantize_decoder_int8()
    assert info["replaced"] == len(layers) * len(names) == 4 * (7 if llama else 4)
    assert info["bytes_before"] == sum(4 * n * k for n, k in shapes)                   # fp32 masters, no biases in either tiny host
    assert info["bytes_after"] == sum(n * k + 4 * n for n, k in shapes)
    got = sorted(n for n, m in model.named_modules() if isinstance(m, Int8FrozenLinear))
    want = sorted("lang_encoder.%s.%d.decoder_layer.%s" % ("model.layers" if llama else "transformer.blocks", i, n)
                  for i in range(len(layers)) for n in names)
    assert got == want
    # CLIP, the perceiver and the gated cross-attention blocks are the same module objects; the embedding and lm_head keep their weights
    assert before_ids == {n: id(m) for n, m in model.named_modules() if n in before_ids}
    assert model.get_input_embeddings() is wte and isinstance(wte.weight, torch.nn.Parameter)
    if llama:
        assert isinstance(model.lang_encoder.lm_head, torch.nn.Linear) and not isinstance(model.lang_encoder.lm_head, Int8FrozenLinear)
    assert not model.training
    m0 = getattr_path(layers[0].decoder_layer, names[0])
    assert m0.qweight.dtype == torch.int8 and m0.scale.dtype == torch.float32 and "int8" in repr(m0)
    assert (m0.out_features, m0.in_features) == shapes[0]
    # a second call is a no-op
    again = model.quantize_decoder_int8()
    assert again == {"replaced": 0, "bytes_before": 0, "bytes_after": 0}


def getattr_path(obj, path):
    for part in path.split("."):
        obj = getattr(obj, part)
    return obj


def test_bias_bytes_are_counted_and_the_bias_is_kept():
    from otter_amd.mpt import MPTConfig, MPTForCausalLM

    torch.manual_seed(1)
    lm = MPTForCausalLM(MPTConfig(d_model=32, n_heads=2, n_layers=2, vocab_size=50, max_seq_len=32, no_bias=False,
                                  attn_config=dict(alibi=True, attn_impl="torch"))).eval().requires_grad_(False)
    with torch.no_grad():
        for p in lm.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    shapes = [(96, 32), (32, 32), (128, 32), (32, 128)]
    ref = copy.deepcopy(lm)
    info = quantize_frozen_decoder(lm)
    assert info["replaced"] == 8
    assert info["bytes_after"] == 2 * sum(n * k + 4 * n + 4 * n for n, k in shapes)
    assert info["bytes_before"] == 2 * sum(4 * n * k + 4 * n for n, k in shapes)
    assert torch.equal(lm.transformer.blocks[1].ffn.up_proj.bias, ref.transformer.blocks[1].ffn.up_proj.bias)
    _fake_quantise(ref)
    ids = torch.randint(0, 50, (2, 9), generator=torch.Generator().manual_seed(2))
    with torch.no_grad(), oracle_backend():
        a, b = lm(input_ids=ids).logits, ref(input_ids=ids).logits
    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


def test_lora_wrapped_and_trainable_layers_are_skipped():
    from otter_amd.lora import LoraLinear

    model = _model(lora=dict(r=4, lora_alpha=8, lora_dropout=0.0))
    layers = model.lang_encoder._get_decoder_layers()
    layers[3].decoder_layer.ffn.down_proj.weight.requires_grad_(True)
    info = model.quantize_decoder_int8()
    assert info["replaced"] == 4 * 3 - 1
    for i, l in enumerate(layers):
        assert isinstance(l.decoder_layer.attn.Wqkv, LoraLinear) and isinstance(l.decoder_layer.attn.out_proj, Int8FrozenLinear)
        assert isinstance(l.decoder_layer.ffn.down_proj, Int8FrozenLinear) == (i != 3)


# ---- forward parity with the fake-quantised model -----------------------------------------------------------------------------------------

def _fake_quantise(model):
    from otter_amd.lora import LoraLinear
    from otter_amd.mpt import FrozenAwareLinear

    lm = getattr(model, "lang_encoder", model)
    n = 0
    with torch.no_grad():
        for name, m in lm.named_modules():
            if (isinstance(m, FrozenAwareLinear) and not isinstance(m, LoraLinear) and "gated_cross_attn_layer" not in name
                    and not m.weight.requires_grad):
                m.weight.copy_(dequantize_weight_int8(*quantize_weight_int8(m.weight), m.weight.dtype))
                n += 1
    return n


def _batch(B=2, T=10):
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, 100, (B, T), generator=g)
    ids[:, 1] = synth.TINY["media_token_id"]
    return torch.randn(B, 1, 1, 3, 28, 28, generator=g), ids


@pytest.mark.parametrize("use_cache", [False, True])
@pytest.mark.parametrize("llama", [False, True])
def test_forward_parity_with_the_fake_quantised_model(llama, use_cache):
    model = _model(llama, seed=3)
    ref = copy.deepcopy(model)
    assert _fake_quantise(ref) == 4 * (7 if llama else 4)
    assert model.quantize_decoder_int8()["replaced"] == 4 * (7 if llama else 4)
    vx, ids = _batch()

    def run(m):
        with torch.no_grad(), oracle_backend():
            if not use_cache:
                return m(vision_x=vx, lang_x=ids).logits
            P = 6
            out = m(vision_x=vx, lang_x=ids[:, :P], use_cache=True, clear_conditioned_layers=False)
            past, steps = out.past_key_values, [out.logits]
            for t in range(P, ids.shape[1]):
                out = m(vision_x=None, lang_x=ids[:, t:t + 1], use_cached_vision_x=True, past_key_values=past, use_cache=True,
                        clear_conditioned_layers=False)
                past = out.past_key_values
                steps.append(out.logits)
            m.lang_encoder.clear_conditioned_layers()
            return torch.cat(steps, dim=1)

    a, b = run(model), run(ref)
    assert a.shape == b.shape == (2, 10, synth.TINY["vocab"])
    assert float(b.abs().max()) > 1e-3
    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())       # fp32 round-off: same numbers, the products in another order at most


# ---- error paths --------------------------------------------------------------------------------------------------------------------------

def test_from_linear_refuses_a_trainable_layer_and_forward_refuses_autograd():
    from otter_amd.mpt import FrozenAwareLinear

    lin = FrozenAwareLinear(32, 48, bias=True)
    with pytest.raises(ValueError, match="trainable"):
        Int8FrozenLinear.from_linear(lin)
    lin.requires_grad_(False)
    q = Int8FrozenLinear.from_linear(lin)
    assert (q.in_features, q.out_features) == (32, 48) and "in_features=32, out_features=48, bias=True" in q.extra_repr()
    assert sorted(k for k, _ in q.named_buffers()) == ["bias", "qweight", "scale"] and not list(q.parameters())
    x = torch.randn(3, 32)
    want = torch.nn.functional.linear(x, dequantize_weight_int8(q.qweight, q.scale), lin.bias)
    assert torch.allclose(q(x), want, rtol=0, atol=1e-6)
    assert torch.allclose(q(x, act="gelu"), torch.nn.functional.gelu(want), rtol=0, atol=1e-6)
    with pytest.raises(RuntimeError, match="inference-only"):
        q(x.clone().requires_grad_(True))
    with torch.no_grad():
        q(x.clone().requires_grad_(True))            # fine without autograd


def test_save_pretrained_of_a_quantised_model_raises(tmp_path):
    model = _model()
    model.save_pretrained(tmp_path / "before")       # an unquantised model saves as ever
    model.quantize_decoder_int8()
    with pytest.raises(RuntimeError, match="quantised in memory"):
        model.save_pretrained(tmp_path / "after")


def test_save_guard_sees_a_directly_quantised_decoder(tmp_path):
    model = _model()
    assert quantize_frozen_decoder(model.lang_encoder)["replaced"] == 16       # not through quantize_decoder_int8()
    with pytest.raises(RuntimeError, match="quantised in memory"):
        model.save_pretrained(tmp_path / "direct")


@pytest.mark.parametrize("cast", ["half", "bfloat16", "double"])
def test_dtype_casts_keep_the_scale_fp32(cast):
    from otter_amd.mpt import FrozenAwareLinear

    lin = FrozenAwareLinear(32, 48, bias=True).requires_grad_(False)
    q = Int8FrozenLinear.from_linear(lin)
    scale, qw = q.scale.clone(), q.qweight.clone()
    holder = torch.nn.Sequential(q)
    getattr(holder, cast)()                          # model.half() / .bfloat16() / .double() after quantising
    assert q.scale.dtype == torch.float32 and torch.equal(q.scale, scale)
    assert q.qweight.dtype == torch.int8 and torch.equal(q.qweight, qw)
    assert q.bias.dtype == getattr(torch, "float16" if cast == "half" else cast)   # the bias follows the cast like any buffer
    x = torch.randn(3, 32).to(q.bias.dtype)
    want = torch.nn.functional.linear(x, dequantize_weight_int8(qw, scale, x.dtype), q.bias)
    assert torch.equal(q(x), want)


def test_unquantised_model_never_touches_the_int8_path(monkeypatch):
    from otter_amd import ops

    def boom(*a, **k):
        raise AssertionError("the int8 path was reached by an unquantised model")

    monkeypatch.setattr(ops, "gemv_w8", boom)
    monkeypatch.setattr(ops, "dequant_w8", boom)
    model = _model()
    assert not any(isinstance(m, Int8FrozenLinear) for m in model.modules())
    vx, ids = _batch()
    with oracle_backend():
        for use_cache in (False, True):
            toks = model.generate(vision_x=vx, lang_x=ids[:, :8], max_new_tokens=4, use_cache=use_cache, eos_token_id=-1)
            assert toks.shape == (2, 12)
