"""CPU: the host side of the int8 weight-only decoder on the OtterHD / Fuyu host (otter_amd/quant.py: quantize_persimmon_decoder,
otter_amd/fuyu.py: quantize_decoder_int8).  Int8FrozenLinear's CPU branch computes F.linear on the dequantised weight, so a quantised
model must reproduce an unquantised twin whose replaced weights hold dequantize(quantize(w)) in fp32 -- the identity and the bound
(atol 1e-6) of tests/test_quant_host.py.  Module swap, the squared-ReLU activation, the last-position un-embedding of generate() and the
error paths are all host logic and need no GPU; the kernels are checked in tests/test_gpu_fuyu_w8.py."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import synth
from oracle.gen_golden_fuyu import SEED, tiny_fuyu_batch, tiny_fuyu_config
from tests import _golden as G

REPLACED = ("query_key_value", "dense", "dense_h_to_4h", "dense_4h_to_h")
P = 14                      # prompt length of the generate() cases (tiny_fuyu_batch has 20 positions, patches at 1..7 / 2..6)


def _model():
    from otter_amd.fuyu import FuyuForCausalLM

    model = FuyuForCausalLM(tiny_fuyu_config())
    m = G.meta()["fuyu_tiny"]
    sd = synth.state_dict_for(SEED, {k: tuple(s) for k, s in m["shapes"].items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model


def _is_replaced(name, lm_head=True):
    return (".layers." in name and name.rsplit(".", 1)[-1] in REPLACED) or (lm_head and name.endswith("lm_head"))


def _twin(model):
    """An unquantised copy whose to-be-replaced weights hold dequantize(quantize(w)) in fp32."""
    from otter_amd.quant import dequantize_weight_int8, quantize_weight_int8

    twin = copy.deepcopy(model)
    n = 0
    with torch.no_grad():
        for name, mod in twin.named_modules():
            if isinstance(mod, nn.Linear) and _is_replaced(name):
                mod.weight.copy_(dequantize_weight_int8(*quantize_weight_int8(mod.weight)))
                n += 1
    assert n == 4 * twin.config.text_config.num_hidden_layers + 1
    return twin.eval()


@pytest.fixture(scope="module")
def pair():
    """(quantised model, fake-quantised twin), built once; neither is modified by the tests that share them."""
    model = _model()
    twin = _twin(model)
    info = model.quantize_decoder_int8()
    assert info["replaced"] == 4 * model.config.text_config.num_hidden_layers + 1
    return model, twin


def test_method_contract():
    from otter_amd.fuyu import FuyuForCausalLM, PersimmonForCausalLM
    from otter_amd.quant import Int8FrozenLinear

    L = tiny_fuyu_config().text_config.num_hidden_layers
    for lm_head in (True, False):
        for on_fuyu in (True, False):
            fuyu = _model().train()
            target = fuyu if on_fuyu else fuyu.language_model
            assert isinstance(target, FuyuForCausalLM if on_fuyu else PersimmonForCausalLM)
            kinds = {n: type(m) for n, m in fuyu.named_modules()}
            lins = [m for n, m in fuyu.named_modules() if isinstance(m, nn.Linear) and _is_replaced(n, lm_head)]
            assert all(m.weight.requires_grad for m in lins)                 # trainable, as C5 leaves them: quantised all the same
            want_before = sum(4 * m.weight.numel() + (4 * m.bias.numel() if m.bias is not None else 0) for m in lins)
            want_after = sum(m.weight.numel() + 4 * m.out_features + (4 * m.bias.numel() if m.bias is not None else 0) for m in lins)
            info = target.quantize_decoder_int8() if lm_head else target.quantize_decoder_int8(lm_head=False)
            assert info["replaced"] == 4 * L + (1 if lm_head else 0) == len(lins)
            assert info["bytes_before"] == want_before and info["bytes_after"] == want_after
            assert info["bytes_after"] < 0.56 * info["bytes_before"]
            assert not target.training and not any(m.training for m in target.modules())
            assert target.quantize_decoder_int8(lm_head=lm_head) == {"replaced": 0, "bytes_before": 0, "bytes_after": 0}
            for n, m in fuyu.named_modules():
                if _is_replaced(n, lm_head):
                    assert type(m) is Int8FrozenLinear and m.qweight.dtype == torch.int8 and m.scale.dtype == torch.float32, n
                else:
                    assert type(m) is kinds[n], n                             # LayerNorms, embed_tokens, vision_embed_tokens, ...
            lm = fuyu.language_model
            assert type(lm.model.embed_tokens) is nn.Embedding and type(fuyu.vision_embed_tokens) is nn.Linear
            assert type(lm.model.final_layernorm) is nn.LayerNorm
            for layer in lm.model.layers:
                for ln in (layer.input_layernorm, layer.post_attention_layernorm, layer.self_attn.q_layernorm, layer.self_attn.k_layernorm):
                    assert type(ln) is nn.LayerNorm
            assert (type(lm.lm_head) is nn.Linear) == (not lm_head)


def test_from_linear_still_refuses_trainable_layers():
    from otter_amd.quant import Int8FrozenLinear

    with pytest.raises(ValueError, match="trainable"):
        Int8FrozenLinear.from_linear(nn.Linear(16, 8))


def test_logits_match_the_fake_quantised_twin(pair):
    model, twin = pair
    ids, patches, idx, _, _ = tiny_fuyu_batch()
    t = torch.from_numpy
    with torch.no_grad():
        outs = []
        for m in (model, twin):
            out = m(input_ids=t(ids[:, :P]), image_patches=t(patches), image_patches_indices=t(idx[:, :P]), use_cache=True)
            past, logits = out.past_key_values, [out.logits]
            for k in range(P, P + 6):
                out = m(input_ids=t(ids[:, k:k + 1]), past_key_values=past, use_cache=True)
                past = out.past_key_values
                logits.append(out.logits)
            outs.append(logits)
    assert outs[0][0].shape == (ids.shape[0], P, 120)
    for a, b in zip(*outs):
        assert a.shape == b.shape and float(b.abs().max()) > 0
        assert torch.allclose(a, b, rtol=0, atol=1e-6), float((a - b).abs().max())


@pytest.mark.parametrize("mode", ["greedy", "beams", "sampling"])
def test_generate_returns_the_twins_tokens(pair, mode):
    model, twin = pair
    ids, patches, idx, _, _ = tiny_fuyu_batch()
    t = torch.from_numpy
    mask = torch.ones(2, P, dtype=torch.long)
    mask[1, :1] = 0                                    # one left-padded row (its first position holds no patch)
    assert idx[1, 0] == -1
    got = []
    for m in (model, twin):
        kw = dict(greedy={}, beams=dict(num_beams=3), sampling=dict(do_sample=True, top_k=20, generator=torch.Generator().manual_seed(5)))[mode]
        got.append(m.generate(input_ids=t(ids[:, :P]), image_patches=t(patches), image_patches_indices=t(idx[:, :P]), attention_mask=mask,
                              max_new_tokens=6, use_cache=True, eos_token_id=-1, **kw))
    assert got[0].shape == (2, P + 6) and torch.equal(got[0], got[1])


def test_relu2_activation_and_unknown_act():
    from otter_amd.quant import Int8FrozenLinear, dequantize_weight_int8, quantize_weight_int8

    g = torch.Generator().manual_seed(0)
    w, b, x = torch.randn(24, 32, generator=g), torch.randn(24, generator=g), torch.randn(3, 5, 32, generator=g)
    q, s = quantize_weight_int8(w)
    lin = Int8FrozenLinear(q, s, b)
    want = F.linear(x, dequantize_weight_int8(q, s), b)
    assert bool((want < 0).any()) and bool((want > 0).any())
    with torch.no_grad():
        assert torch.equal(lin(x, act="relu2"), torch.square(F.relu(want)))
        assert torch.equal(lin(x), want)
        assert torch.equal(lin(x, act="gelu"), F.gelu(want))
        for bad in ("relu", "silu", 3, ""):
            with pytest.raises(ValueError, match="act"):
                lin(x, act=bad)


def _hook_shapes(mod):
    seen = []
    h = mod.register_forward_hook(lambda m, args, out: seen.append(tuple(args[0].shape)))
    return seen, h


def test_last_position_unembedding(pair):
    model, twin = pair
    ids, patches, idx, _, _ = tiny_fuyu_batch()
    t = torch.from_numpy
    D, NEW = 128, 4
    kw = dict(input_ids=t(ids[:, :P]), image_patches=t(patches), image_patches_indices=t(idx[:, :P]), max_new_tokens=NEW, eos_token_id=-1)
    seen, h = _hook_shapes(model.language_model.lm_head)
    try:
        model.generate(use_cache=True, **kw)
        assert seen == [(2, 1, D)] * NEW                                      # the prompt pass and every cached step
        del seen[:]
        model.generate(use_cache=True, num_beams=3, **kw)
        assert seen == [(6, 1, D)] * NEW
        del seen[:]
        model.language_model.generate(t(ids[:, :6]), max_new_tokens=3, eos_token_id=-1)       # the text-only entry point
        assert seen == [(2, 1, D)] * 3
        del seen[:]
        model.generate(use_cache=False, **kw)                                 # without a cache the whole sequence is re-run, one row un-embedded
        assert seen == [(2, 1, D)] * NEW
        del seen[:]
        with torch.no_grad():
            out = model(input_ids=t(ids), image_patches=t(patches), image_patches_indices=t(idx))
        assert seen == [(2, ids.shape[1], D)] and out.logits.shape == (2, ids.shape[1], 120)
    finally:
        h.remove()
    # an unquantised model un-embeds every prompt position, as before.  (Its lm_head is applied through OF.trainable_linear, which reads
    # the module's weight without calling it: a forward hook never fires there, so the functional is watched instead.)
    from otter_amd import functional as OF

    real, calls = OF.trainable_linear, []

    def spy(mod, x):
        if mod is twin.language_model.lm_head:
            calls.append(tuple(x.shape))
        return real(mod, x)

    OF.trainable_linear = spy
    try:
        twin.generate(use_cache=True, **kw)
        with torch.no_grad():
            full = twin(input_ids=t(ids), image_patches=t(patches), image_patches_indices=t(idx))
    finally:
        OF.trainable_linear = real
    assert calls == [(2, P, D)] + [(2, 1, D)] * (NEW - 1) + [(2, ids.shape[1], D)]
    assert full.logits.shape == (2, ids.shape[1], 120)


def test_private_keyword_slices_only_when_asked(pair):
    model, twin = pair
    ids, patches, idx, _, _ = tiny_fuyu_batch()
    t = torch.from_numpy
    with torch.no_grad():
        for m in (model, twin):
            full = m(input_ids=t(ids), image_patches=t(patches), image_patches_indices=t(idx)).logits
            last = m(input_ids=t(ids), image_patches=t(patches), image_patches_indices=t(idx), _last_position_only=True).logits
            assert full.shape == (2, ids.shape[1], 120) and last.shape == (2, 1, 120)
            assert torch.allclose(last, full[:, -1:], rtol=0, atol=1e-6)


def test_errors(pair, tmp_path):
    model, _ = pair
    ids, patches, idx, mask, labels = tiny_fuyu_batch()
    t = torch.from_numpy
    with pytest.raises(RuntimeError, match="quantised in memory"):
        model.save_pretrained(str(tmp_path / "fuyu"))
    with pytest.raises(RuntimeError, match="quantised in memory"):
        model.language_model.save_pretrained(str(tmp_path / "persimmon"))
    assert not list(tmp_path.iterdir())
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="inference-only"):
            model(input_ids=t(ids), image_patches=t(patches), image_patches_indices=t(idx), attention_mask=t(mask), labels=t(labels))
        with pytest.raises(RuntimeError, match="inference-only"):
            model.language_model(input_ids=t(ids), labels=t(labels))
    kw = dict(input_ids=t(ids[:, :P]), image_patches=t(patches), image_patches_indices=t(idx[:, :P]), max_new_tokens=2)
    with pytest.raises(NotImplementedError, match="cache_implementation='static'"):
        model.generate(cache_implementation="static", **kw)
    with pytest.raises(NotImplementedError, match="graph_decode"):
        model.generate(graph_decode=True, **kw)
    with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
        model.generate(kv_cache_dtype="int8", **kw)
    with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
        model.language_model.generate(t(ids[:, :6]), max_new_tokens=2, kv_cache_dtype="int8")


def test_an_unquantised_model_never_loads_the_quant_module(monkeypatch):
    """fuyu.py recognises a quantised module through sys.modules, without importing otter_amd.quant itself."""
    import sys

    import otter_amd.quant  # noqa: F401  (so that monkeypatch has an entry to restore)

    model = _model().eval()
    ids, patches, idx, _, _ = tiny_fuyu_batch()
    t = torch.from_numpy
    monkeypatch.delitem(sys.modules, "otter_amd.quant")
    model.generate(input_ids=t(ids[:, :8]), image_patches=t(patches), image_patches_indices=t(idx[:, :8]), max_new_tokens=2, eos_token_id=-1)
    model.language_model.generate(t(ids[:, :6]), max_new_tokens=2, eos_token_id=-1)
    assert "otter_amd.quant" not in sys.modules
