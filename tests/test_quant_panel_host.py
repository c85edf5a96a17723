"""CPU: the `wide_steps` keyword of `quantize_decoder_int8` on the tiny MPT, LLaMA and Fuyu hosts.  It sets
`panel_rows = quant.PANEL_MAX_ROWS` on every Int8FrozenLinear of the model -- whichever call quantised it --, leaves the returned dict alone
and changes nothing a CPU tensor sees: the logits and greedy tokens of a 72-row cached step are equal with and without it (CPU tensors never
take a kernel).  What the attribute selects on the GPU is tests/test_gpu_w8_panel.py."""
import copy

import pytest
import torch

from tests.test_quant_gated_host import _backend, _model          # (the plain-torch gated block and masked cross-attention of that file)
from tests.test_quant_host import _batch

ROWS = 72                     # 24 sentences x 3 beams: one row past the rows kernel's 64


def _int8(model):
    from otter_amd.quant import Int8FrozenLinear

    return [m for m in model.modules() if isinstance(m, Int8FrozenLinear)]


@pytest.mark.parametrize("llama", [False, True])
def test_keyword_sets_the_attribute_on_every_quantised_linear_of_the_otter_hosts(llama):
    from otter_amd.quant import PANEL_MAX_ROWS, Int8FrozenLinear, Int8Unembedding

    assert Int8FrozenLinear.panel_rows == 0                                           # the default: a class attribute
    model, plain = _model(llama), _model(llama)
    n_dec, n_all = 4 * (7 if llama else 4), 4 * (7 if llama else 4) + 2 * 2 + 1       # decoder; + 2 gated blocks x 2 FFN linears + un-embedding
    want = plain.quantize_decoder_int8(gated_blocks=True, lm_head=True)
    assert want["replaced"] == n_all and all(m.panel_rows == 0 for m in _int8(plain))
    assert "panel_rows" not in plain.state_dict() and not any("panel_rows" in k for k in plain.state_dict())

    info = model.quantize_decoder_int8(gated_blocks=True, lm_head=True, wide_steps=True)
    assert info == want                                                               # the returned dict is unchanged
    lins = _int8(model)
    assert len(lins) == n_all and all(m.panel_rows == PANEL_MAX_ROWS for m in lins)
    assert sum(isinstance(m, Int8Unembedding) for m in lins) == 1

    # a later call switches it on for linears quantised by an earlier one, and for what it quantises itself
    later = _model(llama)
    assert later.quantize_decoder_int8()["replaced"] == n_dec
    assert all(m.panel_rows == 0 for m in _int8(later))
    more = later.quantize_decoder_int8(gated_blocks=True, wide_steps=True)
    assert more["replaced"] == 4 and len(_int8(later)) == n_dec + 4
    assert all(m.panel_rows == PANEL_MAX_ROWS for m in _int8(later))
    assert later.quantize_decoder_int8(wide_steps=True) == {"replaced": 0, "bytes_before": 0, "bytes_after": 0}


def test_keyword_on_the_fuyu_hosts():
    from otter_amd.quant import PANEL_MAX_ROWS
    from tests.test_fuyu_quant_host import _model as fuyu_model

    for on_fuyu in (True, False):
        fuyu, plain = fuyu_model(), fuyu_model()
        target, ptarget = (fuyu, plain) if on_fuyu else (fuyu.language_model, plain.language_model)
        want = ptarget.quantize_decoder_int8()
        assert all(m.panel_rows == 0 for m in _int8(plain))
        assert target.quantize_decoder_int8(lm_head=False)["replaced"] == want["replaced"] - 1
        info = target.quantize_decoder_int8(wide_steps=True)                          # the later call: lm_head, and the switch for all of them
        assert info["replaced"] == 1
        lins = _int8(fuyu)
        assert len(lins) == want["replaced"] and all(m.panel_rows == PANEL_MAX_ROWS for m in lins)


def _steps(model, vx, ids, P=6):
    with torch.no_grad(), _backend():
        out = model(vision_x=vx, lang_x=ids[:, :P], use_cache=True, clear_conditioned_layers=False)
        past, steps = out.past_key_values, []
        for t in range(P, ids.shape[1]):
            out = model(vision_x=None, lang_x=ids[:, t:t + 1], use_cached_vision_x=True, past_key_values=past, use_cache=True,
                        clear_conditioned_layers=False)
            past = out.past_key_values
            steps.append(out.logits)
        model.lang_encoder.clear_conditioned_layers()
    return torch.cat(steps, dim=1)


@pytest.mark.parametrize("llama", [False, True])
def test_cpu_logits_and_greedy_tokens_of_72_row_steps_do_not_depend_on_the_keyword(llama):
    base = _model(llama, seed=3)
    on, off = copy.deepcopy(base), copy.deepcopy(base)
    on.quantize_decoder_int8(gated_blocks=True, lm_head=True, wide_steps=True)
    off.quantize_decoder_int8(gated_blocks=True, lm_head=True)
    vx, ids = _batch(B=ROWS, T=8)
    a, b = _steps(on, vx, ids), _steps(off, vx, ids)
    assert a.shape == b.shape and a.shape[:2] == (ROWS, 2) and float(b.abs().max()) > 1e-3
    assert torch.equal(a, b)
    assert torch.equal(a.argmax(-1), b.argmax(-1))


def test_cpu_logits_and_greedy_tokens_of_72_row_fuyu_steps_do_not_depend_on_the_keyword():
    from oracle.gen_golden_fuyu import tiny_fuyu_batch
    from tests.test_fuyu_quant_host import P
    from tests.test_fuyu_quant_host import _model as fuyu_model

    on, off = fuyu_model(), fuyu_model()
    on.quantize_decoder_int8(wide_steps=True)
    off.quantize_decoder_int8()
    ids, patches, idx, _, _ = tiny_fuyu_batch()
    rep = ROWS // ids.shape[0]
    t = lambda a: torch.from_numpy(a).repeat((rep,) + (1,) * (a.ndim - 1))
    outs = []
    with torch.no_grad():
        for m in (on, off):
            out = m(input_ids=t(ids[:, :P]), image_patches=t(patches), image_patches_indices=t(idx[:, :P]), use_cache=True)
            past, logits = out.past_key_values, []
            for k in range(P, P + 2):
                out = m(input_ids=t(ids[:, k:k + 1]), past_key_values=past, use_cache=True)
                past = out.past_key_values
                logits.append(out.logits)
            outs.append(torch.cat(logits, dim=1))
    assert outs[0].shape[:2] == (ROWS, 2) and float(outs[1].abs().max()) > 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0].argmax(-1), outs[1].argmax(-1))
