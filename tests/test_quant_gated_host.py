"""CPU: the host side of `quantize_decoder_int8(gated_blocks=True, lm_head=True)` on the tiny MPT and LLaMA Otter hosts (otter_amd/quant.py:
quantize_gated_blocks, quantize_unembedding): what each keyword replaces and counts, that staged calls add up,
parity of logits and generated tokens with a fake-quantised twin across the cache modes of generate(), the last-position un-embedding of
the prompt pass, the error paths.

Int8FrozenLinear's CPU branch is F.linear on the dequantised weight, so a quantised model must reproduce a twin whose replaced weights hold
q * scale in fp32 -- within 1e-6 of the largest logit, the criterion of tests/test_fuyu_quant_host.py.  The twin's gated blocks run the
fused GatedCrossAttentionFn and the quantised ones the split path of OtterGatedCrossAttentionBlock._forward_int8_ffn; neither the fused
function nor OF.masked_cross_attention has a CPU form, so this file supplies one plain-torch masked cross-attention and builds both on it
(`_backend`, on top of tests/_cpu_backend.py): the two models then differ only in what the product's int8 path does.  MPT's table is tied:
the twin un-embeds with q * scale and keeps looking tokens up in the original table, as the product does."""
import contextlib
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import synth
from otter_amd import functional as OF
from otter_amd._capi import MASK_EQ, MASK_NONE
from tests._cpu_backend import oracle_backend
from tests.test_media_cache import _cfg

MEDIA = synth.TINY["media_token_id"]
P_LEN, STEPS, NEW = 6, 4, 4
KINDS = pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])


def _attention(x, media, tt, mode, heads, eps, nw, nb, Wq, Wkv, Wo):
    """to_out(masked cross-attention(LayerNorm(x), media)) in plain torch, with the semantics include/otter_hip.h gives otter_attn_fwd: masked
    scores take -FLT_MAX (a fully masked row comes out uniform), a row with text_time 0 is zeroed in EQ mode."""
    B, T, D = x.shape
    _, T_img, n, Dv = media.shape
    q = F.linear(F.layer_norm(x, (D,), nw, nb, eps), Wq)
    k, v = F.linear(media.reshape(B, T_img * n, Dv), Wkv).chunk(2, dim=-1)
    split = lambda t: t.reshape(B, t.shape[1], heads, 64).transpose(1, 2)
    sim = (split(q) * 64 ** -0.5) @ split(k).transpose(-1, -2)
    if mode != MASK_NONE:
        time = torch.arange(1, T_img + 1).repeat_interleave(n)
        ok = (tt[:, :, None] == time) if mode == MASK_EQ else (tt[:, :, None] >= time)
        sim = sim.masked_fill(~ok[:, None], -torch.finfo(sim.dtype).max)
    o = sim.softmax(dim=-1) @ split(v)
    if mode == MASK_EQ:
        o = o.masked_fill((tt == 0)[:, None, :, None], 0.0)
    return F.linear(o.transpose(1, 2).reshape(B, T, heads * 64), Wo)


class _GatedFn:
    """GatedCrossAttentionFn.forward as the product's launch sequence reads, on `_attention`."""

    @staticmethod
    def apply(x, media, tt, mode, heads, eps, nw, nb, Wq, Wkv, Wo, attn_gate, fw, fb, W1, W2, ff_gate, deferred=None):
        assert deferred is None
        x1 = (_attention(x, media, tt, mode, heads, eps, nw, nb, Wq, Wkv, Wo).float() * torch.tanh(attn_gate.float()) + x.float()).to(x.dtype)
        f = F.layer_norm(x1.float(), (x.shape[-1],), fw, fb, eps).to(x.dtype)
        return (F.linear(F.gelu(F.linear(f, W1)), W2).float() * torch.tanh(ff_gate.float()) + x1.float()).to(x.dtype)


@contextlib.contextmanager
def _backend():
    with oracle_backend():
        saved = OF.GatedCrossAttentionFn, OF.masked_cross_attention
        OF.GatedCrossAttentionFn, OF.masked_cross_attention = _GatedFn, _attention
        try:
            yield
        finally:
            OF.GatedCrossAttentionFn, OF.masked_cross_attention = saved


def _model(llama, seed=3):
    from otter_amd.modeling_otter import OtterForConditionalGeneration

    torch.manual_seed(seed + (8 if llama else 0))
    model = OtterForConditionalGeneration(_cfg(llama)).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():            # away from the initialiser's zeros (gates): every block contributes
            if "gate" in n and p.dim() <= 1:
                p.fill_(0.5)
    return model


def _blocks(model):
    return [l.gated_cross_attn_layer for l in model.lang_encoder._get_decoder_layers() if l.gated_cross_attn_layer is not None]


def _twin(model, qmodel):
    """A copy of the unquantised `model` holding the q * scale of every Int8FrozenLinear of `qmodel`."""
    from otter_amd.quant import Int8FrozenLinear, Int8Unembedding, dequantize_weight_int8

    twin = copy.deepcopy(model)
    mods, n = dict(twin.named_modules()), 0
    with torch.no_grad():
        for name, m in qmodel.named_modules():
            if not isinstance(m, Int8FrozenLinear):
                continue
            w = dequantize_weight_int8(m.qweight, m.scale, torch.float32)
            n += 1
            if isinstance(m, Int8Unembedding) and name.endswith("wte.unembed_int8"):
                wte = mods[name[:-len(".unembed_int8")]]
                wte.forward = lambda input, unembed=False, _w=w, _f=wte.forward: F.linear(input, _w.to(input.dtype)) if unembed else _f(input)
            else:
                mods[name].weight.copy_(w)
    return twin, n


_PAIRS = {}


def _pair(llama):
    """(quantised with both keywords, fake-quantised twin), built once per host; the tests that share them modify neither."""
    if llama not in _PAIRS:
        model = _model(llama)
        qmodel = copy.deepcopy(model)
        info = qmodel.quantize_decoder_int8(gated_blocks=True, lm_head=True)
        twin, n = _twin(model, qmodel)
        assert info["replaced"] == n == 4 * (7 if llama else 4) + 2 * 2 + 1
        _PAIRS[llama] = qmodel, twin
    return _PAIRS[llama]


def _batch(B=3, pads=(0, 2, 3), seed=5):
    g = torch.Generator().manual_seed(seed)
    T = P_LEN + STEPS
    ids = torch.randint(1, 100, (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    for r in range(B):
        mask[r, :pads[r]] = 0
        ids[r, pads[r]] = MEDIA
    return torch.randn(B, 1, 1, 3, 28, 28, generator=g), ids, mask


# ---- what is replaced -----------------------------------------------------------------------------------------------------------------------

def _int8_names(model):
    from otter_amd.quant import Int8FrozenLinear

    return sorted(n for n, m in model.named_modules() if isinstance(m, Int8FrozenLinear))


def _gated_names(model, llama):
    layers = "lang_encoder.%s" % ("model.layers" if llama else "transformer.blocks")
    return sorted("%s.%d.gated_cross_attn_layer.feed_forward.%d" % (layers, i, j)
                  for i, l in enumerate(model.lang_encoder._get_decoder_layers()) if l.gated_cross_attn_layer is not None for j in (1, 3))


def _unembed_name(llama):
    return "lang_encoder.lm_head" if llama else "lang_encoder.transformer.wte.unembed_int8"


@KINDS
def test_the_default_call_replaces_what_it_did_and_nothing_of_the_new_ground(llama):
    model = _model(llama)
    kinds = {n: type(m) for n, m in model.named_modules() if "gated_cross_attn_layer" in n or "decoder_layer" not in n}
    info = model.quantize_decoder_int8()
    assert info["replaced"] == 4 * (7 if llama else 4)
    names = _int8_names(model)
    assert len(names) == info["replaced"] and all(".decoder_layer." in n for n in names)
    assert kinds == {n: type(m) for n, m in model.named_modules() if n in kinds}          # gated blocks, embedding, lm_head, CLIP, perceiver
    assert all(type(b.feed_forward[i]) is nn.Linear for b in _blocks(model) for i in (1, 3))
    assert getattr(model.get_input_embeddings(), "unembed_int8", None) is None
    if llama:
        assert type(model.lang_encoder.lm_head) is nn.Linear


@KINDS
def test_keywords_replace_the_gated_ffns_and_the_unembedding_and_count_them(llama):
    from otter_amd.quant import Int8FrozenLinear, Int8Unembedding

    model = _model(llama)
    D, V = model.lang_encoder.get_input_embeddings().weight.shape[1], synth.TINY["vocab"]
    table = model.get_input_embeddings().weight
    blocks = _blocks(model)
    assert len(blocks) == 2 and all(b.feed_forward[1].weight.requires_grad for b in blocks)      # trainable, and quantised all the same
    kinds = {n: type(m) for n, m in model.named_modules()}
    base = model.quantize_decoder_int8()
    # staged: each later call replaces only what is still unquantised and counts only that
    gated = model.quantize_decoder_int8(gated_blocks=True)
    shapes = [(4 * D, D), (D, 4 * D)] * len(blocks)
    assert gated == {"replaced": 4, "bytes_before": sum(4 * n * k for n, k in shapes), "bytes_after": sum(n * k + 4 * n for n, k in shapes)}
    head = model.quantize_decoder_int8(gated_blocks=True, lm_head=True)
    assert head == {"replaced": 1, "bytes_before": 4 * V * D, "bytes_after": V * D + 4 * V}
    zero = {"replaced": 0, "bytes_before": 0, "bytes_after": 0}
    assert model.quantize_decoder_int8(gated_blocks=True, lm_head=True) == zero and model.quantize_decoder_int8() == zero
    # ... and add up to the one call with both keywords
    once = _model(llama).quantize_decoder_int8(gated_blocks=True, lm_head=True)
    assert once == {k: base[k] + gated[k] + head[k] for k in once}
    # module types: the FFN linears and the un-embedding, nothing else of the blocks
    want = sorted([n for n in _int8_names(model) if ".decoder_layer." in n] + _gated_names(model, llama) + [_unembed_name(llama)])
    assert _int8_names(model) == want and len(want) == base["replaced"] + 5
    mods = dict(model.named_modules())
    assert type(mods[_unembed_name(llama)]) is Int8Unembedding
    for b in blocks:
        assert type(b.feed_forward[1]) is Int8FrozenLinear and type(b.feed_forward[3]) is Int8FrozenLinear and b.ffn_is_int8()
        assert (b.feed_forward[1].out_features, b.feed_forward[1].in_features) == (4 * D, D) and b.feed_forward[1].bias is None
        assert type(b.attn.to_q) is type(b.attn.to_kv) is type(b.attn.to_out) is nn.Linear
        assert type(b.attn.norm) is type(b.feed_forward[0]) is nn.LayerNorm and type(b.feed_forward[2]) is nn.GELU
        assert isinstance(b.attn_gate, nn.Parameter) and isinstance(b.ff_gate, nn.Parameter)
    for n, m in model.named_modules():
        if n not in want and not n.endswith("unembed_int8"):
            assert type(m) is kinds[n], n
    # the lookup keeps its table: the same Parameter, the same values
    assert model.get_input_embeddings().weight is table and isinstance(table, nn.Parameter)
    assert not model.training


@KINDS
def test_lm_head_alone_leaves_the_gated_blocks(llama):
    model = _model(llama)
    info = model.quantize_decoder_int8(lm_head=True)
    assert info["replaced"] == 4 * (7 if llama else 4) + 1
    assert all(type(b.feed_forward[i]) is nn.Linear and not b.ffn_is_int8() for b in _blocks(model) for i in (1, 3))
    assert _unembed_name(llama) in _int8_names(model)


def test_replaced_weights_release_their_compute_dtype_copies():
    model = _model(False)
    w = _blocks(model)[0].feed_forward[3].weight
    OF.shadows._w[(id(w), torch.bfloat16)] = (0, w.detach().to(torch.bfloat16))          # what a bf16 forward would have left
    try:
        model.quantize_decoder_int8(gated_blocks=True)
        assert not [k for k in OF.shadows._w if k[0] == id(w)]
    finally:
        OF.shadows._w.pop((id(w), torch.bfloat16), None)


# ---- parity with the fake-quantised twin ------------------------------------------------------------------------------------------------------

CACHES = {
    "tuple": dict(),
    "static": dict(static=True),
    "static_media": dict(static=True, media=True),
    "tuple_media": dict(media=True),
    "static_int8kv_media": dict(static=True, media=True, kv_dtype="int8"),
}


def _logits(model, vx, ids, mask, static=False, media=False, kv_dtype=None):
    """Prompt pass + STEPS cached steps: every logit, [B, P_LEN + STEPS, V]."""
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache

    past = None
    if static:
        n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
        past = StaticKVCache(n_layers, ids.shape[0], n_kv, hd, ids.shape[1], "cpu", torch.float32, kv_dtype=kv_dtype)
    mkw = {"media_cache": MediaCache(ids.shape[0], model.media_token_id)} if media else {}
    out = model(vision_x=vx, lang_x=ids[:, :P_LEN], attention_mask=mask[:, :P_LEN], past_key_values=past, use_cache=True,
                clear_conditioned_layers=False, **mkw)
    logits = [out.logits]
    for t in range(P_LEN, P_LEN + STEPS):
        out = model(vision_x=None, lang_x=ids[:, t:t + 1], attention_mask=mask[:, :t + 1], use_cached_vision_x=True,
                    past_key_values=out.past_key_values, use_cache=True, clear_conditioned_layers=False, **mkw)
        logits.append(out.logits)
    model.lang_encoder.clear_conditioned_layers()
    return torch.cat(logits, dim=1)


@pytest.mark.parametrize("cache", list(CACHES))
@KINDS
def test_logits_of_the_prompt_pass_and_of_cached_steps_match_the_twin(llama, cache):
    qmodel, twin = _pair(llama)
    vx, ids, mask = _batch()
    with torch.no_grad(), _backend():
        a, b = _logits(qmodel, vx, ids, mask, **CACHES[cache]), _logits(twin, vx, ids, mask, **CACHES[cache])
    assert a.shape == b.shape == (3, P_LEN + STEPS, synth.TINY["vocab"])
    valid = mask.bool()
    top = float(b[valid].abs().max())
    assert top > 1e-3 and float((a - b)[valid].abs().max()) <= 1e-6 * top, (float((a - b)[valid].abs().max()), top)


@KINDS
def test_the_full_forward_without_a_cache_matches_the_twin(llama):
    qmodel, twin = _pair(llama)
    vx, ids, mask = _batch()
    with torch.no_grad(), _backend():
        a = qmodel(vision_x=vx, lang_x=ids, attention_mask=mask, use_cache=False).logits
        b = twin(vision_x=vx, lang_x=ids, attention_mask=mask, use_cache=False).logits
    valid = mask.bool()
    assert float((a - b)[valid].abs().max()) <= 1e-6 * float(b[valid].abs().max())


GEN_CACHES = {
    "reforward": dict(use_cache=False),
    "tuple": dict(use_cache=True),
    "static": dict(cache_implementation="static"),
    "static_media": dict(cache_implementation="static", cross_attention_cache=True),
    "static_int8kv_media": dict(cache_implementation="static", cross_attention_cache=True, kv_cache_dtype="int8"),
    "static_media_shared_prompt": dict(cache_implementation="static", cross_attention_cache=True, share_prompt=True),
}
MODES = dict(greedy=lambda: {}, beams=lambda: dict(num_beams=3),
             sampling=lambda: dict(do_sample=True, top_k=20, generator=torch.Generator().manual_seed(5)))


@pytest.mark.parametrize("cache", list(GEN_CACHES))
@KINDS
def test_generate_returns_the_twins_tokens(llama, cache):
    """Greedy, 3 beams and seeded sampling on a left-padded batch, in every cache mode (share_prompt needs beams)."""
    qmodel, twin = _pair(llama)
    vx, ids, mask = _batch()
    for mode, kw in MODES.items():
        if "share_prompt" in GEN_CACHES[cache] and mode != "beams":
            continue
        got = []
        for m in (qmodel, twin):
            with torch.no_grad(), _backend():
                got.append(m.generate(vision_x=vx, lang_x=ids[:, :P_LEN], attention_mask=mask[:, :P_LEN], max_new_tokens=NEW, eos_token_id=-1,
                                      **kw(), **GEN_CACHES[cache]))
        assert got[0].shape == (3, P_LEN + NEW) and torch.equal(got[0], got[1]), (mode, got[0].tolist(), got[1].tolist())
        assert not qmodel.lang_encoder.is_conditioned()


# ---- the un-embedding sees one position per row ---------------------------------------------------------------------------------------------------

@KINDS
def test_generate_unembeds_one_position_per_row(llama):
    qmodel, _ = _pair(llama)
    vx, ids, mask = _batch()
    head = dict(qmodel.named_modules())[_unembed_name(llama)]
    D = head.in_features
    seen = []
    h = head.register_forward_hook(lambda m, args, out: seen.append(tuple(args[0].shape)))
    kw = dict(vision_x=vx, lang_x=ids[:, :P_LEN], attention_mask=mask[:, :P_LEN], max_new_tokens=NEW, eos_token_id=-1)
    try:
        with torch.no_grad(), _backend():
            qmodel.generate(use_cache=True, **kw)
            assert seen == [(3, 1, D)] * NEW                                      # the prompt pass and every cached step: 3 rows each
            del seen[:]
            qmodel.generate(num_beams=3, cache_implementation="static", cross_attention_cache=True, **kw)
            assert seen == [(9, 1, D)] * NEW
            del seen[:]
            qmodel.generate(num_beams=3, cache_implementation="static", share_prompt=True, **kw)
            assert seen == [(3, 1, D)] + [(9, 1, D)] * (NEW - 1)                  # one prompt row per sentence
            del seen[:]
            qmodel.generate(use_cache=False, **kw)                                # the whole sequence is re-run, one position un-embedded
            assert seen == [(3, 1, D)] * NEW
            del seen[:]
            out = qmodel(vision_x=vx, lang_x=ids, attention_mask=mask)            # a plain forward still un-embeds every position
            assert seen == [(3, ids.shape[1], D)] and out.logits.shape == (3, ids.shape[1], synth.TINY["vocab"])
    finally:
        h.remove()


@KINDS
def test_the_private_keyword_slices_only_when_asked(llama):
    qmodel, twin = _pair(llama)
    vx, ids, mask = _batch()
    with torch.no_grad(), _backend():
        for m in (qmodel, twin):
            full = m(vision_x=vx, lang_x=ids, attention_mask=mask).logits
            last = m(vision_x=vx, lang_x=ids, attention_mask=mask, _last_position_only=True).logits
            # (one row through the product instead of ten: fp32 round-off in another order, within 1e-6 of the largest logit)
            assert last.shape == (3, 1, full.shape[-1])
            assert float((last - full[:, -1:]).abs().max()) <= 1e-6 * float(full.abs().max())


# ---- Int8FrozenLinear.forward_gated and Int8Unembedding on the CPU ---------------------------------------------------------------------------------

def test_forward_gated_on_the_cpu_is_the_plain_torch_expression():
    from otter_amd.quant import Int8FrozenLinear, dequantize_weight_int8, quantize_weight_int8

    g = torch.Generator().manual_seed(0)
    w, b, x, res = torch.randn(24, 32, generator=g), torch.randn(24, generator=g), torch.randn(3, 1, 32, generator=g), torch.randn(3, 1, 24, generator=g)
    q, s = quantize_weight_int8(w)
    lin, gate = Int8FrozenLinear(q, s, b), nn.Parameter(torch.tensor([0.7]))
    v = F.linear(x, dequantize_weight_int8(q, s), b)
    with torch.no_grad():
        assert torch.equal(lin.forward_gated(x, gate, res), v * torch.tanh(gate) + res)
        assert torch.equal(lin.forward_gated(x, None, res), v + res)
        assert torch.equal(lin.forward_gated(x, torch.zeros(1), res), res)          # an untrained block: the residual's bits
        assert lin.forward_gated(x, gate, res.to(torch.bfloat16)).dtype == torch.bfloat16
        with pytest.raises(ValueError, match="residual"):
            lin.forward_gated(x, gate, res[:2])
    with pytest.raises(RuntimeError, match="inference-only"):
        lin.forward_gated(x.clone().requires_grad_(True), gate, res)
    with pytest.raises(RuntimeError, match="inference-only"):
        lin.forward_gated(x, gate, res.clone().requires_grad_(True))
    lin.forward_gated(x, gate, res)                                                 # a trainable gate alone is no autograd through the weights


# ---- error paths --------------------------------------------------------------------------------------------------------------------------------

@KINDS
def test_a_training_forward_through_a_quantised_block_raises(llama):
    model = _model(llama)
    model.quantize_decoder_int8(gated_blocks=True)
    vx, ids, mask = _batch()
    assert any(p.requires_grad for p in _blocks(model)[0].attn.parameters())
    with _backend(), pytest.raises(RuntimeError, match="inference-only"):
        model(vision_x=vx, lang_x=ids, attention_mask=mask, labels=ids)
    with torch.no_grad(), _backend():
        model(vision_x=vx, lang_x=ids, attention_mask=mask)                         # the same forward without autograd is fine


@pytest.mark.parametrize("kw", [dict(gated_blocks=True), dict(lm_head=True)], ids=["gated_blocks", "lm_head"])
def test_save_pretrained_raises(kw, tmp_path):
    model = _model(False)
    model.quantize_decoder_int8(**kw)
    with pytest.raises(RuntimeError, match="quantised in memory"):
        model.save_pretrained(tmp_path / "after")
