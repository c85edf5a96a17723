"""CPU, fp32, tiny models: the host side of the cross-attention cache (otter_amd/media_cache.py) -- a cached step over a MediaCache against the
full re-forward (the legacy cached step ignores the image: SURVEY.md section 3.2), generate(cross_attention_cache=True) against
generate(use_cache=False), the running <image> count under beam reorders, the error paths.  The step's attention runs
MediaCache.attend_reference here (the documented CPU / fp32 branch); the fusion modules' arithmetic of every OTHER forward comes from
tests/_cpu_backend.py, as in tests/test_static_kv_cache.py (whose tiny-model helpers are restated here)."""
import contextlib

import pytest
import torch

from oracle import synth
from otter_amd._capi import MASK_EQ, MASK_GE
from otter_amd.configuration_otter import OtterConfig
from otter_amd.kv_cache import StaticKVCache, cache_geometry
from otter_amd.media_cache import MediaCache
from otter_amd.modeling_otter import OtterForConditionalGeneration, OtterGatedCrossAttentionBlock, OtterLayer
from tests._cpu_backend import oracle_backend

MEDIA = synth.TINY["media_token_id"]


def _cfg(llama):
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
    return OtterConfig(vision_config=vis_cfg, text_config=text_cfg, cross_attn_every_n_layers=2)


_MODELS = {}


def _model(llama):
    if llama not in _MODELS:
        torch.manual_seed(11 if llama else 3)
        model = OtterForConditionalGeneration(_cfg(llama)).eval()
        with torch.no_grad():
            for n, p in model.named_parameters():        # away from the initialiser's zeros (gates): every block contributes
                if "gate" in n and p.dim() <= 1:
                    p.fill_(0.5)
        _MODELS[llama] = model
    return _MODELS[llama]


@contextlib.contextmanager
def _attn_gates(model, value):
    gates = [p for n, p in model.named_parameters() if n.endswith("attn_gate")]
    assert gates
    saved = [p.detach().clone() for p in gates]
    with torch.no_grad():
        for p in gates:
            p.fill_(value)
    try:
        yield
    finally:
        with torch.no_grad():
            for p, s in zip(gates, saved):
                p.copy_(s)


P_LEN, STEPS = 6, 8


def _batch(B, pads, seed=5, t_img=1, late_image=None):
    """ids [B, P_LEN + STEPS] with <image> as the first real token of every row; t_img = 2: a second <image> two tokens later (still in
    the prompt); late_image = (row, step): one more <image> among the DECODED ids of that row."""
    g = torch.Generator().manual_seed(seed)
    T = P_LEN + STEPS
    ids = torch.randint(1, 100, (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    for r in range(B):
        n = pads[r] if pads is not None else 0
        mask[r, :n] = 0
        ids[r, n] = MEDIA
        if t_img == 2:
            ids[r, n + 2] = MEDIA
    if late_image is not None:
        ids[late_image[0], P_LEN + late_image[1]] = MEDIA
    return torch.randn(B, t_img, 1, 3, 28, 28, generator=g), ids, (mask if pads is not None else None)


def _cached_run(model, vx, ids, mask, static, media):
    """Teacher-forced prompt + STEPS cached steps; the logits of the last prompt position and of every step, [B, 1 + STEPS, V]."""
    past = None
    if static:
        n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
        past = StaticKVCache(n_layers, ids.shape[0], n_kv, hd, ids.shape[1], "cpu", torch.float32)
    mc = MediaCache(ids.shape[0], model.media_token_id) if media else None
    mkw = {"media_cache": mc} if media else {}
    am = (lambda t: None) if mask is None else (lambda t: mask[:, :t])
    out = model(vision_x=vx, lang_x=ids[:, :P_LEN], attention_mask=am(P_LEN), past_key_values=past, use_cache=True, clear_conditioned_layers=False,
                **mkw)
    logits = [out.logits[:, -1]]
    ptrs = None
    if media:
        assert mc.filled and mc.seen.dtype == torch.int32 and torch.equal(mc.seen.long(), (ids[:, :P_LEN] == MEDIA).sum(1))
        ptrs = mc.data_ptrs()
        assert len(ptrs) == sum(1 for l in model.lang_encoder._get_decoder_layers() if l.gated_cross_attn_layer is not None)
    for t in range(P_LEN, P_LEN + STEPS):
        out = model(vision_x=None, lang_x=ids[:, t:t + 1], attention_mask=am(t + 1), use_cached_vision_x=True, past_key_values=out.past_key_values,
                    use_cache=True, clear_conditioned_layers=False, **mkw)
        logits.append(out.logits[:, -1])
        if media:
            assert torch.equal(mc.seen.long(), (ids[:, :t + 1] == MEDIA).sum(1)) and mc.data_ptrs() == ptrs
            assert all(l.media_step is None for l in model.lang_encoder._get_decoder_layers())
    model.lang_encoder.clear_conditioned_layers()
    return torch.stack(logits, dim=1)


_FULL = {}


def _full_run_once(key, model, vx, ids, mask):
    """The re-forward reference of a case: computed once, shared by the tuple and the static variant, never modified."""
    if key not in _FULL:
        _FULL[key] = _full_run(model, vx, ids, mask)
    return _FULL[key]


def _full_run(model, vx, ids, mask):
    logits = []
    for t in range(P_LEN, P_LEN + STEPS + 1):
        out = model(vision_x=vx, lang_x=ids[:, :t], attention_mask=None if mask is None else mask[:, :t], use_cache=False)
        logits.append(out.logits[:, -1])
    return torch.stack(logits, dim=1)


# ---- step logits ----------------------------------------------------------------------------------------------------------------------

STEP_CASES = {
    "unpadded": dict(pads=None),
    "left_padded": dict(pads=(0, 2, 3)),
    "late_image_uniform_row": dict(pads=(0, 2, 3), late_image=(1, 3)),     # text_time 2 with T_img = 1: every key masked, the uniform row
    "t_img2_two_images": dict(pads=(0, 2, 3), t_img=2),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
@pytest.mark.parametrize("static", [False, True], ids=["tuple", "static"])
@pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
def test_media_cache_steps_match_the_full_reforward(llama, static, case):
    """Bound: err <= 2 s0, with s0 measured here on existing code paths only -- the legacy cached step against the full re-forward with every
    attn_gate at 0, where the attention branch contributes nothing and what remains is the decoder's own rounding between the two modes.
    The legacy cached run with the gates at 0.5 must miss that bound by more than 100x: it does not see the image after the prompt."""
    model = _model(llama)
    vx, ids, mask = _batch(3, **STEP_CASES[case])
    with torch.no_grad(), oracle_backend():
        with _attn_gates(model, 0.0):
            s0 = float((_cached_run(model, vx, ids, mask, static, media=False) - _full_run_once((llama, case, 0), model, vx, ids, mask)).abs().max())
        full = _full_run_once((llama, case, 1), model, vx, ids, mask)
        legacy = _cached_run(model, vx, ids, mask, static, media=False)
        got = _cached_run(model, vx, ids, mask, static, media=True)
    err, err_legacy = float((got - full).abs().max()), float((legacy - full).abs().max())
    print("[media-cache] %s %s %s: |media-cache step - re-forward| %.3e, s0 (gates 0) %.3e, ratio %.2f; legacy cached %.3e; max |logit| %.3e" % (
        "llama" if llama else "mpt", "static" if static else "tuple", case, err, s0, err / s0, err_legacy, float(full.abs().max())))
    assert s0 > 0
    assert torch.equal(got[:, 0], legacy[:, 0])                    # the prompt pass is the ordinary forward
    assert err <= 2 * s0, (err, s0)
    assert err_legacy > 100 * 2 * s0, (err_legacy, s0)


# ---- generate -------------------------------------------------------------------------------------------------------------------------

GEN_CASES = {
    "greedy": dict(),
    "beams3_ngram3": dict(num_beams=3, no_repeat_ngram_size=3),
    "group_beams": dict(num_beams=4, num_beam_groups=2, diversity_penalty=0.5),
    "sample": dict(do_sample=True, top_k=20, temperature=0.9),
}
NEW = 8
NEAR_TIE = 1e-4
GEN_SEED = 21


def _generate(model, vx, lx, mask, kw, **cache_kw):
    """Tokens, and the smallest top-2 logit margin of every decoder call (the prompt pass and each step)."""
    margins = []

    def hook(_m, _a, _k, out):
        top2 = out.logits[:, -1].float().topk(2, dim=-1).values
        margins.append(float((top2[:, 0] - top2[:, 1]).min()))

    kw = dict(kw)
    if kw.get("do_sample"):
        kw["generator"] = torch.Generator().manual_seed(1234)
    h = model.lang_encoder.register_forward_hook(hook, with_kwargs=True)
    try:
        with torch.no_grad(), oracle_backend():
            toks = model.generate(vision_x=vx, lang_x=lx, attention_mask=mask, max_new_tokens=NEW, eos_token_id=-1, **kw, **cache_kw)
    finally:
        h.remove()
    return toks, margins


@pytest.mark.parametrize("case", list(GEN_CASES))
@pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
def test_generate_with_the_media_cache_returns_the_reforward_tokens(llama, case):
    """Tokens are compared up to the first decoder call at which the re-forward path's top-2 margin falls below 1e-4; the seed is chosen so
    that no such call occurs (checked here: no case may be cut short), so the whole output is compared."""
    model = _model(llama)
    vx, ids, mask = _batch(2, (0, 2), seed=GEN_SEED)
    lx, mask = ids[:, :P_LEN], mask[:, :P_LEN]
    want, margins = _generate(model, vx, lx, mask, GEN_CASES[case], use_cache=False)
    print("[media-cache] generate %s %s: smallest re-forward top-2 margin %.3e over %d decoder calls" % (
        "llama" if llama else "mpt", case, min(margins), len(margins)))
    cut = next((i for i, m in enumerate(margins) if m < NEAR_TIE), None)
    assert cut is None, "a near-tie at decoder call %d (margin %.3e): choose another seed" % (cut, margins[cut])
    assert want.shape == (2, P_LEN + NEW) and torch.equal(want[:, :P_LEN], lx)
    for cache_kw in (dict(use_cache=True), dict(cache_implementation="static"), dict(use_cache=True, cache_implementation="dynamic")):
        got, _ = _generate(model, vx, lx, mask, GEN_CASES[case], cross_attention_cache=True, **cache_kw)
        assert torch.equal(got, want), (cache_kw, got.tolist(), want.tolist())
    assert not model.lang_encoder.is_conditioned()


@pytest.mark.parametrize("llama,case", [(True, "greedy"), (False, "beams3_ngram3")], ids=["llama-greedy", "mpt-beams3_ngram3"])
def test_legacy_cached_generate_returns_other_tokens(llama, case):
    """What the feature is for: without the media cache the cached path decodes other tokens than use_cache=False, and stays as it is."""
    model = _model(llama)
    vx, ids, mask = _batch(2, (0, 2), seed=GEN_SEED)
    lx, mask = ids[:, :P_LEN], mask[:, :P_LEN]
    want, _ = _generate(model, vx, lx, mask, GEN_CASES[case], use_cache=False)
    legacy, _ = _generate(model, vx, lx, mask, GEN_CASES[case], use_cache=True)
    off, _ = _generate(model, vx, lx, mask, GEN_CASES[case], use_cache=True, cross_attention_cache=False)
    assert not torch.equal(legacy, want)
    assert torch.equal(off, legacy)


def test_generate_with_the_media_cache_leaves_the_model_unconditioned_and_reusable():
    model = _model(False)
    vx, ids, _ = _batch(2, None, seed=GEN_SEED)
    kw = dict(cache_implementation="static", cross_attention_cache=True)
    a, _ = _generate(model, vx, ids[:, :P_LEN], None, dict(num_beams=3), **kw)
    layers = model.lang_encoder._get_decoder_layers()
    assert not model.lang_encoder.is_conditioned() and all(l.media_step is None and l.media_locations is None for l in layers)
    b, _ = _generate(model, vx, ids[:, :P_LEN], None, dict(num_beams=3), **kw)
    assert torch.equal(a, b)
    legacy1, _ = _generate(model, vx, ids[:, :P_LEN], None, dict(num_beams=3), use_cache=True)      # and the legacy path after it is the legacy path
    legacy2, _ = _generate(model, vx, ids[:, :P_LEN], None, dict(num_beams=3), cache_implementation="static")
    assert torch.equal(legacy1, legacy2)


# ---- seen / reorder / attend_reference ------------------------------------------------------------------------------------------------

def _standalone_cache(rows, rpm, t_img, n, heads, immediate, seed, dtype=torch.float32):
    """A MediaCache filled from two stand-alone OtterLayers (one gated, one not), no decoder."""
    g = torch.Generator().manual_seed(seed)
    block = OtterGatedCrossAttentionBlock(dim=16, dim_visual=8, heads=heads, only_attend_immediate_media=immediate).to(dtype)
    with torch.no_grad():
        block.attn.to_kv.weight.copy_(torch.randn(block.attn.to_kv.weight.shape, generator=g))
    layers = [OtterLayer(None, torch.nn.Identity()), OtterLayer(block, torch.nn.Identity())]
    vis = torch.randn(rows // rpm, t_img, n, 8, generator=g).to(dtype).repeat_interleave(rpm, dim=0)
    for l in layers:
        l.condition_vis_x(vis)
    cache = MediaCache(rows, MEDIA, rows_per_media=rpm)
    prompt = torch.randint(1, 100, (rows, 5), generator=g)
    prompt[:, 1] = MEDIA
    with torch.no_grad():
        cache.check_step(rows, 5)
        cache.fill(prompt == MEDIA, layers)
    return cache, prompt, vis, block, g


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seen_equals_a_recount_on_the_physically_reordered_rows(seed):
    rows, rpm = 6, 3
    cache, toks, _, _, g = _standalone_cache(rows, rpm, 2, 3, 1, True, seed)
    assert cache.kv[0] is None and cache.kv[1].shape == (rows // rpm, 6, 2 * 64) and (cache.T_img, cache.n, cache.heads, cache.mask_mode) == (2, 3, 1, MASK_EQ)
    ptrs = cache.data_ptrs()
    for step in range(20):
        if step % 5 != 4:                              # (some steps without a reorder: greedy rows in between)
            beam_idx = torch.cat([s * rpm + torch.randint(0, rpm, (rpm,), generator=g) for s in range(rows // rpm)])   # within the sentence
            cache.reorder(beam_idx)
            toks = toks[beam_idx]
        new = torch.where(torch.rand(rows, generator=g) < 0.3, torch.full((rows,), MEDIA), torch.randint(1, 100, (rows,), generator=g))
        with torch.no_grad():
            cache.check_step(rows, 1)
        tt = cache.advance(new.view(rows, 1))
        toks = torch.cat([toks, new.view(rows, 1)], dim=1)
        assert tt is cache.seen and cache.seen.dtype == torch.int32 and cache.seen.shape == (rows,)
        assert torch.equal(cache.seen.long(), (toks == MEDIA).sum(1)), step
        assert cache.data_ptrs() == ptrs
    assert int(cache.seen.max()) > 2                    # counts beyond T_img occurred


@pytest.mark.parametrize("immediate", [True, False], ids=["EQ", "GE"])
def test_attend_reference_is_the_masked_attention_of_the_reference(immediate):
    """Against an independent fp64 evaluation with the reference's masked_fill(-finfo.max): text_time 0 (zeroed in EQ, uniform in GE),
    1..T_img, T_img + 1 and 1000 (every key masked in EQ: uniform over all keys; everything admitted in GE)."""
    rows, rpm, t_img, n, H = 6, 3, 2, 5, 2
    cache, _, vis, block, g = _standalone_cache(rows, rpm, t_img, n, H, immediate, 7, torch.float64)
    assert cache.mask_mode == (MASK_EQ if immediate else MASK_GE)
    q = torch.randn(rows, H * 64, generator=g, dtype=torch.float64)
    tt = torch.tensor([0, 1, 2, 3, 1000, 2], dtype=torch.int32)
    o = cache.attend_reference(1, q, text_time=tt)
    kv = torch.nn.functional.linear(vis.reshape(rows, t_img * n, 8), block.attn.to_kv.weight.detach())       # per ROW here, per sentence there
    k, v = kv[..., :H * 64].view(rows, -1, H, 64), kv[..., H * 64:].view(rows, -1, H, 64)
    sim = torch.einsum("nhd,nmhd->nhm", q.view(rows, H, 64) * 64 ** -0.5, k)
    media_time = torch.arange(t_img * n) // n + 1
    ok = (tt.view(-1, 1) == media_time) if immediate else (tt.view(-1, 1) >= media_time)
    sim = sim.masked_fill(~ok[:, None, :], -torch.finfo(torch.float64).max)
    attn = (sim - sim.amax(-1, keepdim=True)).softmax(-1)
    if immediate:
        attn = attn.masked_fill((tt == 0).view(-1, 1, 1), 0.0)
    want = torch.einsum("nhm,nmhd->nhd", attn, v).reshape(rows, H * 64)
    assert float((o - want).abs().max()) < 1e-12
    if immediate:
        assert float(o[0].abs().max()) == 0.0
        assert float((o[3] - v[3].mean(0).reshape(-1)).abs().max()) < 1e-12       # T_img + 1: the uniform row is the mean of V


# ---- errors ---------------------------------------------------------------------------------------------------------------------------

def test_generate_rejects_a_media_cache_without_a_kv_cache():
    model = _model(False)
    vx, ids, _ = _batch(1, None)
    with pytest.raises(ValueError, match="cross_attention_cache"):
        model.generate(vision_x=vx, lang_x=ids[:, :P_LEN], max_new_tokens=2, use_cache=False, cross_attention_cache=True)
    assert not model.lang_encoder.is_conditioned()


@pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
def test_hosts_reject_what_a_media_cache_cannot_do(llama):
    model = _model(llama)
    vx, ids, _ = _batch(2, None)
    cache = MediaCache(2, model.media_token_id)
    step = dict(vision_x=None, use_cached_vision_x=True, use_cache=True, clear_conditioned_layers=False, media_cache=cache)
    with oracle_backend():
        with pytest.raises(RuntimeError, match="no_grad"):       # under autograd
            model(vision_x=vx, lang_x=ids[:, :P_LEN], use_cache=True, media_cache=cache)
        model.lang_encoder.clear_conditioned_layers()
        with torch.no_grad():
            model.lang_encoder.use_media_placement_augmentation = True
            try:
                with pytest.raises(ValueError, match="use_media_placement_augmentation"):
                    model(vision_x=vx, lang_x=ids[:, :P_LEN], use_cache=True, media_cache=cache)
            finally:
                model.lang_encoder.use_media_placement_augmentation = False
                model.lang_encoder.clear_conditioned_layers()
            assert not cache.filled
            out = model(vision_x=vx, lang_x=ids[:, :P_LEN], use_cache=True, clear_conditioned_layers=False, media_cache=cache)
            assert cache.filled
            with pytest.raises(ValueError, match="one-token step"):  # S > 1 over a filled cache
                model(lang_x=ids[:, P_LEN:P_LEN + 2], past_key_values=out.past_key_values, **step)
            with pytest.raises(ValueError, match="rows"):
                model(lang_x=ids[:1, P_LEN:P_LEN + 1], past_key_values=out.past_key_values, **step)
            assert all(l.media_step is None for l in model.lang_encoder._get_decoder_layers())
        model.lang_encoder.clear_conditioned_layers()
    with pytest.raises(ValueError, match="multiple of rows_per_media"):
        MediaCache(4, MEDIA, rows_per_media=3)
