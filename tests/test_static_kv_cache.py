"""CPU, fp32, tiny models: the host side of the static KV cache (otter_amd/kv_cache.py) -- the beam table against a physically reordered legacy
cache, both decoder hosts' static path against their legacy cached path, generate(cache_implementation="static") against
generate(use_cache=True), the error paths.  The cached step runs StaticKVCache.attend_reference here (the documented CPU / fp32 branch); the
fusion modules' arithmetic comes from tests/_cpu_backend.py, as in tests/test_quant_host.py."""
import pytest
import torch

from oracle import synth
from otter_amd.configuration_otter import OtterConfig
from otter_amd.kv_cache import StaticKVCache
from otter_amd.modeling_otter import OtterForConditionalGeneration
from tests._cpu_backend import oracle_backend


# ---- table semantics ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_table_equals_a_physically_reordered_legacy_cache(seed):
    g = torch.Generator().manual_seed(seed)
    L, N, H, d, S0, STEPS = 2, 6, 2, 8, 3, 20
    cache = StaticKVCache(L, N, H, d, S0 + STEPS + 2, "cpu", torch.float32)
    ptrs = cache.data_ptrs()
    legacy = []
    for i in range(L):
        k, v = torch.randn(N, H, S0, d, generator=g), torch.randn(N, H, S0, d, generator=g)
        cache.fill(i, k.transpose(1, 2).contiguous().transpose(1, 2), v)      # a strided view, as the prefill hands over
        legacy.append((k.transpose(2, 3), v))                                # MPT layout: k [N,H,d,S], v [N,H,S,d]
    cache.length = S0
    assert cache.src is None and cache.get_seq_length() == S0
    own = torch.arange(N, dtype=torch.int32).view(-1, 1)
    for step in range(STEPS):
        if step % 5 != 4:                              # (some steps without a reorder: greedy rows in between)
            beam_idx = torch.randint(0, N, (N,), generator=g)
            cache.reorder(beam_idx)
            legacy = [tuple(t.index_select(0, beam_idx) for t in layer) for layer in legacy]
        new = []
        for i in range(L):
            q, k, v = (torch.randn(N, H, d, generator=g) for _ in range(3))
            cache.attend_reference(i, q, k, v, 0.3)
            new.append((torch.cat([legacy[i][0], k.unsqueeze(-1)], dim=3), torch.cat([legacy[i][1], v.unsqueeze(2)], dim=2)))
        legacy = new
        cache.length += 1
        got = cache.to_legacy("mpt")
        for i in range(L):
            assert got[i][0].shape == legacy[i][0].shape and torch.equal(got[i][0], legacy[i][0]), (step, i)
            assert got[i][1].shape == legacy[i][1].shape and torch.equal(got[i][1], legacy[i][1]), (step, i)
        got = cache.to_legacy("llama")
        assert all(torch.equal(got[i][0], legacy[i][0].transpose(2, 3)) and torch.equal(got[i][1], legacy[i][1]) for i in range(L))
        assert cache.src.dtype == torch.int32 and torch.equal(cache.src[:, cache.length:], own.expand(-1, cache.max_len - cache.length))
        assert cache.data_ptrs() == ptrs
    assert cache.get_seq_length() == S0 + STEPS


def test_greedy_never_creates_the_table():
    cache = StaticKVCache(1, 2, 2, 4, 8, "cpu", torch.float32)
    cache.fill(0, torch.randn(2, 2, 3, 4), torch.randn(2, 2, 3, 4))
    cache.length = 3
    for _ in range(3):
        cache.attend_reference(0, torch.randn(2, 2, 4), torch.randn(2, 2, 4), torch.randn(2, 2, 4), 0.5)
        cache.length += 1
    assert cache.src is None and cache.to_legacy("llama")[0][0].shape == (2, 2, 6, 4)


def test_attend_reference_is_plain_attention_with_alibi_rotary_and_mask():
    """Against an independent fp64 evaluation on the gathered legacy tensors; a fully masked row gives 0."""
    from otter_amd.kv_cache import rotate_half

    g = torch.Generator().manual_seed(7)
    N, H, d, S0 = 4, 2, 8, 5
    cache = StaticKVCache(1, N, H, d, 16, "cpu", torch.float64)
    cache.fill(0, torch.randn(N, H, S0, d, generator=g, dtype=torch.float64), torch.randn(N, H, S0, d, generator=g, dtype=torch.float64))
    cache.length = S0
    cache.reorder(torch.tensor([1, 1, 3, 0]))
    past = cache.to_legacy("llama")[0]
    q, k, v = (torch.randn(N, H, d, generator=g, dtype=torch.float64) for _ in range(3))
    cos, sin = torch.rand(d, generator=g), torch.rand(d, generator=g)
    slopes = torch.tensor([0.5, 0.25])
    valid = torch.ones(N, S0 + 1, dtype=torch.uint8)
    valid[0, :2] = 0
    valid[2] = 0
    o = cache.attend_reference(0, q, k, v, 0.35, cos=cos, sin=sin, key_valid=valid, slopes=slopes)
    c, s = cos.double(), sin.double()
    qr, kr = q * c + rotate_half(q) * s, k * c + rotate_half(k) * s
    K, V = torch.cat([past[0], kr[:, :, None]], dim=2), torch.cat([past[1], v[:, :, None]], dim=2)
    sc = torch.einsum("nhd,nhjd->nhj", qr, K) * 0.35 + slopes.double().view(1, H, 1) * torch.arange(-S0, 1, dtype=torch.float64)
    sc = sc.masked_fill(valid[:, None, :] == 0, float("-inf"))
    want = torch.einsum("nhj,nhjd->nhd", torch.softmax(sc[[0, 1, 3]], -1), V[[0, 1, 3]])
    assert float((o.view(N, H, d)[[0, 1, 3]] - want).abs().max()) < 1e-12
    assert float(o[2].abs().max()) == 0.0
    assert torch.equal(cache.k[0, :, :, S0], kr) and torch.equal(cache.v[0, :, :, S0], v)


# ---- hosts ----------------------------------------------------------------------------------------------------------------------------

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
            for n, p in model.named_parameters():        # away from the initialiser's zeros (gates) and tiny spreads: every block contributes
                if "gate" in n and p.dim() <= 1:
                    p.fill_(0.5)
        _MODELS[llama] = model
    return _MODELS[llama]


P_LEN, STEPS = 6, 8


def _batch(B, pads, seed=5):
    g = torch.Generator().manual_seed(seed)
    T = P_LEN + STEPS
    ids = torch.randint(1, 100, (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    for r in range(B):
        n = pads[r] if pads is not None else 0
        mask[r, :n] = 0
        ids[r, n] = synth.TINY["media_token_id"]         # the first real token of the row
    return torch.randn(B, 1, 1, 3, 28, 28, generator=g), ids, (mask if pads is not None else None)


def _cached_run(model, vx, ids, mask, static):
    """Teacher-forced prompt + STEPS cached steps; the logits of the last prompt position and of every step, [B, 1 + STEPS, V]."""
    geo_cfg = model.lang_encoder.config
    past = None
    if static:
        from otter_amd.kv_cache import cache_geometry

        n_layers, n_kv, hd, _ = cache_geometry(geo_cfg)
        past = StaticKVCache(n_layers, ids.shape[0], n_kv, hd, ids.shape[1], "cpu", torch.float32)
        ptrs = past.data_ptrs()
    am = (lambda t: None) if mask is None else (lambda t: mask[:, :t])
    out = model(vision_x=vx, lang_x=ids[:, :P_LEN], attention_mask=am(P_LEN), past_key_values=past, use_cache=True, clear_conditioned_layers=False)
    logits = [out.logits[:, -1]]
    for t in range(P_LEN, P_LEN + STEPS):
        past = out.past_key_values
        if static:
            assert isinstance(past, StaticKVCache) and past.length == t
        out = model(vision_x=None, lang_x=ids[:, t:t + 1], attention_mask=am(t + 1), use_cached_vision_x=True, past_key_values=past, use_cache=True,
                    clear_conditioned_layers=False)
        logits.append(out.logits[:, -1])
    model.lang_encoder.clear_conditioned_layers()
    if static:
        assert out.past_key_values is past and past.length == P_LEN + STEPS and past.data_ptrs() == ptrs and past.src is None
    return torch.stack(logits, dim=1)


def _full_run(model, vx, ids, mask):
    logits = []
    for t in range(P_LEN, P_LEN + STEPS + 1):
        out = model(vision_x=vx, lang_x=ids[:, :t], attention_mask=None if mask is None else mask[:, :t], use_cache=False)
        logits.append(out.logits[:, -1])
    return torch.stack(logits, dim=1)


@pytest.mark.parametrize("pads", [None, (0, 2, 3)], ids=["unpadded", "left_padded"])
@pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
def test_static_steps_match_the_legacy_cached_steps(llama, pads):
    """Tolerance: twice the spread the legacy path itself shows between use_cache=True and the full re-forward on the same inputs."""
    model = _model(llama)
    vx, ids, mask = _batch(3, pads)
    with torch.no_grad(), oracle_backend():
        legacy = _cached_run(model, vx, ids, mask, static=False)
        full = _full_run(model, vx, ids, mask)
        static = _cached_run(model, vx, ids, mask, static=True)
    spread = float((legacy - full).abs().max())
    err = float((static - legacy).abs().max())
    print("[static-kv] %s %s: |static - legacy| %.3e, legacy spread (cache vs re-forward) %.3e, max |logit| %.3e" % (
        "llama" if llama else "mpt", "padded" if pads else "unpadded", err, spread, float(legacy.abs().max())))
    assert spread > 0
    assert err <= 2 * spread, (err, spread)


# ---- generate -------------------------------------------------------------------------------------------------------------------------

GEN_CASES = {
    "greedy": dict(),
    "beams3_ngram3": dict(num_beams=3, no_repeat_ngram_size=3),
    "group_beams": dict(num_beams=4, num_beam_groups=2, diversity_penalty=0.5),
    "sample": dict(do_sample=True, top_k=20, temperature=0.9),
}
NEW = 8
NEAR_TIE = 1e-4


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
def test_generate_static_returns_the_legacy_tokens(llama, case):
    """Tokens are compared up to the first step at which the legacy path's top-2 margin falls below 1e-4; the seeds are chosen so that no
    such step occurs (checked here: no case may be cut short), so the whole output is compared."""
    model = _model(llama)
    vx, ids, mask = _batch(2, (0, 2), seed=21)
    lx, mask = ids[:, :P_LEN], mask[:, :P_LEN]
    want, margins = _generate(model, vx, lx, mask, GEN_CASES[case], use_cache=True)
    got, _ = _generate(model, vx, lx, mask, GEN_CASES[case], cache_implementation="static")
    dyn, _ = _generate(model, vx, lx, mask, GEN_CASES[case], cache_implementation="dynamic", use_cache=True)
    print("[static-kv] generate %s %s: smallest legacy top-2 margin %.3e over %d decoder calls" % (
        "llama" if llama else "mpt", case, min(margins), len(margins)))
    cut = next((i for i, m in enumerate(margins) if m < NEAR_TIE), None)
    assert cut is None, "a near-tie at decoder call %d (margin %.3e): choose another seed" % (cut, margins[cut])
    assert want.shape == (2, P_LEN + NEW) and torch.equal(want[:, :P_LEN], lx)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert torch.equal(dyn, want)


def test_generate_static_leaves_the_model_unconditioned_and_reusable():
    model = _model(False)
    vx, ids, _ = _batch(2, None, seed=21)
    a, _ = _generate(model, vx, ids[:, :P_LEN], None, dict(num_beams=3), cache_implementation="static")
    assert not model.lang_encoder.is_conditioned()
    b, _ = _generate(model, vx, ids[:, :P_LEN], None, dict(num_beams=3), cache_implementation="static")
    assert torch.equal(a, b)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------

def test_unknown_cache_implementation_is_rejected():
    model = _model(False)
    vx, ids, _ = _batch(1, None)
    with pytest.raises(ValueError, match="cache_implementation"):
        model.generate(vision_x=vx, lang_x=ids[:, :P_LEN], max_new_tokens=2, cache_implementation="paged")


def test_fuyu_host_does_not_take_a_static_cache():
    from oracle.gen_golden_fuyu import tiny_fuyu_config
    from otter_amd.fuyu import FuyuForCausalLM

    model = FuyuForCausalLM(tiny_fuyu_config()).eval()
    ids = torch.randint(1, 100, (1, 5), generator=torch.Generator().manual_seed(0))
    with pytest.raises(NotImplementedError, match="static"):
        model.generate(input_ids=ids, max_new_tokens=2, cache_implementation="static")
    with pytest.raises(ValueError, match="cache_implementation"):
        model.generate(input_ids=ids, max_new_tokens=2, cache_implementation="paged")


@pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
def test_hosts_reject_what_a_static_cache_cannot_do(llama):
    from otter_amd.kv_cache import cache_geometry

    model = _model(llama)
    vx, ids, _ = _batch(2, None)
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    cache = StaticKVCache(n_layers, 2, n_kv, hd, 12, "cpu", torch.float32)
    with oracle_backend():
        with pytest.raises(RuntimeError, match="no_grad"):       # under autograd
            model(vision_x=vx, lang_x=ids[:, :P_LEN], past_key_values=cache, use_cache=True)
        model.lang_encoder.clear_conditioned_layers()
        with torch.no_grad():
            model(vision_x=vx, lang_x=ids[:, :P_LEN], past_key_values=cache, use_cache=True, clear_conditioned_layers=False)
            assert cache.length == P_LEN
            with pytest.raises(ValueError, match="one-token step"):  # S > 1 over a non-empty cache
                model(vision_x=None, lang_x=ids[:, P_LEN:P_LEN + 2], use_cached_vision_x=True, past_key_values=cache, use_cache=True,
                      clear_conditioned_layers=False)
            with pytest.raises(ValueError, match="rows"):
                model(vision_x=None, lang_x=ids[:1, P_LEN:P_LEN + 1], use_cached_vision_x=True, past_key_values=cache, use_cache=True,
                      clear_conditioned_layers=False)
            for t in range(P_LEN, 12):
                model(vision_x=None, lang_x=ids[:, t:t + 1], use_cached_vision_x=True, past_key_values=cache, use_cache=True,
                      clear_conditioned_layers=False)
            with pytest.raises(ValueError, match="exceed max_len"):  # the cache is full
                model(vision_x=None, lang_x=ids[:, 12:13], use_cached_vision_x=True, past_key_values=cache, use_cache=True,
                      clear_conditioned_layers=False)
        model.lang_encoder.clear_conditioned_layers()
