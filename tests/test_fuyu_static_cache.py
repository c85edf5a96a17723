"""CPU: the OtterHD / Fuyu-8B (Persimmon) host over a StaticKVCache that the caller passes as `past_key_values` -- the prompt pass fills it, a
one-token step appends in place (the plain-torch restatement here: `StaticKVCache.attend_persimmon_reference`), beam search reorders the
table, and `graph_decode=True` runs the replay-mode step (device position, the cache's own mask) eagerly.  tiny_fuyu_config: head_dim 64,
2 layers, fp32.  The boundary of the interface -- what still raises, word for word -- is at the end of the file."""
import pytest
import torch

from oracle.gen_golden_fuyu import tiny_fuyu_config
from otter_amd.kv_cache import StaticKVCache, cache_geometry

PATCH_DIM = 6 * 6 * 3


@pytest.fixture(scope="module")
def model():
    from otter_amd.fuyu import FuyuForCausalLM

    torch.manual_seed(5)
    m = FuyuForCausalLM(tiny_fuyu_config()).eval()
    with torch.no_grad():       # (the initialiser's 0.02 gives almost flat logits: make the decoding decisions clear ones)
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(4.0)
    return m


def _batch(B, L, pads, seed, n_patches=3):
    """ids [B, L], left padding of pads[b] positions, `n_patches` patch positions right after the longest padding."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 120, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.long)
    for b, p in enumerate(pads):
        mask[b, :p] = 0
    patches = torch.randn(B, n_patches, PATCH_DIM, generator=g)
    idx = torch.full((B, L), -1, dtype=torch.long)
    p0 = max(pads)
    idx[:, p0:p0 + n_patches] = torch.arange(n_patches)
    return ids, mask, patches, idx


@pytest.mark.parametrize("replay", [False, True], ids=["scalar", "replay"])
@pytest.mark.parametrize("host", ["fuyu", "persimmon", "persimmon_model"])
def test_step_logits_equal_the_tuple_cache(model, host, replay):
    """6 steps after a 7-token prompt, B = 3 with 0 / 2 / 4 left-padded positions, against the growing tuple cache: tests/test_fuyu_host.py's
    cached-against-full figure on this config, max-abs difference / max-abs value < 1e-5."""
    B, L, steps = 3, 7, 6
    ids, mask, patches, idx = _batch(B, L, (0, 2, 4), seed=11)
    new = torch.randint(3, 120, (B, steps), generator=torch.Generator().manual_seed(12))
    m = {"fuyu": model, "persimmon": model.language_model, "persimmon_model": model.language_model.model}[host]
    pk = {"image_patches": patches, "image_patches_indices": idx} if host == "fuyu" else {}
    head = (lambda o: o.logits) if host != "persimmon_model" else (lambda o: o.last_hidden_state)
    cache = StaticKVCache.for_model(m, rows=B, max_len=L + steps)
    with torch.no_grad():
        ref = m(input_ids=ids, attention_mask=mask, use_cache=True, **pk)
        out = m(input_ids=ids, attention_mask=mask, past_key_values=cache, use_cache=True, **pk)
        assert out.past_key_values is cache and cache.length == L
        got, want, past, am = [head(out)[:, -1:]], [head(ref)[:, -1:]], ref.past_key_values, mask
        if replay:
            cache.enable_replay(mask)
        for t in range(steps):
            am = torch.cat([am, torch.ones(B, 1, dtype=torch.long)], 1)
            ref = m(input_ids=new[:, t:t + 1], attention_mask=am, past_key_values=past, use_cache=True)
            past = ref.past_key_values
            out = m(input_ids=new[:, t:t + 1], attention_mask=None if replay else am, past_key_values=cache, use_cache=True)
            assert out.past_key_values is cache and cache.length == L + t + 1
            want.append(head(ref))
            got.append(head(out))
        if replay:
            assert int(cache.pos_dev) == cache.length and not cache.kernel_steps
    got, want = torch.cat(got, 1), torch.cat(want, 1)
    err = float((got - want).abs().max() / want.abs().max())
    print("static vs tuple cache: max-abs %.3e, relative to max %.3e" % (float((got - want).abs().max()), err))
    assert err < 1e-5
    # the cache holds what the tuple cache holds
    for (k, v), (ks, vs) in zip(past, cache.to_legacy("persimmon")):
        keep = am.bool()[:, None, :, None]
        assert float(((k - ks) * keep).abs().max()) < 1e-5 and float(((v - vs) * keep).abs().max()) < 1e-5


MODES = {
    "greedy": dict(),
    "beams": dict(num_beams=3, num_return_sequences=2),
    "sample": dict(do_sample=True, top_k=20, temperature=0.9),
}


def _generate(model, mode, with_patches, cache=None, graph=False, B=2, L=9, new=6):
    ids, mask, patches, idx = _batch(B, L, (0, 3), seed=21)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=new, eos_token_id=-1, **MODES[mode])
    if with_patches:
        kw.update(image_patches=patches, image_patches_indices=idx)
    if mode == "sample":
        kw["generator"] = torch.Generator().manual_seed(33)
    if cache is not None:
        kw["past_key_values"] = cache
    if graph:
        kw["graph_decode"] = True
    return model.generate(**kw)


@pytest.mark.parametrize("graph", [False, True], ids=["static", "static+graph_decode"])
@pytest.mark.parametrize("with_patches", [False, True], ids=["text", "patches"])
@pytest.mark.parametrize("mode", list(MODES))
def test_generate_returns_the_default_caches_tokens(model, mode, with_patches, graph):
    want = _generate(model, mode, with_patches)
    rows = 2 * MODES[mode].get("num_beams", 1)
    cache = StaticKVCache.for_model(model, rows=rows, max_len=9 + 6)
    got = _generate(model, mode, with_patches, cache=cache, graph=graph)
    assert got.shape == want.shape and torch.equal(got, want)
    assert cache.length == 9 + 6 - 1                      # the last token is never fed
    assert cache.replay == graph and (cache.src is not None) == (mode == "beams")
    if mode == "greedy":                                  # text only through the decoder's own generate, too
        lm = model.language_model
        ids, mask, _, _ = _batch(2, 9, (0, 3), seed=21)
        cache.reset()
        a = lm.generate(ids, attention_mask=mask, max_new_tokens=6, eos_token_id=-1)
        b = lm.generate(ids, attention_mask=mask, max_new_tokens=6, eos_token_id=-1, past_key_values=cache, graph_decode=graph)
        assert torch.equal(a, b)


def test_to_legacy_after_a_beam_run_is_the_gathered_cache(model):
    cache = StaticKVCache.for_model(model, rows=6, max_len=20)
    _generate(model, "beams", True, cache=cache)
    assert cache.src is not None and cache.length == 14
    assert bool((cache.src[:, :14] != torch.arange(6, dtype=torch.int32)[:, None]).any())     # the beams did cross
    legacy = cache.to_legacy("persimmon")
    by_module = cache.to_legacy(model)
    assert len(legacy) == 2
    for i, (k, v) in enumerate(legacy):
        assert k.shape == v.shape == (6, 2, 14, 64)
        for n in range(6):
            for t in range(14):
                r = int(cache.src[n, t])
                assert torch.equal(k[n, :, t], cache.k[i, r, :, t]) and torch.equal(v[n, :, t], cache.v[i, r, :, t])
        assert torch.equal(by_module[i][0], k) and torch.equal(by_module[i][1], v)
    with pytest.raises(ValueError, match="host must be"):
        cache.to_legacy("gptj")


@pytest.mark.parametrize("graph", [False, True])
def test_reset_serves_the_next_call(model, graph):
    cache = StaticKVCache.for_model(model, rows=6, max_len=15)
    ptrs = cache.data_ptrs()
    a = _generate(model, "beams", True, cache=cache, graph=graph)
    with pytest.raises(ValueError, match="holds 14 positions"):
        _generate(model, "beams", True, cache=cache, graph=graph)
    cache.reset()
    assert cache.length == 0 and cache.src is None and not cache.replay and cache.kernel_steps and cache.data_ptrs() == ptrs
    b = _generate(model, "beams", True, cache=cache, graph=graph)
    assert torch.equal(a, b)


def test_for_model_gives_one_geometry(model):
    from otter_amd.fuyu import PersimmonForCausalLM

    cfg = tiny_fuyu_config()
    assert cache_geometry(cfg) == cache_geometry(cfg.text_config) == (2, 2, 64, 128)
    shapes = set()
    for src in (model, model.language_model, model.language_model.model, PersimmonForCausalLM(cfg.text_config), cfg, cfg.text_config):
        c = StaticKVCache.for_model(src, rows=3, max_len=10)
        shapes.add((tuple(c.k.shape), c.dtype, c.k.device.type, c.kv_dtype))
    assert shapes == {((2, 3, 2, 10, 64), torch.float32, "cpu", None)}
    c = StaticKVCache.for_model(cfg, rows=1, max_len=4, dtype=torch.bfloat16, kv_dtype="int8")
    assert c.int8 and c.dtype == torch.bfloat16 and c.k.dtype == torch.int8


def test_uses_persimmon_kernel_is_false_off_the_gpu(model):
    c = StaticKVCache.for_model(model, rows=1, max_len=4, dtype=torch.bfloat16)
    assert not c.uses_persimmon_kernel(torch.zeros(1, 2, 3, 64, dtype=torch.bfloat16), 32)


# ---- errors -----------------------------------------------------------------------------------------------------------------------------

def test_forward_errors(model):
    lm = model.language_model
    ids, mask, _, _ = _batch(2, 5, (0, 1), seed=3)
    cache = StaticKVCache.for_model(model, rows=2, max_len=8)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="inference only"):
            lm(input_ids=ids, past_key_values=cache)
    with torch.no_grad():
        with pytest.raises(ValueError, match="created for 2 rows"):
            lm(input_ids=ids[:1], past_key_values=cache)
        lm(input_ids=ids, attention_mask=mask, past_key_values=cache)
        with pytest.raises(ValueError, match="only a one-token step"):
            lm(input_ids=ids[:, :2], past_key_values=cache)
        with pytest.raises(ValueError, match="default positions"):
            lm(input_ids=ids[:, :1], position_ids=torch.tensor([[2]]), past_key_values=cache)
        lm(input_ids=ids[:, :1], position_ids=torch.tensor([[5]]), past_key_values=cache)      # (the reference's arange(past, past + 1))
        cache.enable_replay(torch.cat([mask, torch.ones(2, 1, dtype=torch.long)], 1))
        with pytest.raises(ValueError, match="replay mode takes attention_mask=None and position_ids=None"):
            lm(input_ids=ids[:, :1], attention_mask=torch.ones(2, 7, dtype=torch.long), past_key_values=cache)
        with pytest.raises(ValueError, match="replay mode takes attention_mask=None and position_ids=None"):
            lm(input_ids=ids[:, :1], position_ids=torch.tensor([[6]]), past_key_values=cache)
        lm(input_ids=ids[:, :1], past_key_values=cache)
        assert cache.length == 7 and cache.rotary_tables[0].shape[0] >= cache.max_len
        lm.model._tables(cache.rotary_tables[0].shape[0] + 1, ids.device)                        # a longer forward in between
        with pytest.raises(RuntimeError, match="rotary tables were rebuilt"):
            lm(input_ids=ids[:, :1], past_key_values=cache)
        lm.model._tab = None
        cache.reset()
        lm(input_ids=ids, past_key_values=cache)
        cache.length = 8                                                                         # full
        with pytest.raises(ValueError, match="exceed max_len"):
            lm(input_ids=ids[:, :1], past_key_values=cache)


def test_the_environment_switch_takes_the_restatement(model, monkeypatch):
    """OTTER_FUYU_HIP_DECODE=0: `attend_persimmon_reference` directly (on the CPU the dispatcher ends there anyway: same logits)."""
    ids, mask, _, _ = _batch(2, 5, (0, 1), seed=3)
    outs = []
    for env in ("1", "0"):
        monkeypatch.setenv("OTTER_FUYU_HIP_DECODE", env)
        cache = StaticKVCache.for_model(model, rows=2, max_len=8)
        calls = []
        monkeypatch.setattr(cache, "attend_persimmon", lambda *a, _f=cache.attend_persimmon, **k: calls.append(1) or _f(*a, **k))
        with torch.no_grad():
            model.language_model(input_ids=ids, attention_mask=mask, past_key_values=cache)
            outs.append(model.language_model(input_ids=ids[:, :1], past_key_values=cache).logits)
        assert len(calls) == (2 if env == "1" else 0)
    assert torch.equal(outs[0], outs[1])


def test_generate_errors(model):
    ids, mask, _, _ = _batch(2, 5, (0, 1), seed=3)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=3, eos_token_id=-1)
    for m in (model, model.language_model):
        c = StaticKVCache.for_model(model, rows=2, max_len=8)
        c.length = 1
        with pytest.raises(ValueError, match="holds 1 positions"):
            m.generate(past_key_values=c, **kw)
        with pytest.raises(ValueError, match="in torch.bfloat16, the model computes"):
            m.generate(past_key_values=StaticKVCache.for_model(model, rows=2, max_len=8, dtype=torch.bfloat16), **kw)
        with pytest.raises(ValueError, match="2 layers of 4 heads x 64"):
            m.generate(past_key_values=StaticKVCache(2, 2, 4, 64, 8, "cpu", torch.float32), **kw)
        with pytest.raises(ValueError, match="2 layers of 2 heads x 128"):
            m.generate(past_key_values=StaticKVCache(2, 2, 2, 128, 8, "cpu", torch.float32), **kw)
        with pytest.raises(ValueError, match="3 layers"):
            m.generate(past_key_values=StaticKVCache(3, 2, 2, 64, 8, "cpu", torch.float32), **kw)
        with pytest.raises(ValueError, match="has 2 rows, this call needs batch x num_beams = 6"):
            m.generate(past_key_values=StaticKVCache.for_model(model, rows=2, max_len=8), num_beams=3, **kw)
        with pytest.raises(ValueError, match="at most 7 positions, this call can reach 8"):
            m.generate(past_key_values=StaticKVCache.for_model(model, rows=2, max_len=7), **kw)
        with pytest.raises(NotImplementedError, match="int8 StaticKVCache"):
            m.generate(past_key_values=StaticKVCache.for_model(model, rows=2, max_len=8, kv_dtype="int8"), **kw)
        with pytest.raises(NotImplementedError, match="unsupported generation arguments .*past_key_values"):
            m.generate(past_key_values=((None, None),), **kw)
    # the host's position limit bounds what a call can reach (max_position_embeddings = 128)
    c = StaticKVCache.for_model(model, rows=2, max_len=128)
    long_ids = torch.randint(3, 120, (2, 126), generator=torch.Generator().manual_seed(1))
    assert model.generate(input_ids=long_ids, max_new_tokens=2, eos_token_id=-1, past_key_values=c).shape == (2, 128)
    with pytest.raises(NotImplementedError, match="int8 key / value cache is not built for head_dim 64"):
        StaticKVCache.for_model(model, rows=2, max_len=8, kv_dtype="int8").attend_persimmon(0, None, None, None, None, None, None, None, 32, 1e-5, 1.0)
    with pytest.raises(NotImplementedError, match="int8 StaticKVCache"):
        with torch.no_grad():
            model(input_ids=ids, past_key_values=StaticKVCache.for_model(model, rows=2, max_len=8, kv_dtype="int8"))


def test_the_string_keywords_raise_as_before(model):
    """The boundary: `cache_implementation="static"`, `kv_cache_dtype` and `graph_decode=True` without a cache object are refused with
    their earlier messages (tests/test_static_kv_cache.py, test_kv_cache_int8.py, test_graph_decode.py, test_fuyu_quant_host.py)."""
    ids = torch.randint(1, 100, (1, 5), generator=torch.Generator().manual_seed(0))
    with pytest.raises(NotImplementedError, match="cache_implementation='static' is not built for the Persimmon host"):
        model.generate(input_ids=ids, max_new_tokens=2, cache_implementation="static")
    with pytest.raises(ValueError, match="cache_implementation must be None, 'dynamic' or 'static'"):
        model.generate(input_ids=ids, max_new_tokens=2, cache_implementation="paged")
    with pytest.raises(NotImplementedError, match="graph_decode=True replays a step over the static cache, which is not built for the Persimmon host"):
        model.generate(input_ids=ids, max_new_tokens=2, graph_decode=True)
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=ids, max_new_tokens=2, graph_decode=True, cache_implementation="static", cross_attention_cache=True)
    with pytest.raises(NotImplementedError, match="unsupported generation arguments .*graph_decode"):
        model.language_model.generate(ids, max_new_tokens=2, graph_decode=True)
    for m in (model, model.language_model):
        with pytest.raises(NotImplementedError, match="kv_cache_dtype quantises the static cache, which is not built for the Persimmon host"):
            m.generate(input_ids=ids, max_new_tokens=2, kv_cache_dtype="int8")
    c = StaticKVCache.for_model(model, rows=1, max_len=8)
    with pytest.raises(NotImplementedError, match="cache_implementation='static'"):      # (a cache object beside the string changes nothing)
        model.generate(input_ids=ids, max_new_tokens=2, cache_implementation="static", past_key_values=c)
