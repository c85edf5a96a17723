"""StaticKVCache.share_prompt and MediaCache.expand on the CPU: the bookkeeping of a prompt that the beams of a sentence share, and the
plain-torch step over it against an unshared cache that holds the repeated prompt."""
import pytest
import torch

from otter_amd.kv_cache import SHARED_KERNEL_MIN_KEYS, StaticKVCache
from otter_amd.media_cache import MediaCache

L, H, D, MAX_LEN = 2, 2, 8, 16
B, G, S = 2, 3, 5
ROWS = B * G


def _prompt(gen, dtype=torch.float32):
    k = torch.randn(L, B, H, S, D, generator=gen).to(dtype)
    return k, torch.randn(L, B, H, S, D, generator=gen).to(dtype)


def _pair(dtype=torch.float32, kv_dtype=None, seed=0):
    """(a shared cache, an unshared one filled with the repeated prompt, the generator)."""
    gen = torch.Generator().manual_seed(seed)
    k, v = _prompt(gen, dtype)
    shared = StaticKVCache(L, ROWS, H, D, MAX_LEN, "cpu", dtype, kv_dtype=kv_dtype)
    plain = StaticKVCache(L, ROWS, H, D, MAX_LEN, "cpu", dtype, kv_dtype=kv_dtype)
    shared.share_prompt(G)
    with torch.no_grad():
        shared.check_step(B, S)
        plain.check_step(ROWS, S)
    for i in range(L):
        shared.fill(i, k[i], v[i])
        plain.fill(i, k[i].repeat_interleave(G, dim=0), v[i].repeat_interleave(G, dim=0))
    shared.length = plain.length = S
    return shared, plain, gen, (k, v)


def test_share_prompt_bookkeeping():
    c = StaticKVCache(L, ROWS, H, D, MAX_LEN, "cpu", torch.float32)
    assert (c.group, c.shared_len) == (1, 0)
    c.share_prompt(G)
    assert (c.group, c.shared_len, c.src) == (G, 0, None)
    with torch.no_grad():
        c.check_step(B, S)                                           # the leaders' prompt pass
    gen = torch.Generator().manual_seed(1)
    k, v = _prompt(gen)
    c.k.fill_(7.0)
    c.v.fill_(7.0)
    for i in range(L):
        c.fill(i, k[i], v[i])
    c.length = S
    assert c.shared_len == S
    # leaders only: rows 0 and 3 hold the prompt, the other rows' slots are untouched
    assert torch.equal(c.k[:, ::G, :, :S], k) and torch.equal(c.v[:, ::G, :, :S], v)
    others = [n for n in range(ROWS) if n % G]
    assert bool((c.k[:, others] == 7.0).all()) and bool((c.v[:, others] == 7.0).all())
    assert bool((c.k[:, :, :, S:] == 7.0).all())
    # the table
    want = torch.arange(ROWS, dtype=torch.int32)[:, None].repeat(1, MAX_LEN)
    want[:, :S] = (torch.arange(ROWS, dtype=torch.int32) // G * G)[:, None]
    assert c.src.dtype == torch.int32 and torch.equal(c.src, want)
    # what a legacy cache of it holds: the repeated prompt
    for i, (kk, vv) in enumerate(c.to_legacy("llama")):
        assert torch.equal(kk, k[i].repeat_interleave(G, dim=0)) and torch.equal(vv, v[i].repeat_interleave(G, dim=0))
    with torch.no_grad():
        c.check_step(ROWS, 1)                                        # a cached step has every row
        with pytest.raises(ValueError, match="was created for 6 rows, the forward has 2"):
            c.check_step(B, 1)
    c.reset()
    assert (c.group, c.shared_len, c.src, c.length) == (1, 0, None, 0)
    with torch.no_grad(), pytest.raises(ValueError, match="was created for 6 rows, the forward has 2"):
        c.check_step(B, S)                                           # without share_prompt: the refusal as it was


def test_reorder_within_sentences_keeps_the_prefix_on_the_leader():
    shared, _, gen, _ = _pair()
    for step in range(3):
        q = torch.randn(ROWS, H, D, generator=gen)
        for i in range(L):
            shared.attend_reference(i, q, q, q, 0.3)
        shared.end_step()
        idx = torch.cat([torch.randint(0, G, (G,), generator=gen) + b * G for b in range(B)])
        before = shared.src.clone()
        shared.reorder(idx)
        assert torch.equal(shared.src[:, :S], before[:, :S])                         # the prefix columns stay on the leader
        assert torch.equal(shared.src[:, S:shared.length], before[idx][:, S:shared.length])
        assert torch.equal(shared.src[:, shared.length:], before[:, shared.length:])  # the row's own index
    assert bool((shared.src[:, :S] == (torch.arange(ROWS) // G * G)[:, None]).all())


def test_a_cross_sentence_beam_idx_is_refused_on_the_cpu():
    shared, plain, _, _ = _pair()
    with pytest.raises(ValueError, match="every row must continue a row of its own group of 3"):
        shared.reorder(torch.tensor([0, 1, 3, 3, 4, 5]))
    with pytest.raises(ValueError, match="own group"):
        shared.reorder(torch.tensor([0, 1, 2]))
    shared.reorder(torch.tensor([2, 2, 0, 5, 3, 3]))
    plain.reorder(torch.tensor([0, 1, 3, 3, 4, 5]))                  # an unshared cache takes any index, as before


@pytest.mark.parametrize("replay", [False, True], ids=["scalar", "replay"])
@pytest.mark.parametrize("form", ["fp32", "bf16", "int8"])
def test_attend_reference_equals_an_unshared_cache_with_the_repeated_prompt(form, replay):
    """Several steps with reorders, ALiBi on layer 0 and rotary on layer 1, a left-padded sentence: torch.equal at every step."""
    dtype = torch.bfloat16 if form == "bf16" else torch.float32
    shared, plain, gen, _ = _pair(dtype, "int8" if form == "int8" else None, seed=3)
    mask = torch.ones(ROWS, MAX_LEN, dtype=torch.uint8)
    mask[G:, :2] = 0                                                 # sentence 1 is left-padded by two tokens
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    fr = torch.arange(MAX_LEN, dtype=torch.float32)[:, None] * inv[None]
    cos_t, sin_t = torch.cat([fr, fr], -1).cos(), torch.cat([fr, fr], -1).sin()
    slopes = torch.tensor([0.5, 0.125])
    if replay:
        for c in (shared, plain):
            c.enable_replay(mask[:, :S], beams=True)
        assert torch.equal(shared.src[:, :S], (torch.arange(ROWS, dtype=torch.int32) // G * G)[:, None].repeat(1, S))
    table = shared.src
    for step in range(5):
        pos = S + step
        q, kn, vn = (torch.randn(ROWS, H, D, generator=gen).to(dtype) for _ in range(3))
        for i in range(L):
            kw = dict(slopes=slopes) if i == 0 else dict(cos=cos_t if replay else cos_t[pos], sin=sin_t if replay else sin_t[pos])
            if not replay:
                kw["key_valid"] = mask[:, :pos + 1]
            a = shared.attend_reference(i, q, kn, vn, 0.35, **kw)
            b = plain.attend_reference(i, q, kn, vn, 0.35, **kw)
            assert a.dtype == dtype and torch.equal(a, b), (form, replay, step, i)
        shared.end_step()
        plain.end_step()
        idx = torch.cat([torch.randint(0, G, (G,), generator=gen) + b * G for b in range(B)])
        shared.reorder(idx)
        plain.reorder(idx)
    assert shared.src is table                                       # the table's address is fixed from the fill on
    assert shared.length == plain.length == S + 5
    for (ka, va), (kb, vb) in zip(shared.to_legacy("mpt"), plain.to_legacy("mpt")):
        assert torch.equal(ka, kb) and torch.equal(va, vb)


def test_the_int8_form_quantises_the_leaders_rows():
    shared, plain, _, (k, v) = _pair(torch.float32, "int8")
    assert torch.equal(shared.k[:, ::G, :, :S], plain.k[:, ::G, :, :S]) and torch.equal(shared.k_scale[:, ::G, :, :S], plain.k_scale[:, ::G, :, :S])
    others = [n for n in range(ROWS) if n % G]
    assert bool((shared.k[:, others] == 0).all()) and bool((shared.v_scale[:, others] == 1).all())


def test_every_new_error():
    c = StaticKVCache(L, ROWS, H, D, MAX_LEN, "cpu", torch.float32)
    for bad in (4, 0, -1):
        with pytest.raises(ValueError, match="share_prompt: 6 rows are not whole groups of %d" % bad):
            c.share_prompt(bad)
    c.share_prompt(G)
    gen = torch.Generator().manual_seed(1)
    k, v = _prompt(gen)
    with torch.no_grad(), pytest.raises(ValueError, match="shares the prompt among groups of 3 rows: the prompt pass has 2 rows .one per group., "
                                                          "the forward has 4"):
        c.check_step(4, S)
    with pytest.raises(ValueError, match=r"fill: expected k, v \(2, 2, 5, 8\)"):
        c.fill(0, k[0].repeat_interleave(G, dim=0), v[0].repeat_interleave(G, dim=0))    # the repeated prompt is not what a shared cache takes
    c.length = S                                                     # (a prompt pass that never called fill)
    with pytest.raises(ValueError, match="enable_replay: the prompt is shared but `fill` has not laid the table"):
        c.enable_replay(None, beams=True)
    with pytest.raises(ValueError, match="share_prompt: the cache is not empty"):
        c.share_prompt(G)
    c.reset()
    c.share_prompt(1)                                                # one row per group: nothing is shared
    with torch.no_grad():
        c.check_step(ROWS, S)
    # the refusals of a cache without share_prompt, word for word
    d = StaticKVCache(L, ROWS, H, D, MAX_LEN, "cpu", torch.float32)
    with pytest.raises(RuntimeError, match="for inference only: run the forward under torch.no_grad"):
        d.check_step(ROWS, S)
    with torch.no_grad():
        with pytest.raises(ValueError, match="StaticKVCache was created for 6 rows, the forward has 2"):
            d.check_step(2, S)
        with pytest.raises(ValueError, match=r"StaticKVCache: 0 \+ 17 positions exceed max_len=16"):
            d.check_step(ROWS, 17)
        d.length = 3
        with pytest.raises(ValueError, match=r"holds 3 positions: only a one-token step can follow \(got 2 tokens\)"):
            d.check_step(ROWS, 2)


def test_the_kernel_is_not_taken_on_the_cpu_or_when_switched_off(monkeypatch):
    shared, _, gen, _ = _pair()
    q = torch.randn(ROWS, H, D, generator=gen)
    assert not shared.uses_shared_kernel(q, H)                       # fp32 on the CPU: the restatement
    monkeypatch.setattr(StaticKVCache, "uses_kernel", lambda self, q, n_kv: True)
    monkeypatch.delenv("OTTER_SHARED_PREFIX", raising=False)
    shared.head_dim = 128
    assert SHARED_KERNEL_MIN_KEYS == 1536
    assert not shared.uses_shared_kernel(q, H)                       # 2 sentences x 5 shared keys: latency-bound, the table path
    shared.shared_len = 767
    assert not shared.uses_shared_kernel(q, H)
    shared.shared_len = 768                                          # 2 x 768 = 1 536 shared keys per head
    assert shared.uses_shared_kernel(q, H)
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "0")
    assert not shared.uses_shared_kernel(q, H)                       # the A/B lever
    shared.shared_len = S
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "1")
    assert shared.uses_shared_kernel(q, H)                           # forced below the threshold
    shared.group = 7
    assert not shared.uses_shared_kernel(q, H)                       # a group size the kernel is not built for: the table path
    shared.group, shared.kv_dtype = 3, "int8"
    assert not shared.uses_shared_kernel(q, H)                       # the int8 cache has no grouped kernel
    shared.kv_dtype, shared.shared_len = None, 0
    assert not shared.uses_shared_kernel(q, H)


# ---- MediaCache.expand ----------------------------------------------------------------------------------------------------------------

def test_media_cache_expand():
    m = MediaCache(B, 9, rows_per_media=1)
    with pytest.raises(ValueError, match="expand: the cache is empty"):
        m.expand(G)
    m.seen = torch.tensor([1, 2], dtype=torch.int32)
    kv = torch.randn(B, 4, 2 * 64)
    m.kv, m.T_img, m.n, m.heads, m.filled = [None, kv], 1, 4, 1, True
    ptr = kv.data_ptr()
    with pytest.raises(ValueError, match="beams >= 1"):
        m.expand(0)
    m.expand(G)
    assert (m.rows, m.rows_per_media, m.sentences) == (ROWS, G, B)
    assert m.seen.dtype == torch.int32 and m.seen.tolist() == [1, 1, 1, 2, 2, 2]
    assert m.kv[1] is kv and m.kv[1].data_ptr() == ptr               # one copy per sentence, untouched
    # the existing refusals hold for the expanded cache
    with torch.no_grad():
        m.check_step(ROWS, 1)
        with pytest.raises(ValueError, match="MediaCache was created for 6 rows, the forward has 2"):
            m.check_step(B, 1)
        with pytest.raises(ValueError, match="only a one-token step can follow"):
            m.check_step(ROWS, 2)
    with pytest.raises(ValueError, match="only a cache of one row per sentence"):
        m.expand(2)
    # an expanded cache attends like one that was filled with repeated rows
    q = torch.randn(ROWS, 64)
    ref = MediaCache(ROWS, 9, rows_per_media=G)
    ref.seen, ref.kv, ref.T_img, ref.n, ref.heads, ref.filled = m.seen.clone(), [None, kv], 1, 4, 1, True
    assert torch.equal(m.attend_reference(1, q), ref.attend_reference(1, q))
    m.reorder(torch.tensor([1, 1, 0, 5, 4, 3]))
    assert m.seen.tolist() == [1, 1, 1, 2, 2, 2]
    fixed = MediaCache(B, 9)
    fixed.seen, fixed.filled, fixed.fixed_address = torch.zeros(B, dtype=torch.int32), True, True
    with pytest.raises(ValueError, match="no captured graph reads"):
        fixed.expand(G)
