"""CPU: `StaticKVCache.attend_branches` (otter_amd/kv_cache.py) -- candidate rows over a cached prompt.  On the CPU the method runs
`attend_branches_reference`, the plain-torch restatement of the two stages the GPU path runs (flash forward over the prompt, then
csrc/branch_attn.hip).  It is checked against a DIRECT softmax in fp64: one softmax per (row, head) over [the valid prompt keys of the row's
sentence + the keys u <= t of its own candidate] with the ALiBi origin at the row's own key -- no lse, no merge.  Also: the cache comes back
byte-identical, and every raise."""
import pytest
import torch

from otter_amd.kv_cache import StaticKVCache

H, D = 2, 16


def _case(B, C, T, P, seed, dtype=torch.float64, masked=True):
    """A filled cache of B prompts of P keys (+ unused capacity), the projection rows of B*C*T candidate tokens, and a left-padded mask whose
    LAST sentence sees no prompt key at all (the lse1 = -inf rows)."""
    g = torch.Generator().manual_seed(seed)
    cache = StaticKVCache(2, B, H, D, P + 3, "cpu", dtype)
    for layer in range(2):
        cache.fill(layer, torch.randn(B, H, P, D, generator=g, dtype=dtype), torch.randn(B, H, P, D, generator=g, dtype=dtype))
    cache.length = P
    N = B * C * T
    qkv = torch.randn(N, 3, H, D, generator=g, dtype=dtype)
    key_valid = None
    if masked:
        key_valid = torch.ones(B, P, dtype=torch.uint8)
        for b in range(B):
            key_valid[b, :min(b, P)] = 0               # left padding of b keys
        key_valid[B - 1] = 0                           # a fully masked prompt
    return cache, qkv, key_valid


def _direct(cache, layer, qkv, key_valid, scale, C, T, slopes):
    """fp64, row by row: softmax over the visible keys, ALiBi slope * (key position - own position)."""
    B, P = cache.rows, cache.length
    N = qkv.shape[0]
    out = torch.zeros(N, H, D, dtype=torch.float64)
    for n in range(N):
        b, t = n // (C * T), n % T
        ok = torch.ones(P, dtype=torch.bool) if key_valid is None else key_valid[b].bool()
        for h in range(H):
            k = torch.cat([cache.k[layer, b, h, :P].double()[ok], qkv[n - t:n + 1, 1, h].double()])
            v = torch.cat([cache.v[layer, b, h, :P].double()[ok], qkv[n - t:n + 1, 2, h].double()])
            pos = torch.cat([torch.arange(P)[ok], P + torch.arange(t + 1)]).double()
            s = (k @ qkv[n, 0, h].double()) * scale
            if slopes is not None:
                s = s + float(slopes[h]) * (pos - (P + t))
            out[n, h] = torch.softmax(s, dim=0) @ v
    return out.reshape(N, H * D)


@pytest.mark.parametrize("with_slopes", [False, True], ids=["plain", "alibi"])
@pytest.mark.parametrize("masked", [False, True], ids=["all_valid", "left_padded_and_dead_row"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 64])
def test_reference_equals_the_direct_softmax(T, C, masked, with_slopes):
    B, P, scale = 3, 5, 0.31
    cache, qkv, key_valid = _case(B, C, T, P, seed=100 * T + C, masked=masked)
    slopes = torch.tensor([0.5, 0.0625]) if with_slopes else None
    before = (cache.k.clone(), cache.v.clone(), cache.length, cache.src)
    got = cache.attend_branches(1, qkv[:, 0], qkv[:, 1], qkv[:, 2], scale, C, T, key_valid=key_valid, slopes=slopes)
    ref = _direct(cache, 1, qkv, key_valid, scale, C, T, slopes)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B * C * T, H * D)
    # fp64 against fp64: the two differ by the order of a handful of sums
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # nothing is written: the cache is byte-identical and its bookkeeping untouched
    assert torch.equal(cache.k, before[0]) and torch.equal(cache.v, before[1]) and cache.length == before[2] and cache.src is before[3]
    assert not cache.replay and cache.group == 1


def test_fp32_rows_run_in_fp32_and_return_the_input_dtype():
    cache, qkv, key_valid = _case(2, 3, 2, 4, seed=7, dtype=torch.float32)
    got = cache.attend_branches(0, qkv[:, 0], qkv[:, 1], qkv[:, 2], 0.25, 3, 2, key_valid=key_valid, slopes=torch.tensor([0.25, 0.5]))
    ref = _direct(cache, 0, qkv, key_valid, 0.25, 3, 2, torch.tensor([0.25, 0.5]))
    assert got.dtype == torch.float32
    assert float((got.double() - ref).abs().max()) <= 2.0 ** -20 * float(ref.abs().max())      # fp32 scores and sums of < 10 terms


def test_a_row_does_not_see_other_candidates_or_later_positions():
    B, C, T, P = 2, 3, 4, 3
    cache, qkv, _ = _case(B, C, T, P, seed=3, masked=False)
    n = (1 * C + 1) * T + 2                              # sentence 1, candidate 1, position 2
    base = cache.attend_branches(0, qkv[:, 0], qkv[:, 1], qkv[:, 2], 0.5, C, T)[n]
    poisoned = qkv.clone()
    own = torch.zeros(B * C * T, dtype=torch.bool)
    own[n - 2:n + 1] = True
    # every key / value row but the row's own keys 0..t.  (Huge, not NaN: the dense restatement multiplies what a row must not see by an
    # exact zero weight, where the kernel does not load it at all -- tests/test_gpu_branch_attn.py puts NaN there.)
    poisoned[~own, 1:] = 1e30
    got = cache.attend_branches(0, poisoned[:, 0], poisoned[:, 1], poisoned[:, 2], 0.5, C, T)[n]
    assert torch.equal(got, base)


def test_branch_view_is_attend_branches_and_refuses_rotary():
    cache, qkv, key_valid = _case(2, 2, 3, 4, seed=9)
    view = cache.branches(2, 3)
    assert view.length == 4 and view.replay is False
    a = view.attend(1, qkv[:, 0], qkv[:, 1], qkv[:, 2], 0.2, key_valid=key_valid)
    assert torch.equal(a, cache.attend_branches(1, qkv[:, 0], qkv[:, 1], qkv[:, 2], 0.2, 2, 3, key_valid=key_valid))
    with pytest.raises(ValueError, match="rotated"):
        view.attend(1, qkv[:, 0], qkv[:, 1], qkv[:, 2], 0.2, cos=torch.ones(D), sin=torch.zeros(D))


# ---- every raise --------------------------------------------------------------------------------------------------------------------------

def _call(cache, qkv, C=2, T=3, **kw):
    return cache.attend_branches(0, qkv[:, 0], qkv[:, 1], qkv[:, 2], 0.2, C, T, **kw)


def test_raises_on_an_int8_cache():
    cache = StaticKVCache(1, 2, H, D, 8, "cpu", torch.float32, kv_dtype="int8")
    cache.fill(0, torch.randn(2, H, 4, D), torch.randn(2, H, 4, D))
    cache.length = 4
    with pytest.raises(NotImplementedError, match="int8"):
        _call(cache, torch.randn(12, 3, H, D))


def test_raises_in_replay_mode():
    cache, qkv, _ = _case(2, 2, 3, 4, seed=1, dtype=torch.float32)
    cache.enable_replay()
    with pytest.raises(ValueError, match="replay mode"):
        _call(cache, qkv)


def test_raises_on_a_shared_prompt_cache_and_on_a_beam_table():
    cache = StaticKVCache(1, 4, H, D, 8, "cpu", torch.float32)
    cache.share_prompt(2)
    cache.fill(0, torch.randn(2, H, 4, D), torch.randn(2, H, 4, D))
    cache.length = 4
    with pytest.raises(ValueError, match="shared-prompt"):
        _call(cache, torch.randn(24, 3, H, D))
    cache, qkv, _ = _case(2, 2, 3, 4, seed=1, dtype=torch.float32)
    cache.reorder(torch.tensor([1, 0]))
    with pytest.raises(ValueError, match="beam table"):
        _call(cache, qkv)


def test_raises_on_an_empty_cache():
    cache = StaticKVCache(1, 2, H, D, 8, "cpu", torch.float32)
    with pytest.raises(ValueError, match="empty"):
        _call(cache, torch.randn(12, 3, H, D))


@pytest.mark.parametrize("C,T", [(0, 3), (2, 0), (1, 65)])
def test_raises_on_counts_outside_their_range(C, T):
    cache, qkv, _ = _case(2, 2, 3, 4, seed=1, dtype=torch.float32)
    with pytest.raises(ValueError, match="C >= 1 and 1 <= T <= 64"):
        _call(cache, qkv, C=C, T=T)


def test_raises_on_shapes_that_do_not_fit():
    cache, qkv, key_valid = _case(2, 2, 3, 4, seed=1, dtype=torch.float32)
    with pytest.raises(ValueError, match="sentences x 3 candidates"):
        _call(cache, qkv, C=3)                                              # N = 12 rows are not 2 x 3 x 3
    with pytest.raises(ValueError, match="k_new / v_new"):
        cache.attend_branches(0, qkv[:, 0], qkv[:, 1, :1], qkv[:, 2, :1], 0.2, 2, 3)
    with pytest.raises(ValueError, match="key_valid must be the prompt's mask"):
        _call(cache, qkv, key_valid=torch.ones(2, 5, dtype=torch.uint8))    # (the step's [rows, length + 1] form is not it)


def test_a_multi_token_append_still_raises():
    cache, _, _ = _case(2, 2, 3, 4, seed=1, dtype=torch.float32)
    with torch.no_grad(), pytest.raises(ValueError, match="only a one-token step can follow"):
        cache.check_step(2, 3)
