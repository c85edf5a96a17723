"""The OtterHD / Fuyu-8B (Persimmon) cached step over a StaticKVCache on HIP (csrc/persimmon_decode_cache.hip): the two entry points against
the existing kernel (csrc/persimmon_decode.hip) bit for bit, against an fp64 oracle, and against each other; the host's static step against
its default-cache HIP step; the graph-replayed step against the eager one."""
import copy
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS, SCALE = 1e-5, 0.125
POOL_N, POOL_H, POOL_S = 3, 64, 4352
SENTINEL = 7.25     # (exactly representable in bf16)


@pytest.fixture(scope="module")
def pool():
    """One pair of random bf16 [3, 64, 4352, 64] tensors, the past of every kernel case (sliced, never written)."""
    g = torch.Generator(device=DEV).manual_seed(77)
    k = torch.randn(POOL_N, POOL_H, POOL_S, 64, generator=g, device=DEV).bfloat16()
    v = torch.randn(POOL_N, POOL_H, POOL_S, 64, generator=g, device=DEV).bfloat16()
    yield k, v
    del k, v
    gc.collect()
    torch.cuda.empty_cache()


def token(N, H, rot, seed):
    """(qkv, gq, bq, gk, bk) of a new token, and the fp32 rotary tables [POOL_S, rot]."""
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(N, H, 3, 64, generator=g) * 2 + 0.3).bfloat16().to(DEV)
    gq, gk = (1 + 0.3 * torch.randn(64, generator=g)).to(DEV), (1 + 0.3 * torch.randn(64, generator=g)).to(DEV)
    bq, bk = (0.1 * torch.randn(64, generator=g)).to(DEV), (0.1 * torch.randn(64, generator=g)).to(DEV)
    inv = 1.0 / (25000.0 ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    fr = torch.arange(POOL_S, dtype=torch.float32)[:, None] * inv[None, :]
    emb = torch.cat([fr, fr], -1)
    return qkv, (gq, bq, gk, bk), emb.cos().contiguous().to(DEV), emb.sin().contiguous().to(DEV)


def left_padded(N, cols, upto):
    """uint8 [N, cols]: row b has min(5 b + (b > 1), upto) padded keys on the left."""
    kv = torch.ones(N, cols, dtype=torch.uint8)
    for b in range(N):
        kv[b, :min(5 * b + (b > 1), upto)] = 0
    return kv.to(DEV)


def beam_table(N, cols):
    """int32 [N, cols]: a permutation of the rows on the first half of the positions, a repeated ancestor (row 1, twice) on the second."""
    src = torch.empty(N, cols, dtype=torch.int32)
    half = cols // 2
    src[:, :half] = torch.tensor([2, 0, 1], dtype=torch.int32)[:N, None] % N
    src[:, half:] = torch.tensor([1, 1, 0], dtype=torch.int32)[:N, None] % N
    return src.to(DEV)


def gathered(t, src, upto):
    """t [N, H, S, 64] -> the logical past [N, H, upto, 64] of every row: position j of row n from row src[n, j], contiguous."""
    if src is None:
        return t[:, :, :upto].contiguous()
    idx = src[:, :upto].long()
    return t[idx, :, torch.arange(upto, device=t.device)[None]].permute(0, 2, 1, 3).contiguous()


def new_cache(pool, N, H, pos, S_max):
    """k, v [N, H, S_max, 64]: the pool's first `pos` keys, a sentinel in every other slot."""
    out = []
    for t in pool:
        c = torch.full((N, H, S_max, 64), SENTINEL, dtype=torch.bfloat16, device=DEV)
        c[:, :, :pos] = t[:N, :H, :pos]
        out.append(c)
    return out


def against_the_existing_kernel(pool, N, H, pos, rot, masked, S_max, beams, seed):
    from otter_amd import ops

    qkv, ln, cos_t, sin_t = token(N, H, rot, seed)
    kc, vc = new_cache(pool, N, H, pos, S_max)
    src = beam_table(N, pos) if beams else None
    kvalid = left_padded(N, pos + 1, pos) if masked else None
    o_old, kn_old, _ = ops.persimmon_decode_attn(qkv, *ln, cos_t[pos], sin_t[pos], gathered(kc, src, pos), gathered(vc, src, pos), kvalid, rot, EPS,
                                                 SCALE)
    k0, v0 = kc.clone(), vc.clone()
    o = ops.persimmon_decode_attn_cached(qkv, *ln, cos_t[pos], sin_t[pos], kc, vc, pos, rot, EPS, SCALE, src=src, key_valid=kvalid)
    torch.cuda.synchronize()
    tag = (N, H, pos, rot, masked, S_max, beams)
    assert o.shape == (N, H * 64) and not torch.isnan(o).any()
    assert torch.equal(o, o_old), (tag, float((o.float() - o_old.float()).abs().max()))
    assert torch.equal(kc[:, :, pos], kn_old[:, :, pos]), tag            # the stored k': the existing kernel's, bit for bit
    assert torch.equal(vc[:, :, pos], qkv[:, :, 2]), tag                 # v: raw
    k0[:, :, pos], v0[:, :, pos] = kc[:, :, pos], vc[:, :, pos]
    assert torch.equal(kc, k0) and torch.equal(vc, v0), tag              # every other byte as before: the past never moved
    return qkv, ln, cos_t, sin_t, kc, vc, src, kvalid, o


POSITIONS = [1, 17, 127, 128, 129, 1350, 4100]


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H", [2, 64])
def test_scalar_entry_equals_the_existing_kernel(pool, H, N, pos):
    """torch.equal on o and on the written key slot against otter_persimmon_decode_attn over the same past as a contiguous tensor; rot 32
    without a mask and rot 64 with left-padded key_valid; a cache of exactly pos + 1 slots and a larger one.  pos 127: the last
    single-range position at N * H = 2; 128: a range that holds only the new token; 129: the new token and one cached key; 4100: just
    past 4096, where rounding the range length up to whole iterations changes the range count."""
    seed = H * 1000 + N * 100 + pos % 97
    for rot, masked in ((32, False), (64, True)):
        for S_max in (pos + 1, pos + 1 + 200):
            against_the_existing_kernel(pool, N, H, pos, rot, masked, S_max, False, seed)


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("H", [2, 64])
def test_beam_table_equals_the_existing_kernel_on_the_gathered_past(pool, H, pos):
    """N = 3, src a permutation with a repeated ancestor: the existing kernel gets the physically gathered past, the result is bit-equal."""
    against_the_existing_kernel(pool, 3, H, pos, 32, False, pos + 1, True, 5000 + H + pos)
    against_the_existing_kernel(pool, 3, H, pos, 64, True, pos + 40, True, 6000 + H + pos)


def oracle64(qkv, ln, cos_row, sin_row, kp, vp, kvalid, rot):
    """fp64 numpy restatement of one cached step on the kernel's bf16-valued inputs: (o [N,H,64], k' [N,H,64] before its rounding)."""
    f = lambda t: t.double().cpu().numpy()
    qkv, (gq, bq, gk, bk), c, s, kp, vp = f(qkv), [f(t) for t in ln], f(cos_row), f(sin_row), f(kp), f(vp)
    x = qkv[:, :, :2]
    mean = x.mean(-1, keepdims=True)
    y = (x - mean) / np.sqrt(((x - mean) ** 2).mean(-1, keepdims=True) + EPS) * np.stack([gq, gk])[None, None] + np.stack([bq, bk])[None, None]
    h = rot // 2
    y1, y2 = y[..., :h].copy(), y[..., h:rot].copy()
    y[..., :h] = y1 * c[:h] - y2 * s[:h]
    y[..., h:rot] = y2 * c[h:rot] + y1 * s[h:rot]
    q, k = y[:, :, 0], y[:, :, 1]
    sc = np.einsum("nhd,nhkd->nhk", q, np.concatenate([kp, k[:, :, None]], 2)) * SCALE
    if kvalid is not None:
        sc = np.where(kvalid.cpu().numpy()[:, None, :] != 0, sc, -np.inf)
    p = np.exp(sc - sc.max(-1, keepdims=True))
    o = np.einsum("nhk,nhkd->nhd", p / p.sum(-1, keepdims=True), np.concatenate([vp, qkv[:, :, 2][:, :, None]], 2))
    return o, k


@pytest.mark.parametrize("rot,masked", [(32, False), (64, True)])
def test_scalar_entry_against_an_fp64_oracle(pool, rot, masked):
    """o and the stored k' to 1e-2 relative-to-max (tests/test_gpu_persimmon_decode.py's figure for this arithmetic: bf16 q', k' and o),
    N = 3, H = 2, 1350 cached keys in 11 ranges, through a beam table."""
    N, H, pos = 3, 2, 1350
    qkv, ln, cos_t, sin_t, kc, vc, src, kvalid, o = against_the_existing_kernel(pool, N, H, pos, rot, masked, pos + 9, True, 4242)
    o_ref, k_ref = oracle64(qkv, ln, cos_t[pos], sin_t[pos], gathered(kc, src, pos), gathered(vc, src, pos), kvalid, rot)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    e_o, e_k = rel(o.double().cpu().numpy().reshape(N, H, 64), o_ref), rel(kc[:, :, pos].double().cpu().numpy(), k_ref)
    print("[fuyu-static] fp64 oracle rot %d masked %s: o %.2e, k' %.2e" % (rot, masked, e_o, e_k))
    assert e_o < 1e-2 and e_k < 1e-2


@pytest.mark.parametrize("pos", [17, 1350])
def test_fully_masked_row_gives_zero_not_nan(pool, pos):
    """N * H = 8: one range at 18 keys, eleven at 1351."""
    from otter_amd import ops

    N, H = 2, 4
    qkv, ln, cos_t, sin_t = token(N, H, 32, 9)
    kvalid = torch.ones(N, pos + 1, dtype=torch.uint8, device=DEV)
    kvalid[1] = 0
    pos_dev = torch.full((1,), pos, dtype=torch.int32, device=DEV)
    for dyn in (False, True):
        S_max = pos + 3
        kc, vc = new_cache(pool, N, H, pos, S_max)
        if dyn:
            valid = torch.ones(N, S_max, dtype=torch.uint8, device=DEV)
            valid[1] = 0
            o = ops.persimmon_decode_attn_cached_dyn(qkv, *ln, cos_t, sin_t, kc, vc, pos_dev, 32, EPS, SCALE, key_valid=valid)
        else:
            o = ops.persimmon_decode_attn_cached(qkv, *ln, cos_t[pos], sin_t[pos], kc, vc, pos, 32, EPS, SCALE, key_valid=kvalid)
        torch.cuda.synchronize()
        assert not torch.isnan(o).any() and not torch.isnan(kc[:, :, pos]).any()
        assert torch.equal(o[1], torch.zeros_like(o[1])) and o[0].float().abs().max() > 0


CAPACITY = 4224
DYN_POSITIONS = [1, 63, 127, 128, 129, 255, 256, 1350, 2048, 4095, 4100, 4223]


@pytest.mark.parametrize("N,H", [(1, 2), (3, 64)], ids=["NH2", "NH192"])
def test_dyn_entry_equals_the_scalar_entry_at_every_position(pool, N, H):
    """12 positions over a capacity of 4224 (range boundaries included), one workspace and one launch configuration throughout: o and the
    whole cache are torch.equal to the scalar entry's, with a beam table and a left-padded mask."""
    from otter_amd import ops

    qkv, ln, cos_t, sin_t = token(N, H, 32, 31 + N)
    scalar, dyn = new_cache(pool, N, H, CAPACITY, CAPACITY), new_cache(pool, N, H, CAPACITY, CAPACITY)
    src = beam_table(N, CAPACITY - 1) if N == 3 else None
    valid = left_padded(N, CAPACITY, 100)
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = ops._ws.get(ops.persimmon_decode_cached_dyn_workspace_bytes(N, H, CAPACITY), torch.device(DEV, torch.cuda.current_device()))
    for pos in DYN_POSITIONS:
        q = torch.roll(qkv, pos, 0) + (pos % 7) * 0.125                                      # another token at every position
        o_s = ops.persimmon_decode_attn_cached(q, *ln, cos_t[pos], sin_t[pos], scalar[0], scalar[1], pos, 32, EPS, SCALE, src=src, key_valid=valid)
        pos_dev.fill_(pos)
        o_d = ops.persimmon_decode_attn_cached_dyn(q, *ln, cos_t, sin_t, dyn[0], dyn[1], pos_dev, 32, EPS, SCALE, src=src, key_valid=valid)
        torch.cuda.synchronize()
        assert ops._ws.get(1, ws.device) is ws                                                 # one workspace throughout
        assert torch.equal(o_s, o_d), (pos, float((o_s.float() - o_d.float()).abs().max()))
        assert torch.equal(scalar[0], dyn[0]) and torch.equal(scalar[1], dyn[1]), pos


def test_dyn_entry_is_a_no_op_outside_the_cache(pool):
    """pos_dev = 0 and = S_max: o (prefilled with a sentinel) and the cache are unchanged.  The cache tensors are views into a larger
    allocation with guard slots on both sides, which are compared too; the last slot of the cache is then written, and the guards still
    hold."""
    from otter_amd import ops

    N, H, S_max, G = 1, 2, 300, 4
    qkv, ln, cos_t, sin_t = token(N, H, 32, 3)
    big = [torch.full((N, H, G + S_max + G, 64), SENTINEL, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    kc, vc = (b[:, :, G:G + S_max] for b in big)
    kc[:], vc[:] = pool[0][:N, :H, :S_max], pool[1][:N, :H, :S_max]
    before = [b.clone() for b in big]
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    valid = torch.ones(N, S_max, dtype=torch.uint8, device=DEV)
    for p in (0, S_max, S_max + 1, -1):
        pos_dev.fill_(p)
        o = torch.full((N, H * 64), SENTINEL, dtype=torch.bfloat16, device=DEV)
        ops.persimmon_decode_attn_cached_dyn(qkv, *ln, cos_t, sin_t, kc, vc, pos_dev, 32, EPS, SCALE, key_valid=valid, out=o)
        torch.cuda.synchronize()
        assert torch.equal(o, torch.full_like(o, SENTINEL)), p
        assert torch.equal(big[0], before[0]) and torch.equal(big[1], before[1]), p
    pos_dev.fill_(S_max - 1)
    o = ops.persimmon_decode_attn_cached_dyn(qkv, *ln, cos_t, sin_t, kc, vc, pos_dev, 32, EPS, SCALE, key_valid=valid)
    torch.cuda.synchronize()
    assert not torch.isnan(o).any() and torch.equal(vc[:, :, S_max - 1], qkv[:, :, 2])
    for b, b0 in zip(big, before):
        b0[:, :, G + S_max - 1] = b[:, :, G + S_max - 1]
        assert torch.equal(b, b0)


def test_ops_wrappers_validate_before_launch(pool):
    from otter_amd import _capi, ops

    qkv, ln, cos_t, sin_t = token(1, 2, 32, 1)
    kc, vc = new_cache(pool, 1, 2, 5, 8)
    pos_dev = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    with pytest.raises(_capi.OtterHipError, match="pos=8 outside"):
        ops.persimmon_decode_attn_cached(qkv, *ln, cos_t[5], sin_t[5], kc, vc, 8, 32, EPS, SCALE)
    with pytest.raises(_capi.OtterHipError, match="key stride 64"):
        ops.persimmon_decode_attn_cached(qkv, *ln, cos_t[5], sin_t[5], kc[:, :, ::2], vc[:, :, ::2], 2, 32, EPS, SCALE)
    with pytest.raises(_capi.OtterHipError, match="contiguous fp32 \\[rot\\]"):
        ops.persimmon_decode_attn_cached(qkv, *ln, cos_t[5, :16], sin_t[5, :16], kc, vc, 5, 32, EPS, SCALE)
    with pytest.raises(_capi.OtterHipError, match="src must be int32"):
        ops.persimmon_decode_attn_cached(qkv, *ln, cos_t[5], sin_t[5], kc, vc, 5, 32, EPS, SCALE, src=torch.zeros(1, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(_capi.OtterHipError, match=">= S_max, rot"):
        ops.persimmon_decode_attn_cached_dyn(qkv, *ln, cos_t[:7], sin_t[:7], kc, vc, pos_dev, 32, EPS, SCALE)
    with pytest.raises(_capi.OtterHipError, match="key_valid must be uint8 \\[N, >= S_max\\]"):
        ops.persimmon_decode_attn_cached_dyn(qkv, *ln, cos_t, sin_t, kc, vc, pos_dev, 32, EPS, SCALE,
                                             key_valid=torch.ones(1, 7, dtype=torch.uint8, device=DEV))
    with pytest.raises(_capi.OtterHipError, match="pos_dev must be an int32"):
        ops.persimmon_decode_attn_cached_dyn(qkv, *ln, cos_t, sin_t, kc, vc, pos_dev.long(), 32, EPS, SCALE)


# ---------------------------------------------------------------------------------------------------------------------------------------
# host: otter_amd/fuyu.py, 2 layers at Fuyu-8B width
# ---------------------------------------------------------------------------------------------------------------------------------------

B, P_LEN, NEW, PADS, N_PATCH = 2, 40, 12, (0, 5), 6
VOCAB = 1024


@pytest.fixture(scope="module", params=["bf16", "int8"])
def full_width(request):
    from transformers import FuyuConfig

    from otter_amd.fuyu import FuyuForCausalLM

    text = dict(model_type="persimmon", vocab_size=VOCAB, hidden_size=4096, intermediate_size=16384, num_hidden_layers=2, num_attention_heads=64,
                max_position_embeddings=4096, qk_layernorm=True, partial_rotary_factor=0.5, hidden_act="relu2", layer_norm_eps=1e-5,
                rope_theta=25000.0, tie_word_embeddings=False)
    cfg = FuyuConfig(vocab_size=VOCAB, hidden_size=4096, intermediate_size=16384, num_hidden_layers=2, num_attention_heads=64, patch_size=30,
                     num_channels=3, max_position_embeddings=4096, image_size=300, text_config=text, tie_word_embeddings=False)
    torch.manual_seed(41)
    with torch.device(DEV):
        model = FuyuForCausalLM(cfg)
    model = model.to(torch.bfloat16).eval()
    with torch.no_grad():               # (the initialiser's 0.02 gives almost flat logits: make the decoding decisions clear ones)
        model.language_model.lm_head.weight.mul_(8.0)
    if request.param == "int8":
        assert model.quantize_decoder_int8()["replaced"] > 0
    yield model
    del model
    gc.collect()
    torch.cuda.empty_cache()


def batch(seed=99):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, VOCAB, (B, P_LEN), generator=g).to(DEV)
    mask = torch.ones(B, P_LEN, dtype=torch.int64, device=DEV)
    for r, n in enumerate(PADS):
        mask[r, :n] = 0
    patches = torch.randn(B, N_PATCH, 2700, generator=g).to(DEV).bfloat16()
    idx = torch.full((B, P_LEN), -1, dtype=torch.int64, device=DEV)
    idx[:, 8:8 + N_PATCH] = torch.arange(N_PATCH, device=DEV)
    return ids, mask, patches, idx


class Spy:
    def __init__(self, monkeypatch, module, name):
        self.n = 0
        orig = getattr(module, name)

        def f(*a, **k):
            self.n += 1
            return orig(*a, **k)

        monkeypatch.setattr(module, name, f)


def test_static_step_logits_equal_the_default_caches(full_width, monkeypatch):
    """6 steps after a 40-token prompt, B = 2 with 0 / 5 left-padded positions: the logits over the static cache are torch.equal to the
    default-cache HIP step's (the same arithmetic in the attention, the same products everywhere else), and the cache holds the default
    cache's keys and values."""
    from otter_amd import ops
    from otter_amd.kv_cache import StaticKVCache

    model = full_width
    ids, mask, patches, idx = batch()
    new = torch.randint(3, VOCAB, (B, 6), generator=torch.Generator().manual_seed(5)).to(DEV)
    old, stat = Spy(monkeypatch, ops, "persimmon_decode_attn"), Spy(monkeypatch, ops, "persimmon_decode_attn_cached")
    cache = StaticKVCache.for_model(model, rows=B, max_len=P_LEN + 6)
    assert cache.dtype == torch.bfloat16 and cache.k.is_cuda
    with torch.no_grad():
        ref = model(input_ids=ids, attention_mask=mask, image_patches=patches, image_patches_indices=idx, use_cache=True)
        out = model(input_ids=ids, attention_mask=mask, image_patches=patches, image_patches_indices=idx, past_key_values=cache)
        assert torch.equal(out.logits[:, -1], ref.logits[:, -1])
        past, am = ref.past_key_values, mask
        for t in range(6):
            am = torch.cat([am, am.new_ones(B, 1)], 1)
            ref = model(input_ids=new[:, t:t + 1], attention_mask=am, past_key_values=past, use_cache=True)
            past = ref.past_key_values
            out = model(input_ids=new[:, t:t + 1], attention_mask=am, past_key_values=cache)
            assert not torch.isnan(out.logits).any()
            assert torch.equal(out.logits, ref.logits), (t, float((out.logits.float() - ref.logits.float()).abs().max()))
    assert old.n == stat.n == 2 * 6
    for (k, v), (ks, vs) in zip(past, cache.to_legacy("persimmon")):
        assert torch.equal(k, ks) and torch.equal(v, vs)


def _prefilled(model, max_len):
    from otter_amd.kv_cache import StaticKVCache

    ids, mask, patches, idx = batch()
    cache = StaticKVCache.for_model(model, rows=B, max_len=max_len)
    out = model(input_ids=ids, attention_mask=mask, image_patches=patches, image_patches_indices=idx, past_key_values=cache)
    return cache, mask, out.logits[:, -1]


def _twin(cache):
    c2 = copy.copy(cache)
    c2.k, c2.v = cache.k.clone(), cache.v.clone()
    return c2


def test_replayed_steps_equal_the_eager_static_steps(full_width):
    """The logits of every step of the graph path (two eager warm-up steps on the capture stream, the captured step, 8 replays) are
    torch.equal to the eager replay-mode step's and to the position-scalar static step's over caches holding the same prefill."""
    from otter_amd.graph_decode import GraphDecodeStep

    model = full_width
    with torch.no_grad():
        cache, mask, logits = _prefilled(model, P_LEN + NEW)
        c2, c3 = _twin(cache), _twin(cache)
        cache.enable_replay(mask)
        c2.enable_replay(mask)
        step = lambda c: (lambda i: model(input_ids=i, past_key_values=c).logits[:, -1, :])
        graph = GraphDecodeStep(model.language_model, cache, None, step_fn=step(cache), kernel_head_dim=64)
        eager = GraphDecodeStep(model.language_model, c2, None, step_fn=step(c2), kernel_head_dim=64)
        assert graph.use_graph
        eager.use_graph = False
        try:
            nxt, am = logits.float().argmax(-1), mask
            for t in range(NEW - 1):
                lg = graph(nxt[:, None]).clone()
                le = eager(nxt[:, None])
                am = torch.cat([am, am.new_ones(B, 1)], 1)
                ls = model(input_ids=nxt[:, None], attention_mask=am, past_key_values=c3).logits[:, -1, :]
                assert lg.shape == (B, VOCAB)
                assert torch.equal(lg, le), (t, float((lg.float() - le.float()).abs().max()))
                assert torch.equal(lg, ls), (t, float((lg.float() - ls.float()).abs().max()))
                assert cache.length == c2.length == c3.length == P_LEN + t + 1 == int(cache.pos_dev) == int(c2.pos_dev)
                nxt = lg.float().argmax(-1)
            assert torch.equal(cache.k, c2.k) and torch.equal(cache.v, c2.v) and torch.equal(cache.k, c3.k) and torch.equal(cache.v, c3.v)
            assert (graph.captures, graph.replays) == (1, NEW - 1 - 2) and (eager.captures, eager.replays) == (0, 0)
            assert cache.kernel_steps and c2.kernel_steps
            print("[fuyu-static] %d steps bit-equal, capture %.1f ms" % (NEW - 1, graph.capture_seconds * 1e3), flush=True)
        finally:
            graph.release()
            eager.release()


def _gen(model, cache, graph, **kw):
    ids, mask, patches, idx = batch()
    return model.generate(input_ids=ids, attention_mask=mask, image_patches=patches, image_patches_indices=idx, max_new_tokens=NEW,
                          eos_token_id=-1, past_key_values=cache, **(dict(graph_decode=True) if graph else {}), **kw)


@pytest.mark.parametrize("case", ["greedy", "beams3", "sample"])
def test_generate_captures_once_replays_the_rest(full_width, case, monkeypatch):
    """12 new tokens = the prompt pass + 11 cached steps = 2 eager warm-up steps + 1 capture + 9 replays (the captured step's own included).
    No side stream is forked while the step is captured.  The tokens are those of the eager static path; after the call the graph is
    released, and the cache, reset, serves a second call with the same tokens and nothing more allocated."""
    from otter_amd import functional as OF
    from otter_amd.graph_decode import GraphDecodeStep
    from otter_amd.kv_cache import StaticKVCache

    model = full_width
    kw = dict(greedy=dict(), beams3=dict(num_beams=3), sample=dict(do_sample=True, top_k=20, temperature=0.9))[case]
    counts, forks = [], []
    release, fork = GraphDecodeStep.release, OF._SideStream.fork

    def spy_release(self):
        counts.append((self.steps, self.captures, self.replays, self.use_graph, self.cache.kernel_steps))
        out = release(self)
        assert self.graph is None and self.logits is None and self.ids is None and self.stream is None
        return out

    def spy_fork(self):
        if torch.cuda.is_current_stream_capturing():
            forks.append(self.enabled)
        return fork(self)

    monkeypatch.setattr(GraphDecodeStep, "release", spy_release)
    monkeypatch.setattr(OF._SideStream, "fork", spy_fork)
    gen = lambda: dict(generator=torch.Generator(device=DEV).manual_seed(1234)) if case == "sample" else {}
    cache = StaticKVCache.for_model(model, rows=B * kw.get("num_beams", 1), max_len=P_LEN + NEW)
    got = _gen(model, cache, True, **kw, **gen()).cpu()
    assert counts == [(NEW - 1, 1, NEW - 3, True, True)], counts
    assert counts[0][2] == 9 and not any(forks), forks
    gc.collect()
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    cache.reset()
    again = _gen(model, cache, True, **kw, **gen()).cpu()
    assert counts[1:] == [(NEW - 1, 1, NEW - 3, True, True)], counts
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == allocated
    cache.reset()
    want = _gen(model, cache, False, **kw, **gen()).cpu()
    assert len(counts) == 2 and not OF._single_chain
    assert got.shape == want.shape and got.shape[1] == P_LEN + NEW
    assert torch.equal(got, want), (got[:, P_LEN:].tolist(), want[:, P_LEN:].tolist())
    assert torch.equal(again, want)
