"""The int8 static KV cache on HIP (csrc/decode_cache_i8.hip, otter_amd/kv_cache.py with kv_dtype="int8"): the kernel against an fp64 oracle
on the exact stored operands (tolerance measured against the bf16 kernel on the same values), its cache writes bit for bit against the torch
quantiser, the device-position entry against the scalar one, `fill` on the GPU against the CPU, the two decoder hosts on the int8 path, the
composition with the int8 decoder and the graph-replayed step, and memory.

Figures of the run that introduced it are in DESIGN.md section 4.12."""
import copy
import gc
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT8 = 0x5A                 # the byte unwritten code slots hold; four of them are the fp32 pattern unwritten scales hold
FLOOR = 2.0 ** -8            # one bf16 rounding of the output
POSITIONS = [1, 7, 63, 64, 65, 127, 128, 129, 300]   # the 64-key iteration and the 128-key range boundaries; 129 keys: a second range that
                                                     # holds only the new token; 301 keys: three ranges (N x H <= 6)
CAPACITY = 304


def _sent_scale(*shape):
    return torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=DEV).view(torch.float32)


def _deq(codes, scales):
    return codes.double() * scales.double()[..., None]


def _tie_vector():
    """(j + 0.5) * 2^-7 with amax 127 * 2^-7: scale 2^-7 exactly, every quotient an exact tie (all representable in bf16)."""
    j = torch.arange(-63, 64, dtype=torch.float32, device=DEV)
    return torch.cat([(j + 0.5) * 2.0 ** -7, torch.tensor([127 * 2.0 ** -7], device=DEV)]).bfloat16()


def _inputs(N, H, fused, g):
    """q, k_new, v_new views; among the new tokens a zero vector, an exact-tie vector and one whose amax sits on a negative element (they
    reach the key quantiser as they are when there is no rotary, the value quantiser always).  One row of two heads has room for two of the
    three: there the separate-views cases carry the negative-amax vector where the fused ones carry the zero vector.  Returns the views and
    whether vector [0, 0] is the zero one."""
    if fused:
        v4 = torch.randn(N, 3 * H * 128, generator=g, device=DEV).bfloat16().view(N, 3, H, 128)
        q, kn, vn = v4[:, 0], v4[:, 1], v4[:, 2]
    else:
        q, kn, vn = (torch.randn(N, H * 128, generator=g, device=DEV).bfloat16().view(N, H, 128) for _ in range(3))
    zero = N > 1 or fused
    for t in (kn, vn):
        if zero:
            t[0, 0] = 0
        t[0, 1] = _tie_vector()
        if N > 1 or not zero:
            t[N - 1, 0, 5] = -9.0
    return q, kn, vn, zero


def _oracle_i8(q, kn, vn, kc, vc, ks, vs, pos, scale, cos, sin, src, kvalid, slopes):
    """fp64 on the stored operands: codes, fp32 scales, bf16 q, fp32 cos / sin.  The new token is the torch quantiser's on the once-rounded
    rotated k and on v, attended in its dequantised form.  Returns (o [N,H,128] fp64, (k codes, k scale, v codes, v scale) of slot pos)."""
    from otter_amd.kv_cache import quantize_kv_int8
    from tests.test_gpu_decode_cached import _rot, _round_to_bf16_once

    N, H = q.shape[:2]
    qd, kd = q.double(), kn.double()
    if cos is not None:
        c, s = cos.double(), sin.double()
        if c.dim() == 2:
            c, s = c[:, None], s[:, None]
        qd, kd = qd * c + _rot(qd) * s, kd * c + _rot(kd) * s
    kslot = _round_to_bf16_once(kd) if cos is not None else kn
    kq, ksc = quantize_kv_int8(kslot)
    vq, vsc = quantize_kv_int8(vn)
    knew, vnew = _deq(kq, ksc), _deq(vq, vsc)
    o = torch.zeros(N, H, 128, dtype=torch.float64, device=q.device)
    ar = torch.arange(pos, device=q.device)
    bias = torch.arange(-pos, 1, device=q.device, dtype=torch.float64)
    for n in range(N):
        rows = src[n, :pos].long() if src is not None else torch.full((pos,), n, device=q.device, dtype=torch.long)
        K = torch.cat([_deq(kc[rows, :, ar], ks[rows, :, ar]), knew[n][None]], dim=0)       # [pos+1, H, 128]
        V = torch.cat([_deq(vc[rows, :, ar], vs[rows, :, ar]), vnew[n][None]], dim=0)
        s_ = torch.einsum("hd,jhd->hj", qd[n], K) * scale
        if slopes is not None:
            s_ = s_ + slopes.double()[:, None] * bias[None]
        if kvalid is not None:
            ok = kvalid[n, :pos + 1].bool()
            if not bool(ok.any()):
                continue
            s_ = s_.masked_fill(~ok[None], float("-inf"))
        o[n] = torch.einsum("hj,jhd->hd", torch.softmax(s_, dim=-1), V)
    return o, (kq, ksc, vq, vsc)


def _raw(q, kn, vn, kc, vc, ks, vs, pos, scale, cos, sin, src, kvalid, slopes):
    """otter_decode_attn_cached_i8 through ctypes with an o buffer and a workspace of exactly the published size, each inside a sentinel
    frame.  Returns (o [N,H,128] bf16, frames_intact)."""
    from otter_amd import _capi as K
    from otter_amd import ops
    from tests.test_gpu_decode_cached import SENT, _frame

    N, H = q.shape[:2]
    S_max = kc.shape[2]
    obuf, o16 = _frame(N * H * 128)
    need = ops.decode_attn_cached_i8_workspace_bytes(N, H, pos + 1)
    wbuf, w16 = _frame(need // 2)
    K.check(K.lib().otter_decode_attn_cached_i8(
        q.data_ptr(), q.stride(0), q.stride(1), kn.data_ptr(), kn.stride(0), kn.stride(1), vn.data_ptr(), vn.stride(0), vn.stride(1),
        K.ptr(cos), K.ptr(sin), (cos.stride(0) if cos is not None and cos.dim() == 2 else 0), kc.data_ptr(), kc.stride(0), kc.stride(1),
        vc.data_ptr(), vc.stride(0), vc.stride(1), ks.data_ptr(), ks.stride(0), ks.stride(1), vs.data_ptr(), vs.stride(0), vs.stride(1),
        K.ptr(src), src.stride(0) if src is not None else 0, K.ptr(kvalid), kvalid.stride(0) if kvalid is not None else 0, K.ptr(slopes),
        o16.data_ptr(), w16.data_ptr(), need, N, H, pos, S_max, 128, float(scale), K.stream()), "decode_attn_cached_i8")
    ok = all(bool((b[:256] == SENT).all()) and bool((b[-256:] == SENT).all()) for b in (obuf, wbuf))
    return o16.view(torch.bfloat16).view(N, H, 128).clone(), ok


def _cache(N, H, S_max, pos, g):
    """Random codes in [-127, 127] and scales that put the values near unit variance; slots >= pos hold sentinels."""
    kc = torch.randint(-127, 128, (N, H, S_max, 128), generator=g, device=DEV, dtype=torch.int8)
    vc = torch.randint(-127, 128, (N, H, S_max, 128), generator=g, device=DEV, dtype=torch.int8)
    ks = (0.5 + torch.rand(N, H, S_max, generator=g, device=DEV)) * (3.0 / 127)
    vs = (0.5 + torch.rand(N, H, S_max, generator=g, device=DEV)) * (3.0 / 127)
    kc[:, :, pos:], vc[:, :, pos:] = SENT8, SENT8
    ks[:, :, pos:], vs[:, :, pos:] = _sent_scale(1), _sent_scale(1)
    return kc, vc, ks, vs


def _same(a, b):
    """Bit equality of two tuples of tensors (fp32 scales compared as int32: the sentinel pattern is a float like any other)."""
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def _one_position(N, H, pos, g, combos, stats):
    from otter_amd import ops
    from tests.test_gpu_decode_cached import _oracle

    scale = 128 ** -0.5
    S_max = pos + 3
    slopes_t = (2.0 ** -(8.0 * torch.arange(1, H + 1, device=DEV, dtype=torch.float32) / H)).contiguous()
    cache = _cache(N, H, S_max, pos, g)
    kc, vc, ks, vs = cache
    orig = tuple(t.clone() for t in cache)
    # what the bf16 kernel is given for the yardstick: the bf16 rounding of the dequantised values
    kb0, vb0 = (kc.float() * ks[..., None]).bfloat16(), (vc.float() * vs[..., None]).bfloat16()
    table = torch.arange(N, dtype=torch.int32, device=DEV)[:, None].repeat(1, S_max)
    table[:, :pos] = torch.randint(0, N, (N, pos), generator=g, device=DEV, dtype=torch.int32)     # shared ancestors
    valid = (torch.rand(N, pos + 1, generator=g, device=DEV) > 0.3).to(torch.uint8)
    valid[:, pos] = 1
    if N > 1:
        valid[N // 2] = 0                                                                          # a fully masked row
    cos_t, sin_t = torch.rand(128, generator=g, device=DEV) * 2 - 1, torch.rand(128, generator=g, device=DEV) * 2 - 1
    cos_n, sin_n = torch.rand(N, 128, generator=g, device=DEV) * 2 - 1, torch.rand(N, 128, generator=g, device=DEV) * 2 - 1
    for rotary, alibi, masked, tabled, fused in combos:
        q, kn, vn, zero = _inputs(N, H, fused, g)
        neg = N > 1 or not zero
        cos, sin = (None, None) if not rotary else ((cos_t, sin_t) if fused else (cos_n, sin_n))
        src, kvalid, slopes = (table if tabled else None), (valid if masked else None), (slopes_t if alibi else None)
        tag = (N, H, pos, rotary, alibi, masked, tabled, fused)
        ref, slot = _oracle_i8(q, kn, vn, *orig, pos, scale, cos, sin, src, kvalid, slopes)
        o, frames = _raw(q, kn, vn, kc, vc, ks, vs, pos, scale, cos, sin, src, kvalid, slopes)
        assert frames, ("frame around o / workspace overwritten", tag)
        # cache writes, bit for bit: slot pos = the torch quantiser's codes and scales; every other byte untouched
        got_slot = (kc[:, :, pos], ks[:, :, pos], vc[:, :, pos], vs[:, :, pos])
        assert _same(got_slot, slot), ("slot", tag)
        for codes, scales in ((kc, ks), (vc, vs)) if not rotary else ((vc, vs),):
            assert not zero or (float(scales[0, 0, pos]) == 1.0 and not bool(codes[0, 0, pos].any())), ("zero vector", tag)
            assert float(scales[0, 1, pos]) == 2.0 ** -7 and bool((codes[0, 1, pos] % 2 == 0)[:-1].all()), ("tie vector", tag)
            assert not neg or int(codes[N - 1, 0, pos, 5]) == -127, ("negative amax", tag)
        assert int(kc[:, :, pos].min()) >= -127 and int(vc[:, :, pos].min()) >= -127, tag
        o2, _ = _raw(q, kn, vn, kc, vc, ks, vs, pos, scale, cos, sin, src, kvalid, slopes)
        assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), ("not deterministic", tag)
        assert _same((kc[:, :, pos], ks[:, :, pos], vc[:, :, pos], vs[:, :, pos]), slot), ("slot, second call", tag)
        for t, t0 in zip(cache, orig):
            t[:, :, pos] = t0[:, :, pos]
        assert _same(cache, orig), ("cache", tag)
        if masked and N > 1:
            assert float(o[N // 2].float().abs().max()) == 0.0, ("fully masked row", tag)
        # the yardstick: the bf16 kernel's error against ITS fp64 oracle on the bf16 rounding of the same values
        kb, vb = kb0.clone(), vb0.clone()
        ref_b, _ = _oracle(q, kn, vn, kb0, vb0, pos, scale, cos, sin, src, kvalid, slopes)
        o_b = ops.decode_attn_cached(q, kn, vn, kb, vb, pos, scale, cos=cos, sin=sin, src=src, key_valid=kvalid, slopes=slopes).view(N, H, 128)
        mag = float(ref.abs().max())
        err_i8, err_bf16 = float((o.double() - ref).abs().max()), float((o_b.double() - ref_b).abs().max())
        bound = max(1.25 * err_bf16, FLOOR * mag)
        stats["worst"], stats["n"] = max(stats["worst"], err_i8 / bound), stats["n"] + 1
        assert err_i8 <= bound, ("o", tag, err_i8, err_bf16, mag)


@pytest.mark.parametrize("N", [1, 3])
def test_kernel_against_fp64_oracle_on_the_stored_operands(N):
    """H = 2: every position x {rotary} x {ALiBi} x {mask with one fully masked row} x {table with shared ancestors} x {fused / separate q, k,
    v views}.  o: err_i8 <= max(1.25 err_bf16, 2^-8 max|ref|).  Cache: codes and scales of slot pos bit-equal to the torch quantiser's on the
    oracle's once-rounded k' and on v (zero, negative-amax and exact-tie vectors among them), every other byte of the four tensors and the
    frames around o and the workspace untouched; a second call gives the same bits."""
    g = torch.Generator(device=DEV).manual_seed(4000 + N)
    stats = dict(worst=0.0, n=0)
    for pos in POSITIONS:
        _one_position(N, 2, pos, g, list(itertools.product([False, True], repeat=5)), stats)
    print("[kv-int8] N=%d H=2: %d cases, worst err_i8 / bound %.3f" % (N, stats["n"], stats["worst"]), flush=True)
    assert stats["n"] == len(POSITIONS) * 32


def test_kernel_at_full_width():
    """H = 32, N = 16, pos = 1000: full-width indexing, one range per (row, head) on a chip of at most 256 CUs."""
    g = torch.Generator(device=DEV).manual_seed(77)
    stats = dict(worst=0.0, n=0)
    _one_position(16, 32, 1000, g, [(True, True, True, True, True)], stats)
    print("[kv-int8] N=16 H=32 pos=1000: err_i8 / bound %.3f" % stats["worst"], flush=True)


# ---- the device-position entry ---------------------------------------------------------------------------------------------------------------

def _dyn_inputs(N, H, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = torch.randn(N, 3, H, 128, device=DEV, generator=g).bfloat16()
    cache = _cache(N, H, CAPACITY, CAPACITY, g)                          # (every slot random: any position may be stepped)
    inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32, device=DEV) / 128))
    fr = torch.arange(CAPACITY, dtype=torch.float32, device=DEV)[:, None] * inv[None, :]
    emb = torch.cat((fr, fr), dim=-1)
    valid = (torch.rand(N, CAPACITY, device=DEV, generator=g) > 0.2).to(torch.uint8)
    valid[:, :3] = 0
    if N > 1:
        valid[N - 1] = 0
    src = torch.randint(0, N, (N, CAPACITY), device=DEV, generator=g, dtype=torch.int32)
    slopes = (2.0 ** -(8.0 * torch.arange(1, H + 1, device=DEV, dtype=torch.float32) / H)).contiguous()
    return dict(q=qkv[:, 0], k=qkv[:, 1], v=qkv[:, 2], cache=cache, cos=emb.cos().contiguous(), sin=emb.sin().contiguous(), valid=valid, src=src,
                slopes=slopes)


def _step(ops, a, cache, pos, on, pos_dev=None, out=None):
    kw = dict(src=a["src"] if on else None, key_valid=a["valid"] if on else None, slopes=a["slopes"] if on else None)
    if pos_dev is None:
        return ops.decode_attn_cached_i8(a["q"], a["k"], a["v"], *cache, pos, 0.0884, cos=a["cos"][pos] if on else None,
                                         sin=a["sin"][pos] if on else None, **kw)
    return ops.decode_attn_cached_i8_dyn(a["q"], a["k"], a["v"], *cache, pos_dev, 0.0884, cos_table=a["cos"] if on else None,
                                         sin_table=a["sin"] if on else None, out=out, **kw)


@pytest.mark.parametrize("N", [1, 3])
def test_dyn_entry_is_bit_identical_to_the_scalar_entry(N):
    """Inside a capacity of 304, at every position, with everything off and everything on (ALiBi, rotary, mask, table): o and all four cache
    tensors torch.equal to the scalar entry's, no other slot changed."""
    from otter_amd import ops

    a = _dyn_inputs(N, 2, 11 + N)
    ca, cb = tuple(t.clone() for t in a["cache"]), tuple(t.clone() for t in a["cache"])
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    for on in (False, True):
        for pos in POSITIONS:
            want = _step(ops, a, ca, pos, on)
            pos_dev.fill_(pos)
            got = _step(ops, a, cb, pos, on, pos_dev=pos_dev)
            assert torch.equal(got, want), (on, pos, float((got.float() - want.float()).abs().max()))
            assert _same(ca, cb), (on, pos)
            assert not torch.equal(cb[0][:, :, pos], a["cache"][0][:, :, pos])             # (the slot was written)
            if on and N > 1:
                assert float(got[N - 1].float().abs().max()) == 0.0
            for c in (ca, cb):
                for t, t0 in zip(c, a["cache"]):
                    t[:, :, pos] = t0[:, :, pos]
            assert _same(cb, a["cache"]), (on, pos)
    assert int(pos_dev) == POSITIONS[-1]


@pytest.mark.parametrize("bad", [0, CAPACITY])
def test_dyn_entry_ignores_a_position_outside_the_cache(bad):
    from otter_amd import ops

    N, H = 3, 2
    a = _dyn_inputs(N, H, 5)
    cb = tuple(t.clone() for t in a["cache"])
    out = torch.full((N, H * 128), 0x5A5A, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    pos_dev = torch.full((1,), bad, dtype=torch.int32, device=DEV)
    got = _step(ops, a, cb, None, True, pos_dev=pos_dev, out=out)
    torch.cuda.synchronize()
    assert got is out and bool((out.view(torch.int16) == 0x5A5A).all())
    assert _same(cb, a["cache"])


def test_wrappers_reject_what_the_kernel_cannot_take():
    from otter_amd import ops
    from otter_amd._capi import OtterHipError

    a = _dyn_inputs(3, 2, 9)
    kc, vc, ks, vs = (t.clone() for t in a["cache"])
    pos_dev = torch.full((1,), 8, dtype=torch.int32, device=DEV)
    for bad in ((kc.to(torch.int16), vc, ks, vs), (kc, vc.transpose(1, 2), ks, vs), (kc, vc, ks.double(), vs), (kc, vc, ks, vs[:, :, :-1]),
                (kc, vc, ks.transpose(1, 2).contiguous().transpose(1, 2), vs)):
        with pytest.raises(OtterHipError):
            ops.decode_attn_cached_i8(a["q"], a["k"], a["v"], *bad, 8, 0.09)
        with pytest.raises(OtterHipError):
            ops.decode_attn_cached_i8_dyn(a["q"], a["k"], a["v"], *bad, pos_dev, 0.09)
    for pos in (0, CAPACITY):
        with pytest.raises(OtterHipError):
            ops.decode_attn_cached_i8(a["q"], a["k"], a["v"], kc, vc, ks, vs, pos, 0.09)
    with pytest.raises(OtterHipError):
        ops.decode_attn_cached_i8_dyn(a["q"], a["k"], a["v"], kc, vc, ks, vs, pos_dev.long(), 0.09)
    with pytest.raises(OtterHipError):
        ops.decode_attn_cached_i8(a["q"].cpu(), a["k"], a["v"], kc, vc, ks, vs, 8, 0.09)
    assert _same((kc, vc, ks, vs), a["cache"])


# ---- fill -------------------------------------------------------------------------------------------------------------------------------------

def test_fill_on_the_gpu_equals_fill_on_the_cpu():
    """The quantiser is a handful of IEEE-exact ops: the same codes and scales on both devices, from fp32 and bf16 prompts handed over as
    strided views, with zero, exact-tie and negative-amax vectors among them."""
    from otter_amd.kv_cache import StaticKVCache

    g = torch.Generator().manual_seed(3)
    N, H, S = 3, 4, 37
    for dtype in (torch.float32, torch.bfloat16):
        k = (torch.randn(N, S, H, 128, generator=g) * 3).to(dtype).transpose(1, 2)          # [N,H,S,128] view of a token-major buffer
        v = torch.randn(N, H, 128, S, generator=g).to(dtype).transpose(2, 3)
        k[0, 0, 1] = 0
        k[0, 1, 2] = _tie_vector().cpu().to(dtype)
        k[1, 0, 3, 7] = -40.0
        caches = []
        for dev in ("cpu", DEV):
            c = StaticKVCache(2, N, H, 128, S + 3, dev, torch.bfloat16, kv_dtype="int8")
            c.fill(1, k.to(dev), v.to(dev))
            caches.append(c)
        a, b = caches
        assert b.k.is_cuda and b.k.dtype == torch.int8 and b.k_scale.dtype == torch.float32
        for x, y in ((a.k, b.k), (a.v, b.v), (a.k_scale, b.k_scale), (a.v_scale, b.v_scale)):
            assert torch.equal(x, y.cpu()), dtype
        assert float(a.k_scale[1, 0, 0, 1]) == 1.0 and float(a.k_scale[1, 0, 1, 2]) == 2.0 ** -7 and int(a.k[1, 1, 0, 3, 7]) == -127
        assert not bool(a.k[0].any()) and int(a.k.min()) == -127


# ---- model level --------------------------------------------------------------------------------------------------------------------------------

def _run_static_kv(model, bench, B, pads, bf16, kv_dtype):
    """tests/test_gpu_decode_cached._run_static with a choice of compute dtype and cache form: step logits [B, STEPS, V] fp32."""
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from tests.test_gpu_w8 import P_LEN, STEPS

    vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN + STEPS, DEV, seed=99, frames=1)
    if pads is not None:
        for r, n in enumerate(pads):
            mask[r, :n] = 0
    am = mask if pads is not None else None
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    cache = StaticKVCache(n_layers, B, n_kv, hd, P_LEN + STEPS, DEV, torch.bfloat16 if bf16 else torch.float32, kv_dtype=kv_dtype)
    ptrs = cache.data_ptrs()
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if bf16 else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), ctx:
        out = model(vision_x=vx.to(torch.bfloat16) if bf16 else vx, lang_x=ids[:, :P_LEN], attention_mask=None if am is None else am[:, :P_LEN],
                    past_key_values=cache, use_cache=True, clear_conditioned_layers=False)
        assert out.past_key_values is cache and cache.length == P_LEN
        steps = []
        for t in range(P_LEN, P_LEN + STEPS):
            out = model(vision_x=None, lang_x=ids[:, t:t + 1], attention_mask=None if am is None else am[:, :t + 1], use_cached_vision_x=True,
                        past_key_values=cache, use_cache=True, clear_conditioned_layers=False)
            assert cache.length == t + 1 and cache.data_ptrs() == ptrs and cache.src is None
            steps.append(out.logits.float())
        model.lang_encoder.clear_conditioned_layers()
    return torch.cat(steps, dim=1)


# d_i8 / d_bf16, where d_i8 = the drift of the bf16-compute int8-cache steps against the fp32 run over an int8 cache (the restatement) and
# d_bf16 = the yardstick of test_static_model_stays_within_twice_the_existing_bf16_drift: the bf16 static path against its fp32 run.  A bf16
# perturbation of a key flips a code about one time in four for large elements, so the ratio is above 1 and seed-sensitive; the constant is
# 1.5 x the worst ratio measured on the MI355X when the test was written (worst over B1 / B4 / B4_left_padded).
# Measured: mpt 1.561 (B1 1.56, B4 1.09, B4_left_padded 0.92), llama 1.566 (1.35, 1.57, 1.22).
MEASURED_WORST_RATIO = {"mpt": 1.561, "llama": 1.566}


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_int8_cache_model_drift_against_the_bf16_static_drift(kind, monkeypatch):
    from otter_amd import ops
    from tests.test_gpu_decode_cached import _Count
    from tests.test_gpu_w8 import BATCHES, STEPS, _build, _drift, _run

    model, bench = _build(kind)
    i8 = _Count(monkeypatch, ops, "decode_attn_cached_i8")
    worst = 0.0
    for tag, B, pads in BATCHES:
        _, ref_steps, _ = _run(model, bench, False, B, pads)
        d_bf16 = _drift(_run_static_kv(model, bench, B, pads, True, None), ref_steps)
        assert i8.n == 0
        ref_i8 = _run_static_kv(model, bench, B, pads, False, "int8")
        assert i8.n == 0                                                 # fp32 compute: the restatement
        new_i8 = _run_static_kv(model, bench, B, pads, True, "int8")
        assert i8.n == 2 * STEPS                                         # every step of both layers on the new kernel
        i8.n = 0
        d_i8, d_quant = _drift(new_i8, ref_i8), _drift(ref_i8, ref_steps)
        worst = max(worst, d_i8 / d_bf16)
        print("[kv-int8] %s %s: decode d_bf16 %.3e d_i8 %.3e ratio %.2f | fp32 int8-cache against fp32 %.3e" % (
            kind, tag, d_bf16, d_i8, d_i8 / d_bf16, d_quant), flush=True)
        assert d_bf16 > 0 and d_i8 > 0
    print("[kv-int8] %s: worst ratio %.3f" % (kind, worst), flush=True)
    assert worst <= 1.5 * MEASURED_WORST_RATIO[kind], (kind, worst)
    del model
    gc.collect()
    torch.cuda.empty_cache()


# ---- composition: the int8 decoder and the graph-replayed step ------------------------------------------------------------------------------------

P_LEN, NEW, B = 40, 12, 2
PADS = (0, 9)


def _prefilled(model, bench, rows_total):
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache

    vx, ids, mask, _, _ = bench.synth_batch(model, B, rows_total, DEV, seed=99, frames=1)
    for r, n in enumerate(PADS):
        mask[r, :n] = 0
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    cache, mc = StaticKVCache(n_layers, B, n_kv, hd, rows_total, DEV, kv_dtype="int8"), MediaCache(B, model.media_token_id)
    out = model(vision_x=vx.to(torch.bfloat16), lang_x=ids[:, :P_LEN], attention_mask=mask[:, :P_LEN], past_key_values=cache, use_cache=True,
                clear_conditioned_layers=False, media_cache=mc)
    return cache, mc, mask[:, :P_LEN], out.logits[:, -1]


def _twin(cache, mc):
    c2, m2 = copy.copy(cache), copy.copy(mc)
    c2.k, c2.v, c2.k_scale, c2.v_scale = cache.k.clone(), cache.v.clone(), cache.k_scale.clone(), cache.v_scale.clone()
    m2.seen, m2.kv = mc.seen.clone(), list(mc.kv)
    return c2, m2


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_replayed_int8_cache_steps_equal_the_eager_steps(kind, monkeypatch):
    """2-layer full-width host with quantize_decoder_int8(), bf16 autocast, 40-token left-padded prompt, B = 2, 12 new tokens: the logits of
    every step of the graph path (two eager warm-up steps, the captured step, 8 replays) are torch.equal to the eager replay-mode step over a
    second int8 cache holding the same prefill, and so are the caches afterwards."""
    from otter_amd import ops
    from otter_amd.graph_decode import GraphDecodeStep
    from tests.test_gpu_decode_cached import _Count
    from tests.test_gpu_media_cache import _build

    model, bench = _build(kind)
    assert model.quantize_decoder_int8()["replaced"] > 0
    dyn, bf16_dyn = _Count(monkeypatch, ops, "decode_attn_cached_i8_dyn"), _Count(monkeypatch, ops, "decode_attn_cached_dyn")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        cache, mc, mask, logits = _prefilled(model, bench, P_LEN + NEW)
        c2, m2 = _twin(cache, mc)
        cache.enable_replay(mask)
        c2.enable_replay(mask)
        graph, eager = GraphDecodeStep(model.lang_encoder, cache, mc), GraphDecodeStep(model.lang_encoder, c2, m2)
        assert graph.use_graph
        eager.use_graph = False
        try:
            nxt = logits.float().argmax(-1)
            for t in range(NEW - 1):
                lg = graph(nxt[:, None]).clone()
                le = eager(nxt[:, None])
                assert torch.equal(lg, le), (kind, t, float((lg.float() - le.float()).abs().max()))
                assert cache.length == c2.length == P_LEN + t + 1 == int(cache.pos_dev) == int(c2.pos_dev)
                nxt = lg.float().argmax(-1)
            assert _same((cache.k, cache.v, cache.k_scale, cache.v_scale), (c2.k, c2.v, c2.k_scale, c2.v_scale))
            assert (graph.captures, graph.replays) == (1, NEW - 1 - 2) and (eager.captures, eager.replays) == (0, 0)
            # Python issued the kernel for the eager twin's 11 steps, the graph path's 2 warm-up steps and its capture: 2 layers each
            assert dyn.n == 2 * (NEW - 1 + 3) and bf16_dyn.n == 0 and cache.kernel_steps
        finally:
            graph.release()
            eager.release()
            model.lang_encoder.clear_conditioned_layers()
    del model
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", ["greedy", "beams3", "sample"])
def test_tiny_generate_under_replay_returns_the_eager_int8_cache_tokens(case):
    """The tiny MPT-host Otter in bf16 autocast (head_dim 16: the step is the restatement's int8 branch on the GPU, run eagerly in replay
    mode): token for token the eager static + media-cache path over an int8 cache."""
    from oracle import synth
    from tests.test_gpu_w8 import _tiny

    model, m = _tiny(DEV)
    vision_x, ids, _, _ = synth.tiny_batch(m["seed"])
    vx, lx = torch.from_numpy(vision_x).to(DEV).to(torch.bfloat16), torch.from_numpy(ids[:, :8]).to(DEV)
    kw = dict(greedy=dict(), beams3=dict(num_beams=3), sample=dict(do_sample=True, top_k=20, temperature=0.9))[case]
    kw.update(max_new_tokens=8, eos_token_id=-1, cache_implementation="static", kv_cache_dtype="int8", cross_attention_cache=True)
    gen = lambda: dict(generator=torch.Generator(device=DEV).manual_seed(1234)) if case == "sample" else {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        want = model.generate(vision_x=vx, lang_x=lx, **kw, **gen())
        got = model.generate(vision_x=vx, lang_x=lx, graph_decode=True, **kw, **gen())
    assert got.shape == want.shape == (lx.shape[0], 16) and torch.equal(got, want), (got.tolist(), want.tolist())
    assert not model.lang_encoder.is_conditioned()


# ---- memory -----------------------------------------------------------------------------------------------------------------------------------------

def test_int8_cache_bytes_and_steps_that_allocate_nothing_that_grows():
    """nbytes <= 0.52 x the bf16 cache's (132 / 256), and memory_allocated agrees; memory_allocated before and after each of 16 int8-cache
    steps differs by no more than the step's own logits, and the cache's four data_ptrs never change."""
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from tests.test_gpu_w8 import _build

    model, bench = _build("mpt")
    P, NSTEP, Bm = 24, 16, 2
    vx, ids, _, _, _ = bench.synth_batch(model, Bm, P + NSTEP + 2, DEV, seed=7, frames=1)
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    gc.collect()
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    plain = StaticKVCache(n_layers, Bm, n_kv, hd, 2048, DEV)
    m1 = torch.cuda.memory_allocated()
    del plain
    big = StaticKVCache(n_layers, Bm, n_kv, hd, 2048, DEV, kv_dtype="int8")
    m2 = torch.cuda.memory_allocated()
    assert big.nbytes() * 256 == (m1 - m0) * 132 and big.nbytes() <= 0.52 * (m1 - m0) and m2 - m0 <= 0.52 * (m1 - m0), (m0, m1, m2)
    del big
    cache = StaticKVCache(n_layers, Bm, n_kv, hd, P + NSTEP + 2, DEV, kv_dtype="int8")
    ptrs = cache.data_ptrs()
    assert len(ptrs) == 4

    def one(t):
        return model(vision_x=None, lang_x=ids[:, t:t + 1], use_cached_vision_x=True, past_key_values=cache, use_cache=True,
                     clear_conditioned_layers=False).logits

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        model(vision_x=vx.to(torch.bfloat16), lang_x=ids[:, :P], past_key_values=cache, use_cache=True, clear_conditioned_layers=False)
        one(P)                                        # warm-up: workspaces, tables, autocast weight copies
        one(P + 1)
        gc.collect()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        for t in range(P + 2, P + 2 + NSTEP):
            a0 = torch.cuda.memory_allocated()
            logits = one(t)
            a1 = torch.cuda.memory_allocated()
            own = -(-logits.numel() * logits.element_size() // 512) * 512
            assert a0 == base, (t, a0, base)
            assert a1 - a0 <= own, (t, a1 - a0, own)
            del logits
        model.lang_encoder.clear_conditioned_layers()
    assert cache.data_ptrs() == ptrs and cache.length == P + 2 + NSTEP
    del model
    gc.collect()
    torch.cuda.empty_cache()
