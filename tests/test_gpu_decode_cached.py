"""The cached decode step over a static KV cache on HIP (csrc/decode_cache.hip, otter_amd/kv_cache.py): the kernel against an fp64 oracle on
the bf16-rounded inputs (tolerance measured against the existing decode kernel on the same operands), its cache writes bit for bit, a beam
scenario through the table, and the two decoder hosts / generate() on the static path.

Figures of the run that introduced it are in DESIGN.md section 4.9."""
import copy
import gc
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x5A5A          # bf16 bit pattern the unwritten cache slots, the frame around o and the frame around the workspace hold
FLOOR = 2.0 ** -8      # one bf16 rounding of the output


# ---- oracle -----------------------------------------------------------------------------------------------------------------------------

def _round_to_bf16_once(x):
    """fp64 -> bf16, round-to-nearest-even in ONE rounding (torch converts through fp32: a value that fp32 rounds exactly onto a bf16
    midpoint would be rounded twice)."""
    f = x.float()
    bits = f.view(torch.int32)
    r = x - f.double()
    mid = ((bits & 0xFFFF) == 0x8000) & (r != 0)
    away = (r > 0) == (f > 0)
    bits = torch.where(mid, torch.where(away, bits + 1, bits - 1), bits)
    return bits.view(torch.float32).bfloat16()


def _rot(x):
    return torch.cat((-x[..., 64:], x[..., :64]), dim=-1)


def _oracle(q, kn, vn, kc, vc, pos, scale, cos, sin, src, kvalid, slopes):
    """fp64 on the bf16 inputs.  Returns (o [N,H,128] fp64, k slot [N,H,128] bf16: the rotated k rounded once)."""
    N, H = q.shape[:2]
    qd, kd = q.double(), kn.double()
    if cos is not None:
        c, s = cos.double(), sin.double()
        if c.dim() == 2:
            c, s = c[:, None], s[:, None]
        qd, kd = qd * c + _rot(qd) * s, kd * c + _rot(kd) * s
    kslot = _round_to_bf16_once(kd) if cos is not None else kn.clone()
    o = torch.zeros(N, H, 128, dtype=torch.float64, device=q.device)
    ar = torch.arange(pos, device=q.device)
    bias = torch.arange(-pos, 1, device=q.device, dtype=torch.float64)
    for n in range(N):
        rows = src[n, :pos].long() if src is not None else torch.full((pos,), n, device=q.device, dtype=torch.long)
        K = torch.cat([kc[rows, :, ar].double(), kslot[n].double()[None]], dim=0)          # [pos+1, H, 128]
        V = torch.cat([vc[rows, :, ar].double(), vn[n].double()[None]], dim=0)
        s_ = torch.einsum("hd,jhd->hj", qd[n], K) * scale
        if slopes is not None:
            s_ = s_ + slopes.double()[:, None] * bias[None]
        if kvalid is not None:
            ok = kvalid[n, :pos + 1].bool()
            if not bool(ok.any()):
                continue
            s_ = s_.masked_fill(~ok[None], float("-inf"))
        o[n] = torch.einsum("hj,jhd->hd", torch.softmax(s_, dim=-1), V)
    return o, kslot


def _gathered(t, src, pos, new):
    """[N,H,pos+1,128] contiguous: the operands of the step as the existing decode kernel takes them."""
    N = t.shape[0]
    ar = torch.arange(pos, device=t.device)
    rows = src[:, :pos].long() if src is not None else torch.arange(N, device=t.device)[:, None].expand(N, pos)
    past = t[rows, :, ar[None]].permute(0, 2, 1, 3)
    return torch.cat([past, new[:, :, None]], dim=2).contiguous()


# ---- raw call with framed buffers ---------------------------------------------------------------------------------------------------------

def _frame(nelem, dtype=torch.int16, pad=256):
    buf = torch.full((nelem + 2 * pad,), SENT, dtype=torch.int16, device=DEV)
    return buf, buf[pad:pad + nelem]


def _raw(q, kn, vn, kc, vc, pos, scale, cos, sin, src, kvalid, slopes):
    """otter_decode_attn_cached through ctypes with an o buffer and a workspace of exactly the published size, each inside a sentinel frame.
    Returns (o [N,H,128] bf16, frames_intact)."""
    from otter_amd import _capi as K
    from otter_amd import ops

    N, H = q.shape[:2]
    S_max = kc.shape[2]
    obuf, o16 = _frame(N * H * 128)
    need = ops.decode_attn_cached_workspace_bytes(N, H, pos + 1)
    wbuf, w16 = _frame(need // 2)
    K.check(K.lib().otter_decode_attn_cached(
        q.data_ptr(), q.stride(0), q.stride(1), kn.data_ptr(), kn.stride(0), kn.stride(1), vn.data_ptr(), vn.stride(0), vn.stride(1),
        K.ptr(cos), K.ptr(sin), (cos.stride(0) if cos is not None and cos.dim() == 2 else 0), kc.data_ptr(), kc.stride(0), kc.stride(1),
        vc.data_ptr(), vc.stride(0), vc.stride(1), K.ptr(src), src.stride(0) if src is not None else 0, K.ptr(kvalid),
        kvalid.stride(0) if kvalid is not None else 0, K.ptr(slopes), o16.data_ptr(), w16.data_ptr(), need, N, H, pos, S_max, 128, float(scale),
        K.stream()), "decode_attn_cached")
    ok = all(bool((b[:256] == SENT).all()) and bool((b[-256:] == SENT).all()) for b in (obuf, wbuf))
    return o16.view(torch.bfloat16).view(N, H, 128).clone(), ok


def _inputs(N, H, fused, g):
    if fused:
        qkv = (torch.randn(N, 3 * H * 128, generator=g, device=DEV)).bfloat16()
        v4 = qkv.view(N, 3, H, 128)
        return v4[:, 0], v4[:, 1], v4[:, 2]
    return tuple(torch.randn(N, H * 128, generator=g, device=DEV).bfloat16().view(N, H, 128) for _ in range(3))


POSITIONS = [1, 7, 127, 128, 129, 1000, 4095, 20000]     # the last one is beyond the existing kernel's LDS limit (16384 keys)
OLD_LIMIT = 16384


@pytest.mark.parametrize("H", [2, 32])
@pytest.mark.parametrize("N", [1, 3, 4, 16])
def test_kernel_against_fp64_oracle_and_the_existing_kernel(N, H):
    """Every position x {ALiBi} x {key_valid, with a fully masked row} x {rotary} x {table} x {fused / separate inputs}.
    o: err_new <= max(1.25 err_old, 2^-8 max|ref|) wherever ops.decode_attn takes the case (no rotary, <= 16384 keys; same operands gathered
    into a contiguous cache); elsewhere 2^-8 max|ref| + (the largest err_old / max|ref| seen in the comparable cases of this test) max|ref|.
    Cache: slot pos bit-equal to v_new / k_new (the oracle's once-rounded rotated k with rotary), every other element and the frames around
    o and the workspace untouched; a second call gives the same bits."""
    from otter_amd import ops

    g = torch.Generator(device=DEV).manual_seed(1000 * N + H)
    scale = 128 ** -0.5
    slopes_t = (2.0 ** -(8.0 * torch.arange(1, H + 1, device=DEV, dtype=torch.float32) / H)).contiguous()
    worst_old_rel, worst_ratio, deferred, n_cases = 0.0, 0.0, [], 0
    for pos in POSITIONS:
        S_max = pos + 3
        kc = torch.randn(N, H, S_max, 128, generator=g, device=DEV).bfloat16()
        vc = torch.randn(N, H, S_max, 128, generator=g, device=DEV).bfloat16()
        kc.view(torch.int16)[:, :, pos:] = SENT
        vc.view(torch.int16)[:, :, pos:] = SENT
        k0, v0 = kc.clone(), vc.clone()
        table = torch.arange(N, dtype=torch.int32, device=DEV)[:, None].repeat(1, S_max)
        table[:, :pos] = torch.randint(0, N, (N, pos), generator=g, device=DEV, dtype=torch.int32)
        valid = (torch.rand(N, pos + 1, generator=g, device=DEV) > 0.3).to(torch.uint8)
        valid[:, pos] = 1
        if N > 1:
            valid[N // 2] = 0                                                   # a fully masked row
        cos_t = torch.rand(128, generator=g, device=DEV) * 2 - 1
        sin_t = torch.rand(128, generator=g, device=DEV) * 2 - 1
        cos_n, sin_n = torch.rand(N, 128, generator=g, device=DEV) * 2 - 1, torch.rand(N, 128, generator=g, device=DEV) * 2 - 1
        # rotary last: the cases the existing kernel cannot take use the largest ratio of the comparable ones
        for rotary, alibi, masked, tabled, fused in itertools.product([False, True], [False, True], [False, True], [False, True], [False, True]):
            q, kn, vn = _inputs(N, H, fused, g)
            cos, sin = (None, None) if not rotary else ((cos_t, sin_t) if fused else (cos_n, sin_n))   # a shared row / one row per n
            src = table if tabled else None
            kvalid = valid if masked else None
            slopes = slopes_t if alibi else None
            ref, kslot = _oracle(q, kn, vn, k0, v0, pos, scale, cos, sin, src, kvalid, slopes)
            o, frames = _raw(q, kn, vn, kc, vc, pos, scale, cos, sin, src, kvalid, slopes)
            tag = (N, H, pos, rotary, alibi, masked, tabled, fused)
            assert frames, ("frame around o / workspace overwritten", tag)
            # cache writes: slot pos = (rotated) k / v of the new token, everything else untouched
            assert torch.equal(kc[:, :, pos].view(torch.int16), kslot.view(torch.int16)), ("k slot", tag)
            assert torch.equal(vc[:, :, pos].view(torch.int16), vn.view(torch.int16)), ("v slot", tag)
            kc.view(torch.int16)[:, :, pos] = SENT
            vc.view(torch.int16)[:, :, pos] = SENT
            assert torch.equal(kc.view(torch.int16), k0.view(torch.int16)) and torch.equal(vc.view(torch.int16), v0.view(torch.int16)), ("cache", tag)
            o2, _ = _raw(q, kn, vn, kc, vc, pos, scale, cos, sin, src, kvalid, slopes)
            assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), ("not deterministic", tag)
            kc.view(torch.int16)[:, :, pos] = SENT
            vc.view(torch.int16)[:, :, pos] = SENT
            if masked and N > 1:
                assert float(o[N // 2].float().abs().max()) == 0.0, ("fully masked row", tag)
            mag = float(ref.abs().max())
            err_new = float((o.double() - ref).abs().max())
            n_cases += 1
            if not rotary and pos + 1 <= OLD_LIMIT:
                old = ops.decode_attn(q, _gathered(k0, src, pos, kn), _gathered(v0, src, pos, vn), slopes,
                                      kvalid[:, :pos + 1].contiguous() if masked else None, scale)
                err_old = float((old.double() - ref).abs().max())
                worst_old_rel = max(worst_old_rel, err_old / mag)
                bound = max(1.25 * err_old, FLOOR * mag)
                worst_ratio = max(worst_ratio, err_new / bound)
                assert err_new <= bound, ("o", tag, err_new, err_old, mag)
            else:
                deferred.append((tag, err_new, mag))
    for tag, err_new, mag in deferred:
        bound = (FLOOR + worst_old_rel) * mag
        worst_ratio = max(worst_ratio, err_new / bound)
        assert err_new <= bound, ("o (no comparable run of the existing kernel)", tag, err_new, worst_old_rel, mag)
    print("[decode-cached] N=%d H=%d: %d cases, worst err_new / bound %.3f, worst err_old / max|ref| %.3e" % (N, H, n_cases, worst_ratio, worst_old_rel),
          flush=True)
    assert n_cases == len(POSITIONS) * 32


def test_ops_wrapper_equals_the_raw_call_and_rejects_bad_arguments():
    from otter_amd import ops
    from otter_amd._capi import OtterHipError

    g = torch.Generator(device=DEV).manual_seed(5)
    N, H, pos, S_max = 3, 4, 300, 320
    kc = torch.randn(N, H, S_max, 128, generator=g, device=DEV).bfloat16()
    vc = torch.randn(N, H, S_max, 128, generator=g, device=DEV).bfloat16()
    q, kn, vn = _inputs(N, H, True, g)
    cos, sin = torch.rand(128, generator=g, device=DEV), torch.rand(128, generator=g, device=DEV)
    src = torch.randint(0, N, (N, S_max), generator=g, device=DEV, dtype=torch.int32)
    valid = torch.ones(N, pos + 5, dtype=torch.uint8, device=DEV)
    valid[1, :40] = 0
    slopes = torch.tensor([0.5, 0.25, 0.125, 0.0625], device=DEV)
    k1, v1 = kc.clone(), vc.clone()
    want, _ = _raw(q, kn, vn, k1, v1, pos, 0.09, cos, sin, src, valid, slopes)
    got = ops.decode_attn_cached(q, kn, vn, kc, vc, pos, 0.09, cos=cos, sin=sin, src=src, key_valid=valid, slopes=slopes)
    assert got.shape == (N, H * 128) and torch.equal(got.view(N, H, 128), want) and torch.equal(kc, k1) and torch.equal(vc, v1)
    for bad in (dict(pos=0), dict(pos=S_max), dict(cos=cos, sin=None), dict(src=src.long()), dict(key_valid=valid[:, :pos]),
                dict(slopes=slopes[:3]), dict(src=src[:, :pos - 1])):
        kw = dict(pos=pos, cos=None, sin=None, src=None, key_valid=None, slopes=None)
        kw.update(bad)
        with pytest.raises(OtterHipError):
            ops.decode_attn_cached(q, kn, vn, kc, vc, kw.pop("pos"), 0.09, **kw)
    with pytest.raises(OtterHipError):
        ops.decode_attn_cached(q.float(), kn, vn, kc, vc, pos, 0.09)
    with pytest.raises(OtterHipError):
        ops.decode_attn_cached(q, kn, vn, kc.transpose(1, 2), vc, pos, 0.09)
    with pytest.raises(OtterHipError):
        ops.decode_attn_cached(q.cpu(), kn, vn, kc, vc, pos, 0.09)


def test_beam_scenario_through_the_table():
    """Eight steps with a reorder before each on a StaticKVCache (the kernel through cache.attend) against the oracle, and against the existing
    kernel, on a cache that is physically index_select-ed and cat-ed."""
    from otter_amd import ops
    from otter_amd.kv_cache import StaticKVCache

    g = torch.Generator(device=DEV).manual_seed(9)
    L, N, H, S0 = 2, 6, 4, 130
    scale = 128 ** -0.5
    cache = StaticKVCache(L, N, H, 128, S0 + 8, DEV)
    ptrs = cache.data_ptrs()
    phys = []
    for i in range(L):
        k, v = torch.randn(N, H, S0, 128, generator=g, device=DEV).bfloat16(), torch.randn(N, H, S0, 128, generator=g, device=DEV).bfloat16()
        cache.fill(i, k, v)
        phys.append((k, v))
    cache.length = S0
    slopes = torch.tensor([0.5, 0.25, 0.125, 0.0625], device=DEV)
    for step in range(8):
        beam_idx = torch.randint(0, N, (N,), generator=g, device=DEV)
        cache.reorder(beam_idx)
        phys = [(k.index_select(0, beam_idx), v.index_select(0, beam_idx)) for k, v in phys]
        pos = cache.length
        for i in range(L):
            q, kn, vn = _inputs(N, H, True, g)
            assert cache.uses_kernel(q, H)
            got = cache.attend(i, q, kn, vn, scale, slopes=slopes).view(N, H, 128)
            pk = torch.cat([phys[i][0], torch.zeros_like(phys[i][0][:, :, :1])], dim=2)
            pv = torch.cat([phys[i][1], torch.zeros_like(phys[i][1][:, :, :1])], dim=2)
            ref, _ = _oracle(q, kn, vn, pk, pv, pos, scale, None, None, None, None, slopes)
            phys[i] = (torch.cat([phys[i][0], kn[:, :, None]], dim=2), torch.cat([phys[i][1], vn[:, :, None]], dim=2))
            old = ops.decode_attn(q, phys[i][0], phys[i][1], slopes, None, scale)
            mag = float(ref.abs().max())
            err_new, err_old = float((got.double() - ref).abs().max()), float((old.double() - ref).abs().max())
            assert err_new <= max(1.25 * err_old, FLOOR * mag), (step, i, err_new, err_old, mag)
        cache.length += 1
        leg = cache.to_legacy("llama")
        assert all(torch.equal(leg[i][0], phys[i][0]) and torch.equal(leg[i][1], phys[i][1]) for i in range(L)), step
        assert cache.data_ptrs() == ptrs


# ---- model level --------------------------------------------------------------------------------------------------------------------------

def _run_static(model, bench, B, pads, spy=None):
    """tests/test_gpu_w8._run on the static path (bf16 autocast): prefill logits, step logits."""
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from tests.test_gpu_w8 import P_LEN, STEPS

    vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN + STEPS, DEV, seed=99, frames=1)
    if pads is not None:
        for r, n in enumerate(pads):
            mask[r, :n] = 0
    am = mask if pads is not None else None
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    cache = StaticKVCache(n_layers, B, n_kv, hd, P_LEN + STEPS, DEV)
    ptrs = cache.data_ptrs()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(vision_x=vx.to(torch.bfloat16), lang_x=ids[:, :P_LEN], attention_mask=None if am is None else am[:, :P_LEN],
                    past_key_values=cache, use_cache=True, clear_conditioned_layers=False)
        assert out.past_key_values is cache and cache.length == P_LEN
        pre, steps = out.logits.float(), []
        for t in range(P_LEN, P_LEN + STEPS):
            out = model(vision_x=None, lang_x=ids[:, t:t + 1], attention_mask=None if am is None else am[:, :t + 1], use_cached_vision_x=True,
                        past_key_values=cache, use_cache=True, clear_conditioned_layers=False)
            assert out.past_key_values is cache and cache.length == t + 1 and cache.data_ptrs() == ptrs and cache.src is None
            steps.append(out.logits.float())
        model.lang_encoder.clear_conditioned_layers()
    return pre, torch.cat(steps, dim=1)


class _Count:
    def __init__(self, monkeypatch, mod, name):
        self.n, orig = 0, getattr(mod, name)

        def f(*a, **k):
            self.n += 1
            return orig(*a, **k)

        monkeypatch.setattr(mod, name, f)


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_static_model_stays_within_twice_the_existing_bf16_drift(kind, monkeypatch):
    """2-layer full-width hosts: step logits of the static path against the fp32 run within twice the drift of the existing (legacy cache) bf16
    path against that same fp32 run -- the criterion of test_quantised_model_stays_within_twice_the_existing_bf16_drift."""
    from otter_amd import ops
    from tests.test_gpu_w8 import BATCHES, STEPS, _build, _drift, _run

    model, bench = _build(kind)
    cached, legacy = _Count(monkeypatch, ops, "decode_attn_cached"), _Count(monkeypatch, ops, "decode_attn")
    for tag, B, pads in BATCHES:
        ref_pre, ref_steps, valid = _run(model, bench, False, B, pads)
        old_pre, old_steps, _ = _run(model, bench, True, B, pads)
        n_old, cached.n = legacy.n, 0
        new_pre, new_steps = _run_static(model, bench, B, pads)
        assert cached.n == 2 * STEPS and legacy.n == n_old, (cached.n, legacy.n, n_old)      # every step on the new kernel, none on the old
        d = dict(d_ref_prefill=_drift(old_pre, ref_pre, valid), d_new_prefill=_drift(new_pre, ref_pre, valid),
                 d_ref_decode=_drift(old_steps, ref_steps), d_new_decode=_drift(new_steps, ref_steps))
        print("[decode-cached] %s %s: prefill d_ref %.3e d_new %.3e | decode d_ref %.3e d_new %.3e" % (
            kind, tag, d["d_ref_prefill"], d["d_new_prefill"], d["d_ref_decode"], d["d_new_decode"]), flush=True)
        assert d["d_ref_prefill"] > 0 and d["d_ref_decode"] > 0
        assert d["d_new_prefill"] <= 2 * d["d_ref_prefill"], (kind, tag, d)
        assert d["d_new_decode"] <= 2 * d["d_ref_decode"], (kind, tag, d)
    del model
    gc.collect()
    torch.cuda.empty_cache()


def test_static_cache_composes_with_the_int8_decoder(monkeypatch):
    """MPT host, left-padded batch of 4: the int8 decoder's static path against the fp32 fake-quantised model, within twice the drift of the int8
    decoder's legacy cached path against the same reference."""
    from otter_amd import ops
    from otter_amd.quant import Int8FrozenLinear, dequantize_weight_int8
    from tests.test_gpu_w8 import STEPS, _build, _drift, _run

    model, bench = _build("mpt")
    qmodel = copy.deepcopy(model)
    assert qmodel.quantize_decoder_int8()["replaced"] == 2 * 4
    fq = dict(model.named_modules())
    with torch.no_grad():
        for name, m in qmodel.named_modules():
            if isinstance(m, Int8FrozenLinear):
                fq[name].weight.copy_(dequantize_weight_int8(m.qweight, m.scale, torch.float32))
    B, pads = 4, (0, 3, 7, 5)
    _, ref_steps, _ = _run(model, bench, False, B, pads)
    _, old_steps, _ = _run(qmodel, bench, True, B, pads)
    cached, gemv = _Count(monkeypatch, ops, "decode_attn_cached"), _Count(monkeypatch, ops, "gemv_w8")
    _, new_steps = _run_static(qmodel, bench, B, pads)
    assert cached.n == 2 * STEPS and gemv.n == 2 * 4 * STEPS
    d_ref, d_new = _drift(old_steps, ref_steps), _drift(new_steps, ref_steps)
    print("[decode-cached] int8 mpt B4_left_padded: decode d_ref %.3e d_new %.3e" % (d_ref, d_new), flush=True)
    assert d_ref > 0 and d_new <= 2 * d_ref, (d_new, d_ref)
    del model, qmodel
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_static_steps_allocate_nothing_that_grows(kind):
    """memory_allocated before and after each of 16 static steps differs by no more than the step's own outputs (the logits the caller holds), and
    not at all once they are dropped: no growth with the position.  The cache's data_ptrs never change."""
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from tests.test_gpu_w8 import _build

    model, bench = _build(kind)
    P, NSTEP, B = 24, 16, 2
    vx, ids, _, _, _ = bench.synth_batch(model, B, P + NSTEP + 2, DEV, seed=7, frames=1)
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    cache = StaticKVCache(n_layers, B, n_kv, hd, P + NSTEP + 2, DEV)
    ptrs = cache.data_ptrs()

    def one(t):
        return model(vision_x=None, lang_x=ids[:, t:t + 1], use_cached_vision_x=True, past_key_values=cache, use_cache=True,
                     clear_conditioned_layers=False).logits

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        model(vision_x=vx.to(torch.bfloat16), lang_x=ids[:, :P], past_key_values=cache, use_cache=True, clear_conditioned_layers=False)
        one(P)                                        # warm-up: workspaces, tables, autocast weight copies
        one(P + 1)
        gc.collect()
        torch.cuda.synchronize()
        base, deltas = torch.cuda.memory_allocated(), []
        for t in range(P + 2, P + 2 + NSTEP):
            m0 = torch.cuda.memory_allocated()
            logits = one(t)
            m1 = torch.cuda.memory_allocated()
            own = -(-logits.numel() * logits.element_size() // 512) * 512
            deltas.append(m1 - m0)
            assert m0 == base, (t, m0, base)
            assert m1 - m0 <= own, (t, m1 - m0, own)
            del logits
        model.lang_encoder.clear_conditioned_layers()
    print("[decode-cached] %s: memory_allocated growth over each of %d static steps %s (logits held: %d bytes)" % (kind, NSTEP, sorted(set(deltas)), own))
    assert cache.data_ptrs() == ptrs and cache.length == P + 2 + NSTEP
    del model
    gc.collect()
    torch.cuda.empty_cache()


NEAR_TIE = 1e-4


@pytest.mark.parametrize("case", ["greedy", "beams3"])
def test_tiny_generate_static_equals_legacy_up_to_the_first_near_tie(case):
    """Tiny MPT-host Otter in bf16 autocast (head_dim 16: the static step runs the cache's documented torch branch on the GPU):
    generate(cache_implementation="static") against generate(use_cache=True), tokens equal up to the first decoder call at which the legacy
    path's top-2 logit margin falls below 1e-4."""
    from oracle import synth
    from tests import _golden as G
    from tests.test_gpu_w8 import _tiny

    model, m = _tiny(DEV)
    vision_x, ids, _, _ = synth.tiny_batch(m["seed"])
    vx, lx = torch.from_numpy(vision_x).to(DEV).to(torch.bfloat16), torch.from_numpy(ids[:, :8]).to(DEV)
    kw = dict(num_beams=3) if case == "beams3" else {}
    NEW = 8
    margins = []

    def hook(_m, _a, _k, out):
        top2 = out.logits[:, -1].float().topk(2, dim=-1).values
        margins.append(float((top2[:, 0] - top2[:, 1]).min()))

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        h = model.lang_encoder.register_forward_hook(hook, with_kwargs=True)
        try:
            want = model.generate(vision_x=vx, lang_x=lx, max_new_tokens=NEW, use_cache=True, eos_token_id=-1, **kw)
        finally:
            h.remove()
        got = model.generate(vision_x=vx, lang_x=lx, max_new_tokens=NEW, cache_implementation="static", eos_token_id=-1, **kw)
    cut = next((i for i, x in enumerate(margins) if x < NEAR_TIE), NEW)
    print("[decode-cached] tiny generate %s: legacy top-2 margins %s, compared %d of %d new tokens" % (case, ["%.2e" % x for x in margins], cut, NEW))
    assert got.shape == want.shape == (lx.shape[0], 8 + NEW)
    assert torch.equal(got[:, :8 + cut], want[:, :8 + cut]), (got.tolist(), want.tolist())
