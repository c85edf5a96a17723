"""The cross-attention cache on HIP (csrc/xattn_decode.hip, otter_amd/media_cache.py): the kernel against an fp64 oracle on the bf16 inputs
(tolerance measured against the existing attention kernel on the same operands, Tq = 1, K / V repeated per row), and the two decoder hosts /
generate() with `media_cache=` / `cross_attention_cache=True` against the full re-forward.

Figures of the run that introduced it are in DESIGN.md section 4.10."""
import copy
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x5A5A          # bf16 bit pattern of the frame around o
FLOOR = 2.0 ** -8      # one bf16 rounding of the output


# ---- kernel -----------------------------------------------------------------------------------------------------------------------------

def _oracle(q, k, v, tt, n, rpm, eq, scale):
    """fp64 on the bf16 inputs, the reference's formulation: masked_fill(-finfo.max), softmax, EQ rows with text_time 0 zeroed.
    q [N, H, 64]; k, v [sentences, M, H, 64]; tt [N].  Returns o [N, H * 64] fp64."""
    N, H = q.shape[:2]
    M = k.shape[1]
    sent = torch.arange(N, device=q.device) // rpm
    kd, vd = k.double()[sent], v.double()[sent]
    sim = torch.einsum("nhd,nmhd->nhm", q.double() * scale, kd)
    media_time = torch.arange(M, device=q.device) // n + 1
    t = tt.long().view(N, 1)
    ok = (t == media_time) if eq else (t >= media_time)
    sim = sim.masked_fill(~ok[:, None, :], -torch.finfo(torch.float64).max)
    attn = (sim - sim.amax(-1, keepdim=True)).softmax(-1)
    if eq:
        attn = attn.masked_fill((t == 0).view(N, 1, 1), 0.0)
    return torch.einsum("nhm,nmhd->nhd", attn, vd).reshape(N, H * 64)


@pytest.mark.parametrize("mode", ["EQ", "GE"])
def test_kernel_against_the_fp64_oracle_and_the_existing_kernel(mode):
    """Per case: err_new <= max(1.25 err_old, 2^-8 max|ref|), err_old the existing kernel's error against the same oracle; both are the bf16
    rounding of the output.  Every shape x every rotation of text_time over 0, 1..T_img, T_img + 1, 1000 (so every row meets every value);
    q is a slice of a wider row, k / v the two halves of one buffer; rows that must be zero are exactly 0, uniform rows are the mean of V,
    the frame around o is untouched, a second call gives the same bits."""
    from otter_amd import ops
    from otter_amd._capi import MASK_EQ, MASK_GE

    eq = mode == "EQ"
    mm = MASK_EQ if eq else MASK_GE
    scale = 64 ** -0.5
    g = torch.Generator(device=DEV).manual_seed(17 if eq else 18)
    worst, cases = 0.0, 0
    for N, rpms in ((1, (1,)), (3, (1, 3)), (16, (1, 4))):
        for H in (1, 8):
            HD = H * 64
            for T_img in (1, 3):
                for n in (24, 64, 100):
                    M = T_img * n
                    tt_values = [0] + list(range(1, T_img + 1)) + [T_img + 1, 1000]
                    for rpm in rpms:
                        S = N // rpm
                        qwide = torch.randn(N, HD + 24, generator=g, device=DEV).bfloat16()
                        q = qwide[:, 8:8 + HD]
                        q3 = qwide.as_strided((N, 1, HD), (HD + 24, HD + 24, 1), 8)      # the same slice as [N, Tq = 1, HD] for the existing kernel
                        kv = torch.randn(S, M, 2 * HD, generator=g, device=DEV).bfloat16()
                        k, v = kv[..., :HD], kv[..., HD:]
                        kvrep = kv[torch.arange(N, device=DEV) // rpm].contiguous()
                        vmean = v.double().view(S, M, HD).mean(1)[torch.arange(N, device=DEV) // rpm]
                        for shift in range(len(tt_values)):
                            tt = torch.tensor([tt_values[(r + shift) % len(tt_values)] for r in range(N)], dtype=torch.int32, device=DEV)
                            frame = torch.full((N + 2, HD), SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
                            got = ops.xattn_decode(q, k, v, H, tt, n, rpm, mm, scale, out=frame[1:N + 1])
                            again = ops.xattn_decode(q, k, v, H, tt, n, rpm, mm, scale)
                            old, _ = ops.attn_fwd(q3, kvrep[..., :HD], kvrep[..., HD:], H, tt.view(N, 1), n, mm, scale)
                            ref = _oracle(q.view(N, H, 64), k.view(S, M, H, 64), v.view(S, M, H, 64), tt, n, rpm, eq, scale)
                            mag = float(ref.abs().max())
                            err_new, err_old = float((got.double() - ref).abs().max()), float((old.view(N, HD).double() - ref).abs().max())
                            bound = max(1.25 * err_old, FLOOR * mag) if mag > 0 else 0.0
                            case = (N, H, T_img, n, rpm, shift)
                            assert err_new <= bound, (case, err_new, err_old, mag)
                            if bound > 0:
                                worst = max(worst, err_new / bound)
                            assert torch.equal(got, again), case
                            bits = frame.view(torch.int16)
                            assert bool((bits[0] == SENT).all()) and bool((bits[N + 1] == SENT).all()), case
                            ttl = tt.long()
                            if eq:
                                zero = ttl == 0
                                assert bool((got[zero].view(torch.int16) == 0).all()), case
                                uni = (ttl > T_img) | (ttl < 0)
                            else:
                                uni = ttl < 1
                            if bool(uni.any()):
                                e_uni = float((got[uni].double() - vmean[uni]).abs().max())
                                assert e_uni <= max(1.25 * err_old, FLOOR * float(vmean[uni].abs().max())), (case, e_uni)
                            cases += 1
    print("[media-cache] kernel %s: %d cases, worst err_new / bound %.3f" % (mode, cases, worst), flush=True)


def test_wrapper_rejects_what_the_kernel_cannot_take():
    from otter_amd import ops
    from otter_amd._capi import MASK_EQ, MASK_NONE, OtterHipError

    N, H, M, n = 4, 2, 48, 24
    q = torch.randn(N, H * 64, device=DEV).bfloat16()
    kv = torch.randn(2, M, 2 * H * 64, device=DEV).bfloat16()
    k, v = kv[..., :H * 64], kv[..., H * 64:]
    tt = torch.ones(N, dtype=torch.int32, device=DEV)
    ops.xattn_decode(q, k, v, H, tt, n, 2, MASK_EQ, 0.125)
    for bad in (dict(q=q.float()), dict(q=q[:, 1:]), dict(tt=tt.long()), dict(tt=tt[:3]), dict(rpm=4), dict(n=5), dict(mode=MASK_NONE),
                dict(k=k[:, :, 1:]), dict(v=v.contiguous()), dict(q=q.cpu())):
        a = dict(q=q, k=k, v=v, tt=tt, n=n, rpm=2, mode=MASK_EQ)
        a.update(bad)
        with pytest.raises(OtterHipError):
            ops.xattn_decode(a["q"], a["k"], a["v"], H, a["tt"], a["n"], a["rpm"], a["mode"], 0.125)


# ---- model level --------------------------------------------------------------------------------------------------------------------------

def _build(kind):
    """2-layer full-width Otter on the MPT or the LLaMA host with a gated block before EACH decoder layer (the benchmark's architecture has
    one every 4 layers: none in 2), fp32 everywhere, every parameter from oracle.synth (gates away from 0)."""
    import bench
    from oracle import synth
    from otter_amd.configuration_otter import OtterConfig
    from otter_amd.modeling_otter import OtterForConditionalGeneration

    llama = kind == "llama"
    text, vis = dict(bench.LLAMA7B_TEXT if llama else bench.MPT7B_TEXT), dict(bench.CLIP_L14)
    text["num_hidden_layers" if llama else "n_layers"] = 2
    vis["num_hidden_layers"] = 2
    cfg = OtterConfig(vision_config=vis, text_config=text, cross_attn_every_n_layers=1, **(dict(max_num_frames=8) if llama else {}))
    with torch.device(DEV):
        model = OtterForConditionalGeneration(cfg)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.from_numpy(synth.param_for(1234, name, tuple(p.shape))).to(DEV))
    assert sum(1 for l in model.lang_encoder._get_decoder_layers() if l.gated_cross_attn_layer is not None) == 2
    return model.eval(), bench


def _batch(model, bench, B, pads):
    from tests.test_gpu_w8 import P_LEN, STEPS

    vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN + STEPS, DEV, seed=99, frames=1)
    if B > 1:
        ids[B - 1, P_LEN + 3] = model.media_token_id      # a second <image> among the decoded ids: text_time 2 with T_img = 1, the uniform row
    if pads is not None:
        for r, n in enumerate(pads):
            mask[r, :n] = 0
    return vx, ids, (mask if pads is not None else None)


def _ctx(bf16):
    return torch.autocast("cuda", dtype=torch.bfloat16) if bf16 else torch.autocast("cuda", enabled=False)


def _run_full(model, bench, bf16, B, pads):
    """The full re-forward (use_cache=False) at every step's length: the logits of the last position, [B, STEPS, V]."""
    from tests.test_gpu_w8 import P_LEN, STEPS

    vx, ids, am = _batch(model, bench, B, pads)
    steps = []
    with torch.no_grad(), _ctx(bf16):
        v = vx.to(torch.bfloat16) if bf16 else vx
        for t in range(P_LEN, P_LEN + STEPS):
            out = model(vision_x=v, lang_x=ids[:, :t + 1], attention_mask=None if am is None else am[:, :t + 1], use_cache=False)
            steps.append(out.logits[:, -1:].float())
    return torch.cat(steps, dim=1)


def _run_cached(model, bench, B, pads, static, media):
    """Teacher-forced prefill + STEPS cached steps in bf16 autocast, with or without a MediaCache: step logits [B, STEPS, V]."""
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache
    from tests.test_gpu_w8 import P_LEN, STEPS

    vx, ids, am = _batch(model, bench, B, pads)
    past = None
    if static:
        n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
        past = StaticKVCache(n_layers, B, n_kv, hd, P_LEN + STEPS, DEV)
    mc = MediaCache(B, model.media_token_id) if media else None
    mkw = {"media_cache": mc} if media else {}
    steps = []
    with torch.no_grad(), _ctx(True):
        out = model(vision_x=vx.to(torch.bfloat16), lang_x=ids[:, :P_LEN], attention_mask=None if am is None else am[:, :P_LEN],
                    past_key_values=past, use_cache=True, clear_conditioned_layers=False, **mkw)
        ptrs = mc.data_ptrs() if media else None
        for t in range(P_LEN, P_LEN + STEPS):
            out = model(vision_x=None, lang_x=ids[:, t:t + 1], attention_mask=None if am is None else am[:, :t + 1], use_cached_vision_x=True,
                        past_key_values=out.past_key_values, use_cache=True, clear_conditioned_layers=False, **mkw)
            steps.append(out.logits.float())
        model.lang_encoder.clear_conditioned_layers()
    if media:
        assert mc.data_ptrs() == ptrs and all(t.dtype == torch.bfloat16 for t in mc.kv if t is not None)
        assert torch.equal(mc.seen.long(), (ids == model.media_token_id).sum(1))
    return torch.cat(steps, dim=1)


class _Count:
    def __init__(self, monkeypatch, mod, name):
        self.n, orig = 0, getattr(mod, name)

        def f(*a, **k):
            self.n += 1
            return orig(*a, **k)

        monkeypatch.setattr(mod, name, f)


MODEL_BATCHES = [("B1", 1, None), ("B4_left_padded", 4, (0, 3, 7, 5))]


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_media_cache_steps_stay_within_twice_the_bf16_reforward_drift(kind, monkeypatch):
    """2-layer full-width hosts, bf16, 24-token prompt + 8 steps: the row-wise relative logits drift of the media-cache steps against the
    fp32-mode full re-forward is at most twice the drift of the bf16 full re-forward against that same fp32 run.  The legacy cached path's
    drift (it ignores the image) is printed beside it."""
    from otter_amd import ops
    from tests.test_gpu_w8 import STEPS, _drift

    model, bench = _build(kind)
    new_k, old_k = _Count(monkeypatch, ops, "xattn_decode"), _Count(monkeypatch, ops, "attn_fwd")
    for tag, B, pads in MODEL_BATCHES:
        ref = _run_full(model, bench, False, B, pads)
        d_ref = _drift(_run_full(model, bench, True, B, pads), ref)
        n0 = old_k.n
        d_legacy = _drift(_run_cached(model, bench, B, pads, False, False), ref)
        n_legacy = old_k.n - n0                           # the existing attention kernel: perceiver + gated blocks of the prompt pass, gated blocks of every step
        assert d_ref > 0
        for static in (False, True):
            new_k.n, n_old = 0, old_k.n
            d_new = _drift(_run_cached(model, bench, B, pads, static, True), ref)
            n_gated = sum(1 for l in model.lang_encoder._get_decoder_layers() if l.gated_cross_attn_layer is not None)
            assert new_k.n == n_gated * STEPS and old_k.n - n_old == n_legacy - n_gated * STEPS, (new_k.n, old_k.n - n_old, n_legacy)   # steps on the new kernel only
            print("[media-cache] %s %s %s: decode drift vs fp32 re-forward: bf16 re-forward %.3e, media cache %.3e (ratio %.2f), legacy cached %.3e" % (
                kind, tag, "static" if static else "tuple", d_ref, d_new, d_new / d_ref, d_legacy), flush=True)
            assert d_new <= 2 * d_ref, (kind, tag, static, d_new, d_ref)
    del model
    gc.collect()
    torch.cuda.empty_cache()


def test_media_cache_composes_with_the_int8_decoder(monkeypatch):
    """MPT host, left-padded batch of 4, static cache: the int8 decoder's media-cache steps against the fp32 fake-quantised model's full
    re-forward, within twice the drift of the int8 decoder's own bf16 full re-forward against the same reference."""
    from otter_amd import ops
    from otter_amd.quant import Int8FrozenLinear, dequantize_weight_int8
    from tests.test_gpu_w8 import STEPS, _drift

    model, bench = _build("mpt")
    qmodel = copy.deepcopy(model)
    assert qmodel.quantize_decoder_int8()["replaced"] == 2 * 4
    fq = dict(model.named_modules())
    with torch.no_grad():
        for name, m in qmodel.named_modules():
            if isinstance(m, Int8FrozenLinear):
                fq[name].weight.copy_(dequantize_weight_int8(m.qweight, m.scale, torch.float32))
    B, pads = 4, (0, 3, 7, 5)
    ref = _run_full(model, bench, False, B, pads)
    d_ref = _drift(_run_full(qmodel, bench, True, B, pads), ref)
    new_k, gemv = _Count(monkeypatch, ops, "xattn_decode"), _Count(monkeypatch, ops, "gemv_w8")
    d_new = _drift(_run_cached(qmodel, bench, B, pads, True, True), ref)
    assert new_k.n == 2 * STEPS and gemv.n == 2 * 4 * STEPS, (new_k.n, gemv.n)
    print("[media-cache] int8 mpt B4_left_padded static: decode drift bf16 re-forward %.3e, media cache %.3e (ratio %.2f)" % (d_ref, d_new, d_new / d_ref),
          flush=True)
    assert d_ref > 0 and d_new <= 2 * d_ref, (d_new, d_ref)
    del model, qmodel
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_media_cache_steps_allocate_nothing_that_grows(kind):
    """memory_allocated before and after each of 16 steps over a static KV cache and a media cache differs by no more than the logits the
    caller holds, and not at all once they are dropped.  The media cache's pointers never change."""
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache

    model, bench = _build(kind)
    P, NSTEP, B = 24, 16, 2
    vx, ids, _, _, _ = bench.synth_batch(model, B, P + NSTEP + 2, DEV, seed=7, frames=1)
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    cache, mc = StaticKVCache(n_layers, B, n_kv, hd, P + NSTEP + 2, DEV), MediaCache(B, model.media_token_id)

    def one(t):
        return model(vision_x=None, lang_x=ids[:, t:t + 1], use_cached_vision_x=True, past_key_values=cache, use_cache=True,
                     clear_conditioned_layers=False, media_cache=mc).logits

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        model(vision_x=vx.to(torch.bfloat16), lang_x=ids[:, :P], past_key_values=cache, use_cache=True, clear_conditioned_layers=False, media_cache=mc)
        ptrs, seen_ptr = mc.data_ptrs(), mc.seen.data_ptr()
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
    print("[media-cache] %s: memory_allocated growth over each of %d steps %s (logits held: %d bytes)" % (kind, NSTEP, sorted(set(deltas)), own))
    assert mc.data_ptrs() == ptrs and mc.seen.data_ptr() == seen_ptr and cache.length == P + 2 + NSTEP
    del model
    gc.collect()
    torch.cuda.empty_cache()


NEAR_TIE = 1e-4


@pytest.mark.parametrize("case", ["greedy", "beams3"])
def test_tiny_generate_with_the_media_cache_equals_the_reforward_up_to_the_first_near_tie(case):
    """Tiny MPT-host Otter in bf16 autocast: generate(cross_attention_cache=True) over the tuple and the static cache against
    generate(use_cache=False), tokens equal up to the first decoder call at which the re-forward's top-2 logit margin falls below 1e-4."""
    from oracle import synth
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
            want = model.generate(vision_x=vx, lang_x=lx, max_new_tokens=NEW, use_cache=False, eos_token_id=-1, **kw)
        finally:
            h.remove()
        got_t = model.generate(vision_x=vx, lang_x=lx, max_new_tokens=NEW, use_cache=True, cross_attention_cache=True, eos_token_id=-1, **kw)
        got_s = model.generate(vision_x=vx, lang_x=lx, max_new_tokens=NEW, cache_implementation="static", cross_attention_cache=True, eos_token_id=-1, **kw)
    cut = next((i for i, x in enumerate(margins) if x < NEAR_TIE), NEW)
    print("[media-cache] tiny generate %s: re-forward top-2 margins %s, compared %d of %d new tokens" % (case, ["%.2e" % x for x in margins], cut, NEW))
    assert got_t.shape == got_s.shape == want.shape == (lx.shape[0], 8 + NEW)
    assert torch.equal(got_t[:, :8 + cut], want[:, :8 + cut]), (got_t.tolist(), want.tolist())
    assert torch.equal(got_s[:, :8 + cut], want[:, :8 + cut]), (got_s.tolist(), want.tolist())
    assert not model.lang_encoder.is_conditioned()
