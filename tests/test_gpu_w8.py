"""GPU: the int8 weight-only frozen decoder (csrc/w8.hip, otter_amd/quant.py).

Kernel level: otter_gemv_w8 against an fp64 oracle computed from the exact inputs (bf16 x as stored, integer q, fp32 scale, the bias, GELU
in fp64), every element inside the a-priori bound of an fp32 summation
    |y - ref| <= K 2^-24 (sum_k |x[m,k] q[n,k]|) scale[n]        (x 1.13, the largest slope of GELU, + 2^-22 |ref| with act = 1;
                                                                 + 2^-8 |ref| for a bf16 output),
padding sentinels, run-to-run determinism, otter_dequant_w8 and the GPU quantiser bit for bit.

Model level, in the bf16 production mode (bf16 autocast), on 2-layer full-width OTTER-MPT7B / OTTER-LLaMA7B shapes with oracle.synth weights:
the quantised model against the fp32 run of the fake-quantised model (the same q * scale weights in fp32) stays within twice the drift
d_ref that the EXISTING bf16 path shows against that same fp32 run -- the new path differs from the existing one only in where bf16
roundings fall.  Prefill logits and 8 cached decode steps, B = 1 and B = 4, left padding included; every cached step runs the GEMV.
The models hold fp32 masters and run under bf16 autocast (the deployed model stores its frozen weights in bf16): q * scale is not a bf16
number, and the fp32 reference, the existing bf16 path and the int8 path must all start from exactly the same weights; autocast rounds
them to bf16 per call, which is what a bf16-stored copy of them would hold."""
import copy
import gc
import math

import numpy as np
import pytest
import torch

from oracle import synth
from tests import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(12288, 4096), (4096, 4096), (16384, 4096), (4096, 16384), (22016, 4096), (4096, 11008), (1000, 272), (1, 16), (257, 4112)]
MPT_SHAPES = SHAPES[:4]
MS = [1, 2, 3, 5, 8, 13, 16]


def _case(N, K, seed):
    from otter_amd.quant import quantize_weight_int8

    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)
    q, scale = quantize_weight_int8(w)
    x = torch.randn(16, K, device=DEV, generator=g).to(torch.bfloat16)
    bias = 0.05 * torch.randn(N, device=DEV, generator=g)
    return q, scale, x, bias


def _oracle(x, q, scale, bias, act):
    """fp64 reference and the bound's sum_k |x q| scale term, from the inputs as stored."""
    xd, qd, sd = x.double(), q.double(), scale.double()
    ref = (xd @ qd.t()) * sd[None, :]
    mag = (xd.abs() @ qd.abs().t()) * sd[None, :]
    if bias is not None:
        ref = ref + bias.double()[None, :]
    if act:
        ref = 0.5 * ref * (1.0 + torch.erf(ref / math.sqrt(2.0)))
    return ref, mag


def _bound(ref, mag, K, act, out_dtype):
    tol = K * 2.0 ** -24 * mag
    if act:
        tol = 1.13 * tol + 2.0 ** -22 * ref.abs()
    if out_dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * ref.abs()
    return tol


@pytest.mark.parametrize("N,K", SHAPES)
def test_gemv_w8_against_fp64_oracle(N, K):
    """Every (M, act, bias, output dtype, leading-dimension) combination below, every element; the worst ratio error / bound is printed."""
    from otter_amd import ops

    q, scale, x16, bias = _case(N, K, seed=N * 31 + K)
    # padded operands: leading dimensions larger than the logical widths
    q_pad = torch.zeros(N, K + 32, dtype=torch.int8, device=DEV)
    q_pad[:, :K] = q
    q_pad[:, K:] = 77                                  # never read
    worst = 0.0
    combos = [(0, None, torch.float32, False), (1, bias, torch.float32, True), (0, bias.to(torch.bfloat16), torch.bfloat16, True),
              (1, None, torch.bfloat16, False), (0, bias, torch.float32, False), (1, bias, torch.bfloat16, True)]
    for M in MS:
        for act, b, odt, padded in combos:
            if padded:
                x_full = torch.full((M, K + 16), 3.0, dtype=torch.bfloat16, device=DEV)
                x_full[:, :K] = x16[:M]
                x = x_full[:, :K]
                y_full = torch.full((M + 2, N + 5), -7.0, dtype=odt, device=DEV)
                y = ops.gemv_w8(x, q_pad[:, :K], scale, b, act, out=y_full[:M, :N])
                assert y.data_ptr() == y_full.data_ptr()
                # sentinels: the padding columns and the rows from M on are untouched
                assert bool((y_full[:M, N:] == -7.0).all()) and bool((y_full[M:] == -7.0).all()), (M, act, odt)
            else:
                x = x16[:M].contiguous()
                y = ops.gemv_w8(x, q, scale, b, act, out_dtype=odt)
            assert y.dtype == odt and tuple(y.shape) == (M, N)
            ref, mag = _oracle(x, q, scale, b, act)
            tol = _bound(ref, mag, K, act, odt)
            err = (y.double() - ref).abs()
            ratio = float((err / tol.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert bool((err <= tol).all()), "N=%d K=%d M=%d act=%d bias=%s out=%s padded=%s: worst error / bound = %.3f" % (
                N, K, M, act, None if b is None else b.dtype, odt, padded, ratio)
    print("[w8] gemv N=%d K=%d: worst error / bound = %.4f over %d calls" % (N, K, worst, len(MS) * len(combos)))


@pytest.mark.parametrize("N,K", MPT_SHAPES)
def test_gemv_w8_is_deterministic(N, K):
    from otter_amd import ops

    q, scale, x16, bias = _case(N, K, seed=7)
    x = x16[:4].contiguous()
    for act, odt in ((0, torch.float32), (1, torch.bfloat16)):
        a = ops.gemv_w8(x, q, scale, bias, act, out_dtype=odt)
        b = ops.gemv_w8(x, q, scale, bias, act, out_dtype=odt)
        torch.cuda.synchronize()
        assert torch.equal(a, b)


@pytest.mark.parametrize("N,K", [(4096, 4096), (1000, 272), (1, 16), (257, 4112)])
def test_dequant_w8_is_bit_exact(N, K):
    from otter_amd import ops

    q, scale, _, _ = _case(N, K, seed=11)
    want = (q.float() * scale[:, None]).bfloat16()
    assert torch.equal(ops.dequant_w8(q, scale), want)
    q_pad = torch.zeros(N, K + 16, dtype=torch.int8, device=DEV)
    q_pad[:, :K] = q
    out_full = torch.full((N + 1, K + 8), 9.0, dtype=torch.bfloat16, device=DEV)
    ops.dequant_w8(q_pad[:, :K], scale, out=out_full[:N, :K])
    assert torch.equal(out_full[:N, :K], want) and bool((out_full[:N, K:] == 9.0).all()) and bool((out_full[N:] == 9.0).all())


def test_gpu_quantiser_equals_cpu_quantiser_bit_for_bit():
    from otter_amd.quant import quantize_weight_int8

    w = torch.randn(4096, 4096, generator=torch.Generator().manual_seed(3)) * 0.02
    scale = 2.0 ** -7
    j = torch.arange(-126, 126, dtype=torch.float32)
    w[7] = 0
    w[9, :252] = scale * (j + 0.5)                     # exact ties at scale 2^-7 ...
    w[9, 252:] = 0
    w[9, 300] = 127 * scale                            # ... which this element pins
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        wc = w.to(dt)
        qc, sc = quantize_weight_int8(wc)
        qg, sg = quantize_weight_int8(wc.to(DEV))
        assert qg.is_cuda and torch.equal(qg.cpu(), qc) and torch.equal(sg.cpu(), sc), dt
    qc, sc = quantize_weight_int8(w)
    assert float(sc[7]) == 1.0 and int(qc[7].abs().max()) == 0 and float(sc[9]) == scale
    assert torch.equal(qc[9, :252].float(), torch.round(j + 0.5))


# ---- model level ---------------------------------------------------------------------------------------------------------------------------

P_LEN, STEPS = 24, 8
BATCHES = [("B1", 1, None), ("B4", 4, None), ("B4_left_padded", 4, (0, 3, 7, 5))]


def _build(kind):
    """2-layer full-width Otter (bench.build_model's architecture), fp32 everywhere, every parameter from oracle.synth."""
    import bench

    model = bench.build_model(DEV, seed=0, debug_layers=2, config="c4" if kind == "llama" else "c2", frozen_dtype=torch.float32)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.from_numpy(synth.param_for(1234, name, tuple(p.shape))).to(DEV))
    return model.eval(), bench


def _run(model, bench, bf16, B, pads, count=None):
    """Teacher-forced prefill (P_LEN tokens) + STEPS cached decode steps.  Returns (prefill logits [B,P,V], step logits [B,STEPS,V], valid [B,P])."""
    vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN + STEPS, DEV, seed=99, frames=1)
    if pads is not None:
        for r, n in enumerate(pads):
            mask[r, :n] = 0
    am = mask if pads is not None else None
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if bf16 else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), ctx:
        v = vx.to(torch.bfloat16) if bf16 else vx
        out = model(vision_x=v, lang_x=ids[:, :P_LEN], attention_mask=None if am is None else am[:, :P_LEN], use_cache=True,
                    clear_conditioned_layers=False)
        if count is not None:
            count["prefill"] = dict(count["now"])
        past, pre, steps = out.past_key_values, out.logits.float(), []
        for t in range(P_LEN, P_LEN + STEPS):
            before = dict(count["now"]) if count is not None else None
            out = model(vision_x=None, lang_x=ids[:, t:t + 1], attention_mask=None if am is None else am[:, :t + 1], use_cached_vision_x=True,
                        past_key_values=past, use_cache=True, clear_conditioned_layers=False)
            past = out.past_key_values
            steps.append(out.logits.float())
            if count is not None:
                count.setdefault("steps", []).append({k: count["now"][k] - before[k] for k in before})
        model.lang_encoder.clear_conditioned_layers()
    return pre, torch.cat(steps, dim=1), mask[:, :P_LEN].bool()


def _drift(got, ref, valid=None):
    """max over positions of the row-wise relative logits error max_v |got - ref| / max_v |ref|."""
    e = (got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)
    if valid is not None:
        e = e[valid]
    return float(e.max())


_RESULTS = {}


def _model_level(kind):
    """Everything the model-level assertions need, computed once per host kind."""
    if kind in _RESULTS:
        return _RESULTS[kind]
    from otter_amd import ops, quant
    from otter_amd.quant import Int8FrozenLinear, dequantize_weight_int8

    model, bench = _build(kind)
    torch.cuda.synchronize()
    qmodel = copy.deepcopy(model)
    gc.collect()
    mem0 = torch.cuda.memory_allocated()
    info = qmodel.quantize_decoder_int8()
    gc.collect()
    mem1 = torch.cuda.memory_allocated()
    # the fake-quantised reference: the SAME q and scale, as q * scale in fp32
    n_fake = 0
    fq = dict(model.named_modules())
    with torch.no_grad():
        for name, m in qmodel.named_modules():
            if isinstance(m, Int8FrozenLinear):
                fq[name].weight.copy_(dequantize_weight_int8(m.qweight, m.scale, torch.float32))
                n_fake += 1
    res = dict(info=info, mem_drop=mem0 - mem1, n_fake=n_fake, drift={}, counts={})
    calls = {"gemv": 0, "dequant": 0}
    orig_gemv, orig_deq = ops.gemv_w8, ops.dequant_w8

    def gemv_spy(*a, **k):
        calls["gemv"] += 1
        return orig_gemv(*a, **k)

    def deq_spy(*a, **k):
        calls["dequant"] += 1
        return orig_deq(*a, **k)

    for tag, B, pads in BATCHES:
        ref_pre, ref_steps, valid = _run(model, bench, False, B, pads)
        old_pre, old_steps, _ = _run(model, bench, True, B, pads)
        count = {"now": calls}
        calls["gemv"] = calls["dequant"] = 0
        ops.gemv_w8, ops.dequant_w8 = gemv_spy, deq_spy
        try:
            new_pre, new_steps, _ = _run(qmodel, bench, True, B, pads, count=count)
        finally:
            ops.gemv_w8, ops.dequant_w8 = orig_gemv, orig_deq
        res["drift"][tag] = dict(d_ref_prefill=_drift(old_pre, ref_pre, valid), d_new_prefill=_drift(new_pre, ref_pre, valid),
                                 d_ref_decode=_drift(old_steps, ref_steps), d_new_decode=_drift(new_steps, ref_steps))
        res["counts"][tag] = dict(prefill=count["prefill"], steps=count["steps"])
        print("[w8] %s %s: prefill d_ref %.3e d_new %.3e | decode d_ref %.3e d_new %.3e" % (
            kind, tag, res["drift"][tag]["d_ref_prefill"], res["drift"][tag]["d_new_prefill"], res["drift"][tag]["d_ref_decode"],
            res["drift"][tag]["d_new_decode"]), flush=True)
    res["qmodel"], res["bench"], res["scratch"] = qmodel, bench, {k: v.numel() for k, v in quant._scratch.items()}
    del model
    gc.collect()
    torch.cuda.empty_cache()
    _RESULTS[kind] = res
    return res


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_quantised_model_stays_within_twice_the_existing_bf16_drift(kind):
    res = _model_level(kind)
    layers, per_layer = 2, (4 if kind == "mpt" else 7)
    assert res["info"]["replaced"] == res["n_fake"] == layers * per_layer
    for tag, _, _ in BATCHES:
        d = res["drift"][tag]
        assert d["d_ref_prefill"] > 0 and d["d_ref_decode"] > 0
        assert d["d_new_prefill"] <= 2 * d["d_ref_prefill"], (kind, tag, d)
        assert d["d_new_decode"] <= 2 * d["d_ref_decode"], (kind, tag, d)
        c = res["counts"][tag]
        # the prefill (more than 16 rows) dequantises and never calls the GEMV; every cached step is GEMVs only
        assert c["prefill"] == {"gemv": 0, "dequant": layers * per_layer}, (kind, tag, c["prefill"])
        assert len(c["steps"]) == STEPS and all(s == {"gemv": layers * per_layer, "dequant": 0} for s in c["steps"]), (kind, tag, c["steps"])


def test_memory_of_the_quantised_mpt_model():
    from otter_amd import quant

    res = _model_level("mpt")
    info = res["info"]
    want = info["bytes_before"] - info["bytes_after"]
    shapes = [(12288, 4096), (4096, 4096), (16384, 4096), (4096, 16384)]
    assert info["bytes_before"] == 2 * sum(4 * n * k for n, k in shapes) and info["bytes_after"] == 2 * sum(n * k + 4 * n for n, k in shapes)
    assert abs(res["mem_drop"] - want) <= 0.01 * want, (res["mem_drop"], want)
    # one shared dequantisation scratch, the size of the largest weight -- not one per layer or per linear
    largest = 16384 * 4096
    assert list(res["scratch"].values()) == [largest]
    qmodel, bench = res["qmodel"], res["bench"]
    quant.release_scratch()
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()

    def prefill_and_decode():
        vx, ids, _, _, _ = bench.synth_batch(qmodel, 1, 512 + STEPS, DEV, seed=5, frames=1)
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            out = qmodel(vision_x=vx.to(torch.bfloat16), lang_x=ids[:, :512], use_cache=True, clear_conditioned_layers=False)
            past = out.past_key_values
            for t in range(512, 512 + STEPS):
                out = qmodel(vision_x=None, lang_x=ids[:, t:t + 1], use_cached_vision_x=True, past_key_values=past, use_cache=True,
                             clear_conditioned_layers=False)
                past = out.past_key_values
            qmodel.lang_encoder.clear_conditioned_layers()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out, past
        gc.collect()
        return peak, torch.cuda.memory_allocated() - base

    peak1, kept1 = prefill_and_decode()         # allocates the scratch
    peak2, kept2 = prefill_and_decode()         # finds it
    slack = 32 << 20                            # kernel workspaces (ops._ws) and allocator rounding
    print("[w8] memory: drop %d (expected %d); first run peak %d kept %d, second run peak %d kept %d; scratch %d" % (
        res["mem_drop"], want, peak1, kept1, peak2, kept2, 2 * largest))
    assert {k: v.numel() for k, v in quant._scratch.items()} == {("cuda", 0): largest}
    assert 2 * largest <= kept1 <= 2 * largest + slack and abs(kept2) <= slack
    assert peak1 <= peak2 + 2 * largest + slack      # the peak above the int8 weights holds ONE scratch beyond the activations


def _tiny(device):
    from otter_amd.configuration_otter import OtterConfig
    from otter_amd.modeling_otter import OtterForConditionalGeneration

    t = synth.TINY
    text_cfg = dict(architectures=["MPTForCausalLM"], d_model=t["d_model"], n_heads=t["n_heads"], n_layers=t["n_layers"],
                    expansion_ratio=4, max_seq_len=t["max_seq_len"], vocab_size=t["vocab"], no_bias=True,
                    attn_config=dict(alibi=True, attn_impl="torch"))
    vis_cfg = dict(hidden_size=1024, intermediate_size=t["clip_inter"], num_hidden_layers=t["clip_layers"],
                   num_attention_heads=t["clip_heads"], image_size=t["image"], patch_size=t["patch"], hidden_act="quick_gelu",
                   layer_norm_eps=1e-5, projection_dim=64)
    model = OtterForConditionalGeneration(OtterConfig(vision_config=vis_cfg, text_config=text_cfg, cross_attn_every_n_layers=t["every"]))
    m = G.meta()["otter_tiny"]
    sd = synth.state_dict_for(m["seed"], {k: tuple(v) for k, v in m["state_dict_shapes"].items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.to(device).eval(), m


def _tiny_reference(new):
    """CPU, fp32: greedy ids of the fake-quantised tiny model through generate(use_cache=True) and the top-2 logit gap of every step,
    relative to the step's largest logit (the logits come from the same cached steps, replayed)."""
    from otter_amd.mpt import FrozenAwareLinear
    from otter_amd.quant import dequantize_weight_int8, quantize_weight_int8
    from tests._cpu_backend import oracle_backend

    ref, m = _tiny("cpu")
    with torch.no_grad():
        for name, mod in ref.lang_encoder.named_modules():
            if isinstance(mod, FrozenAwareLinear) and "gated_cross_attn_layer" not in name:
                mod.weight.copy_(dequantize_weight_int8(*quantize_weight_int8(mod.weight)))
    vision_x, ids, _, _ = synth.tiny_batch(m["seed"])
    vx, lx = torch.from_numpy(vision_x), torch.from_numpy(ids[:, :8])
    with torch.no_grad(), oracle_backend():
        want = ref.generate(vision_x=vx, lang_x=lx, max_new_tokens=new, use_cache=True, eos_token_id=-1)
        out = ref(vision_x=vx, lang_x=lx, use_cache=True, clear_conditioned_layers=False)
        past, steps = out.past_key_values, [out.logits[:, -1]]
        for t in range(8, 8 + new - 1):
            out = ref(vision_x=None, lang_x=want[:, t:t + 1], use_cached_vision_x=True, past_key_values=past, use_cache=True,
                      clear_conditioned_layers=False)
            past = out.past_key_values
            steps.append(out.logits[:, -1])
        ref.lang_encoder.clear_conditioned_layers()
    logits = torch.stack(steps, dim=1)                                                  # [B, new, V]
    assert torch.equal(logits.argmax(-1), want[:, 8:])
    top2 = logits.topk(2, dim=-1).values
    return want, (top2[..., 0] - top2[..., 1]) / logits.abs().amax(dim=-1), lx, vx


def test_generate_on_the_quantised_tiny_otter():
    """generate(use_cache=True, max_new_tokens=8): same shapes as the unquantised model; ids equal to the CPU fp32 fake-quantised model's
    except where that reference's top-2 logit gap (relative to its largest logit) is below the bf16 drift of the model-level leg, at most 1
    step in 8 per sample; that the reference itself has at most one such step per sample is checked first, on the CPU."""
    drift = max(max(d["d_ref_prefill"], d["d_ref_decode"]) for d in _model_level("mpt")["drift"].values())
    NEW = 8
    want, gap, lx, vx = _tiny_reference(NEW)
    B = lx.shape[0]
    close = gap < drift
    print("[w8] tiny generate: drift %.3e, reference top-2 gaps min %.3e, steps inside the drift per sample %s" % (
        drift, float(gap.min()), close.sum(1).tolist()))
    assert int(close.sum(1).max()) <= 1, (gap.tolist(), drift)

    model, _ = _tiny(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        plain = model.generate(vision_x=vx.to(DEV).to(torch.bfloat16), lang_x=lx.to(DEV), max_new_tokens=NEW, use_cache=True, eos_token_id=-1)
        assert model.quantize_decoder_int8()["replaced"] == 4 * 4
        got = model.generate(vision_x=vx.to(DEV).to(torch.bfloat16), lang_x=lx.to(DEV), max_new_tokens=NEW, use_cache=True, eos_token_id=-1)
    assert got.shape == plain.shape == want.shape == (B, 8 + NEW) and got.dtype == plain.dtype
    got = got.cpu()
    assert torch.equal(got[:, :8], lx)
    for r in range(B):
        excused = 0
        for t in range(NEW):
            if got[r, 8 + t] != want[r, 8 + t]:
                assert bool(close[r, t]), "sample %d step %d: ids differ (%d vs %d) at a top-2 gap of %.3e >= drift %.3e" % (
                    r, t, int(got[r, 8 + t]), int(want[r, 8 + t]), float(gap[r, t]), drift)
                excused += 1
                break                                 # later steps are conditioned on another prefix
        assert excused <= 1
