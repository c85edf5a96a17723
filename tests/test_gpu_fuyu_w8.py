"""GPU: the int8 weight-only decoder on the OtterHD / Fuyu host (csrc/w8.hip epilogue code 3, otter_amd/quant.py, otter_amd/fuyu.py).

Kernel level.  otter_gemv_w8 and otter_gemm_w8_rows with act = 3 (y = relu(v)^2, v = sum * scale + bias) against an fp64 oracle computed from
the inputs as stored, every element.  With v_ref the fp64 pre-activation, mag = (|x| . |q|^T) scale and delta = K 2^-24 mag (the
project's a-priori bound of the fp32 summation for act = 0, tests/test_gpu_w8.py), relu is 1-Lipschitz, so |relu(v) - r| <= delta for
r = relu(v_ref) and
    |y - r^2| <= delta (2 r + delta) + 2^-22 r^2        (+ 2^-8 r^2 for a bf16 output)
-- derived, not tuned.  The un-embedding of Fuyu-8B is the first caller with N = 262144: grid and index arithmetic at that width are
checked once at K = 64 (act = 0, the existing bound), where the operands stay at 16 MB.

Model level, on a 2-layer full-width Persimmon (hidden 4096, 64 heads, FFN 16384, rotary 32; vocabulary 8192) holding fp32 masters under
bf16 autocast, by the scheme of tests/test_gpu_w8.py: the int8 model's logits (c) against the fp32 run of the fake-quantised model (a)
stay within twice the distance of the existing bf16 HIP path (b) from that same run, per pass and per cached step; routing, the shared
scratch and generate() end to end on the bf16-stored form of the quantised model."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(16384, 4096), (4096, 4096), (1000, 272), (257, 4112), (1, 16)]
GEMV_MS = [1, 3, 16]
ROWS_MS = [17, 24, 33, 64]


def _case(N, K, seed, rows=64):
    from otter_amd.quant import quantize_weight_int8

    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)
    q, scale = quantize_weight_int8(w)
    x = torch.randn(rows, K, device=DEV, generator=g).to(torch.bfloat16)
    bias = 0.05 * torch.randn(N, device=DEV, generator=g)
    return q, scale, x, bias


class _Oracle:
    """fp64 pre-activation sum and magnitude term of all 64 x rows against one weight, computed once per shape."""

    def __init__(self, x, q, scale):
        xd, qd, sd = x.double(), q.double(), scale.double()
        self.v = (xd @ qd.t()) * sd[None, :]
        self.mag = (xd.abs() @ qd.abs().t()) * sd[None, :]

    def sqrelu(self, M, bias, K, out_dtype):
        v = self.v[:M] if bias is None else self.v[:M] + bias.double()[None, :]
        r = v.clamp_min(0.0)
        delta = K * 2.0 ** -24 * self.mag[:M]
        tol = delta * (2.0 * r + delta) + 2.0 ** -22 * r * r
        if out_dtype == torch.bfloat16:
            tol = tol + 2.0 ** -8 * r * r
        return r * r, tol

    def plain(self, M, K):
        return self.v[:M], K * 2.0 ** -24 * self.mag[:M]


# (bias, output dtype, padded leading dimension with sentinels)
def _combos(bias):
    return [(bias, torch.float32, False), (bias.to(torch.bfloat16), torch.bfloat16, False), (None, torch.float32, False),
            (bias, torch.bfloat16, True)]


@pytest.mark.parametrize("N,K", SHAPES)
def test_sqrelu_epilogue_against_fp64_oracle(N, K):
    """act = 3 in both kernels: (16384, 4096) is Fuyu's dense_h_to_4h (GEMV: two rows per workgroup, split 1; rows: split 1),
    (4096, 4096) has a K split > 1 in both, so the epilogue runs in the reduce kernel; the rest are ragged edges."""
    from otter_amd import ops

    q, scale, x64, bias = _case(N, K, seed=N * 31 + K + 3)
    orc = _Oracle(x64, q, scale)
    worst = {"gemv": 0.0, "rows": 0.0}
    calls = 0
    for kind, product, ms in (("gemv", ops.gemv_w8, GEMV_MS), ("rows", ops.gemm_w8_rows, ROWS_MS)):
        for M in ms:
            for b, odt, padded in _combos(bias):
                if padded:
                    x_full = torch.full((M, K + 16), 3.0, dtype=torch.bfloat16, device=DEV)
                    x_full[:, :K] = x64[:M]
                    y_full = torch.full((M + 2, N + 5), -7.0, dtype=odt, device=DEV)
                    y = product(x_full[:, :K], q, scale, b, 3, out=y_full[:M, :N])
                    assert y.data_ptr() == y_full.data_ptr()
                    assert bool((y_full[:M, N:] == -7.0).all()) and bool((y_full[M:] == -7.0).all()), (kind, M, odt)
                else:
                    y = product(x64[:M].contiguous(), q, scale, b, 3, out_dtype=odt)
                assert y.dtype == odt and tuple(y.shape) == (M, N)
                ref, tol = orc.sqrelu(M, b, K, odt)
                err = (y.double() - ref).abs()
                ratio = float((err / tol.clamp_min(1e-300)).max())
                worst[kind] = max(worst[kind], ratio)
                calls += 1
                assert bool((y >= 0).all()) and (M * N < 64 or bool((ref > 0).any()))
                assert bool((err <= tol).all()), "%s N=%d K=%d M=%d bias=%s out=%s padded=%s: worst error / bound = %.3f" % (
                    kind, N, K, M, None if b is None else b.dtype, odt, padded, ratio)
    print("[fuyu-w8] act=3 N=%d K=%d: worst error / bound gemv %.4f rows %.4f over %d calls" % (N, K, worst["gemv"], worst["rows"], calls))


@pytest.mark.parametrize("N,K", [(16384, 4096), (4096, 4096)])
def test_rows_invariance_and_determinism_with_sqrelu(N, K):
    from otter_amd import ops

    q, scale, x64, bias = _case(N, K, seed=17)
    for odt in (torch.float32, torch.bfloat16):
        y64 = ops.gemm_w8_rows(x64, q, scale, bias, 3, out_dtype=odt)
        y17 = ops.gemm_w8_rows(x64[:17].contiguous(), q, scale, bias, 3, out_dtype=odt)
        assert torch.equal(y64[:17], y17)
        # the same rows in other places among other neighbours
        x17 = torch.randn(17, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)).to(torch.bfloat16)
        x17[5], x17[16] = x64[40], x64[63]
        z17 = ops.gemm_w8_rows(x17, q, scale, bias, 3, out_dtype=odt)
        assert torch.equal(z17[5], y64[40]) and torch.equal(z17[16], y64[63])
        assert torch.equal(ops.gemm_w8_rows(x64, q, scale, bias, 3, out_dtype=odt), y64)
        g = ops.gemv_w8(x64[:16].contiguous(), q, scale, bias, 3, out_dtype=odt)
        assert torch.equal(ops.gemv_w8(x64[:16].contiguous(), q, scale, bias, 3, out_dtype=odt), g)
    assert float(y64.float().abs().max()) > 0


def test_unembedding_width():
    """N = 262144 (Fuyu-8B's vocabulary): one workgroup per 16 / 32 / 64 output columns, 64-bit element offsets, the padded tail of y."""
    from otter_amd import ops

    N, K = 262144, 64
    q, scale, x64, _ = _case(N, K, seed=23, rows=24)
    orc = _Oracle(x64, q, scale)
    for product, M in ((ops.gemv_w8, 1), (ops.gemv_w8, 16), (ops.gemm_w8_rows, 24)):
        y_full = torch.full((M + 1, N + 8), -7.0, dtype=torch.float32, device=DEV)
        y = product(x64[:M].contiguous(), q, scale, None, 0, out=y_full[:M, :N])
        ref, tol = orc.plain(M, K)
        err = (y.double() - ref).abs()
        ratio = float((err / tol.clamp_min(1e-300)).max())
        print("[fuyu-w8] N=262144 K=64 M=%d: worst error / bound = %.4f" % (M, ratio))
        assert bool((err <= tol).all()), (M, ratio)
        assert bool((y_full[:M, N:] == -7.0).all()) and bool((y_full[M:] == -7.0).all()), M
        assert float(y[:, N - 64:].abs().max()) > 0


# ---- model level ---------------------------------------------------------------------------------------------------------------------------

LAYERS, VOCAB, P_LEN, STEPS = 2, 8192, 40, 8
BATCHES = [("B1", 1, None), ("B4_left_padded", 4, (0, 5, 0, 0))]
_STATE = {}


def _models():
    """(fake-quantised fp32 model, int8 model with fp32 masters, quantisation report), built once."""
    if "models" in _STATE:
        return _STATE["models"]
    from transformers import PersimmonConfig

    from otter_amd.fuyu import PersimmonForCausalLM
    from otter_amd.quant import Int8FrozenLinear, dequantize_weight_int8

    cfg = PersimmonConfig(vocab_size=VOCAB, hidden_size=4096, intermediate_size=16384, num_hidden_layers=LAYERS, num_attention_heads=64,
                          max_position_embeddings=4096, qk_layernorm=True, partial_rotary_factor=0.5, hidden_act="relu2", layer_norm_eps=1e-5,
                          rope_theta=25000.0, tie_word_embeddings=False, use_cache=True)
    torch.manual_seed(0)
    with torch.device(DEV):
        model = PersimmonForCausalLM(cfg)
    g = torch.Generator(device=DEV).manual_seed(1)
    with torch.no_grad():
        for name, p in model.named_parameters():          # the default init leaves every bias 0 and every LayerNorm at (1, 0)
            if name.endswith("bias"):
                p.copy_(0.02 * torch.randn(p.shape, device=DEV, generator=g))
            elif "layernorm" in name:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, device=DEV, generator=g))
    model.eval()
    qmodel = copy.deepcopy(model)
    info = qmodel.quantize_decoder_int8()
    fq = dict(model.named_modules())
    n = 0
    with torch.no_grad():
        for name, m in qmodel.named_modules():
            if isinstance(m, Int8FrozenLinear):
                fq[name].weight.copy_(dequantize_weight_int8(m.qweight, m.scale, torch.float32))
                assert torch.equal(fq[name].bias, m.bias) if m.bias is not None else fq[name].bias is None
                n += 1
    assert n == info["replaced"] == 4 * LAYERS + 1
    _STATE["models"] = (model, qmodel, info)
    return _STATE["models"]


def _qmodel_bf16():
    """The deployed form: the int8 model with everything else stored in bf16 (scales stay fp32)."""
    if "q16" not in _STATE:
        _STATE["q16"] = copy.deepcopy(_models()[1]).to(torch.bfloat16).eval()
    return _STATE["q16"]


def _inputs(B, pads, length):
    g = torch.Generator(device=DEV).manual_seed(99 + B)
    ids = torch.randint(3, VOCAB, (B, length), device=DEV, generator=g)
    mask = torch.ones(B, length, dtype=torch.long, device=DEV)
    if pads is not None:
        for r, n in enumerate(pads):
            mask[r, :n] = 0
    return ids, mask


def _run(model, bf16, B, pads):
    """Prompt pass (P_LEN tokens) + STEPS teacher-forced cached steps: (prompt logits [B,P,V], step logits [B,STEPS,V], valid [B,P])."""
    ids, mask = _inputs(B, pads, P_LEN + STEPS)
    am = mask if pads is not None else None
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if bf16 else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), ctx:
        out = model(input_ids=ids[:, :P_LEN], attention_mask=None if am is None else am[:, :P_LEN], use_cache=True)
        past, pre, steps = out.past_key_values, out.logits.float(), []
        for t in range(P_LEN, P_LEN + STEPS):
            out = model(input_ids=ids[:, t:t + 1], attention_mask=None if am is None else am[:, :t + 1], past_key_values=past, use_cache=True)
            past = out.past_key_values
            steps.append(out.logits.float())
    return pre, torch.cat(steps, dim=1), mask[:, :P_LEN].bool()


def test_int8_model_stays_within_twice_the_existing_bf16_drift():
    """max |c - a| <= 2 max |b - a| for the prompt pass and for each of the 8 cached steps (a: fp32 run of the fake-quantised model,
    b: the existing bf16 HIP path on it, c: the int8 model)."""
    from otter_amd import ops

    model, qmodel, info = _models()
    shapes = [(12288, 4096), (4096, 4096), (16384, 4096), (4096, 16384)]
    assert info["bytes_before"] == LAYERS * sum(4 * n * k + 4 * n for n, k in shapes) + 4 * VOCAB * 4096
    assert info["bytes_after"] == LAYERS * sum(n * k + 8 * n for n, k in shapes) + VOCAB * 4096 + 4 * VOCAB
    fused = {"n": 0}
    real = ops.persimmon_decode_attn

    def spy(*a, **k):
        fused["n"] += 1
        return real(*a, **k)

    for tag, B, pads in BATCHES:
        a_pre, a_steps, valid = _run(model, False, B, pads)
        b_pre, b_steps, _ = _run(model, True, B, pads)
        ops.persimmon_decode_attn = spy
        try:
            c_pre, c_steps, _ = _run(qmodel, True, B, pads)
        finally:
            ops.persimmon_decode_attn = real
        assert fused["n"] == LAYERS * STEPS                     # every cached step of the int8 model ran the fused decode kernel
        fused["n"] = 0
        assert c_pre.shape == a_pre.shape == (B, P_LEN, VOCAB) and c_steps.shape == (B, STEPS, VOCAB)
        d_b, d_c = float((b_pre - a_pre)[valid].abs().max()), float((c_pre - a_pre)[valid].abs().max())
        print("[fuyu-w8] %s prompt: max|b-a| %.4e max|c-a| %.4e ratio %.3f (max|a| %.3f)" % (tag, d_b, d_c, d_c / d_b, float(a_pre[valid].abs().max())))
        assert d_b > 0 and d_c <= 2 * d_b, (tag, "prompt", d_c, d_b)
        ratios = []
        for s in range(STEPS):
            d_b, d_c = float((b_steps[:, s] - a_steps[:, s]).abs().max()), float((c_steps[:, s] - a_steps[:, s]).abs().max())
            ratios.append(d_c / d_b)
            assert d_b > 0 and d_c <= 2 * d_b, (tag, "step %d" % s, d_c, d_b)
        print("[fuyu-w8] %s steps: max|c-a| / max|b-a| = %s" % (tag, " ".join("%.3f" % r for r in ratios)))


class _Spies:
    """Counts ops.gemv_w8 / gemm_w8_rows / dequant_w8 calls, one record per forward of `model` (the pattern of tests/test_gpu_w8_rows.py)."""

    NAMES = ("gemv_w8", "gemm_w8_rows", "dequant_w8")

    def __init__(self, model):
        self.model, self.now, self.passes = model, dict.fromkeys(self.NAMES, 0), []

    def __enter__(self):
        from otter_amd import ops

        self.real = {n: getattr(ops, n) for n in self.NAMES}
        for n in self.NAMES:
            setattr(ops, n, self._wrap(n))
        fwd = self.model.forward

        def forward(*a, **k):
            before = dict(self.now)
            out = fwd(*a, **k)
            self.passes.append({n: self.now[n] - before[n] for n in self.NAMES})
            return out

        self.model.forward = forward
        return self

    def _wrap(self, n):
        def f(*a, **k):
            self.now[n] += 1
            return self.real[n](*a, **k)
        return f

    def __exit__(self, *exc):
        from otter_amd import ops

        for n in self.NAMES:
            setattr(ops, n, self.real[n])
        del self.model.forward


def test_routing_over_the_whole_model():
    from otter_amd import quant

    qm = _qmodel_bf16()
    per = 4 * LAYERS
    quant.release_scratch()
    NEW = 4
    ids, _ = _inputs(2, None, P_LEN)
    with _Spies(qm) as sp:
        out = qm.generate(ids, max_new_tokens=NEW, eos_token_id=-1)
    assert out.shape == (2, P_LEN + NEW) and len(sp.passes) == NEW
    # the prompt pass (80 rows) dequantises the decoder's linears; the un-embedding sees the last position only: a 2-row GEMV
    assert sp.passes[0] == {"gemv_w8": 1, "gemm_w8_rows": 0, "dequant_w8": per}, sp.passes[0]
    assert all(p == {"gemv_w8": per + 1, "gemm_w8_rows": 0, "dequant_w8": 0} for p in sp.passes[1:]), sp.passes
    ids, _ = _inputs(8, None, P_LEN)
    with _Spies(qm) as sp:
        out = qm.generate(ids, max_new_tokens=NEW, num_beams=3, eos_token_id=-1)
    assert out.shape == (8, P_LEN + NEW) and len(sp.passes) == NEW
    # 8 sentences x 3 beams = 24 rows: the last-position un-embedding of the prompt pass is a one-token product of 24 rows
    assert sp.passes[0] == {"gemv_w8": 0, "gemm_w8_rows": 1, "dequant_w8": per}, sp.passes[0]
    assert all(p == {"gemv_w8": 0, "gemm_w8_rows": per + 1, "dequant_w8": 0} for p in sp.passes[1:]), sp.passes
    assert 0 < sum(b.numel() for b in quant._scratch.values()) <= 16384 * 4096


@pytest.mark.parametrize("mode", ["greedy", "beams", "sampling"])
def test_generate_end_to_end(mode, monkeypatch):
    from otter_amd import ops

    qm = _qmodel_bf16()
    NEW, B = 5, 3
    ids, mask = _inputs(B, (0, 4, 0), P_LEN)
    kw = dict(greedy={}, beams=dict(num_beams=3), sampling=dict(do_sample=True, top_k=50, generator=torch.Generator(device=DEV).manual_seed(7)))[mode]
    fused = {"n": 0}
    real = ops.persimmon_decode_attn

    def spy(*a, **k):
        fused["n"] += 1
        return real(*a, **k)

    monkeypatch.setattr(ops, "persimmon_decode_attn", spy)
    out = qm.generate(ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=-1, **kw)
    assert out.shape == (B, P_LEN + NEW) and out.dtype == ids.dtype and torch.equal(out[:, :P_LEN], ids)
    assert bool(((out[:, P_LEN:] >= 0) & (out[:, P_LEN:] < VOCAB)).all())
    assert fused["n"] == LAYERS * (NEW - 1)                      # the fused decode kernel on every cached step
    if mode == "greedy":
        fused["n"] = 0
        monkeypatch.setenv("OTTER_FUYU_HIP_DECODE", "0")
        plain = qm.generate(ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=-1)
        assert fused["n"] == 0 and plain.shape == out.shape and torch.equal(plain[:, :P_LEN], ids)
        assert bool(((plain[:, P_LEN:] >= 0) & (plain[:, P_LEN:] < VOCAB)).all())
