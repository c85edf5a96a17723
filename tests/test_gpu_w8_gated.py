"""GPU: the gated-residual tail of the int8 products (otter_gemv_w8_gated / otter_gemm_w8_rows_gated, csrc/w8.hip) and the hosts that use it
(quantize_decoder_int8(gated_blocks=True, lm_head=True)).

Kernel level.  y = v s + R with v = (x . q) scale (+ bias) and s = tanh(gate) (1 without a gate), against the fp64 value of the same
expression from the inputs as stored; every element inside

    |y - ref| <= |s| K 2^-24 mag  +  2^-21 |s v|  +  2^-23 (|s v| + |ref|)      (+ 2^-8 |ref| for a bf16 y),      mag = sum_k |x q| scale

-- the fp32 summation bound of tests/test_gpu_w8.py scaled by the gate, 4 ulp for the device tanhf (2^-21 = 4 x 2^-23), one rounding each
for the multiply and the add whether the compiler fuses them or not, and the output rounding.  The (N, K) are the smallest that reach each
branch of the split rules of w8.hip:

    (48, 64)         GEMV S = 1                                       rows S = 1
    (40, 2048)       GEMV S = 2, N no multiple of 16                  rows S = 4
    (17, 8192)       GEMV S = 8
    (16400, 64)      GEMV two row tiles per workgroup, S = 1
    (4096, 16384)    GEMV S = 2 (the product it is built for)         rows S = 8

Exact cases (small integers, power-of-two scales: every fp32 sum is exact), guard frames around x, q, R and y, run-to-run equality and the
rows kernel's row independence.

Host level.  2-layer full-width MPT and LLaMA hosts with a gated block in front of each layer, quantised with both keywords, against the
fp32 run of the fake-quantised twin (the same q * scale in its weights; MPT's lookup keeps the original table, as in the product): twice the
existing bf16 path's drift, the rule of tests/test_gpu_w8.py; which entries a cached step calls; graph replay; a tiny generate()."""
import copy
import gc
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GEMV_SHAPES = [(48, 64), (40, 2048), (17, 8192), (16400, 64), (4096, 16384)]
ROWS_SHAPES = [(48, 64), (40, 2048), (4096, 16384)]
GEMV_MS, ROWS_MS = [1, 3, 16], [1, 17, 24, 64]
GATES = [0.7, -3.0, None]
ENTRIES = [("gemv_w8_gated", N, K) for N, K in GEMV_SHAPES] + [("gemm_w8_rows_gated", N, K) for N, K in ROWS_SHAPES]

_CASES = {}


def _case(N, K):
    """Operands and the fp64 products for all 64 rows, once per shape and shared (read-only) by every test of that shape."""
    if (N, K) in _CASES:
        return _CASES[(N, K)]
    from otter_amd.quant import quantize_weight_int8

    g = torch.Generator(device=DEV).manual_seed(N * 31 + K)
    q, scale = quantize_weight_int8(torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K))
    x = torch.randn(64, K, device=DEV, generator=g).to(torch.bfloat16)
    bias = 0.05 * torch.randn(N, device=DEV, generator=g)
    R = torch.randn(64, N, device=DEV, generator=g)
    xd, qd = x.double(), q.double()
    c = dict(q=q, scale=scale, x=x, bias=bias, R=R, raw=(xd @ qd.t()) * scale.double()[None, :],
             mag=(xd.abs() @ qd.abs().t()) * scale.double()[None, :])
    _CASES[(N, K)] = c
    return c


def _padded(t, pad_rows, pad_cols, fill):
    """t as the top-left block of a larger tensor full of `fill`: (view, frame)."""
    frame = torch.full((t.shape[0] + pad_rows, t.shape[1] + pad_cols), fill, dtype=t.dtype, device=t.device)
    frame[:t.shape[0], :t.shape[1]] = t
    return frame[:t.shape[0], :t.shape[1]], frame


@pytest.mark.parametrize("entry,N,K", ENTRIES)
def test_gated_tail_against_the_fp64_oracle(entry, N, K):
    """gate 0.7 / -3 / none x R bf16 / fp32 x y bf16 / fp32 x bias on / off at every M, every element; every other call runs on padded
    operands (x, q, R, y inside frames of sentinels: an over-read changes the result, an over-write changes a sentinel)."""
    from otter_amd import ops

    c, op = _case(N, K), getattr(ops, entry)
    q_pad, _ = _padded(c["q"], 0, 32, 77)
    worst, n_calls = 0.0, 0
    for M in (GEMV_MS if entry == "gemv_w8_gated" else ROWS_MS):
        for gate in GATES:
            s = math.tanh(gate) if gate is not None else 1.0
            gt = torch.tensor([gate], dtype=torch.float32, device=DEV) if gate is not None else None
            for rdt in (torch.bfloat16, torch.float32):
                R = c["R"][:M].to(rdt).contiguous()
                for odt in (torch.bfloat16, torch.float32):
                    for bias in (None, c["bias"]):
                        padded = n_calls % 2 == 1
                        n_calls += 1
                        if padded:
                            x, _ = _padded(c["x"][:M], 0, 16, 3.0)
                            Rv, _ = _padded(R, 1, 3, 1e4)
                            y_view, y_frame = _padded(torch.zeros(M, N, dtype=odt, device=DEV), 2, 5, -7.0)
                            y = op(x, q_pad, c["scale"], gt, Rv, bias, out=y_view)
                            assert y.data_ptr() == y_frame.data_ptr()
                            assert bool((y_frame[:M, N:] == -7.0).all()) and bool((y_frame[M:] == -7.0).all()), (M, gate, rdt, odt)
                        else:
                            y = op(c["x"][:M].contiguous(), c["q"], c["scale"], gt, R, bias, out_dtype=odt)
                        assert y.dtype == odt and tuple(y.shape) == (M, N)
                        v = c["raw"][:M] + (bias.double()[None, :] if bias is not None else 0.0)
                        ref = s * v + R.double()
                        sv = (s * v).abs()
                        tol = abs(s) * K * 2.0 ** -24 * c["mag"][:M] + 2.0 ** -21 * sv + 2.0 ** -23 * (sv + ref.abs())
                        if odt == torch.bfloat16:
                            tol = tol + 2.0 ** -8 * ref.abs()
                        err = (y.double() - ref).abs()
                        ratio = float((err / tol.clamp_min(1e-300)).max())
                        worst = max(worst, ratio)
                        assert bool((err <= tol).all()), "%s N=%d K=%d M=%d gate=%s R=%s y=%s bias=%s padded=%s: worst error / bound = %.3f" % (
                            entry, N, K, M, gate, rdt, odt, bias is not None, padded, ratio)
    print("[w8-gated] %s N=%d K=%d: worst error / bound = %.4f over %d calls" % (entry, N, K, worst, n_calls))


@pytest.mark.parametrize("entry,N,K", ENTRIES)
def test_exact_cases(entry, N, K):
    """Small integers and power-of-two scales, so that every sum is exact in fp32 (|x . q| <= 3 x 127 K < 2^24 up to K = 16384): without a
    gate y == R + v exactly; with a gate of 0.0 -- an untrained block -- y has R's bits, rounded to y's dtype."""
    from otter_amd import ops

    op = getattr(ops, entry)
    M = 16 if entry == "gemv_w8_gated" else 24
    g = torch.Generator(device=DEV).manual_seed(5)
    q = torch.randint(-127, 128, (N, K), device=DEV, generator=g).to(torch.int8)
    x = torch.randint(-3, 4, (M, K), device=DEV, generator=g).to(torch.bfloat16)
    scale = torch.full((N,), 2.0 ** -7, device=DEV)
    scale[::3] = 2.0 ** -5
    bias = torch.randint(-40, 41, (N,), device=DEV, generator=g).float() / 8
    v = (x.double() @ q.double().t()) * scale.double()[None, :] + bias.double()[None, :]
    assert float(v.abs().max()) * 2 ** 7 < 2 ** 24
    R_int = torch.randint(-64, 65, (M, N), device=DEV, generator=g).float() / 4
    R_any = torch.randn(M, N, device=DEV, generator=g)
    zero = torch.zeros(1, device=DEV)
    for rdt in (torch.float32, torch.bfloat16):
        R = R_int.to(rdt)                                        # (multiples of 1/4 up to 16: exact in bf16 as well)
        want = (v + R.double()).float()
        assert torch.equal(want.double(), v + R.double())        # the expected value is an fp32 number: nothing for the kernel to round
        assert torch.equal(op(x, q, scale, None, R, bias, out_dtype=torch.float32), want), (entry, N, K, rdt)
        assert torch.equal(op(x, q, scale, None, R, bias, out_dtype=torch.bfloat16), want.to(torch.bfloat16)), (entry, N, K, rdt)
        R = R_any.to(rdt)
        for odt in (torch.float32, torch.bfloat16):
            assert torch.equal(op(x, q, scale, zero, R, bias, out_dtype=odt), R.to(odt)), (entry, N, K, rdt, odt)


@pytest.mark.parametrize("entry,N,K", ENTRIES)
def test_two_calls_give_the_same_bits(entry, N, K):
    from otter_amd import ops

    c, op = _case(N, K), getattr(ops, entry)
    M = 16 if entry == "gemv_w8_gated" else 64
    gt = torch.tensor([0.7], device=DEV)
    for odt in (torch.float32, torch.bfloat16):
        a = op(c["x"][:M], c["q"], c["scale"], gt, c["R"][:M], c["bias"], out_dtype=odt)
        b = op(c["x"][:M], c["q"], c["scale"], gt, c["R"][:M], c["bias"], out_dtype=odt)
        assert torch.equal(a, b)


@pytest.mark.parametrize("N,K", ROWS_SHAPES)
def test_rows_entry_is_row_independent(N, K):
    """Row m of y has the same bits for M = 17 and M = 64, and with the other rows of x and R replaced."""
    from otter_amd import ops

    c = _case(N, K)
    gt = torch.tensor([-3.0], device=DEV)
    for odt in (torch.float32, torch.bfloat16):
        full = ops.gemm_w8_rows_gated(c["x"], c["q"], c["scale"], gt, c["R"], c["bias"], out_dtype=odt)
        part = ops.gemm_w8_rows_gated(c["x"][:17], c["q"], c["scale"], gt, c["R"][:17], c["bias"], out_dtype=odt)
        assert torch.equal(part, full[:17]), (N, K, odt)
        g = torch.Generator(device=DEV).manual_seed(99)
        x2, R2 = c["x"].clone(), c["R"].clone()
        x2[17:] = (5.0 * torch.randn(64 - 17, K, device=DEV, generator=g)).to(torch.bfloat16)
        R2[17:] = torch.randn(64 - 17, N, device=DEV, generator=g)
        moved = ops.gemm_w8_rows_gated(x2, c["q"], c["scale"], gt, R2, c["bias"], out_dtype=odt)
        assert torch.equal(moved[:17], full[:17]) and not torch.equal(moved[17:], full[17:]), (N, K, odt)


def test_wrapper_refuses_aliased_and_misshapen_operands():
    from otter_amd import ops
    from otter_amd._capi import OtterHipError

    c = _case(48, 64)
    x, R = c["x"][:4].contiguous(), c["R"][:4].contiguous()
    with pytest.raises(OtterHipError, match="overlap"):
        ops.gemv_w8_gated(x, c["q"], c["scale"], None, R, out=R)
    with pytest.raises(OtterHipError, match="R must be"):
        ops.gemv_w8_gated(x, c["q"], c["scale"], None, c["R"][:5])
    with pytest.raises(OtterHipError, match="gate must be"):
        ops.gemv_w8_gated(x, c["q"], c["scale"], torch.zeros(2, device=DEV), R)
    with pytest.raises(OtterHipError, match="1 <= M <= 16"):
        ops.gemv_w8_gated(c["x"][:17], c["q"], c["scale"], None, c["R"][:17])


# ---- hosts ---------------------------------------------------------------------------------------------------------------------------------

P_LEN, STEPS = 24, 8
NAMES = ("gemv", "gemv_gated", "rows", "rows_gated", "dequant", "gemm_nt", "linear")


class _Spies:
    """Counts, while installed, the calls of the four int8 products, of ops.dequant_w8, of the project's GEMM (ops.gemm_nt: what the
    unquantised gated block runs) and of torch.nn.functional.linear (the library GEMM behind nn.Linear, the dequantising route and the
    unquantised un-embedding)."""

    def __init__(self):
        from otter_amd import ops

        F = torch.nn.functional
        self.where = dict(gemv=(ops, "gemv_w8"), gemv_gated=(ops, "gemv_w8_gated"), rows=(ops, "gemm_w8_rows"),
                          rows_gated=(ops, "gemm_w8_rows_gated"), dequant=(ops, "dequant_w8"), gemm_nt=(ops, "gemm_nt"), linear=(F, "linear"))
        self.orig = {k: getattr(m, n) for k, (m, n) in self.where.items()}
        self.now = dict.fromkeys(NAMES, 0)

    def _spy(self, name):
        def f(*a, **k):
            self.now[name] += 1
            return self.orig[name](*a, **k)
        return f

    def __enter__(self):
        for k, (m, n) in self.where.items():
            setattr(m, n, self._spy(k))
        return self

    def __exit__(self, *exc):
        for k, (m, n) in self.where.items():
            setattr(m, n, self.orig[k])


def _pair(kind):
    """(fake-quantised twin in fp32, quantised model, bench): the twin holds the same q * scale in its weights, gated FFNs and un-embedding
    included.  MPT's table is tied: the twin un-embeds with q * scale and keeps looking tokens up in the original table, as the product does."""
    from otter_amd.quant import Int8FrozenLinear, Int8Unembedding, dequantize_weight_int8
    from tests.test_gpu_media_cache import _build

    model, bench = _build(kind)
    qmodel = copy.deepcopy(model)
    info = qmodel.quantize_decoder_int8(gated_blocks=True, lm_head=True)
    per_layer = 4 if kind == "mpt" else 7
    assert info["replaced"] == 2 * per_layer + 2 * 2 + 1, info
    twin = dict(model.named_modules())
    with torch.no_grad():
        for name, m in qmodel.named_modules():
            if not isinstance(m, Int8FrozenLinear):
                continue
            w = dequantize_weight_int8(m.qweight, m.scale, torch.float32)
            if isinstance(m, Int8Unembedding) and name.endswith("wte.unembed_int8"):
                wte = twin[name[:-len(".unembed_int8")]]
                lookup = wte.forward
                wte.forward = lambda input, unembed=False, _w=w, _f=lookup: (
                    torch.nn.functional.linear(input, _w.to(input.dtype)) if unembed else _f(input))
            else:
                twin[name].weight.copy_(w)
    return model, qmodel, bench


def _reference(model, bench, B, pads):
    """fp32 run of the twin: the prompt pass's logits [B, P, V] and, per step, the last position of the full re-forward [B, STEPS, V]
    (what a cached step over a media cache computes: tests/test_gpu_media_cache.py)."""
    from tests.test_gpu_media_cache import _batch, _ctx, _run_full

    vx, ids, am = _batch(model, bench, B, pads)
    with torch.no_grad(), _ctx(False):
        prompt = model(vision_x=vx, lang_x=ids[:, :P_LEN], attention_mask=None if am is None else am[:, :P_LEN], use_cache=False).logits.float()
    valid = am[:, :P_LEN].bool() if am is not None else torch.ones(B, P_LEN, dtype=torch.bool, device=DEV)
    return prompt, _run_full(model, bench, False, B, pads), valid


def _prompt_and_steps(model, bench, B, pads, spies=None):
    """bf16: teacher-forced prompt pass + STEPS cached steps over a static KV cache and a media cache (the path generate() takes with
    cache_implementation="static", cross_attention_cache=True): (prompt logits [B, P, V], step logits [B, STEPS, V], calls per step)."""
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache
    from tests.test_gpu_media_cache import _batch, _ctx

    vx, ids, am = _batch(model, bench, B, pads)
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    steps, per_step = [], []
    with torch.no_grad(), _ctx(True):
        past, mc = StaticKVCache(n_layers, B, n_kv, hd, P_LEN + STEPS, DEV), MediaCache(B, model.media_token_id)
        out = model(vision_x=vx.to(torch.bfloat16), lang_x=ids[:, :P_LEN], attention_mask=None if am is None else am[:, :P_LEN],
                    past_key_values=past, use_cache=True, clear_conditioned_layers=False, media_cache=mc)
        prompt = out.logits.float()
        for t in range(P_LEN, P_LEN + STEPS):
            before = dict(spies.now) if spies is not None else None
            out = model(vision_x=None, lang_x=ids[:, t:t + 1], attention_mask=None if am is None else am[:, :t + 1], use_cached_vision_x=True,
                        past_key_values=out.past_key_values, use_cache=True, clear_conditioned_layers=False, media_cache=mc)
            steps.append(out.logits.float())
            if spies is not None:
                per_step.append({k: spies.now[k] - before[k] for k in before})
        model.lang_encoder.clear_conditioned_layers()
    return prompt, torch.cat(steps, dim=1), per_step


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_quantised_hosts_stay_within_twice_the_bf16_drift_and_call_only_the_int8_entries(kind, monkeypatch):
    from tests.test_gpu_w8 import _drift

    monkeypatch.delenv("OTTER_W8_ROWS", raising=False)
    model, qmodel, bench = _pair(kind)
    n_dec, n_blocks = 2 * (4 if kind == "mpt" else 7), 2
    try:
        for tag, B, pads in [("B1", 1, None), ("B4_left_padded", 4, (0, 3, 7, 5))]:
            ref_p, ref_s, valid = _reference(model, bench, B, pads)
            old_p, old_s, _ = _prompt_and_steps(model, bench, B, pads)
            with _Spies() as sp:
                new_p, new_s, per_step = _prompt_and_steps(qmodel, bench, B, pads, sp)
            d = dict(ref_prompt=_drift(old_p, ref_p, valid), new_prompt=_drift(new_p, ref_p, valid), ref_steps=_drift(old_s, ref_s),
                     new_steps=_drift(new_s, ref_s))
            print("[w8-gated] %s %s: prompt d_ref %.3e d_new %.3e | steps d_ref %.3e d_new %.3e" % (
                kind, tag, d["ref_prompt"], d["new_prompt"], d["ref_steps"], d["new_steps"]), flush=True)
            # every cached step: the decoder's linears, each block's first FFN product and the un-embedding on the GEMV, each block's second
            # FFN product on the gated GEMV; what is left on the project's GEMM is to_q and to_out; nothing dequantises, no library GEMM
            want = dict(gemv=n_dec + n_blocks + 1, gemv_gated=n_blocks, rows=0, rows_gated=0, dequant=0, gemm_nt=2 * n_blocks, linear=0)
            assert len(per_step) == STEPS and all(s == want for s in per_step), (kind, tag, per_step[0], want)
            assert d["ref_prompt"] > 0 and d["ref_steps"] > 0
            assert d["new_prompt"] <= 2 * d["ref_prompt"], (kind, tag, d)
            assert d["new_steps"] <= 2 * d["ref_steps"], (kind, tag, d)
        # 24 rows: the same chain on the rows entries (the un-embedding included: one slice of at most 64 rows)
        with _Spies() as sp:
            _, _, per_step = _prompt_and_steps(qmodel, bench, 24, None, sp)
        want = dict(gemv=0, gemv_gated=0, rows=n_dec + n_blocks + 1, rows_gated=n_blocks, dequant=0, gemm_nt=2 * n_blocks, linear=0)
        assert all(s == want for s in per_step), (kind, per_step[0], want)
    finally:
        del model, qmodel
        gc.collect()
        torch.cuda.empty_cache()


NEW = 8


@pytest.mark.parametrize("B", [4, 24])
def test_graph_replayed_step_equals_the_eager_step(B, monkeypatch):
    """MPT host, both keywords, static cache + cross-attention cache: the logits of every step of the graph path (two eager warm-up steps,
    the captured step, the replays) are torch.equal to the eager replay-mode step over a second pair of caches holding the same prompt pass;
    one capture and NEW - 3 replays, as without the keywords (tests/test_gpu_w8_rows.py)."""
    from otter_amd.graph_decode import GraphDecodeStep
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache
    from tests.test_gpu_graph_decode import _twin
    from tests.test_gpu_media_cache import _build

    monkeypatch.delenv("OTTER_W8_ROWS", raising=False)
    model, bench = _build("mpt")
    assert model.quantize_decoder_int8(gated_blocks=True, lm_head=True)["replaced"] == 8 + 4 + 1
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN + NEW, DEV, seed=99, frames=1)
            n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
            cache, mc = StaticKVCache(n_layers, B, n_kv, hd, P_LEN + NEW, DEV), MediaCache(B, model.media_token_id)
            out = model(vision_x=vx.to(torch.bfloat16), lang_x=ids[:, :P_LEN], attention_mask=mask[:, :P_LEN], past_key_values=cache,
                        use_cache=True, clear_conditioned_layers=False, media_cache=mc)
            c2, m2 = _twin(cache, mc)
            cache.enable_replay(mask[:, :P_LEN])
            c2.enable_replay(mask[:, :P_LEN])
            graph, eager = GraphDecodeStep(model.lang_encoder, cache, mc), GraphDecodeStep(model.lang_encoder, c2, m2)
            assert graph.use_graph
            eager.use_graph = False
            try:
                nxt = out.logits[:, -1].float().argmax(-1)
                with _Spies() as sp:
                    for t in range(NEW - 1):
                        lg = graph(nxt[:, None]).clone()
                        le = eager(nxt[:, None])
                        assert torch.equal(lg, le), (t, float((lg.float() - le.float()).abs().max()))
                        nxt = lg.float().argmax(-1)
                assert (graph.captures, graph.replays) == (1, NEW - 1 - 2) and (eager.captures, eager.replays) == (0, 0)
                gated = "gemv_gated" if B <= 16 else "rows_gated"
                assert sp.now[gated] >= 2 * NEW and sp.now["dequant"] == sp.now["linear"] == 0, sp.now
            finally:
                graph.release()
                eager.release()
                model.lang_encoder.clear_conditioned_layers()
    finally:
        del model
        gc.collect()
        torch.cuda.empty_cache()


def test_tiny_generate_with_every_keyword_returns_the_eager_tokens(monkeypatch):
    """8 sentences x 3 beams on the tiny MPT Otter with both keywords, static int8 KV cache, cross-attention cache and a shared prompt:
    graph_decode=True returns the tokens of the same call without it; the gated entries run and nothing dequantises after the prompt pass."""
    from oracle import synth
    from otter_amd.quant import Int8FrozenLinear
    from tests.test_gpu_w8 import _tiny

    monkeypatch.delenv("OTTER_W8_ROWS", raising=False)
    model, m = _tiny(DEV)
    n_blocks = sum(1 for l in model.lang_encoder._get_decoder_layers() if l.gated_cross_attn_layer is not None)
    assert model.quantize_decoder_int8(gated_blocks=True, lm_head=True)["replaced"] == 4 * 4 + 2 * n_blocks + 1
    assert all(isinstance(l.gated_cross_attn_layer.feed_forward[3], Int8FrozenLinear)
               for l in model.lang_encoder._get_decoder_layers() if l.gated_cross_attn_layer is not None)
    vision_x, ids, _, _ = synth.tiny_batch(m["seed"], B=8)
    vx, lx = torch.from_numpy(vision_x).to(DEV).to(torch.bfloat16), torch.from_numpy(ids[:, :8]).to(DEV)
    kw = dict(max_new_tokens=8, eos_token_id=-1, num_beams=3, cache_implementation="static", cross_attention_cache=True, kv_cache_dtype="int8",
              share_prompt=True)
    got = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for extra in (dict(), dict(graph_decode=True)):
            with _Spies() as sp:
                got.append(model.generate(vision_x=vx, lang_x=lx, **kw, **extra))
            assert sp.now["rows_gated"] >= n_blocks * 6 and sp.now["rows"] >= (4 * 4 + n_blocks + 1) * 6, sp.now
    assert got[0].shape == got[1].shape == (8, 16) and torch.equal(got[0], got[1]), (got[0].tolist(), got[1].tolist())
    assert not model.lang_encoder.is_conditioned()
