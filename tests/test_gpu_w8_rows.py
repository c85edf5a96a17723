"""GPU: one-token steps of 17 to 64 rows of the int8 decoder on otter_gemm_w8_rows (csrc/w8.hip, otter_amd/quant.py: route).

Kernel level: against the fp64 oracle of tests/test_gpu_w8.py, restated here -- the fp64 product of the operands as stored (bf16 x, integer
q, fp32 scale, the bias, GELU in fp64), every element inside the a-priori bound of an fp32 summation
    |y - ref| <= K 2^-24 (sum_k |x[m,k] q[n,k]|) scale[n]        (x 1.13, the largest slope of GELU, + 2^-22 |ref| with act = 1;
                                                                 + 2^-8 |ref| for a bf16 output),
at row counts on both sides of every 16-row block edge, with padding sentinels; run-to-run determinism; row independence (row m has the
same bits whatever M is and whatever the other rows hold).

Model level: 2-layer full-width hosts, 24 rows: the prompt pass still dequantises, every cached step runs the rows kernel once per replaced
linear, the step logits stay within twice the drift of the unquantised bf16 path (the criterion of tests/test_gpu_w8.py), OTTER_W8_ROWS=0
restores the dequantising step; a graph-replayed 24-row step equals the eager one bit for bit; generate() with 8 sentences x 3 beams."""
import copy
import gc
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(4096, 4096), (4096, 16384), (16384, 4096), (1000, 272), (1, 16), (257, 4112)]
MS = [1, 16, 17, 24, 31, 32, 33, 48, 63, 64]
MAX_M = 64


def _case(N, K, seed):
    from otter_amd.quant import quantize_weight_int8

    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)
    q, scale = quantize_weight_int8(w)
    x = torch.randn(MAX_M, K, device=DEV, generator=g).to(torch.bfloat16)
    bias = 0.05 * torch.randn(N, device=DEV, generator=g)
    return q, scale, x, bias


def _products(x, q):
    """fp64 x . q^T and |x| . |q|^T for all 64 rows, once per shape (the rows of a product do not depend on each other)."""
    xd, qd = x.double(), q.double()
    return xd @ qd.t(), xd.abs() @ qd.abs().t()


def _oracle(raw, absraw, scale, bias, act):
    """fp64 reference and the bound's sum_k |x q| scale term, from the inputs as stored."""
    sd = scale.double()
    ref, mag = raw * sd[None, :], absraw * sd[None, :]
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
def test_gemm_w8_rows_against_fp64_oracle(N, K):
    """Every (M, act, bias, output dtype, leading-dimension) combination below, every element; the worst ratio error / bound is printed."""
    from otter_amd import ops

    q, scale, x64, bias = _case(N, K, seed=N * 31 + K)
    raw, absraw = _products(x64, q)
    q_pad = torch.zeros(N, K + 32, dtype=torch.int8, device=DEV)
    q_pad[:, :K] = q
    q_pad[:, K:] = 77                                  # never read: an over-read along K changes the result
    worst = 0.0
    combos = [(0, None, torch.float32, False), (1, bias, torch.float32, True), (0, bias.to(torch.bfloat16), torch.bfloat16, True),
              (1, None, torch.bfloat16, False), (0, bias, torch.float32, False), (1, bias, torch.bfloat16, True)]
    for M in MS:
        for act, b, odt, padded in combos:
            if padded:
                x_full = torch.full((M, K + 16), 3.0, dtype=torch.bfloat16, device=DEV)
                x_full[:, :K] = x64[:M]
                y_full = torch.full((M + 2, N + 5), -7.0, dtype=odt, device=DEV)
                y = ops.gemm_w8_rows(x_full[:, :K], q_pad[:, :K], scale, b, act, out=y_full[:M, :N])
                assert y.data_ptr() == y_full.data_ptr()
                # sentinels: the padding columns and the rows from M on are untouched
                assert bool((y_full[:M, N:] == -7.0).all()) and bool((y_full[M:] == -7.0).all()), (M, act, odt)
            else:
                y = ops.gemm_w8_rows(x64[:M].contiguous(), q, scale, b, act, out_dtype=odt)
            assert y.dtype == odt and tuple(y.shape) == (M, N)
            ref, mag = _oracle(raw[:M], absraw[:M], scale, b, act)
            tol = _bound(ref, mag, K, act, odt)
            err = (y.double() - ref).abs()
            ratio = float((err / tol.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert bool((err <= tol).all()), "N=%d K=%d M=%d act=%d bias=%s out=%s padded=%s: worst error / bound = %.3f" % (
                N, K, M, act, None if b is None else b.dtype, odt, padded, ratio)
    print("[w8-rows] N=%d K=%d: worst error / bound = %.4f over %d calls" % (N, K, worst, len(MS) * len(combos)))


@pytest.mark.parametrize("N,K", [(4096, 4096), (4096, 16384), (257, 4112)])
def test_gemm_w8_rows_is_deterministic_and_row_independent(N, K):
    from otter_amd import ops

    q, scale, x64, bias = _case(N, K, seed=7)
    for act, odt in ((0, torch.float32), (1, torch.bfloat16)):
        full = ops.gemm_w8_rows(x64, q, scale, bias, act, out_dtype=odt)
        again = ops.gemm_w8_rows(x64, q, scale, bias, act, out_dtype=odt)
        assert torch.equal(full, again)
        for M in (17, 24, 33, 48):                                           # the same row in a smaller call: the same bits
            part = ops.gemm_w8_rows(x64[:M].contiguous(), q, scale, bias, act, out_dtype=odt)
            assert torch.equal(part, full[:M]), (N, K, M, act)
        other = x64.clone()                                                  # ... and beside other neighbours
        other[24:] = torch.randn(MAX_M - 24, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(99)).to(torch.bfloat16) * 5.0
        moved = ops.gemm_w8_rows(other, q, scale, bias, act, out_dtype=odt)
        assert torch.equal(moved[:24], full[:24]) and not torch.equal(moved[24:], full[24:]), (N, K, act)


# ---- model level: 24 rows ------------------------------------------------------------------------------------------------------------------

P_LEN, STEPS, B = 24, 4, 24
NAMES = ("gemv", "dequant", "rows")


class _Spies:
    """Counts the calls of ops.gemv_w8 / ops.dequant_w8 / ops.gemm_w8_rows (and keeps their order) while installed."""

    def __init__(self):
        from otter_amd import ops

        self.ops, self.now, self.order = ops, dict.fromkeys(NAMES, 0), []
        self.orig = dict(gemv=ops.gemv_w8, dequant=ops.dequant_w8, rows=ops.gemm_w8_rows)

    def _spy(self, name):
        def f(*a, **k):
            self.now[name] += 1
            self.order.append(name)
            return self.orig[name](*a, **k)
        return f

    def __enter__(self):
        self.ops.gemv_w8, self.ops.dequant_w8, self.ops.gemm_w8_rows = self._spy("gemv"), self._spy("dequant"), self._spy("rows")
        return self

    def __exit__(self, *exc):
        self.ops.gemv_w8, self.ops.dequant_w8, self.ops.gemm_w8_rows = self.orig["gemv"], self.orig["dequant"], self.orig["rows"]


def _run(model, bench, bf16, spies=None):
    """Teacher-forced prompt pass (P_LEN tokens, B sentences) + STEPS cached steps.  Returns (step logits [B, STEPS, V], calls of the
    prompt pass, calls per step)."""
    vx, ids, _, _, _ = bench.synth_batch(model, B, P_LEN + STEPS, DEV, seed=99, frames=1)
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if bf16 else torch.autocast("cuda", enabled=False)
    prefill, per_step, steps = None, [], []
    with torch.no_grad(), ctx:
        out = model(vision_x=vx.to(torch.bfloat16) if bf16 else vx, lang_x=ids[:, :P_LEN], use_cache=True, clear_conditioned_layers=False)
        if spies is not None:
            prefill = dict(spies.now)
        past = out.past_key_values
        for t in range(P_LEN, P_LEN + STEPS):
            before = dict(spies.now) if spies is not None else None
            out = model(vision_x=None, lang_x=ids[:, t:t + 1], use_cached_vision_x=True, past_key_values=past, use_cache=True,
                        clear_conditioned_layers=False)
            past = out.past_key_values
            steps.append(out.logits.float())
            if spies is not None:
                per_step.append({k: spies.now[k] - before[k] for k in before})
        model.lang_encoder.clear_conditioned_layers()
    return torch.cat(steps, dim=1), prefill, per_step


def _drift(got, ref):
    """max over positions of the row-wise relative logits error max_v |got - ref| / max_v |ref|."""
    return float(((got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)).max())


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_24_row_steps_run_the_rows_kernel_within_twice_the_bf16_drift(kind, monkeypatch):
    from otter_amd.quant import Int8FrozenLinear, dequantize_weight_int8
    from tests.test_gpu_w8 import _build

    monkeypatch.delenv("OTTER_W8_ROWS", raising=False)
    model, bench = _build(kind)
    qmodel = copy.deepcopy(model)
    n_lin = 2 * (4 if kind == "mpt" else 7)
    assert qmodel.quantize_decoder_int8()["replaced"] == n_lin
    fq = dict(model.named_modules())                    # the fake-quantised reference: the SAME q and scale, as q * scale in fp32
    with torch.no_grad():
        for name, m in qmodel.named_modules():
            if isinstance(m, Int8FrozenLinear):
                fq[name].weight.copy_(dequantize_weight_int8(m.qweight, m.scale, torch.float32))
    try:
        ref, _, _ = _run(model, bench, False)
        old, _, _ = _run(model, bench, True)
        with _Spies() as sp:
            new, prefill, per_step = _run(qmodel, bench, True, sp)
        d_ref, d_new = _drift(old, ref), _drift(new, ref)
        print("[w8-rows] %s B=%d: decode d_ref %.3e d_new %.3e" % (kind, B, d_ref, d_new), flush=True)
        # the prompt pass (576 rows) dequantises and calls neither kernel; every cached step is the rows kernel only
        assert prefill == {"gemv": 0, "dequant": n_lin, "rows": 0}, prefill
        assert len(per_step) == STEPS and all(s == {"gemv": 0, "dequant": 0, "rows": n_lin} for s in per_step), per_step
        assert d_ref > 0 and d_new <= 2 * d_ref, (kind, d_ref, d_new)

        monkeypatch.setenv("OTTER_W8_ROWS", "0")         # the switch: the same steps dequantise
        with _Spies() as sp:
            off, prefill, per_step = _run(qmodel, bench, True, sp)
        assert prefill == {"gemv": 0, "dequant": n_lin, "rows": 0}, prefill
        assert all(s == {"gemv": 0, "dequant": n_lin, "rows": 0} for s in per_step), per_step
        assert _drift(off, ref) <= 2 * d_ref
    finally:
        del model, qmodel
        gc.collect()
        torch.cuda.empty_cache()


NEW = 8


def test_graph_replayed_24_row_step_equals_the_eager_step(monkeypatch):
    """2-layer full-width MPT host, int8, static cache + cross-attention cache, 24 sentences: the logits of every step of the graph path
    (two eager warm-up steps, the captured step, the replays) are torch.equal to the eager replay-mode step over a second pair of caches
    holding the same prompt pass; one capture; the rows kernel is what the steps run."""
    from otter_amd.graph_decode import GraphDecodeStep
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache
    from tests.test_gpu_graph_decode import _twin
    from tests.test_gpu_media_cache import _build

    monkeypatch.delenv("OTTER_W8_ROWS", raising=False)
    model, bench = _build("mpt")
    assert model.quantize_decoder_int8()["replaced"] == 8
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
                assert sp.now["rows"] >= 8 * NEW and sp.now["gemv"] == sp.now["dequant"] == 0, sp.now
            finally:
                graph.release()
                eager.release()
                model.lang_encoder.clear_conditioned_layers()
    finally:
        del model
        gc.collect()
        torch.cuda.empty_cache()


def test_generate_8_sentences_3_beams_on_the_quantised_tiny_otter(monkeypatch):
    """24 rows per cached step: the tokens with and without graph_decode are the same, the rows kernel runs, and nothing dequantises once
    the prompt pass is over."""
    from oracle import synth
    from tests.test_gpu_w8 import _tiny

    monkeypatch.delenv("OTTER_W8_ROWS", raising=False)
    model, m = _tiny(DEV)
    assert model.quantize_decoder_int8()["replaced"] == 4 * 4
    vision_x, ids, _, _ = synth.tiny_batch(m["seed"], B=8)
    vx, lx = torch.from_numpy(vision_x).to(DEV).to(torch.bfloat16), torch.from_numpy(ids[:, :8]).to(DEV)
    kw = dict(max_new_tokens=8, eos_token_id=-1, num_beams=3, cache_implementation="static", cross_attention_cache=True)
    orders = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for extra in (dict(), dict(graph_decode=True)):
            with _Spies() as sp:
                orders.append((model.generate(vision_x=vx, lang_x=lx, **kw, **extra), sp.order))
    (want, o1), (got, o2) = orders
    assert got.shape == want.shape == (8, 16) and torch.equal(got, want), (got.tolist(), want.tolist())
    for order in (o1, o2):
        assert "rows" in order
        first = order.index("rows")
        assert "dequant" not in order[first:] and "gemv" not in order[first:], order
        assert order.count("rows") >= 16 * 6
    assert not model.lang_encoder.is_conditioned()
