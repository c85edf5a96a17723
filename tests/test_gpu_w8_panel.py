"""GPU: one-token steps of 65 to 256 rows of the int8 decoder on otter_gemm_w8_panel / otter_gemm_w8_panel_gated (csrc/w8_panel.hip,
otter_amd/quant.py: route, `quantize_decoder_int8(wide_steps=True)`).

Kernel level, at M in {1, 17, 64, 65, 80, 129, 255, 256} (one row past the rows kernel's range, a partly filled 16-row block, both ends),
N in {16, 72, 128, 136, 1000} (below a workgroup's 128 columns, no multiple of 16, exact, one tile over) and K in {16, 144, 272, 512, 4096}
(a single 16-wide step, this kernel's 128-wide chunk plus one step, the rows kernel's chunk plus one step, the smallest K that this
kernel splits at N = 128 -- SPLIT_K below, from the kernel's rule --, and a long one that splits eight ways):

  * exact: integers in x and q, power-of-two scales, an integer bias, fp32 y -- every partial sum is exact in fp32, so the result must EQUAL
    the integer oracle: a lost or doubled K step, a wrong tile or a wrong row moves an integer;
  * random operands against the fp64 oracle on the operands as stored, every element inside the a-priori bounds the existing tests derive for
    the same arithmetic: tests/test_gpu_w8_rows.py (act 0 / 1), tests/test_gpu_fuyu_w8.py (act 3), tests/test_gpu_w8_gated.py (the gated tail);
  * row independence, bit for bit: row m alone, inside M = 65 and inside M = 256 at another index, the other rows random or NaN;
  * frames: sentinels around y, NaN rows behind x, ldx > K, ldw > K;  two calls give the same bits;  the existing entries are untouched.

Model level: 2-layer full-width MPT, LLaMA and Persimmon hosts at 72 rows (24 sentences x 3 beams)."""
import copy
import gc
import hashlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MS = [1, 17, 64, 65, 80, 129, 255, 256]
NS = [16, 72, 128, 136, 1000]
MAX_M = 256


def _split(N, K):
    """The kernel's split rule (csrc/w8_panel.hip: gemm_w8_panel_run): S doubles while the grid stays within 256 workgroups of 128 columns,
    S < 8 and every range keeps 256 K elements."""
    base, S = (N + 127) // 128, 1
    while base * 2 * S <= 256 and S < 8 and K // (2 * S) >= 256:
        S *= 2
    return S


SPLIT_K = next(K for K in range(16, 8192, 16) if _split(128, K) > 1)          # the smallest K that splits at N = 128
KS = [16, 144, 272, SPLIT_K, 4096]


def test_the_split_rule_restated_here_gives_the_documented_points():
    assert SPLIT_K == 512 and _split(128, 496) == 1 and _split(128, 512) == 2
    assert [_split(128, K) for K in KS] == [1, 1, 1, 2, 8] and _split(1000, 4096) == 8 and _split(136, 272) == 1
    assert (_split(4096, 4096), _split(12288, 4096), _split(16384, 4096), _split(4096, 16384), _split(50432, 4096)) == (8, 2, 2, 8, 1)


# ---- exact ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_exact_integer_cases_equal_the_integer_oracle(K):
    """|x| <= 4, |q| <= 31, scale in {1/4, 1/2, 1, 2}, bias and R integers: 4 y is an integer below 4 * (4 * 31 * 4096 * 2 + 72) < 2^23, so
    every partial sum, the scaled sum, the biased sum and the residual sum are exact in fp32 whatever the order."""
    from otter_amd import ops

    g = torch.Generator(device=DEV).manual_seed(1000 + K)
    zero = torch.zeros(1, device=DEV)
    for N in NS:
        q = torch.randint(-31, 32, (N, K), device=DEV, generator=g).to(torch.int8)
        x = torch.randint(-4, 5, (MAX_M, K), device=DEV, generator=g).to(torch.bfloat16)
        scale = (2.0 ** torch.randint(-2, 2, (N,), device=DEV, generator=g).float()).contiguous()
        bias = torch.randint(-8, 9, (N,), device=DEV, generator=g).float()
        R = torch.randint(-64, 65, (MAX_M, N), device=DEV, generator=g).float()
        sums = (x.double() @ q.double().t()).to(torch.int64)                  # integers below 2^53: the fp64 product is exact
        v4 = sums * (4 * scale).to(torch.int64)[None, :] + (4 * bias).to(torch.int64)[None, :]
        assert int(v4.abs().max()) + 4 * 64 < 2 ** 23
        for M in MS:
            y = ops.gemm_w8_panel(x[:M], q, scale, bias, 0, out_dtype=torch.float32)
            assert torch.equal((4 * y.double()).to(torch.int64), v4[:M]) and torch.equal(y.double() * 4, v4[:M].double()), (N, K, M, "plain")
            y = ops.gemm_w8_panel_gated(x[:M], q, scale, None, R[:M], bias, out_dtype=torch.float32)       # no gate: y = v + R
            assert torch.equal(y.double() * 4, (v4[:M] + 4 * R[:M].to(torch.int64)).double()), (N, K, M, "gated, no gate")
            y = ops.gemm_w8_panel_gated(x[:M], q, scale, zero, R[:M], bias, out_dtype=torch.float32)       # a gate of 0: y has R's bits
            assert torch.equal(y, R[:M]), (N, K, M, "gated, gate 0")


# ---- random operands against the fp64 oracle -------------------------------------------------------------------------------------------------

_CASES = {}


def _case(N, K):
    """Operands and the fp64 products for all 256 rows, once per shape and shared (read-only) by every test of that shape."""
    if (N, K) not in _CASES:
        from otter_amd.quant import quantize_weight_int8

        g = torch.Generator(device=DEV).manual_seed(N * 31 + K)
        q, scale = quantize_weight_int8(torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K))
        x = torch.randn(MAX_M, K, device=DEV, generator=g).to(torch.bfloat16)
        bias = 0.05 * torch.randn(N, device=DEV, generator=g)
        R = torch.randn(MAX_M, N, device=DEV, generator=g)
        xd, qd, sd = x.double(), q.double(), scale.double()
        _CASES[(N, K)] = dict(q=q, scale=scale, x=x, bias=bias, R=R, raw=(xd @ qd.t()) * sd[None, :], mag=(xd.abs() @ qd.abs().t()) * sd[None, :])
    return _CASES[(N, K)]


def _plain_ref(c, M, K, bias, act, odt):
    """(fp64 reference, bound): act 0 / 1 as tests/test_gpu_w8_rows.py, act 3 as tests/test_gpu_fuyu_w8.py."""
    v = c["raw"][:M] + (bias.double()[None, :] if bias is not None else 0.0)
    delta = K * 2.0 ** -24 * c["mag"][:M]
    if act == 3:
        r = v.clamp_min(0.0)
        ref, tol = r * r, delta * (2.0 * r + delta) + 2.0 ** -22 * r * r
    elif act == 1:
        ref = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
        tol = 1.13 * delta + 2.0 ** -22 * ref.abs()
    else:
        ref, tol = v, delta
    return ref, tol + (2.0 ** -8 * ref.abs() if odt == torch.bfloat16 else 0.0)


def _gated_ref(c, M, K, bias, gate, R, odt):
    """(fp64 reference, bound) of tests/test_gpu_w8_gated.py."""
    s = math.tanh(gate) if gate is not None else 1.0
    v = c["raw"][:M] + (bias.double()[None, :] if bias is not None else 0.0)
    ref, sv = s * v + R.double(), (s * v).abs()
    tol = abs(s) * K * 2.0 ** -24 * c["mag"][:M] + 2.0 ** -21 * sv + 2.0 ** -23 * (sv + ref.abs())
    return ref, tol + (2.0 ** -8 * ref.abs() if odt == torch.bfloat16 else 0.0)


def _ratio(y, ref, tol, what):
    err = (y.double() - ref).abs()
    ratio = float((err / tol.clamp_min(1e-300)).max())
    assert bool((err <= tol).all()), "%s: worst error / bound = %.3f" % (what, ratio)
    return ratio


# (act, bias dtype or None, output dtype) of the plain entry; (gate, R dtype, bias dtype or None, output dtype) of the gated one
PLAIN = [(0, None, torch.float32), (1, torch.float32, torch.float32), (3, torch.bfloat16, torch.bfloat16), (1, None, torch.bfloat16),
         (3, torch.float32, torch.float32), (0, torch.bfloat16, torch.bfloat16)]
GATED = [(0.7, torch.bfloat16, None, torch.bfloat16), (-3.0, torch.float32, torch.float32, torch.float32), (None, torch.bfloat16, torch.bfloat16,
         torch.float32), (0.7, torch.float32, None, torch.bfloat16)]
BIG = [(4096, 4096), (12288, 4096)]                     # two of the MPT-7B linears: full grids, S = 8 and S = 2


@pytest.mark.parametrize("N,K", [(N, K) for K in KS for N in NS] + BIG)
def test_random_operands_against_the_fp64_oracle(N, K):
    from otter_amd import ops

    c, worst, n = _case(N, K), 0.0, 0
    for M in (MS if (N, K) not in BIG else [72, 256]):
        for act, bdt, odt in PLAIN:
            bias = None if bdt is None else c["bias"].to(bdt)
            y = ops.gemm_w8_panel(c["x"][:M], c["q"], c["scale"], bias, act, out_dtype=odt)
            assert y.dtype == odt and tuple(y.shape) == (M, N)
            ref, tol = _plain_ref(c, M, K, bias, act, odt)
            worst = max(worst, _ratio(y, ref, tol, "N=%d K=%d M=%d act=%d bias=%s y=%s" % (N, K, M, act, bdt, odt)))
        for gate, rdt, bdt, odt in GATED:
            bias = None if bdt is None else c["bias"].to(bdt)
            R = c["R"][:M].to(rdt)
            gt = None if gate is None else torch.tensor([gate], dtype=torch.float32, device=DEV)
            y = ops.gemm_w8_panel_gated(c["x"][:M], c["q"], c["scale"], gt, R, bias, out_dtype=odt)
            ref, tol = _gated_ref(c, M, K, bias, gate, R, odt)
            worst = max(worst, _ratio(y, ref, tol, "gated N=%d K=%d M=%d gate=%s R=%s bias=%s y=%s" % (N, K, M, gate, rdt, bdt, odt)))
        n += len(PLAIN) + len(GATED)
    print("[w8-panel] N=%d K=%d (S=%d): worst error / bound = %.4f over %d calls" % (N, K, _split(N, K), worst, n))


# ---- row independence, determinism, frames -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K", [(136, 272), (136, 4096), (4096, 4096)], ids=["unsplit", "split8_two_panels", "split8_full_grid"])
@pytest.mark.parametrize("others", ["random", "nan"])
def test_a_row_has_the_same_bits_alone_in_65_rows_and_in_256_rows(N, K, others):
    """Row 5 of the case computed alone (M = 1), as row 64 of M = 65 and as row 201 of M = 256, the other rows random or all NaN (x, and R
    of the gated entry): the three results are bit-equal, and no NaN reaches the row."""
    from otter_amd import ops

    c = _case(N, K)
    assert _split(N, K) == (1 if K == 272 else 8)
    g = torch.Generator(device=DEV).manual_seed(7)
    gt = torch.tensor([0.7], device=DEV)
    row, Rrow = c["x"][5:6].contiguous(), c["R"][5:6].contiguous()

    def batch(M, at):
        if others == "nan":
            x, R = torch.full((M, K), float("nan"), dtype=torch.bfloat16, device=DEV), torch.full((M, N), float("nan"), device=DEV)
        else:
            x, R = (3.0 * torch.randn(M, K, device=DEV, generator=g)).to(torch.bfloat16), torch.randn(M, N, device=DEV, generator=g)
        x[at], R[at] = row[0], Rrow[0]
        return x, R

    for act, odt in ((0, torch.float32), (1, torch.bfloat16), (3, torch.float32)):
        alone = ops.gemm_w8_panel(row, c["q"], c["scale"], c["bias"], act, out_dtype=odt)
        assert bool(torch.isfinite(alone.float()).all())
        for M, at in ((65, 64), (256, 201)):
            x, _ = batch(M, at)
            y = ops.gemm_w8_panel(x, c["q"], c["scale"], c["bias"], act, out_dtype=odt)
            assert torch.equal(y[at], alone[0]), (N, K, others, act, M, at)
            if others == "nan" and act == 0:
                assert bool(torch.isnan(y[:at].float()).all())               # (the other rows are what their inputs make them)
    for odt in (torch.float32, torch.bfloat16):
        alone = ops.gemm_w8_panel_gated(row, c["q"], c["scale"], gt, Rrow, c["bias"], out_dtype=odt)
        assert bool(torch.isfinite(alone.float()).all())
        for M, at in ((65, 64), (256, 201)):
            x, R = batch(M, at)
            y = ops.gemm_w8_panel_gated(x, c["q"], c["scale"], gt, R, c["bias"], out_dtype=odt)
            assert torch.equal(y[at], alone[0]), (N, K, others, "gated", odt, M, at)


@pytest.mark.parametrize("N,K", [(136, 272), (1000, 4096), (12288, 4096)])
def test_two_calls_give_the_same_bits_and_smaller_calls_are_prefixes(N, K):
    from otter_amd import ops

    c = _case(N, K)
    gt = torch.tensor([-3.0], device=DEV)
    for odt in (torch.float32, torch.bfloat16):
        full = ops.gemm_w8_panel(c["x"], c["q"], c["scale"], c["bias"], 1, out_dtype=odt)
        assert torch.equal(full, ops.gemm_w8_panel(c["x"], c["q"], c["scale"], c["bias"], 1, out_dtype=odt))
        gfull = ops.gemm_w8_panel_gated(c["x"], c["q"], c["scale"], gt, c["R"], c["bias"], out_dtype=odt)
        assert torch.equal(gfull, ops.gemm_w8_panel_gated(c["x"], c["q"], c["scale"], gt, c["R"], c["bias"], out_dtype=odt))
        for M in (1, 65, 72, 80, 96, 129, 192):                               # every instantiated block count
            assert torch.equal(ops.gemm_w8_panel(c["x"][:M], c["q"], c["scale"], c["bias"], 1, out_dtype=odt), full[:M]), (N, K, M, odt)
            assert torch.equal(ops.gemm_w8_panel_gated(c["x"][:M], c["q"], c["scale"], gt, c["R"][:M], c["bias"], out_dtype=odt), gfull[:M])


@pytest.mark.parametrize("N,K", [(72, 144), (136, SPLIT_K), (1000, 4096)])
def test_frames_around_every_operand(N, K):
    """y with ldy > N inside a frame of sentinels (columns beyond N and rows beyond M untouched); x the first M rows of a larger buffer whose
    other rows and whose columns beyond K hold NaN (ldx > K); q with ldw > K and 77 beyond K; R inside a frame of 1e4.  No NaN reaches y and
    every element stays inside the oracle's bound."""
    from otter_amd import ops

    c = _case(N, K)
    q_frame = torch.full((N, K + 32), 77, dtype=torch.int8, device=DEV)
    q_frame[:, :K] = c["q"]
    gt = torch.tensor([0.7], device=DEV)
    for M in (65, 80, 255):
        x_frame = torch.full((MAX_M + 3, K + 16), float("nan"), dtype=torch.bfloat16, device=DEV)
        x_frame[:M, :K] = c["x"][:M]
        for odt in (torch.float32, torch.bfloat16):
            y_frame = torch.full((M + 2, N + 5), -7.0, dtype=odt, device=DEV)
            y = ops.gemm_w8_panel(x_frame[:M, :K], q_frame[:, :K], c["scale"], c["bias"], 0, out=y_frame[:M, :N])
            assert y.data_ptr() == y_frame.data_ptr()
            assert bool((y_frame[:M, N:] == -7.0).all()) and bool((y_frame[M:] == -7.0).all()), (N, K, M, odt)
            assert not bool(torch.isnan(y.float()).any())
            _ratio(y, *_plain_ref(c, M, K, c["bias"], 0, odt), "framed N=%d K=%d M=%d y=%s" % (N, K, M, odt))
            R_frame = torch.full((M + 1, N + 3), 1e4, device=DEV)
            R_frame[:M, :N] = c["R"][:M]
            y_frame.fill_(-7.0)
            y = ops.gemm_w8_panel_gated(x_frame[:M, :K], q_frame[:, :K], c["scale"], gt, R_frame[:M, :N], None, out=y_frame[:M, :N])
            assert bool((y_frame[:M, N:] == -7.0).all()) and bool((y_frame[M:] == -7.0).all()), (N, K, M, odt, "gated")
            _ratio(y, *_gated_ref(c, M, K, None, 0.7, c["R"][:M], odt), "framed gated N=%d K=%d M=%d y=%s" % (N, K, M, odt))


def test_wrapper_refuses_what_the_entries_cannot_take():
    from otter_amd import ops
    from otter_amd._capi import OtterHipError

    c = _case(136, 272)
    with pytest.raises(OtterHipError, match="1 <= M <= 256"):
        ops.gemm_w8_panel(torch.zeros(257, 272, dtype=torch.bfloat16, device=DEV), c["q"], c["scale"])
    with pytest.raises(OtterHipError, match="1 <= M <= 256"):
        ops.gemm_w8_panel_gated(torch.zeros(257, 272, dtype=torch.bfloat16, device=DEV), c["q"], c["scale"], None, torch.zeros(257, 136, device=DEV))
    R = c["R"][:72].contiguous()
    with pytest.raises(OtterHipError, match="overlap"):
        ops.gemm_w8_panel_gated(c["x"][:72], c["q"], c["scale"], None, R, out=R)
    with pytest.raises(OtterHipError, match="x must be bf16"):
        ops.gemm_w8_panel(c["x"][:72].float(), c["q"], c["scale"])


# the sha256 below was recorded with the library built from the parent commit (before csrc/w8_panel.hip existed) on an MI355X
EXISTING_ENTRIES_SHA256 = "94cf929529b487d9a721f51c1d2d12ed62927d631965d402f8a4af0d029e29a4"


def existing_entries_digest():
    """sha256 over the outputs of the entries that were there before the panel kernel -- otter_gemv_w8, otter_gemm_w8_rows, their gated forms,
    otter_dequant_w8 -- on seeded inputs: three shapes that reach every split branch, every act code, both output dtypes, bias on and off."""
    from otter_amd import ops
    from otter_amd.quant import quantize_weight_int8

    h = hashlib.sha256()
    put = lambda t: h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    for N, K in [(4096, 4096), (1000, 2048), (16400, 64)]:
        g = torch.Generator(device=DEV).manual_seed(N + K)
        q, scale = quantize_weight_int8(torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K))
        x = torch.randn(64, K, device=DEV, generator=g).to(torch.bfloat16)
        bias, R = 0.05 * torch.randn(N, device=DEV, generator=g), torch.randn(64, N, device=DEV, generator=g)
        gt = torch.tensor([0.7], device=DEV)
        put(ops.dequant_w8(q, scale))
        for odt in (torch.float32, torch.bfloat16):
            for b in (None, bias):
                for act in (0, 1, 3):
                    for M in (1, 16):
                        put(ops.gemv_w8(x[:M], q, scale, b, act, out_dtype=odt))
                    for M in (17, 64):
                        put(ops.gemm_w8_rows(x[:M], q, scale, b, act, out_dtype=odt))
                put(ops.gemv_w8_gated(x[:16], q, scale, gt, R[:16], b, out_dtype=odt))
                put(ops.gemm_w8_rows_gated(x[:48], q, scale, gt, R[:48], b, out_dtype=odt))
    return h.hexdigest()


def test_the_existing_entries_give_the_bits_they_gave_before_the_panel_kernel():
    assert existing_entries_digest() == EXISTING_ENTRIES_SHA256


# ---- model level: 72 rows ----------------------------------------------------------------------------------------------------------------------

ROWS = 72                                       # 24 sentences x 3 beams
NAMES = ("gemv", "gemv_gated", "rows", "rows_gated", "panel", "panel_gated", "dequant", "gemm_nt", "linear")


class _Spies:
    """Counts, while installed, the calls of the six int8 products, of ops.dequant_w8, of the project's GEMM (ops.gemm_nt: to_q and to_out of
    a gated block) and of torch.nn.functional.linear (the library GEMM behind the dequantising route): tests/test_gpu_w8_gated.py's, with the
    panel pair."""

    def __init__(self):
        from otter_amd import ops

        F = torch.nn.functional
        self.where = dict(gemv=(ops, "gemv_w8"), gemv_gated=(ops, "gemv_w8_gated"), rows=(ops, "gemm_w8_rows"), rows_gated=(ops, "gemm_w8_rows_gated"),
                          panel=(ops, "gemm_w8_panel"), panel_gated=(ops, "gemm_w8_panel_gated"), dequant=(ops, "dequant_w8"),
                          gemm_nt=(ops, "gemm_nt"), linear=(F, "linear"))
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


def _counted_steps(model, bench, spies):
    """tests/test_gpu_w8_gated.py's prompt pass + cached steps over a static KV cache and a media cache at 72 rows, with this file's spies:
    (prompt logits, step logits, calls of the prompt pass, calls per step)."""
    from tests import test_gpu_w8_gated as G

    before = dict(spies.now)
    prompt, steps, per_step = G._prompt_and_steps(model, bench, ROWS, None, spies)
    total = {k: spies.now[k] - before[k] for k in before}
    pre = {k: total[k] - sum(s[k] for s in per_step) for k in total}
    return prompt, steps, pre, per_step


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_72_row_steps_run_the_panel_kernel_within_twice_the_bf16_drift(kind, monkeypatch):
    """2-layer full-width host, a gated block per layer, `quantize_decoder_int8(gated_blocks=True, lm_head=True, wide_steps=True)`, static +
    cross-attention cache.  The prompt pass dequantises as before; every cached step runs the panel entry once per replaced linear and
    nothing else of the int8 family; the step logits stay within twice the unquantised bf16 path's distance from the fp32 run of the
    fake-quantised twin; without the keyword the same model runs exactly the parent's calls."""
    from otter_amd.quant import PANEL_MAX_ROWS
    from tests import test_gpu_w8_gated as G
    from tests.test_gpu_w8 import _drift

    monkeypatch.delenv("OTTER_W8_ROWS", raising=False)
    monkeypatch.delenv("OTTER_W8_PANEL", raising=False)
    assert ROWS <= PANEL_MAX_ROWS
    model, qmodel, bench = G._pair(kind)
    n_dec, n_blocks = 2 * (4 if kind == "mpt" else 7), 2
    try:
        ref_p, ref_s, valid = G._reference(model, bench, ROWS, None)
        _, old_s, _ = G._prompt_and_steps(model, bench, ROWS, None)
        with _Spies() as sp:                                                   # without the keyword: the parent's calls
            _, off_s, off_pre, off_steps = _counted_steps(qmodel, bench, sp)
        assert all(s["panel"] == s["panel_gated"] == 0 and s["dequant"] == n_dec + 2 * n_blocks for s in off_steps), off_steps[0]
        assert all(s == off_steps[0] for s in off_steps)

        zero = {"replaced": 0, "bytes_before": 0, "bytes_after": 0}
        assert qmodel.quantize_decoder_int8(gated_blocks=True, lm_head=True, wide_steps=True) == zero       # a later call switches it on
        with _Spies() as sp:
            new_p, new_s, pre, per_step = _counted_steps(qmodel, bench, sp)
        # the prompt pass (72 x 24 rows, many tokens per row): the decoder and the gated FFNs dequantise as before; only the un-embedding,
        # which never dequantises, takes its slices through the panel entry instead of the rows entry
        assert pre["dequant"] == off_pre["dequant"] == n_dec + 2 * n_blocks and pre["rows"] == pre["rows_gated"] == pre["panel_gated"] == 0, pre
        assert pre["panel"] == math.ceil(ROWS * G.P_LEN / PANEL_MAX_ROWS) and off_pre["rows"] == math.ceil(ROWS * G.P_LEN / 64), (pre, off_pre)
        want = dict(gemv=0, gemv_gated=0, rows=0, rows_gated=0, panel=n_dec + n_blocks + 1, panel_gated=n_blocks, dequant=0, gemm_nt=2 * n_blocks,
                    linear=0)
        assert len(per_step) == G.STEPS and all(s == want for s in per_step), (kind, per_step[0], want)
        d_ref, d_new, d_off = _drift(old_s, ref_s), _drift(new_s, ref_s), _drift(off_s, ref_s)
        print("[w8-panel] %s %d rows: steps d_ref %.3e d_new %.3e (ratio %.3f) dequantising route %.3e (ratio %.3f)" % (
            kind, ROWS, d_ref, d_new, d_new / d_ref, d_off, d_off / d_ref), flush=True)
        assert d_ref > 0 and d_new <= 2 * d_ref, (kind, d_ref, d_new)

        monkeypatch.setenv("OTTER_W8_PANEL", "0")                              # the switch: the same steps dequantise again
        with _Spies() as sp:
            _, _, _, per_step = _counted_steps(qmodel, bench, sp)
        assert all(s == off_steps[0] for s in per_step), (per_step[0], off_steps[0])
    finally:
        del model, qmodel
        gc.collect()
        torch.cuda.empty_cache()


NEW = 6


def test_graph_replayed_72_row_step_equals_the_eager_step(monkeypatch):
    """MPT host, every keyword, static cache + cross-attention cache, 72 rows: the logits of every step of the graph path (two eager warm-up
    steps, the captured step, the replays) are torch.equal to the eager replay-mode step over a second pair of caches holding the same prompt
    pass; one capture; the panel entries are what the steps run."""
    from otter_amd.graph_decode import GraphDecodeStep
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache
    from tests.test_gpu_graph_decode import _twin
    from tests.test_gpu_media_cache import _build

    monkeypatch.delenv("OTTER_W8_PANEL", raising=False)
    P_LEN = 24
    model, bench = _build("mpt")
    assert model.quantize_decoder_int8(gated_blocks=True, lm_head=True, wide_steps=True)["replaced"] == 8 + 4 + 1
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            vx, ids, mask, _, _ = bench.synth_batch(model, ROWS, P_LEN + NEW, DEV, seed=99, frames=1)
            n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
            cache, mc = StaticKVCache(n_layers, ROWS, n_kv, hd, P_LEN + NEW, DEV), MediaCache(ROWS, model.media_token_id)
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
                assert sp.now["panel_gated"] >= 2 * NEW and sp.now["panel"] >= 11 * NEW, sp.now
                assert sp.now["dequant"] == sp.now["linear"] == sp.now["rows"] == sp.now["rows_gated"] == 0, sp.now
            finally:
                graph.release()
                eager.release()
                model.lang_encoder.clear_conditioned_layers()
    finally:
        del model
        gc.collect()
        torch.cuda.empty_cache()


def test_72_row_steps_of_a_persimmon_host_run_the_panel_kernel_with_the_squared_relu(monkeypatch):
    """The 2-layer full-width Persimmon of tests/test_gpu_fuyu_w8.py (act 3 in dense_h_to_4h, biases everywhere) at 72 rows: every cached step
    runs the panel entry once per replaced linear, the un-embedding included, and stays within twice the bf16 path's distance from the fp32 run
    of the fake-quantised model; without the keyword the same steps dequantise."""
    from tests import test_gpu_fuyu_w8 as F8

    monkeypatch.delenv("OTTER_W8_PANEL", raising=False)
    model, qmodel, _ = F8._models()
    wide = copy.deepcopy(qmodel)
    assert wide.quantize_decoder_int8(wide_steps=True)["replaced"] == 0
    n_lin = 4 * F8.LAYERS + 1
    try:
        a_pre, a_steps, _ = F8._run(model, False, ROWS, None)
        _, b_steps, _ = F8._run(model, True, ROWS, None)
        with _Spies() as sp:
            _, _, _ = F8._run(qmodel, True, ROWS, None)
        assert sp.now["panel"] == 0 and sp.now["dequant"] == n_lin * (1 + F8.STEPS), sp.now
        with _Spies() as sp:
            _, c_steps, _ = F8._run(wide, True, ROWS, None)
        assert sp.now["panel"] == n_lin * F8.STEPS and sp.now["dequant"] == n_lin and sp.now["rows"] == sp.now["gemv"] == 0, sp.now
        ratios = []
        for s in range(F8.STEPS):
            d_b, d_c = float((b_steps[:, s] - a_steps[:, s]).abs().max()), float((c_steps[:, s] - a_steps[:, s]).abs().max())
            ratios.append(d_c / d_b)
            assert d_b > 0 and d_c <= 2 * d_b, ("step %d" % s, d_c, d_b)
        print("[w8-panel] persimmon %d rows: max|c-a| / max|b-a| per step = %s" % (ROWS, " ".join("%.3f" % r for r in ratios)), flush=True)
    finally:
        del wide
        gc.collect()
        torch.cuda.empty_cache()
