"""Inputs with exactly known answers for the GEMM kernels (csrc/gemm.hip and gemm_*.hip, gemm_t4_ktile.inc: C = epilogue(A[M, K] . B[N, K]^T)), an fp64
reference, the frames the operands and outputs are placed in, and the checkers.  Pure torch, device-agnostic: tests/test_gpu_gemm_exact.py
feeds the checkers with ops.gemm_nt / ops.gemm, tests/test_gemm_cases_cpu.py with a plain fp64 step and with deliberately wrong ones.

A *case* is a SimpleNamespace: the logical operands A [M, K] and B [N, K] (bf16 or fp32, on the CPU), the layout the harness allocates
(a_kmajor / b_kmajor, `pads`: extra leading-dimension elements per tensor, `kw`: operand columns behind the reduction length of a `k=`
case), the epilogue (`epi` in store / gelu / scale_res / gate_bwd, `accumulate` with a prior C, R, aux and `aux_mode` in None / "sqrelu" /
"stash" / "gelu", `gate`, `want_partial`, `want_c2`, `stash`), the output dtype and what the builder knows about the answer (`acc`, the exact
accumulator in fp64; `km` / `edges` of a one-hot case).  `Placed(case, device)` is the case in memory; a *step* maps a Placed to
Result(C, C2, partial).

Why the answers are exact: bf16 and fp32 hold small integers exactly, a product of two of them is exact in fp32, and a sum of integers whose
partial sums stay below 2^24 is exact in fp32 in ANY order -- any K-tile rotation, any split, any order inside an MFMA.  With s = 1 every
epilogue but the GELU value then has one right bit pattern: fp32 outputs equal the expected integer, bf16 outputs its round-to-nearest-even cast.

Kinds of input:
  onehot  row m of A is zero except A[m, km(m)] = r(m) in {+-1, +-2, +-4}; B random integers in [-8, 8]: C[m, n] = r(m) B[n, km(m)], a
          gather with a closed form and no library in it.  km walks the first and last k of every 64-wide K-tile and 128-wide pair, 0, K - 1
          and both sides of the start of the K tail (K % 64 != 0); the other rows draw k at random.  `mirrored`: the one-hot operand is B.
          acc[0, 0] is exactly 1: from a gated fp32 STORE that element IS the kernel's s (read_s_dev).
  count   A and B in {0, 1} with densities pa = 2 pb: C[m, n] is a count.  No count exceeds COUNT_CAP = 256 (bf16 holds it without rounding),
          and where partials are wanted no per-tile sum of |terms| reaches 2^24.  Both are asserted by the builder.
  ints    dense random integers in [-4, 4]; K * 16 < 2^24 asserted.
  gelu    ints with A scaled by a power of two so that the pre-activations have a standard deviation near 3 and cover [-8, 8].

Toleranced checks (the only ones; everything else is torch.equal), each per element, constants below with their derivation:
  gated forms   |got - ref64(s_dev)| <= GATE_ROUNDINGS 2^-24 A (+ one bf16 rounding), A = |s acc f'| + |R or prior C|
  s_dev         against fp64 tanh(gate): TANH_ULPS
  GELU / stash  CDF_F32 / CDF_BF16 / EXP_REL, never looser than GELU_CEILING of the largest reference value
"""
import math
from types import SimpleNamespace

import torch

BF16, F32 = torch.bfloat16, torch.float32
GUARD = 8                      # sentinel / NaN rows before and after every view
SENT = 2.0 ** 28               # exact in bf16; no output here comes near it
LIMIT = 2 ** 24                # integers below it are exact in fp32
COUNT_CAP = 256                # integers up to it are exact in bf16
KT = 64                        # K-tile of every bf16 kernel (the fp32 kernel: 32, a divisor)

H32 = 2.0 ** -24               # one fp32 rounding, relative (half an ulp is at most 2^-24 of the value)
HBF = 2.0 ** -8                # one bf16 rounding, relative (8 significant bits: half an ulp is at most 2^-8 of the value)
# epilogue4 / epilogue8 / tail_apply: STORE o = s v (one product), with accumulate o = c + s v, SCALE_RES o = v s + r: one product and one
# sum, or one fused multiply-add -- at most two roundings, each at most 2^-24 of a value that is at most A (1 + 2^-24).  GATE_BWD with
# sqrelu / stash: o = (s v) (2 r) / (s v) a: two products (2 r is exact).  The factor 1 + 2^-20 absorbs the second-order term.
GATE_ROUNDINGS = 2
GATE_SLACK = 1.0 + 2.0 ** -20
# otter_reduce_partials with a gate: th * th, 1 - th^2 (or one fma for both) and the final product: three roundings of values of at most
# |sum| (1 - s^2 >= 1/2 is asserted, so an absolute 2^-24 on 1 - s^2 is at most 2^-23 of it): 2^-24 + 2^-23 + 2^-24 = 4 * 2^-24.
PART_ROUNDINGS = 4
# tanhf of the device library: no accuracy statement for it is on the build machine (no OCML documentation ships with the toolchain), so
# the distance is printed by the GPU test and bounded at 4 ulp, as the issue that introduced this file lays down.
TANH_ULPS = 4
# fp32 results, gelu_cdf_pdf (common.h): Abramowitz-Stegun 7.1.26 has |erf error| <= 1.5e-7, so Phi is off by at most 0.75e-7; v_rcp_f32
# (1 ulp) feeds a degree-5 Horner form times exp, whose relative error of ~5e-7 on erfc <= 1 is halved: at most 1.2e-7 more on Phi where
# |u| is not small, and the rounding of 1 - half is 3e-8.  Sum 2.3e-7; doubled: 4.6e-7 -> 5e-7.
CDF_F32 = 5.0e-7
# bf16 results, gelu_cdf_fast (common.h): "|error| <= 1.5e-5 absolute in fp32 Horner form", as stated beside the polynomial.
CDF_BF16 = 1.5e-5
# exp(-u^2 / 2) of the derivative: the argument (|.| <= 0.73 u^2 <= 47 for |u| <= 8) is rounded twice, 2 * 2^-24 * 47 in log2 units =
# 3.9e-6 relative, v_exp_f32 adds 2 ulp: below 2^-17 = 7.6e-6.  It multiplies |u| phi(u) <= 0.25.
EXP_REL = 2.0 ** -17
GELU_CEILING = 6e-3            # the relative-to-max bound of tests/test_gpu_kernels.py: no per-element bound here may be looser

# shapes of tests/test_gpu_gemm_exact.py that tests/test_gemm_cases_cpu.py proves the builder conditions at
TILE_OF = {1: (128, 128), 2: (256, 256), 3: (256, 256), 13: (256, 256), 25: (128, 128), 26: (256, 256), 30: (128, 128)}   # of the partials:
#   cfg_tiles of pick_cfg(M, N, 64) -- a forced 25 / 30 counts 128 x 128 tiles (30 runs as 25 when partials are asked for)
MULTI_SHAPE = (520, 772)
MULTI_K = {1: [72], 2: [136], 3: [192], 13: [192], 25: [512], 30: [768], 26: [128, 256, 384]}
LARGE_SHAPES = [(3072, 4096), (2824, 4040)]
LARGE_K = [128, 256, 384, 129, 200, 333]

WORST = {}                     # (kind, epilogue, output) -> largest error / bound seen by the toleranced checks


class Result(SimpleNamespace):
    pass


class CheckFailure(AssertionError):
    def __init__(self, reason, detail):
        super().__init__("%s: %s" % (reason, detail))
        self.reason = reason


# reasons
READ_OUTSIDE = "read outside an operand"
C_NOT_EXACT = "C is not the exact answer"
C2_NOT_EXACT = "C2 is not the exact answer"
FRAME_WRITTEN = "written outside the output view"
NOT_WRITTEN = "output not written"
PARTIAL_MULTISET = "per-tile partials differ from the per-tile sums"
PARTIAL_TOTAL = "reduced partials differ from the exact total"
PARTIAL_CHANGES_C = "C differs with and without partials"
C_BEYOND_BOUND = "C beyond its rounding bound"
C2_BEYOND_BOUND = "C2 beyond its rounding bound"
S_DEV = "s read back from the kernel"


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(int(seed))
    return g


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------------------------ builders

def k_edges(K):
    """The reduction indices a kernel with 64-wide K-tiles, handled in 128-wide pairs, can lose, double or shift."""
    e = [0, K - 1]
    for t in range(cdiv(K, 64)):
        e += [64 * t, min(64 * t + 63, K - 1)]
    for t in range(cdiv(K, 128)):
        e += [128 * t, min(128 * t + 127, K - 1)]
    if K % 64 and K > 64:
        e += [K // 64 * 64 - 1, K // 64 * 64]
    return sorted(set(e))


def _onehot(rows, K, g, reverse):
    edges = k_edges(K)
    order = edges[::-1] if reverse else edges
    km = torch.randint(0, K, (rows,), generator=g)
    n = min(rows, len(order))
    km[:n] = torch.tensor(order[:n])
    r = torch.tensor([1.0, -1.0, 2.0, -2.0, 4.0, -4.0])[torch.randint(0, 6, (rows,), generator=g)]
    r[0] = 1.0
    hot = torch.zeros(rows, K)
    hot[torch.arange(rows), km] = r
    return hot, km, r, edges


def count_density(M, N, K, want_partial):
    """(pa, pb): mean count pa pb K = mu, pa = 2 pb.  mu = 6 keeps the largest count far below COUNT_CAP.  Where partials are wanted the
    sum over the WHOLE output of (count + prior)^2 -- mean mu^2 + mu + 2 mu / 8 + 1 / 8 with the sparse prior C of a count case -- must
    stay below 2^24 as well (otter_reduce_partials adds the per-tile sums in fp32): the largest mu of 2, 1, 1/2, 1/4 that leaves a fifth
    of 2^24 free."""
    mu = 6.0
    if want_partial:
        mu = next((m for m in (2.0, 1.0, 0.5, 0.25) if (m * m + 1.25 * m + 0.125) * M * N <= 0.8 * LIMIT), 0.125)
    mu = min(mu, 0.4 * K)
    pa = min(0.9, math.sqrt(2.0 * mu / K))
    return pa, mu / (K * pa)


def make_case(kind, M, N, K, in_dtype=BF16, out_dtype=BF16, epi="store", accumulate=False, gate=None, r_dtype=F32, aux_dtype=BF16,
              aux_mode=None, want_partial=False, want_c2=False, stash=False, a_kmajor=False, b_kmajor=False, pads=None, kw=0, mirrored=False,
              tile=None, seed=0, with_acc=True):
    """`tile` = (bm, bn) of the kernel that will write the partials (needed with want_partial).  with_acc = False leaves case.acc to the
    harness (device fp64 product at the large shapes); the builder then bounds its conditions on the operands alone."""
    g = _gen(seed * 7919 + M * 131 + N * 17 + K)
    c = SimpleNamespace(kind=kind, M=M, N=N, K=K, in_dtype=in_dtype, out_dtype=out_dtype, epi=epi, accumulate=accumulate, gate=gate,
                        aux_mode=aux_mode, want_partial=want_partial, want_c2=want_c2 or stash, stash=stash, a_kmajor=a_kmajor,
                        b_kmajor=b_kmajor, pads=dict(pads or {}), kw=kw, mirrored=mirrored, tile=tile, acc=None, R=None, aux=None,
                        prior=None, km=None, edges=None)
    c.name = "%s%s %dx%dx%d %s->%s %s%s%s%s%s" % (
        kind, "-mirrored" if mirrored else "", M, N, K, str(in_dtype)[6:], str(out_dtype)[6:], epi, "+acc" if accumulate else "",
        "+" + str(aux_mode) if aux_mode else "", "+gate" if gate is not None else "", "+partial" if want_partial else "")
    if kind == "onehot":
        if not mirrored:
            A, c.km, c.r, c.edges = _onehot(M, K, g, False)
            B = torch.randint(-8, 9, (N, K), generator=g).float()
            B[0, c.km[0]] = 1.0
            c.acc = (c.r[:, None] * B[:, c.km].T).double()
        else:
            B, c.km, c.r, c.edges = _onehot(N, K, g, True)
            A = torch.randint(-8, 9, (M, K), generator=g).float()
            A[0, c.km[0]] = 1.0
            c.acc = (A[:, c.km] * c.r[None, :]).double()
    elif kind == "count":
        c.pa, c.pb = count_density(M, N, K, want_partial)
        A = (torch.rand(M, K, generator=g) < c.pa).float()
        B = (torch.rand(N, K, generator=g) < c.pb).float()
        c.count_bound = int(min(A.sum(1).max(), B.sum(1).max()))     # count[m, n] <= min(ones in row m of A, ones in row n of B)
        assert c.count_bound <= COUNT_CAP, "%s: a count may reach %d" % (c.name, c.count_bound)
    elif kind in ("ints", "gelu"):
        assert K * 16 < LIMIT
        A = torch.randint(-4, 5, (M, K), generator=g).float()
        B = torch.randint(-4, 5, (N, K), generator=g).float()
        if kind == "gelu":
            c.shift = max(0, round(math.log2(max(1.0, 20.0 / 3.0 * math.sqrt(K) / 3.0))))      # std of acc is 20/3 sqrt(K): bring it near 3
            A = A * 2.0 ** -c.shift
    else:
        raise ValueError(kind)
    c.A, c.B = A.to(in_dtype), B.to(in_dtype)
    assert torch.equal(c.A.float(), A) and torch.equal(c.B.float(), B)
    if c.acc is None and with_acc:
        c.acc = A.double() @ B.double().T
    if epi == "scale_res":
        c.R = torch.randint(-16, 17, (M, N), generator=g).to(r_dtype)
    if epi == "gate_bwd":
        lo, hi = (-2, 2) if aux_mode in (None, "sqrelu") else (-4, 4)
        c.aux = torch.randint(lo, hi + 1, (M, N), generator=g).to(aux_dtype)
    if accumulate:
        assert epi == "store" and out_dtype == F32
        c.prior = (torch.rand(M, N, generator=g) < 0.125).float() if kind == "count" else torch.randint(-2, 3, (M, N), generator=g).float()
    if want_partial:
        assert tile is not None and ((epi == "store" and out_dtype == F32) or (epi == "gate_bwd" and aux_mode in (None, "sqrelu")))
        if kind == "count":                                   # the other kinds: on the exact product, in finish()
            c.tile_bound = tile_sum_bound(c, *tile)
            assert c.tile_bound < LIMIT, "%s: a per-tile sum may reach %d" % (c.name, c.tile_bound)
    if c.acc is not None:
        finish(c)
    return c


def finish(c):
    """The builder's conditions on the exact product (called by the harness once case.acc exists at the large shapes)."""
    if c.kind == "count":
        c.count_max = int(c.acc.max())
        assert c.count_max <= COUNT_CAP, "%s: count %d" % (c.name, c.count_max)
    if c.kind != "gelu":
        assert float(c.acc.abs().max()) * 64 < LIMIT                     # room for f'(aux) <= 8, R and the prior C
    if c.want_partial:
        t = expected(c, c.acc, 1.0).terms.abs()
        c.tile_max = int(tile_sums(t, *c.tile).max())
        assert c.tile_max < LIMIT, "%s: per-tile sum %d" % (c.name, c.tile_max)
        # otter_reduce_partials adds the per-tile sums in fp32: its total has one right value only below 2^24.  The densities of a count
        # case and the range of a one-hot case keep it there; dense integers in [-4, 4] cannot at every shape (520 x 772 x 768: 7e7), so
        # an `ints` case is held to the exact per-tile multiset always and to the exact total where it fits.
        c.total_exact = float(t.sum()) < LIMIT
        assert c.total_exact or c.kind == "ints", "%s: total %d" % (c.name, int(t.sum()))


def tile_sum_bound(c, bm, bn):
    """Upper bound of every per-tile sum of |terms| from the operands alone.  The sum of |acc| over a tile is at most sum_k (column sum of
    |A| over the tile's rows)(column sum of |B| over its columns); each term is at most |acc| (or |acc| + 2 under accumulate) times
    max(|acc| + 2, f): |acc| <= amax = min(largest row sum of |A| times max |B|, the mirror)."""
    A, B = c.A.double().abs(), c.B.double().abs()
    amax = float(torch.minimum(A.sum(1).max() * B.max(), B.sum(1).max() * A.max()))
    gm, gn = cdiv(c.M, bm), cdiv(c.N, bn)
    ca = torch.stack([A[i * bm:(i + 1) * bm].sum(0) for i in range(gm)])
    cb = torch.stack([B[j * bn:(j + 1) * bn].sum(0) for j in range(gn)])
    s_acc = float((ca @ cb.T).max())
    if c.epi == "store":
        return int((amax + 2) * (s_acc + 2 * bm * bn))
    return int(s_acc * (4 if c.aux_mode == "sqrelu" else 2))


# ------------------------------------------------------------------------------------------------------------------ reference

def gelu64(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_grad64(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def expected(c, acc, s):
    """fp64: C and C2 before the output rounding, `terms` whose per-tile sums are the partials, `A` the sum of the absolute values that
    bounds the roundings of a gated form, `fp` the factor f'(aux)."""
    dev = acc.device
    e = SimpleNamespace(C2=None, terms=None, A=None)
    if c.epi == "store":
        add = c.prior.double().to(dev) if c.accumulate else 0.0
        e.C = s * acc + add
        e.A = (s * acc).abs() + (add.abs() if c.accumulate else 0.0)
        if c.out_dtype == F32:
            e.terms = e.C * e.C
    elif c.epi == "scale_res":
        r = c.R.double().to(dev)
        e.C = acc * s + r
        e.A = (s * acc).abs() + r.abs()
    elif c.epi == "gate_bwd":
        a = c.aux.double().to(dev)
        if c.aux_mode is None:
            fp, f = torch.ones_like(a), a
        elif c.aux_mode == "sqrelu":
            fp, f = 2.0 * a.clamp(min=0), a.clamp(min=0) ** 2
        elif c.aux_mode == "stash":
            fp, f = a, None
        else:
            fp, f = gelu_grad64(a), gelu64(a)
        e.C = s * acc * fp
        e.A = e.C.abs()
        e.terms = acc * f if f is not None else None
    elif c.epi == "gelu":
        e.C = gelu64(acc)
        if c.want_c2:
            e.C2 = gelu_grad64(acc) if c.stash else acc
    else:
        raise ValueError(c.epi)
    return e


def tile_sums(t, bm, bn):
    """Sums of t [M, N] over the bm x bn tiles, edge tiles counting their in-bounds elements only: [gm * gn], row-major."""
    M, N = t.shape
    gm, gn = cdiv(M, bm), cdiv(N, bn)
    p = torch.zeros(gm * bm, gn * bn, dtype=t.dtype, device=t.device)
    p[:M, :N] = t
    return p.view(gm, bm, gn, bn).sum((1, 3)).reshape(-1)


# ------------------------------------------------------------------------------------------------------------------ frames

class Placed:
    """The case in memory, as a kernel gets it.  Every tensor is a view [rows, cols] at row GUARD of a buffer [GUARD + rows + GUARD, ld]:
    outputs (C, C2) in buffers filled with SENT -- the prior C of an accumulate case copied into the view --, inputs (A, B, R, aux) in
    buffers filled with NaN.  A K-major operand is stored [K, M or N]: the rows behind K are guard rows, the columns behind M / N padding.
    A `k=` case stores operands kw columns wider than K, with NaN behind column K.  `full[name]` is the buffer, for the steps that read or
    write where they should not."""

    def __init__(self, c, device="cpu"):
        self.case, self.device, self.full, self.view = c, device, {}, {}
        al = 8 if c.in_dtype == BF16 else 4
        for nm, t, kmaj in (("A", c.A, c.a_kmajor), ("B", c.B, c.b_kmajor)):
            if kmaj:
                v = self._alloc(nm, c.K, t.shape[0], c.in_dtype, float("nan"), al)
                v.copy_(t.T)
            else:
                v = self._alloc(nm, t.shape[0], c.K + c.kw, c.in_dtype, float("nan"), al)
                v[:, :c.K].copy_(t)
        for nm, t in (("R", c.R), ("aux", c.aux)):
            if t is not None:
                self._alloc(nm, c.M, c.N, t.dtype, float("nan"), 4).copy_(t)
        self._alloc("C", c.M, c.N, c.out_dtype, SENT, 4)
        if c.accumulate:
            self.view["C"].copy_(c.prior)
        if c.want_c2:
            self._alloc("C2", c.M, c.N, c.out_dtype, SENT, 4)
        self.partial = None

    def _alloc(self, nm, rows, cols, dtype, fill, al):
        ld = cols + self.case.pads.get(nm, 0)
        assert ld % al == 0, "%s: ld %d of %s" % (self.case.name, ld, nm)
        self.full[nm] = torch.full((rows + 2 * GUARD, ld), fill, dtype=dtype, device=self.device)
        self.view[nm] = self.full[nm][GUARD:GUARD + rows, :cols]
        return self.view[nm]

    def alloc_partial(self, n):
        self.partial = torch.full((n,), float("nan"), dtype=F32, device=self.device)
        return self.partial

    def reset_outputs(self):
        for nm in ("C", "C2"):
            if nm in self.full:
                self.full[nm].fill_(SENT)
        if self.case.accumulate:
            self.view["C"].copy_(self.case.prior)
        if self.partial is not None:
            self.partial.fill_(float("nan"))

    def result(self):
        """Result of the launch that just ran (copies), after checking the frames: everything outside the views must still be SENT."""
        c = self.case
        out = {nm: self.view[nm].clone() for nm in ("C", "C2") if nm in self.view}
        for nm, t in out.items():
            self.view[nm].fill_(SENT)
            f = self.full[nm]
            if not bool((f == SENT).all()):
                bad = (f != SENT).nonzero()[0].tolist()
                raise CheckFailure(FRAME_WRITTEN, "%s: %s buffer row %d column %d (view: rows %d..%d, columns 0..%d)"
                                   % (c.name, nm, bad[0], bad[1], GUARD, GUARD + c.M - 1, c.N - 1))
            self.view[nm].copy_(t)
        return Result(C=out["C"], C2=out.get("C2"), partial=None if self.partial is None else self.partial.clone())


# ------------------------------------------------------------------------------------------------------------------ checkers

def _where(bad):
    i = bad.nonzero()
    return "%d elements, first at %s" % (i.shape[0], tuple(i[0].tolist()))


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def worst_table():
    rows = ["[gemm-exact] %-8s %-22s %-4s worst error / bound %.3f" % (k + (v,)) for k, v in sorted(WORST.items())]
    return "\n".join(rows) if rows else "[gemm-exact] no toleranced check ran"


def _epi_name(c):
    return c.epi + ("+acc" if c.accumulate else "") + ("+" + str(c.aux_mode) if c.aux_mode else "") + ("+stash" if c.stash else "")


def _basic(c, res):
    for nm in ("C", "C2"):
        t = getattr(res, nm)
        if t is None:
            continue
        if bool(torch.isnan(t).any()):
            raise CheckFailure(READ_OUTSIDE, "%s: NaN in %s, %s" % (c.name, nm, _where(torch.isnan(t))))
        if bool((t.float() == SENT).any()):
            raise CheckFailure(NOT_WRITTEN, "%s: %s, %s" % (c.name, nm, _where(t.float() == SENT)))


def _exact(c, got, want64, reason, nm):
    want = want64.float().to(got.dtype)               # fp64 -> fp32 is exact here (integers below 2^24); -> bf16 rounds to nearest even
    assert torch.equal(want64.float().double(), want64)
    if not torch.equal(got, want):
        bad = got != want
        i = tuple(bad.nonzero()[0].tolist())
        raise CheckFailure(reason, "%s: %s, %s: got %r, exact %r" % (c.name, nm, _where(bad), float(got[i]), float(want[i])))


def _bounded(c, got, want64, bound64, reason, nm, ceiling=None):
    if c.out_dtype == BF16:
        bound64 = bound64 + HBF * (want64.abs() + bound64)
    if ceiling is not None:
        assert bool((bound64 <= ceiling).all()), "%s: a per-element bound of %s exceeds the ceiling %g" % (c.name, nm, ceiling)
    err = (got.double() - want64).abs()
    bad = err > bound64
    ratio = float((err / bound64.clamp(min=1e-300)).max())
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise CheckFailure(reason, "%s: %s, %s: got %r, reference %r, bound %.3g" % (c.name, nm, _where(bad), float(got[i]), float(want64[i]),
                                                                                    float(bound64[i])))
    _note((c.kind, _epi_name(c), nm), ratio)
    return ratio


def check_s_dev(s_dev, gate):
    """s_dev against fp64 tanh(gate); returns the distance in fp32 ulps of tanh(gate)."""
    t = math.tanh(gate)
    ulp = 2.0 ** (math.floor(math.log2(abs(t))) - 23)
    d = abs(float(s_dev) - t) / ulp
    _note(("s_dev", "tanhf", "ulps/%d" % TANH_ULPS), d / TANH_ULPS)
    if not d <= TANH_ULPS:
        raise CheckFailure(S_DEV, "tanhf(%r) = %r is %.2f ulp from %r" % (gate, float(s_dev), d, t))
    assert 1.0 - float(s_dev) ** 2 >= 0.5
    return d


def read_s_dev(c, res):
    """The kernel's s from a gated fp32 STORE of a one-hot case: every element whose accumulator is exactly 1 holds it."""
    assert c.kind == "onehot" and c.epi == "store" and not c.accumulate and c.out_dtype == F32 and c.gate is not None
    _basic(c, res)
    ones = res.C[c.acc.to(res.C.device) == 1.0]
    assert ones.numel() > 0
    if not bool((ones == ones[0]).all()):
        raise CheckFailure(S_DEV, "%s: elements with accumulator 1 hold different values (%r .. %r)" % (c.name, float(ones.min()), float(ones.max())))
    return float(ones[0])


def check(c, res, s_dev=None):
    """C and C2 of one launch: bit equality without a gate (GELU value and stashed derivative: per-element bound), the rounding bound
    around the fp64 value with the kernel's own s (s_dev) with one.  Returns the worst error / bound of the toleranced part (0: none)."""
    _basic(c, res)
    dev = res.C.device
    acc = c.acc.to(dev)
    worst = 0.0
    if c.epi == "gelu":
        e = expected(c, acc, 1.0)
        u = acc.abs()
        cdf_err = CDF_BF16 if c.out_dtype == BF16 else CDF_F32
        ceil = GELU_CEILING * float(e.C.abs().max())
        worst = _bounded(c, res.C, e.C, u * cdf_err + 2 * H32 * e.C.abs(), C_BEYOND_BOUND, "C", ceil)
        if c.want_c2 and not c.stash:
            _exact(c, res.C2, e.C2, C2_NOT_EXACT, "C2")
        elif c.stash:
            phi = torch.exp(-0.5 * acc * acc) / math.sqrt(2.0 * math.pi)
            b2 = cdf_err + u * phi * EXP_REL + 3 * H32 * (e.C2.abs() + 1.0)
            worst = max(worst, _bounded(c, res.C2, e.C2, b2, C2_BEYOND_BOUND, "C2", GELU_CEILING * float(e.C2.abs().max())))
        return worst
    if c.gate is None:
        e = expected(c, acc, 1.0)
        _exact(c, res.C, e.C, C_NOT_EXACT, "C")
        return 0.0
    assert s_dev is not None
    e = expected(c, acc, float(s_dev))
    return _bounded(c, res.C, e.C, GATE_ROUNDINGS * H32 * GATE_SLACK * e.A, C_BEYOND_BOUND, "C")


def check_partials(c, res, reduced=None, s_dev=None, reduced_gated=None):
    """The multiset of per-tile partials against the exact per-tile sums (edge tiles count their in-bounds elements only); `reduced`
    (otter_reduce_partials without gate) against the exact total; `reduced_gated` within PART_ROUNDINGS of (1 - s_dev^2) total."""
    assert c.want_partial
    p = res.partial
    e = expected(c, c.acc.to(p.device), 1.0)
    want = tile_sums(e.terms, *c.tile).float()
    if p.numel() != want.numel():
        raise CheckFailure(PARTIAL_MULTISET, "%s: %d partials for %d tiles of %d x %d" % ((c.name, p.numel(), want.numel()) + tuple(c.tile)))
    if bool(torch.isnan(p).any()):
        raise CheckFailure(PARTIAL_MULTISET, "%s: %d of %d partials were not written" % (c.name, int(torch.isnan(p).sum()), p.numel()))
    a, b = torch.sort(p)[0], torch.sort(want)[0]
    if not torch.equal(a, b):
        i = int((a != b).nonzero()[0])
        raise CheckFailure(PARTIAL_MULTISET, "%s: %d of %d sorted partials differ, first %r against %r (largest exact per-tile sum %d)"
                           % (c.name, int((a != b).sum()), p.numel(), float(a[i]), float(b[i]), int(want.abs().max())))
    total = float(e.terms.sum())
    if not c.total_exact:
        return
    if reduced is not None and float(reduced) != total:
        raise CheckFailure(PARTIAL_TOTAL, "%s: %r against %r" % (c.name, float(reduced), total))
    if reduced_gated is not None:
        ref = (1.0 - float(s_dev) ** 2) * total
        bound = PART_ROUNDINGS * H32 * GATE_SLACK * abs(total)
        ratio = abs(float(reduced_gated) - ref) / bound if bound > 0 else 0.0
        _note((c.kind, _epi_name(c), "gate partial"), ratio)
        if abs(float(reduced_gated) - ref) > bound:
            raise CheckFailure(PARTIAL_TOTAL, "%s: gated %r against %r, bound %.3g" % (c.name, float(reduced_gated), ref, bound))


def check_same_bits(c, a, b, reason=PARTIAL_CHANGES_C, what="C"):
    if not torch.equal(a.view(torch.int16 if a.dtype == BF16 else torch.int32), b.view(torch.int16 if b.dtype == BF16 else torch.int32)):
        raise CheckFailure(reason, "%s: %s, %s" % (c.name, what, _where(a != b)))


# ------------------------------------------------------------------------------------------------------------------ one case, start to end

def run_case(c, step, device="cpu", s_dev=None, reduce=None, placed=None):
    """Places the case, runs `step(placed)` (twice where partials are wanted: without and with the partial buffer, C must keep its bits),
    checks the frames, C, C2 and the partials.  `reduce(partial, gate or None)` is otter_reduce_partials or its stand-in.  Returns
    (Result, worst error / bound)."""
    p = placed or Placed(c, device)
    p.reset_outputs()
    res0 = None
    if c.want_partial:
        step(p)
        res0 = p.result()
        p.reset_outputs()
        p.alloc_partial(cdiv(c.M, c.tile[0]) * cdiv(c.N, c.tile[1]))
    step(p)
    res = p.result()
    worst = check(c, res, s_dev)
    if c.want_partial:
        check_same_bits(c, res0.C, res.C)
        check_partials(c, res, reduced=reduce(res.partial, None) if reduce else None, s_dev=s_dev,
                       reduced_gated=reduce(res.partial, c.gate) if (reduce and c.gate is not None) else None)
    return res, worst
