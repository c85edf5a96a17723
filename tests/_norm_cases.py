"""Inputs with exactly known answers for the row kernels of csrc/norm.hip (LayerNorm / RMSNorm forward and backward, the fused residual add,
row-mapped outputs, the two-stage dgamma / dbeta reduction, otter_colsum), an fp64 reference, the frames every tensor is placed in, and the
checkers.  Pure torch, device-agnostic: tests/test_gpu_norm_exact.py feeds the checkers with steps made of _capi / ops calls,
tests/test_norm_cases_cpu.py with a plain fp64 step, a kernel-shaped fp32 step and deliberately wrong ones.

A *case* is a SimpleNamespace of one `family`:
  fwd     op ln / rms; x [rows, D], optional delta (fused add), gamma, beta, a row map for y, a second output y2, mean / rstd wanted or not.
          Results: y, y2, xsum, mean, rstd.
  bwd     op ln / rms; dy (optionally behind a row map), x, gamma, mean and rstd AS INPUTS (the exact ones, from the host: nothing here
          depends on the forward kernel), optional dres, dx_bf16, need_dx, need_dw, need_dbeta, accumulate with prior dgamma / dbeta.
          Results: dx, dx_bf16, dgamma, dbeta.
  colsum  src (bf16 / fp32, optionally behind a row map), accumulate with a prior.  Result: out.
`Placed(case, device)` is the case in memory; a *step* maps a Placed to results by writing into its buffers.

Why the answers are exact.  Small integers times a power of two are exact in bf16 and fp32; a sum of such values is exact in fp32 in ANY
order while every partial sum stays below 2^24 units -- any lane assignment, any butterfly, any split into row chunks; a product of two such
values is exact, so -ffp-contract=fast (an fma rounds once where mul + add rounds twice) cannot change a bit.  What is left are one fp32
division, one sqrtf and one reciprocal per row, each with an exactly representable result (D c / D = c, sqrt(a^2) = a, 1 / a with a a power of
two): a correctly rounded operation returns it.  The library is built without fast-math (otter_amd/build.py: -O3 -ffp-contract=fast only),
and hipcc then keeps fp32 `/` and sqrtf correctly rounded (clang's -fhip-fp32-correctly-rounded-divide-sqrt, on by default).  Confirmed from
the generated code of csrc/norm.hip for gfx950: every `/` is the v_div_scale_f32 / v_rcp_f32 / v_fma_f32 ... / v_div_fmas_f32 /
v_div_fixup_f32 sequence and sqrtf is v_sqrt_f32 followed by its two-fma correction and v_cmp_class fix-up, not a bare v_rcp_f32 / v_sqrt_f32.
Every condition above is asserted by the builders (_units, _witnesses, the closed forms against the fp64 reference), and
tests/test_norm_cases_cpu.py builds every case of the GPU file.

Kinds of input (row r has a scale a_r = 2^k and an offset c_r = m_r a_r, both different from row to row):
  balanced    LayerNorm forward.  x = c_r + a_r s, s = +-1 with exactly D / 2 of each in a random arrangement, eps = 0: mean = c_r,
              var = a_r^2, rstd = 1 / a_r exactly, y = s gamma + beta with integer gamma / beta that differ per column; eight columns give
              257, 259, 513, 515 (ties and non-ties above 2^8: a truncating or round-half-up bf16 store fails).
  + delta     x and delta integers (times a_r) whose sum is the balanced row.  For a bf16 stream some rows have m_r = 257 / 259 and a few
              sums on a bf16 tie (257 a -> 256 a, 259 a -> 260 a): the balanced row is the ROUNDED sum, as round_to(x + delta) feeds the
              statistics.
  rms         `pm`: x = +-a_r, rstd = 1 / a_r.  `ratio`: |x| in {a, 7 a} in the ratio 15 : 1, mean square 4 a^2, rstd = 1 / (2 a)
              (D % 16 == 0).  y = t w.
  backward    x^ = s.  g = dy gamma = m1 + s m2 + h with integers m1, m2 per row and integers h whose sums over the +1 and over the -1
              columns are both zero (a few entries of each row are fixed up after the draw): sum g = D m1 and sum g x^ = D m2 exactly, also
              where D is no power of two, so dx = h rstd + dres.  gamma is +-1, +-2, +-4, so dy = g / gamma stays exact in bf16.  RMSNorm:
              the same rows (sum g = D m1 != 0, which a kernel that subtracts the mean of g gets wrong); with a bf16 x the supplied rstd
              is 257 / (256 a_r) in every other row: x rstd = +-257 / 256 is a bf16 tie that round_to turns into +-1 -- a kernel without
              round_to gets another dx and dw.  dres = e / a_r with integers e, some of them 256 and 512 so that dx lands on bf16 ties.
  dw forms    `random` (the rows above), `count` (dy = 1, x^ = +1: dgamma = dbeta = rows, one lost or doubled row is off by one),
              `onerow` (only row r* has a nonzero dy; row_edges() walks r*), `onehot` (column j has its only nonzero dy in row r*(j): every
              r* of row_edges() in ONE launch; dw only).  colsum has the same forms.
  general     the only toleranced kind: seeded normal data at the default eps against the fp64 reference PER ELEMENT; bounds below.

Bounds of the general kind (u = 2^-24, one fp32 rounding; K = SUM_DEPTH(D), the longest chain of additions an element's value goes through
in the row sums: 8 per 512-column chunk in a lane, then six butterfly levels; a sum of n terms by any tree of depth K is within K u sum|term|):
  mean        the sum, then one division: (K + 1) u mean|x|                                                             =: e_mu
  rstd        x - mean: the common shift of e_mu drops out of sum (x - mean)^2 to first order (sum (x - mean) = 0) and leaves (e_mu / sigma)^2;
              rounding of x - mean 2 u (it is squared), the square u, the sum K u, the division u: var within (K + 4) u + (e_mu / sigma)^2.
              var + eps (u), sqrtf (halves what came before, adds u), 1 / . (u):  ((K + 4) / 2 + 2.5) u + (e_mu / sigma)^2 / 2  =: E_rs
              (RMSNorm: x^2 u, the sum K u, the division u: ((K + 2) / 2 + 2.5) u.)
              [Three correctly rounded operations after var give 0.5 + 1 + 1 = 2.5 u = 1.25 * 2^-23 relative.]
  y           x - mean (e_mu, u), times rstd (E_rs, u), times gamma (u), plus beta (u):
              |gamma| (e_mu rstd + |x^| (E_rs + 3 u)) + u (|x^ gamma| + |beta|); a bf16 y adds 2^-8 (|y| + bound).
              (RMSNorm with an fp32 x: x rstd (E_rs, u), times w (u): |x^ w| (E_rs + 2 u).)
  HF RMSNorm  bf16 x: y = w bf16(x rstd).  x rstd carries E_rs + u <= 2^-20 (asserted: this is why these cases have D <= 1024), so every
              element whose fp64 x rstd is further than 2^-20 relative from a bf16 rounding boundary has ONE right bf16(x rstd); those
              nearer are left out (expected share 2^-10, cap 1 %, asserted from the reference alone).  y then carries one product: u |y|.
  dx          mean and rstd are inputs.  x^ within 2 u |x^| (bf16 RMSNorm: the reference rounds exactly as the kernel does, fp32 then bf16).
              m1 within (K + 2) u mean|g| =: e1, m2 within (K + 5) u mean|g x^| =: e2.  With S = |g| + |m1| + |x^ m2|:
              rstd (e1 + |x^| e2 + 6 u S) + u |dx|  (dy gamma, x^, x^ m2, two subtractions, times rstd: six roundings of values <= S; + dres: u |dx|).
  dgamma / dbeta / colsum   Kc = COL_DEPTH(rows): ceil(per / 4) rows per wave, 3 to fold four waves, ceil(rch / 4) + 2 in the final kernel.
              dbeta, colsum: Kc u sum|term|; dgamma: (Kc + 4) u sum|dy x^|; accumulate adds u (|prior| + |sum|).
Every bound is multiplied by SLACK = 1 + 2^-10 for the second-order terms and is cut to the relative-to-max bound tests/test_gpu_kernels.py
uses for the same quantity (CEILING), so none is looser.
"""
import math
from types import SimpleNamespace

import torch

BF16, F32 = torch.bfloat16, torch.float32
SENT = 2.0 ** 28               # exact in bf16 and fp32; no value here comes near it
LIMIT = 2 ** 24                # integers below it are exact in fp32
U32 = 2.0 ** -24               # one fp32 rounding, relative
HBF = 2.0 ** -8                # one bf16 rounding, relative
SLACK = 1.0 + 2.0 ** -10
HF_WINDOW = 2.0 ** -20         # relative distance from a bf16 rounding boundary below which an HF RMSNorm element is left out
HF_CAP = 0.01                  # at most this share of a case's elements may be left out
EPS_LN, EPS_RMS = 1e-5, 1e-6   # the defaults of ops.layernorm_fwd / ops.rmsnorm_fwd
# relative-to-max bounds of tests/test_gpu_kernels.py for the same quantities: no per-element bound here may be looser
CEILING = {"mean": 1e-5, "rstd": 1e-4, "y_f32": 2e-5, "y_bf16": 1e-2, "dx_f32": 5e-5, "dx_bf16": 8e-3, "dgamma": 1e-4, "dbeta": 1e-4,
           "out": 1e-5}

# ---- the shapes of tests/test_gpu_norm_exact.py; tests/test_norm_cases_cpu.py builds every one of them
D_LIST = [8, 504, 512, 520, 1024, 1032, 2048, 2056, 3584, 4096, 4104, 4608, 8184, 8192]
ROUTES = [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)]        # (stream dtype, branch dtype): x -> y forward, x / dx <- dy backward
SMALL_ROWS = [1, 2, 3, 4, 5]
SMALL_ROWS_D = [520, 1024]
EDGE_ROWS = [31, 32, 33, 63, 64, 65, 127, 8191, 8192, 8193]
EDGE_D = [520, 512]            # generic / coalesced dx

WORST = {}                     # (family, what, quantity) -> largest error / bound seen by the toleranced checks


class Result(SimpleNamespace):
    pass


class CheckFailure(AssertionError):
    def __init__(self, reason, detail):
        super().__init__("%s: %s" % (reason, detail))
        self.reason = reason


# reasons
READ_OUTSIDE = "read outside an operand"
NOT_WRITTEN = "output not written"
FRAME_WRITTEN = "written outside the output view"
XSUM_NOT_EXACT = "xsum is not the exact (rounded) sum"
MEAN_NOT_EXACT = "mean is not the exact answer"
RSTD_NOT_EXACT = "rstd is not the exact answer"
Y_NOT_EXACT = "y is not the exact answer"
Y2_DIFFERS = "y2 and y hold different bits"
DX_NOT_EXACT = "dx is not the exact answer"
DXB_NOT_EXACT = "dx_bf16 is not the nearest-even cast of the exact dx"
DGAMMA_NOT_EXACT = "dgamma is not the exact answer"
DBETA_NOT_EXACT = "dbeta is not the exact answer"
OUT_NOT_EXACT = "column sums are not the exact answer"
BEYOND_BOUND = "beyond its rounding bound"
EXACT_REASON = {"xsum": XSUM_NOT_EXACT, "mean": MEAN_NOT_EXACT, "rstd": RSTD_NOT_EXACT, "y": Y_NOT_EXACT, "y2": Y_NOT_EXACT,
                "dx": DX_NOT_EXACT, "dx_bf16": DXB_NOT_EXACT, "dgamma": DGAMMA_NOT_EXACT, "dbeta": DBETA_NOT_EXACT, "out": OUT_NOT_EXACT}


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(int(seed))
    return g


def cdiv(a, b):
    return (a + b - 1) // b


def dname(dt):
    return "bf16" if dt == BF16 else "f32"


# ------------------------------------------------------------------------------------------------------------------ mirrors of norm.hip

def pick_nch(D):
    n = 1
    while n * 512 < D:
        n <<= 1
    return n


def pick_rch(rows):
    return max(1, min(256, rows // 32))


def coalesced_fwd(D, xdt, ydt):
    return xdt == F32 and ydt == BF16 and D % 512 == 0 and pick_nch(D) <= 8


def coalesced_bwd(D, xdt, dydt, dxdt):
    return xdt == F32 and dydt == BF16 and dxdt == F32 and D % 512 == 0 and pick_nch(D) <= 8


def map_rows(rows, rowmap):
    """Physical row of every logical row under otter_rowmap (grp_rows, grp_stride, row_off)."""
    r = torch.arange(rows)
    if rowmap is None:
        return r
    gr, gs, off = rowmap
    return (r // gr) * gs + off + r % gr


def default_map(rows):
    """Groups of ceil(rows / 2) rows, two gap rows before each group and one more between groups."""
    gr = max(1, cdiv(rows, 2))
    return (gr, gr + 3, 2)


def SUM_DEPTH(D):
    return 8 * cdiv(D, 512) + 6


def COL_DEPTH(rows):
    rch = pick_rch(rows)
    return cdiv(cdiv(rows, rch), 4) + 3 + cdiv(rch, 4) + 2


def row_edges(rows):
    """The rows a column reduction in pick_rch(rows) chunks of four strided waves can lose or double: the first and last row of every row
    chunk, the four residues r % 4 at the start and at the end, and rows - 1."""
    rch = pick_rch(rows)
    per = cdiv(rows, rch)
    e = {rows - 1}
    for k in range(rch):
        r0, r1 = k * per, min(k * per + per, rows)
        if r0 < r1:
            e |= {r0, r1 - 1}
    e |= {r for r in range(4) if r < rows} | {r for r in range(rows - 4, rows) if r >= 0}
    return sorted(e)


# ------------------------------------------------------------------------------------------------------------------ builder conditions

def _is32(t64):
    return torch.equal(t64.float().double(), t64)


def _isdt(t64, dt):
    return torch.equal(t64.float().to(dt).double(), t64)


def _units(t64, unit, dim, what, name):
    """Every value is an integer multiple of `unit` (a power of two, broadcastable) and the sum of the absolute values along `dim`, in
    units, stays below 2^24: the fp32 sum is then exact in any order."""
    q = t64 / unit
    assert torch.equal(q, q.round()), "%s: %s is not a multiple of its unit" % (name, what)
    top = float(q.abs().sum(dim).max())
    assert top < LIMIT, "%s: partial sums of %s may reach %d units" % (name, what, top)


def _bits(t32):
    return t32.contiguous().view(torch.int32)


def bf16_trunc(t64):
    return (_bits(t64.float()) & -65536).view(F32).double()


def bf16_half_up(t64):
    """Round half away from zero on the magnitude (the add-0x8000-and-truncate store)."""
    return ((_bits(t64.float()) + 0x8000) & -65536).view(F32).double()


def bf16_rne(t64):
    return t64.float().to(BF16).double()


def _witnesses(t64, name, what):
    """A bf16 output must hold values a truncating store and values a round-half-up store get wrong."""
    r = bf16_rne(t64)
    assert bool((bf16_trunc(t64) != r).any()), "%s: no %s value tells truncation from nearest-even" % (name, what)
    assert bool((bf16_half_up(t64) != r).any()), "%s: no %s value tells round-half-up from nearest-even" % (name, what)


def _ranks(rows, D, g):
    """rank[r, j]: position of column j in a random order of row r's columns."""
    perm = torch.rand(rows, D, generator=g).argsort(1)
    rank = torch.empty_like(perm)
    rank.scatter_(1, perm, torch.arange(D).expand(rows, D).contiguous())
    return rank


def _row_scales(rows):
    r = torch.arange(rows)
    a = 2.0 ** ((r % 6) - 2).double()                   # 1/4 .. 8, a different one in adjacent rows
    m = (((3 * r + 1) % 7) - 3).double()                # -3 .. 3, period 7 against period 6: 42 different (a, m) pairs
    return a, m


# ------------------------------------------------------------------------------------------------------------------ reference (fp64)

def _eps64(eps):
    return float(torch.tensor(eps, dtype=F32).double())


def reference_fwd(c):
    """fp64 forward of the inputs as stored.  xsum = round_to(fl32(x + delta), stream dtype), as both kernels form it."""
    e = SimpleNamespace(xsum=None, mean=None, left_out=None)
    xs = c.x.double()
    if c.delta is not None:
        xs = (xs + c.delta.double()).float().to(c.xdt).double()
        e.xsum = xs
    if c.op == "ln":
        e.mean = xs.mean(1)
        d = xs - e.mean[:, None]
    else:
        d = xs
    e.var = (d * d).mean(1)
    e.rstd = 1.0 / torch.sqrt(e.var + _eps64(c.eps))
    e.xhat = d * e.rstd[:, None]
    e.xs = xs
    t = e.xhat
    if c.op == "rms" and c.xdt == BF16:                  # HF LlamaRMSNorm: weight * normalised.to(input_dtype)
        a = t.abs()
        lo = bf16_trunc(a)
        ulp = 2.0 ** (torch.floor(torch.log2(lo.clamp(min=1e-300))) - 7)
        mid = lo + ulp / 2
        e.left_out = ((a - mid).abs() <= HF_WINDOW * a) & (a > 0)
        t = bf16_rne(t)
    e.t = t
    y = t
    if c.gamma is not None:
        y = y * c.gamma.double()[None, :]
    if c.beta is not None:
        y = y + c.beta.double()[None, :]
    e.y = y
    return e


def xhat_bwd(c):
    """x^ as the backward kernels form it from the supplied fp32 mean / rstd; a bf16 RMSNorm x^ is rounded fp32 then bf16, as they do."""
    x = c.x.double()
    if c.op == "ln":
        x = x - c.mean.double()[:, None]
    t = x * c.rstd.double()[:, None]
    if c.op == "rms" and c.xdt == BF16:
        t = t.float().to(BF16).double()
    return t


def reference_bwd(c):
    e = SimpleNamespace(dx=None, dgamma=None, dbeta=None)
    dy = c.dy.double()
    e.xhat = xhat_bwd(c)
    e.g = dy * c.gamma.double()[None, :] if c.gamma is not None else dy
    e.m1 = e.g.mean(1) if c.op == "ln" else torch.zeros(c.rows, dtype=torch.float64)
    e.m2 = (e.g * e.xhat).mean(1)
    if c.need_dx:
        e.dx = (e.g - e.m1[:, None] - e.xhat * e.m2[:, None]) * c.rstd.double()[:, None]
        if c.dres is not None:
            e.dx = e.dx + c.dres.double()
    if c.need_dw:
        e.dgamma = (dy * e.xhat).sum(0) + (c.prior_g.double() if c.accumulate else 0.0)
        if c.need_dbeta:
            e.dbeta = dy.sum(0) + (c.prior_b.double() if c.accumulate else 0.0)
    return e


def reference_colsum(c):
    return SimpleNamespace(out=c.src.double().sum(0) + (c.prior.double() if c.accumulate else 0.0))


# ------------------------------------------------------------------------------------------------------------------ builders

def _special_columns(D):
    return [0, 1, 2, 3, D - 4, D - 3, D - 2, D - 1]


def make_fwd(op, rows, D, xdt=F32, ydt=F32, wdt=F32, gamma=True, beta=True, ddt=None, ymap=None, y2=False, stats=True, form="pm",
             entry=None, kind="exact", seed=0):
    """entry: the C function a GPU step calls -- layernorm_fwd / add_layernorm_fwd / rmsnorm_fwd / add_rmsnorm_fwd (default: by op and delta)."""
    assert D % 8 == 0 and op in ("ln", "rms")
    if op == "rms":
        beta, ymap, y2 = False, None, False
        assert gamma
    if entry is None:
        entry = ("add_layernorm_fwd" if ddt is not None else "layernorm_fwd") if op == "ln" else \
            ("rmsnorm_fwd" if (ddt is None and xdt == ydt) else "add_rmsnorm_fwd")
    assert entry != "rmsnorm_fwd" or (xdt == ydt and ddt is None)
    assert entry != "add_layernorm_fwd" or (ymap is None and not y2 and ddt is not None)
    g = _gen(seed * 7919 + rows * 131 + D * 17 + (op == "rms") * 5 + (xdt == BF16) * 3 + (ydt == BF16))
    c = SimpleNamespace(family="fwd", kind=kind, op=op, rows=rows, D=D, xdt=xdt, ydt=ydt, wdt=wdt, ddt=ddt, ymap=ymap, want_y2=y2,
                        stats=stats, form=form, entry=entry, delta=None, gamma=None, beta=None, left_out_share=0.0)
    c.name = "%s %s %s %dx%d %s->%s w=%s%s%s%s%s%s%s" % (
        kind, entry, form if op == "rms" else "balanced", rows, D, dname(xdt), dname(ydt), dname(wdt), "" if gamma else " -gamma",
        "" if beta or op == "rms" else " -beta", " +delta(%s)" % dname(ddt) if ddt is not None else "", " +ymap" if ymap else "",
        " +y2" if y2 else "", "" if stats else " -stats")
    if kind == "general":
        return _general_fwd(c, g, gamma, beta)
    c.eps = 0.0
    a, m = _row_scales(rows)
    rank = _ranks(rows, D, g)
    s = torch.where(rank < D // 2, 1.0, -1.0).double()
    ties = op == "ln" and ddt is not None and xdt == BF16
    if op == "ln":
        if ties:                                             # rows whose values are 256 a / 258 a and 258 a / 260 a
            rr = torch.arange(rows)
            m = torch.where(rr % 3 == 1, 257.0, torch.where(rr % 3 == 2, 259.0, m.float())).double()
        row = a[:, None] * (m[:, None] + s)
        want_mean, want_rstd = a * m, 1.0 / a
    elif form == "pm":
        row = a[:, None] * s
        want_mean, want_rstd = None, 1.0 / a
    else:
        assert form == "ratio" and D % 16 == 0
        row = a[:, None] * s * torch.where(rank % 16 == 15, 7.0, 1.0).double()
        want_mean, want_rstd = None, 1.0 / (2.0 * a)
    if ddt is None:
        x = row
    else:
        step = torch.where(m.abs() > 100, 2.0, 1.0).double()[:, None]          # even deltas where the row values exceed 2^8
        dl = a[:, None] * step * torch.randint(-2, 3, (rows, D), generator=g).double()
        x = row - dl
        if ties:
            t257 = (m == 257)[:, None] & (rank >= D // 2) & (rank < D // 2 + 2)      # value 256 a: 128 a + 129 a = 257 a -> 256 a
            t259 = (m == 259)[:, None] & (rank < 2)                                   # value 260 a: 130 a + 129 a = 259 a -> 260 a
            x = torch.where(t257, 128.0 * a[:, None], torch.where(t259, 130.0 * a[:, None], x))
            dl = torch.where(t257 | t259, 129.0 * a[:, None], dl)
            c.n_ties = int(t257.sum() + t259.sum())
            assert rows < 2 or c.n_ties > 0
        c.delta = dl.to(ddt)
        assert torch.equal(c.delta.double(), dl)
    c.x = x.to(xdt)
    assert torch.equal(c.x.double(), x), "%s: x is not exact in %s" % (c.name, dname(xdt))
    if gamma:
        gm = (torch.randint(1, 5, (D,), generator=g) * (2 * torch.randint(0, 2, (D,), generator=g) - 1)).double()
    if beta:
        bt = torch.randint(-8, 9, (D,), generator=g).double()
    sp = _special_columns(D)
    if op == "ln" and beta:
        if gamma:
            gm[sp] = torch.tensor([1.0, 3.0, 1.0, 3.0] * 2, dtype=torch.float64)
            bt[sp] = torch.tensor([256.0, 256.0, 512.0, 512.0] * 2, dtype=torch.float64)
        else:
            bt[sp] = torch.tensor([256.0, 258.0, 512.0, 512.0] * 2, dtype=torch.float64)
    elif op == "rms" and wdt == F32 and form == "pm":
        gm[sp] = torch.tensor([257.0, 259.0, 513.0, 515.0] * 2, dtype=torch.float64)
    if gamma:
        c.gamma = gm.to(wdt)
        assert torch.equal(c.gamma.double(), gm)
    if beta:
        c.beta = bt.to(wdt)
        assert torch.equal(c.beta.double(), bt)
    e = c.exp = reference_fwd(c)
    # the conditions under which every fp32 kernel has one right answer
    if ddt is not None:
        assert torch.equal(e.xsum, row), "%s: the (rounded) sum is not the constructed row" % c.name
    u = a[:, None]
    _units(e.xs, u, 1, "x", c.name)
    if op == "ln":
        assert torch.equal(e.mean, want_mean)
        _units((e.xs - e.mean[:, None]) ** 2, u * u, 1, "(x - mean)^2", c.name)
    else:
        _units(e.xs ** 2, u * u, 1, "x^2", c.name)
    assert torch.equal(e.rstd, want_rstd) and _is32(e.rstd) and _is32(e.var)
    assert _isdt(e.xhat, xdt if op == "rms" else F32), "%s: x^ is not exact in the stream dtype" % c.name
    assert e.left_out is None or not bool(e.left_out.any()), "%s: x^ next to a bf16 rounding boundary" % c.name
    assert _is32(e.y) and float(e.y.abs().max()) < 2 ** 12
    if ydt == BF16 and ((op == "ln" and beta) or (op == "rms" and wdt == F32 and form == "pm")) and rows >= 2:
        _witnesses(e.y, c.name, "y")
    return c


def _general_fwd(c, g, gamma, beta):
    rows, D = c.rows, c.D
    c.eps = EPS_LN if c.op == "ln" else EPS_RMS
    x = torch.randn(rows, D, generator=g) * 2 + 1.0
    if c.ddt is not None:
        c.delta = torch.randn(rows, D, generator=g).to(c.ddt)
    c.x = x.to(c.xdt)
    if gamma:
        c.gamma = (1 + 0.25 * torch.randn(D, generator=g)).to(c.wdt)
    if beta:
        c.beta = (0.25 * torch.randn(D, generator=g)).to(c.wdt)
    e = c.exp = reference_fwd(c)
    K = SUM_DEPTH(D)
    A1 = e.xs.abs().mean(1)
    sig = torch.sqrt(e.var)
    gm = c.gamma.double().abs()[None, :] if c.gamma is not None else torch.ones(1, D, dtype=torch.float64)
    bt = c.beta.double().abs()[None, :] if c.beta is not None else torch.zeros(1, D, dtype=torch.float64)
    b = c.bound = SimpleNamespace()
    if c.op == "ln":
        e_mu = (K + 1) * U32 * A1 * SLACK
        E_rs = (((K + 4) / 2 + 2.5) * U32 + 0.5 * (e_mu / sig) ** 2) * SLACK
        b.mean = e_mu
    else:
        e_mu = torch.zeros(rows, dtype=torch.float64)
        E_rs = torch.full((rows,), ((K + 2) / 2 + 2.5) * U32 * SLACK, dtype=torch.float64)
    b.rstd = E_rs * e.rstd
    if e.left_out is not None:
        assert ((K + 2) / 2 + 3.5) * U32 <= HF_WINDOW, "%s: x rstd may be off by more than the window left out" % c.name
        c.left_out_share = float(e.left_out.double().mean())
        assert c.left_out_share <= HF_CAP, "%s: %.4f of the elements lie within 2^-20 of a bf16 boundary" % (c.name, c.left_out_share)
        b.y = U32 * e.y.abs() * SLACK
    else:
        nr = 3 if c.op == "ln" else 1                        # x - mean, times rstd, times gamma; RMSNorm: x rstd (times w is the last term)
        b.y = (gm * (e_mu[:, None] * e.rstd[:, None] + e.xhat.abs() * (E_rs[:, None] + nr * U32)) + U32 * (e.xhat.abs() * gm + bt)) * SLACK
    return c


def _fixed_up(rows, D, g, rank):
    """m1, m2 [rows] and h [rows, D]: integers, sum of h over the +1 columns (rank < D / 2) = 0 = sum over the -1 columns."""
    r = torch.arange(rows)
    m1 = (((2 * r + 1) % 5) - 2).double()                   # -2 .. 2
    m2 = (((3 * r + 2) % 7) - 3).double()                   # -3 .. 3
    m2 = torch.where(m2 == 0, 2.0, m2.float()).double()
    m1 = torch.where(m1 == 0, -1.0, m1.float()).double()
    h = torch.randint(-2, 3, (rows, D), generator=g).double()
    half = D // 2
    nf = min(8, half)
    for lo in (0, half):                                      # the +1 columns, then the -1 columns
        side = (rank >= lo) & (rank < lo + half)
        deficit = -(h * side).sum(1)                          # integer
        each = torch.div(deficit, nf, rounding_mode="floor")
        fix = (rank >= lo) & (rank < lo + nf)
        h = h + fix * each[:, None]
        h = h + (rank == lo) * (deficit - nf * each)[:, None]
        assert bool(((h * side).sum(1) == 0).all())
    return m1, m2, h


def make_bwd(op, rows, D, xdt=F32, dydt=F32, dxdt=F32, wdt=F32, gamma=True, dres=True, dx_bf16=False, need_dx=True, need_dw=True,
             need_dbeta=True, accumulate=False, dymap=None, form="random", rstar=None, entry=None, kind="exact", seed=0):
    """entry: layernorm_bwd / rmsnorm_bwd (dy, x and dx of one dtype, no dres, dx and dw always) / rmsnorm_bwd_ex."""
    assert D % 8 == 0 and op in ("ln", "rms") and form in ("random", "count", "onerow", "onehot")
    if op == "rms":
        need_dbeta, dymap = False, None
        assert gamma
    if entry is None:
        entry = "layernorm_bwd" if op == "ln" else "rmsnorm_bwd_ex"
    if entry == "rmsnorm_bwd":
        assert xdt == dydt == dxdt and not dres and not dx_bf16 and need_dx and need_dw
    if entry == "rmsnorm_bwd_ex":
        assert need_dx
    if form == "onehot":
        need_dx = False
    if not need_dx:
        dres, dx_bf16 = False, False
    if not need_dw:
        need_dbeta, accumulate = False, False
    g = _gen(seed * 7919 + rows * 131 + D * 17 + (op == "rms") * 5 + (xdt == BF16) * 3 + (dydt == BF16) + 11)
    c = SimpleNamespace(family="bwd", kind=kind, op=op, rows=rows, D=D, xdt=xdt, dydt=dydt, dxdt=dxdt, wdt=wdt, need_dx=need_dx,
                        need_dw=need_dw, need_dbeta=need_dbeta and op == "ln", accumulate=accumulate, dymap=dymap, form=form, rstar=rstar,
                        entry=entry, want_dxb=dx_bf16, gamma=None, dres=None, prior_g=None, prior_b=None, mean=None)
    c.name = "%s %s %s%s %dx%d x=%s dy=%s dx=%s w=%s%s%s%s%s%s%s%s%s" % (
        kind, entry, form, "" if rstar is None else "(r*=%d)" % rstar, rows, D, dname(xdt), dname(dydt), dname(dxdt), dname(wdt),
        "" if gamma else " -gamma", " +dres" if dres else "", " +dx_bf16" if dx_bf16 else "", "" if need_dx else " -dx",
        "" if need_dw else " -dw", "" if c.need_dbeta or op == "rms" else " -dbeta", " +acc" if accumulate else "", " +dymap" if dymap else "")
    if kind == "general":
        return _general_bwd(c, g, gamma, dres)
    a, m = _row_scales(rows)
    rank = _ranks(rows, D, g) if form in ("random", "onerow") else None
    if form in ("random", "onerow"):
        s = torch.where(rank < D // 2, 1.0, -1.0).double()
    elif form == "count":
        s = torch.ones(rows, D, dtype=torch.float64)
    else:
        s = torch.where(torch.rand(rows, D, generator=g) < 0.5, 1.0, -1.0).double()
    rstd = 1.0 / a
    if op == "ln":
        x = a[:, None] * (m[:, None] + s)
        c.mean = (a * m).float()
    else:
        x = a[:, None] * s
        if xdt == BF16:                                       # x rstd = +-257 / 256: a tie that round_to turns into +-1
            rstd = torch.where(torch.arange(rows) % 2 == 1, rstd * (257.0 / 256.0), rstd)
    c.x = x.to(xdt)
    assert torch.equal(c.x.double(), x)
    c.rstd = rstd.float()
    assert torch.equal(c.rstd.double(), rstd)
    gm = None
    if gamma and form != "count":
        gm = (2.0 ** torch.randint(0, 3, (D,), generator=g).double()) * (2 * torch.randint(0, 2, (D,), generator=g) - 1).double()
    elif gamma:
        gm = torch.ones(D, dtype=torch.float64)
    if form in ("random", "onerow"):
        m1, m2, h = _fixed_up(rows, D, g, rank)
        gg = m1[:, None] + s * m2[:, None] + h
        c.m1, c.m2, c.h = m1, m2, h
        dy = gg / gm[None, :] if gm is not None else gg
        if form == "onerow":
            assert rstar is not None and 0 <= rstar < rows
            keep = (torch.arange(rows) == rstar)[:, None]
            dy = dy * keep
            c.m1, c.m2, c.h = m1 * keep[:, 0], m2 * keep[:, 0], h * keep
    elif form == "count":
        dy = torch.ones(rows, D, dtype=torch.float64)
    else:
        edges = row_edges(rows)
        rs_ = torch.randint(0, rows, (D,), generator=g)
        n = min(D, len(edges))
        rs_[torch.randperm(D, generator=g)[:n]] = torch.tensor(edges[:n])
        c.rstars, c.edges_covered = rs_, n == len(edges)
        v = (2.0 ** torch.randint(0, 3, (D,), generator=g).double()) * (2 * torch.randint(0, 2, (D,), generator=g) - 1).double()
        dy = torch.zeros(rows, D, dtype=torch.float64)
        dy[rs_, torch.arange(D)] = v
    c.dy = dy.to(dydt)
    assert torch.equal(c.dy.double(), dy), "%s: dy is not exact in %s" % (c.name, dname(dydt))
    if gm is not None:
        c.gamma = gm.to(wdt)
    if dres:
        e_ = torch.randint(-16, 17, (rows, D), generator=g).double()
        sp = torch.rand(rows, D, generator=g)
        e_ = torch.where(sp < 0.03, 256.0, torch.where(sp < 0.06, 512.0, e_.float())).double()
        dr = e_ * (1.0 / a)[:, None]
        c.dres = dr.to(dxdt)
        assert torch.equal(c.dres.double(), dr)
    if accumulate:
        c.prior_g = torch.randint(-64, 65, (D,), generator=g).float()
        c.prior_b = torch.randint(-64, 65, (D,), generator=g).float()
    e = c.exp = reference_bwd(c)
    assert _isdt(e.xhat, F32) and float(e.xhat.abs().max()) == 1.0, "%s: x^ is not +-1" % c.name
    if need_dx:
        _units(e.g, torch.tensor(1.0, dtype=torch.float64), 1, "g", c.name)
        _units(e.g * e.xhat, torch.tensor(1.0, dtype=torch.float64), 1, "g x^", c.name)
        assert torch.equal(e.m2, e.m2.round()) and torch.equal(e.m1, e.m1.round())
        if form in ("random", "onerow"):
            assert torch.equal(e.m2, c.m2) and (op == "rms" or torch.equal(e.m1, c.m1))
            core = c.h + (c.m1[:, None] if op == "rms" else 0.0)
            if form == "onerow":
                core = core * keep
            want = core * rstd[:, None] + (c.dres.double() if dres else 0.0)
            assert torch.equal(e.dx, want), "%s: dx is not h rstd + dres" % c.name
        assert _is32(e.dx), "%s: dx is not exact in fp32" % c.name
        if dres and rows * D >= 2048 and (dxdt == BF16 or dx_bf16):
            _witnesses(e.dx, c.name, "dx")
    if need_dw:
        _units(dy * e.xhat, torch.tensor(0.25, dtype=torch.float64), 0, "dy x^", c.name)
        assert _is32(e.dgamma) and (e.dbeta is None or _is32(e.dbeta))
        if form == "count" and not accumulate:
            assert bool((e.dgamma == rows).all()) and (e.dbeta is None or bool((e.dbeta == rows).all()))
    return c


def _general_bwd(c, g, gamma, dres):
    rows, D = c.rows, c.D
    x = (torch.randn(rows, D, generator=g) * 2 + 1.0).to(c.xdt)
    c.x = x
    xd = x.double()
    eps = _eps64(EPS_LN if c.op == "ln" else EPS_RMS)
    if c.op == "ln":
        mu = xd.mean(1)
        c.mean = mu.float()
        c.rstd = (1.0 / torch.sqrt(((xd - mu[:, None]) ** 2).mean(1) + eps)).float()
    else:
        c.rstd = (1.0 / torch.sqrt((xd * xd).mean(1) + eps)).float()
    c.dy = torch.randn(rows, D, generator=g).to(c.dydt)
    if gamma:
        c.gamma = (1 + 0.25 * torch.randn(D, generator=g)).to(c.wdt)
    if dres:
        c.dres = torch.randn(rows, D, generator=g).to(c.dxdt)
    if c.accumulate:
        c.prior_g = torch.randn(D, generator=g) * 5
        c.prior_b = torch.randn(D, generator=g) * 5
    e = c.exp = reference_bwd(c)
    K, Kc = SUM_DEPTH(D), COL_DEPTH(rows)
    b = c.bound = SimpleNamespace()
    rs = c.rstd.double()[:, None]
    if c.need_dx:
        e1 = (K + 2) * U32 * e.g.abs().mean(1)[:, None] if c.op == "ln" else 0.0
        e2 = (K + 5) * U32 * (e.g * e.xhat).abs().mean(1)[:, None]
        S = e.g.abs() + e.m1.abs()[:, None] + (e.xhat * e.m2[:, None]).abs()
        b.dx = (rs * (e1 + e.xhat.abs() * e2 + 6 * U32 * S) + U32 * e.dx.abs()) * SLACK
    if c.need_dw:
        dy = c.dy.double()
        acc_g = U32 * (c.prior_g.double().abs() + (dy * e.xhat).sum(0).abs()) if c.accumulate else 0.0
        b.dgamma = ((Kc + 4) * U32 * (dy * e.xhat).abs().sum(0) + acc_g) * SLACK
        if c.need_dbeta:
            acc_b = U32 * (c.prior_b.double().abs() + dy.sum(0).abs()) if c.accumulate else 0.0
            b.dbeta = (Kc * U32 * dy.abs().sum(0) + acc_b) * SLACK
    return c


def make_colsum(rows, D, sdt=F32, smap=None, accumulate=False, form="random", rstar=None, kind="exact", seed=0):
    assert D % 8 == 0
    g = _gen(seed * 7919 + rows * 131 + D * 17 + (sdt == BF16) + 23)
    c = SimpleNamespace(family="colsum", kind=kind, rows=rows, D=D, sdt=sdt, smap=smap, accumulate=accumulate, form=form, rstar=rstar, prior=None)
    c.name = "%s colsum %s%s %dx%d %s%s%s" % (kind, form, "" if rstar is None else "(r*=%d)" % rstar, rows, D, dname(sdt),
                                              " +acc" if accumulate else "", " +map" if smap else "")
    if kind == "general":
        c.src = torch.randn(rows, D, generator=g).to(sdt)
        if accumulate:
            c.prior = torch.randn(D, generator=g) * 5
        c.exp = reference_colsum(c)
        s = c.src.double()
        acc = U32 * (c.prior.double().abs() + s.sum(0).abs()) if accumulate else 0.0
        c.bound = SimpleNamespace(out=(COL_DEPTH(rows) * U32 * s.abs().sum(0) + acc) * SLACK)
        return c
    if form == "random":
        src = torch.randint(-4, 5, (rows, D), generator=g).double()
    elif form == "count":
        src = torch.ones(rows, D, dtype=torch.float64)
    elif form == "onerow":
        src = torch.zeros(rows, D, dtype=torch.float64)
        src[rstar] = torch.randint(1, 5, (D,), generator=g).double()
    else:
        edges = row_edges(rows)
        rs_ = torch.randint(0, rows, (D,), generator=g)
        n = min(D, len(edges))
        rs_[torch.randperm(D, generator=g)[:n]] = torch.tensor(edges[:n])
        c.rstars, c.edges_covered = rs_, n == len(edges)
        src = torch.zeros(rows, D, dtype=torch.float64)
        src[rs_, torch.arange(D)] = torch.randint(1, 5, (D,), generator=g).double()
    c.src = src.to(sdt)
    assert torch.equal(c.src.double(), src)
    if accumulate:
        c.prior = torch.randint(-64, 65, (D,), generator=g).float()
    _units(src, torch.tensor(1.0, dtype=torch.float64), 0, "src", c.name)
    c.exp = reference_colsum(c)
    assert _is32(c.exp.out)
    if form == "count" and not accumulate:
        assert bool((c.exp.out == rows).all())
    return c


# ------------------------------------------------------------------------------------------------------------------ frames

OUTPUTS = {"fwd": ("xsum", "mean", "rstd", "y", "y2"), "bwd": ("dx", "dx_bf16", "dgamma", "dbeta"), "colsum": ("out",)}


class Placed:
    """The case in memory, as a kernel gets it.  Every tensor is `rows` rows of a buffer [guard + physical rows + guard, cols] -- vectors are
    one row -- with guard >= 2 rows and >= 1024 elements (two 512-column chunks).  Outputs lie in buffers filled with SENT (the prior of an
    accumulate case copied in), inputs in buffers filled with NaN.  Behind a row map the logical rows are scattered over the physical rows
    and the gaps between the groups belong to the frame.  base[name] is what a kernel is handed (physical row 0), get / put read and write
    the logical rows; result() checks that everything outside them still holds SENT."""

    def __init__(self, c, device="cpu"):
        self.case, self.device = c, device
        self.full, self.base, self.rows_of, self.inside, self.outputs = {}, {}, {}, {}, []
        nan = float("nan")
        if c.family == "fwd":
            self._alloc("x", c.x, nan)
            for nm in ("delta", "gamma", "beta"):
                if getattr(c, nm) is not None:
                    self._alloc(nm, getattr(c, nm), nan)
            if c.ddt is not None:
                self._out("xsum", c.rows, c.D, c.xdt)
            if c.stats:
                if c.op == "ln":
                    self._out("mean", 1, c.rows, F32)
                self._out("rstd", 1, c.rows, F32)
            self._out("y", c.rows, c.D, c.ydt, c.ymap)
            if c.want_y2:
                self._out("y2", c.rows, c.D, c.ydt)
        elif c.family == "bwd":
            self._alloc("x", c.x, nan)
            self._alloc("dy", c.dy, nan, c.dymap)
            for nm in ("gamma", "mean", "rstd", "dres"):
                if getattr(c, nm) is not None:
                    self._alloc(nm, getattr(c, nm), nan)
            if c.need_dx:
                self._out("dx", c.rows, c.D, c.dxdt)
            if c.want_dxb:
                self._out("dx_bf16", c.rows, c.D, BF16)
            if c.need_dw:
                self._out("dgamma", 1, c.D, F32)
                if c.need_dbeta:
                    self._out("dbeta", 1, c.D, F32)
        else:
            self._alloc("src", c.src, nan, c.smap)
            self._out("out", 1, c.D, F32)
        self.reset()

    def _buffer(self, nm, rows, cols, dtype, fill, rowmap):
        guard = max(2, cdiv(1024, cols))
        idx = map_rows(rows, rowmap)
        phys = int(idx.max()) + 1 + (1 if rowmap is not None else 0)
        self.full[nm] = torch.full((phys + 2 * guard, cols), fill, dtype=dtype, device=self.device)
        self.base[nm] = self.full[nm][guard:guard + phys]
        self.rows_of[nm] = idx.to(self.device)
        inside = torch.zeros(phys + 2 * guard, dtype=torch.bool, device=self.device)
        inside[guard + self.rows_of[nm]] = True
        self.inside[nm] = inside

    def _alloc(self, nm, t, fill, rowmap=None):
        t2 = t if t.dim() == 2 else t[None, :]
        self._buffer(nm, t2.shape[0], t2.shape[1], t.dtype, fill, rowmap)
        self.put(nm, t2.to(self.device))

    def _out(self, nm, rows, cols, dtype, rowmap=None):
        self._buffer(nm, rows, cols, dtype, SENT, rowmap)
        self.outputs.append(nm)

    def has(self, nm):
        return nm in self.base

    def ptr(self, nm):
        return self.base[nm].data_ptr() if nm in self.base else None

    def get(self, nm):
        """The logical rows (a copy); a vector comes back 1-D."""
        t = self.base[nm][self.rows_of[nm]]
        return t[0] if nm in ("gamma", "beta", "mean", "rstd", "dgamma", "dbeta", "out") else t

    def put(self, nm, t):
        self.base[nm][self.rows_of[nm]] = (t if t.dim() == 2 else t[None, :]).to(self.base[nm].dtype)

    def reset(self):
        c = self.case
        for nm in self.outputs:
            self.full[nm].fill_(SENT)
        if getattr(c, "accumulate", False):
            if c.family == "bwd":
                self.put("dgamma", c.prior_g.to(self.device))
                if c.need_dbeta:
                    self.put("dbeta", c.prior_b.to(self.device))
            else:
                self.put("out", c.prior.to(self.device))

    def result(self):
        """Result of the launch that just ran (copies), after checking the frames: every element outside the logical rows must be SENT."""
        res = Result(**{nm: None for nm in OUTPUTS[self.case.family]})
        for nm in self.outputs:
            f = self.full[nm]
            outside = f[~self.inside[nm]]
            ok = outside == SENT
            if not bool(ok.all()):
                rows = (~self.inside[nm]).nonzero()[:, 0]
                i = (~ok).nonzero()[0].tolist()
                guard = (f.shape[0] - self.base[nm].shape[0]) // 2
                raise CheckFailure(FRAME_WRITTEN, "%s: %s buffer row %d column %d holds %r (physical row 0 of the tensor is buffer row %d)"
                                   % (self.case.name, nm, int(rows[i[0]]), i[1], float(outside[i[0], i[1]]), guard))
            setattr(res, nm, self.get(nm).clone())
        return res


# ------------------------------------------------------------------------------------------------------------------ checkers

def _where(bad):
    i = bad.nonzero()
    return "%d elements, first at %s" % (i.shape[0], tuple(i[0].tolist()))


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


def worst_table():
    rows = ["[norm-exact] %-8s %-34s %-8s worst error / bound %.3f" % (k + (v,)) for k, v in sorted(WORST.items())]
    return "\n".join(rows) if rows else "[norm-exact] no toleranced check ran"


def _basic(c, res, skip=()):
    for nm in OUTPUTS[c.family]:
        t = getattr(res, nm)
        if t is None or nm in skip:
            continue
        if bool(torch.isnan(t).any()):
            raise CheckFailure(READ_OUTSIDE, "%s: NaN in %s, %s" % (c.name, nm, _where(torch.isnan(t))))
        if bool((t == SENT).any()):
            raise CheckFailure(NOT_WRITTEN, "%s: %s, %s" % (c.name, nm, _where(t == SENT)))


def _exact(c, got, want64, nm):
    assert _is32(want64), "%s: the expected %s is not exact in fp32" % (c.name, nm)
    want = want64.float().to(got.dtype).to(got.device)                 # fp64 -> fp32 exact; -> bf16 rounds to nearest even
    if not torch.equal(got, want):
        bad = got != want
        i = tuple(bad.nonzero()[0].tolist())
        raise CheckFailure(EXACT_REASON[nm], "%s: %s, %s: got %r, exact %r" % (c.name, nm, _where(bad), float(got[i]), float(want[i])))


def _what(c):
    if c.family == "fwd":
        return "%s %s->%s%s" % (c.entry, dname(c.xdt), dname(c.ydt), " c" if coalesced_fwd(c.D, c.xdt, c.ydt) else "")
    if c.family == "bwd":
        return "%s %s<-%s%s" % (c.entry, dname(c.xdt), dname(c.dydt), " c" if coalesced_bwd(c.D, c.xdt, c.dydt, c.dxdt) else "")
    return "colsum %s" % dname(c.sdt)


def _bounded(c, got, want64, bound64, nm, ceil_key, keep=None):
    want64, bound64 = want64.to(got.device), bound64.to(got.device)
    if got.dtype == BF16:
        bound64 = bound64 + HBF * (want64.abs() + bound64)
    bound64 = torch.minimum(bound64, torch.full_like(bound64, CEILING[ceil_key] * float(want64.abs().max())))
    err = (got.double() - want64).abs()
    if keep is not None:
        err = err * keep.to(got.device)
    ratio = float((err / bound64.clamp(min=1e-300)).max())
    bad = err > bound64
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise CheckFailure(BEYOND_BOUND, "%s: %s, %s: got %r, reference %r, bound %.3g (worst error / bound %.3f)"
                           % (c.name, nm, _where(bad), float(got[i]), float(want64[i]), float(bound64[i]), ratio))
    _note((c.family, _what(c), nm), ratio)
    return ratio


def _same_bits(c, a, b, what):
    view = torch.int16 if a.dtype == BF16 else torch.int32
    if a.dtype != b.dtype or not torch.equal(a.contiguous().view(view), b.contiguous().view(view)):
        raise CheckFailure(Y2_DIFFERS, "%s: %s, %s" % (c.name, what, _where(a != b)))


def check(c, res):
    """Every result of one launch: bit equality for the exact kinds (xsum always), the per-element bounds of the module docstring for the
    general kind.  Returns the worst error / bound of the toleranced part (0: none)."""
    _basic(c, res)
    e, worst = c.exp, 0.0
    exact = c.kind == "exact"
    if c.family == "fwd":
        if res.xsum is not None:
            _exact(c, res.xsum, e.xsum, "xsum")
        stats = [("mean", e.mean, "mean"), ("rstd", e.rstd, "rstd")]
        for nm, want, key in stats:
            got = getattr(res, nm)
            if got is None:
                continue
            if exact:
                _exact(c, got, want, nm)
            else:
                worst = max(worst, _bounded(c, got, want, getattr(c.bound, nm), nm, key))
        if exact:
            _exact(c, res.y, e.y, "y")
        else:
            keep = None if e.left_out is None else (~e.left_out).double()
            worst = max(worst, _bounded(c, res.y, e.y, c.bound.y, "y", "y_bf16" if c.ydt == BF16 else "y_f32", keep))
        if res.y2 is not None:
            _same_bits(c, res.y, res.y2, "y2 against y")
    elif c.family == "bwd":
        if res.dx is not None:
            if exact:
                _exact(c, res.dx, e.dx, "dx")
            else:
                worst = max(worst, _bounded(c, res.dx, e.dx, c.bound.dx, "dx", "dx_bf16" if c.dxdt == BF16 else "dx_f32"))
        if res.dx_bf16 is not None:
            if exact:
                _exact(c, res.dx_bf16, e.dx, "dx_bf16")
            elif c.dxdt == F32:                                     # one pass: the copy is the nearest-even cast of the dx just stored
                if not torch.equal(res.dx_bf16, res.dx.to(BF16)):
                    raise CheckFailure(DXB_NOT_EXACT, "%s: %s" % (c.name, _where(res.dx_bf16 != res.dx.to(BF16))))
            else:
                worst = max(worst, _bounded(c, res.dx_bf16, e.dx, c.bound.dx, "dx_bf16", "dx_bf16"))
        for nm in ("dgamma", "dbeta"):
            got = getattr(res, nm)
            if got is None:
                continue
            if exact:
                _exact(c, got, getattr(e, nm), nm)
            else:
                worst = max(worst, _bounded(c, got, getattr(e, nm), getattr(c.bound, nm), nm, nm))
    else:
        if exact:
            _exact(c, res.out, e.out, "out")
        else:
            worst = _bounded(c, res.out, e.out, c.bound.out, "out", "out")
    return worst


def run_case(c, step, device="cpu", placed=None):
    """Places the case, runs `step(placed)`, checks the frames and every result.  Returns (Result, worst error / bound)."""
    p = placed or Placed(c, device)
    p.reset()
    step(p)
    res = p.result()
    return res, check(c, res)


# ------------------------------------------------------------------------------------------------------------------ the cases of the GPU file

def fwd_cases(D, rows=None):
    """Every dtype route and weight dtype at one D, each option present and absent: [(id, kwargs of make_fwd)]."""
    out = []
    for i, (xdt, ydt) in enumerate(ROUTES):
        for wdt in (F32, BF16):
            r = rows or (5 if (i + (wdt == BF16)) % 2 else 6)
            k = dict(rows=r, D=D, xdt=xdt, ydt=ydt, wdt=wdt)
            out.append(dict(op="ln", ymap=default_map(r), y2=True, **k))
            out.append(dict(op="ln", ddt=BF16 if wdt == BF16 else F32, **k))
            out.append(dict(op="ln", ddt=F32 if wdt == BF16 else BF16, stats=False, beta=False, **k))
            if wdt == F32:
                out.append(dict(op="ln", gamma=False, y2=True, **k))
                out.append(dict(op="ln", gamma=False, beta=False, stats=False, ymap=default_map(r), **k))
            if xdt == ydt:
                out.append(dict(op="rms", form="pm", **k))
            out.append(dict(op="rms", form="ratio" if D % 16 == 0 else "pm", entry="add_rmsnorm_fwd", **k))
            out.append(dict(op="rms", form="pm", ddt=BF16 if wdt == F32 else F32, **k))
    return out


def bwd_cases(D, rows=None):
    out = []
    for i, (xdt, dydt) in enumerate(ROUTES):
        for wdt in (F32, BF16):
            r = rows or (5 if (i + (wdt == BF16)) % 2 else 6)
            for dxdt in ((xdt,) if xdt == F32 else (BF16, F32)):
                k = dict(rows=r, D=D, xdt=xdt, dydt=dydt, dxdt=dxdt, wdt=wdt)
                out.append(dict(op="ln", dres=True, dx_bf16=True, dymap=default_map(r), **k))
                out.append(dict(op="ln", dres=False, need_dbeta=False, accumulate=True, **k))
                if wdt == F32:
                    out.append(dict(op="ln", gamma=False, need_dw=False, **k))
                    out.append(dict(op="ln", need_dx=False, **k))
                out.append(dict(op="rms", dres=True, dx_bf16=True, need_dw=True, **k))
                out.append(dict(op="rms", dres=False, need_dw=False, **k))
                if xdt == dydt == dxdt:
                    out.append(dict(op="rms", entry="rmsnorm_bwd", dres=False, **k))
    return out


def edge_row_cases(rows):
    """dgamma / dbeta at one row count on both sides of a pick_rch edge: [(kwargs of make_bwd)]."""
    out = []
    big = rows > 4096
    for D in EDGE_D:
        dydt = BF16 if D == 512 else F32
        k = dict(rows=rows, D=D, xdt=F32, dydt=dydt, dxdt=F32)
        out.append(dict(op="ln", form="random", **k))
        if big and D == 512:                                  # the dw kernels do not depend on the dx route: one large case is enough
            continue
        out.append(dict(op="ln", form="count", accumulate=True, gamma=False, dres=False, **k))
        out.append(dict(op="ln", form="onehot", dymap=default_map(rows), **k))
        if D == 520:
            out.append(dict(op="rms", form="random", need_dw=True, accumulate=True, xdt=BF16, dydt=BF16, dxdt=BF16, rows=rows, D=D))
        if D == 520 and not big:
            out.append(dict(op="ln", form="count", need_dbeta=False, need_dx=False, **k))
            out.append(dict(op="rms", form="count", need_dw=True, dres=False, **k))
        if not big and D == 520:
            for rstar in row_edges(rows):
                out.append(dict(op="ln", form="onerow", rstar=rstar, need_dx=(rstar % 4 == 0), dres=False, **k))
    return out


def edge_colsum_cases(rows):
    out = []
    for sdt in (F32, BF16):
        k = dict(rows=rows, D=520, sdt=sdt)
        out.append(dict(form="random", accumulate=True, **k))
        out.append(dict(form="count", **k))
        out.append(dict(form="onehot", smap=default_map(rows), **k))
        if rows <= 4096:
            for rstar in row_edges(rows):
                out.append(dict(form="onerow", rstar=rstar, **k))
    return out


def general_cases():
    """(family, kwargs).  The last forward case is HF's RMSNorm rounding: bf16 x, fp32 y through add_rmsnorm_fwd."""
    out = []
    for D in (520, 1024, 4104):
        for xdt, ydt in ROUTES:
            out.append(("fwd", dict(op="ln", rows=9, D=D, xdt=xdt, ydt=ydt, kind="general", ymap=default_map(9), y2=True)))
            out.append(("fwd", dict(op="ln", rows=9, D=D, xdt=xdt, ydt=ydt, ddt=BF16, kind="general")))
            if xdt == F32:
                out.append(("fwd", dict(op="rms", rows=9, D=D, xdt=xdt, ydt=ydt, ddt=BF16, kind="general")))
            dxs = (F32,) if xdt == F32 else (BF16, F32)
            for dxdt in dxs:
                out.append(("bwd", dict(op="ln", rows=67, D=D, xdt=xdt, dydt=ydt, dxdt=dxdt, dx_bf16=True, accumulate=(D == 520), kind="general")))
                out.append(("bwd", dict(op="rms", rows=67, D=D, xdt=xdt, dydt=ydt, dxdt=dxdt, need_dw=True, kind="general")))
    for D in (520, 1024):
        for seed in (0, 1):
            out.append(("fwd", dict(op="rms", rows=33, D=D, xdt=BF16, ydt=F32, entry="add_rmsnorm_fwd", kind="general", seed=seed)))
        out.append(("fwd", dict(op="rms", rows=33, D=D, xdt=BF16, ydt=BF16, kind="general")))
    for sdt in (F32, BF16):
        out.append(("colsum", dict(rows=300, D=520, sdt=sdt, accumulate=True, kind="general")))
    return out


def make(family, kw):
    return {"fwd": make_fwd, "bwd": make_bwd, "colsum": make_colsum}[family](**kw)
