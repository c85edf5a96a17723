"""tests/_norm_cases.py judged on the CPU: its checkers pass on a plain fp64 step and on a kernel-shaped fp32 step (512-column chunks, 8 per
lane or 4 + 4 per lane, serial lane sums and a six-level butterfly, blocks of four waves striding the rows, pick_rch row chunks with an LDS
fold and the four-thread final reduction of csrc/norm.hip), every builder condition holds at every shape tests/test_gpu_norm_exact.py
visits, and each deliberately wrong step makes the checker NAMED beside it fail -- an arithmetic fault by an arithmetic check, never by
the output frames."""
from types import SimpleNamespace

import pytest
import torch

from tests import _norm_cases as C

BF16, F32 = C.BF16, C.F32


# ------------------------------------------------------------------------------------------------------------------ plain fp64 step

def _inputs(p, names):
    return {nm: (p.get(nm).cpu() if p.has(nm) else None) for nm in names}


def plain_step(p):
    c = p.case
    if c.family == "fwd":
        ns = SimpleNamespace(op=c.op, xdt=c.xdt, eps=c.eps, **_inputs(p, ("x", "delta", "gamma", "beta")))
        e = C.reference_fwd(ns)
        outs = dict(xsum=e.xsum, mean=e.mean, rstd=e.rstd, y=e.y, y2=e.y)
    elif c.family == "bwd":
        ns = SimpleNamespace(op=c.op, xdt=c.xdt, rows=c.rows, need_dx=c.need_dx, need_dw=c.need_dw, need_dbeta=c.need_dbeta,
                             accumulate=c.accumulate, prior_g=p.get("dgamma").cpu() if c.need_dw else None,
                             prior_b=p.get("dbeta").cpu() if c.need_dbeta else None, **_inputs(p, ("x", "dy", "gamma", "mean", "rstd", "dres")))
        e = C.reference_bwd(ns)
        outs = dict(dx=e.dx, dx_bf16=e.dx, dgamma=e.dgamma, dbeta=e.dbeta)
    else:
        ns = SimpleNamespace(src=p.get("src").cpu(), accumulate=c.accumulate, prior=p.get("out").cpu())
        outs = dict(out=C.reference_colsum(ns).out)
    for nm, t in outs.items():
        if p.has(nm) and nm in p.outputs:
            p.put(nm, t.float())                              # fp64 -> fp32 (exact for the exact kinds), put() rounds to bf16 (nearest even)


# ------------------------------------------------------------------------------------------------------------------ kernel-shaped fp32 step

def _own(D, coalesced):
    """cols[lane, k]: the columns a lane adds up, in its order.  Generic: 8 consecutive per chunk; coalesced: 4 + 4, 256 apart."""
    nch = C.cdiv(D, 512)
    lane = torch.arange(64)[:, None]
    k = torch.arange(nch * 8)[None, :]
    ch, i = k // 8, k % 8
    if coalesced:
        return ch * 512 + (i // 4) * 256 + lane * 4 + i % 4
    return ch * 512 + lane * 8 + i


def _wave_sum(vals, drop_last_lane=False):
    """vals [rows, 64, n] fp32: each lane adds its n values in order, then the xor butterfly 32, 16, .. 1; lane 0's total."""
    s = torch.zeros(vals.shape[:2], dtype=F32)
    for k in range(vals.shape[2]):
        s = s + vals[:, :, k]
    if drop_last_lane:
        s[:, 63] = 0
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, 0]


def _by_lane(t, cols):
    """t [rows, D] -> [rows, 64, n], zeros where a lane's column lies past D (the kernel's col < D test)."""
    D = t.shape[1]
    pad = torch.zeros(t.shape[0], int(cols.max()) + 1, dtype=F32)
    pad[:, :D] = t
    return pad[:, cols]


def _by_lane_unmasked(p, nm, cols):
    """The same without the col < D test: what lies behind a row in memory (the next row, NaN behind the last)."""
    c = p.case
    f = p.full[nm]
    guard = (f.shape[0] - p.base[nm].shape[0]) // 2
    flat = f.reshape(-1).float()
    idx = (guard + torch.arange(c.rows))[:, None, None] * c.D + cols[None]
    return flat[idx]


def _round_to(t, dt):
    return t.to(dt).float()


def _trunc_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(F32)


def _col_reduce(term, rows, bug, prior):
    """dgamma / dbeta / colsum: partial kernel (pick_rch chunks, four waves striding a chunk's rows, serial LDS fold) into a workspace that
    holds stale values, then the final kernel (four threads per column, k = j, j + 4, ..)."""
    D = term.shape[1]
    rch = C.pick_rch(rows)
    per = C.cdiv(rows, rch)
    r0 = torch.arange(rch) * per
    r1 = torch.clamp(r0 + per, max=rows)
    acc = torch.zeros(rch, 4, D, dtype=F32)
    wave = torch.arange(4)[None, :]
    for t in range(C.cdiv(per, 4)):
        r = r0[:, None] + wave + 4 * t
        ok = r < r1[:, None]
        if bug == "last row of a row chunk lost":
            ok = ok & (r < (r1 - 1)[:, None])
        if bug == "wave 3's rows lost":
            ok = ok & (wave != 3)
        acc = acc + term[r.clamp(max=rows - 1)] * ok[:, :, None]
    folded = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    part = torch.full((rch, D), 7.0, dtype=F32)             # a workspace another call has used
    written = (r0 < rows) if bug == "empty trailing chunks left unwritten" else torch.ones(rch, dtype=torch.bool)
    part[written] = folded[written]
    n = rch // 4 * 4 if bug == "final reduction rounds rch down to a multiple of 4" else rch
    s = torch.zeros(4, D, dtype=F32)
    for j in range(4):
        for k in range(j, n, 4):
            s[j] = s[j] + part[k]
    total = (s[0] + s[1]) + (s[2] + s[3])
    if prior is not None and bug != "accumulate ignored":
        total = prior + total
    return total


def kernel_step(bug=None):
    def step(p):
        c = p.case
        if c.family == "colsum":
            p.put("out", _col_reduce(p.get("src").float(), c.rows, bug, p.get("out") if c.accumulate else None))
            return
        rows, D = c.rows, c.D
        x = p.get("x").float()
        if c.family == "fwd":
            cols = _own(D, C.coalesced_fwd(D, c.xdt, c.ydt))
            rms = c.op == "rms"
            v = stat = x
            if p.has("delta"):
                v = x + p.get("delta").float()
                stat = _round_to(v, c.xdt)
                if bug == "xsum not rounded to the stream dtype":
                    stat = v                                  # the store rounds, the registers do not
                if bug == "statistics taken before the add":
                    stat = x
                v = _round_to(v, c.xdt)
                p.put("xsum", v)
            lanes = _by_lane(stat, cols)
            if bug == "statistics of a chunk taken past D":
                lanes = _by_lane_unmasked(p, "x", cols)
            s = _wave_sum(lanes * lanes if rms else lanes, drop_last_lane=(bug == "last lane's columns left out of the mean"))
            Df = torch.tensor(float(D), dtype=F32)
            if rms:
                mu, var = torch.zeros(rows, dtype=F32), s / Df
            else:
                mu = s / Df
                d = torch.where(cols[None] < D, lanes - mu[:, None, None], torch.zeros((), dtype=F32))
                var = _wave_sum(d * d) / Df
            rs = 1.0 / torch.sqrt(var + torch.tensor(c.eps, dtype=F32))
            t = (v - mu[:, None]) * rs[:, None]
            if rms:
                t = _round_to(t, c.xdt)
            if p.has("gamma"):
                g = p.get("gamma").float()
                if bug == "the two 256-column halves swapped for gamma":
                    g = g[torch.arange(D) ^ 256]
                t = t * g[None, :]
            if p.has("beta"):
                t = t + p.get("beta").float()[None, :]
            if bug == "truncating bf16 store":
                t = _trunc_bf16(t)
            mapped = C.map_rows(rows, c.ymap)
            if bug == "y written at the plain row":
                p.base["y"][torch.arange(rows)] = t.to(c.ydt)
            else:
                p.put("y", t)
            if bug == "stores a chunk past D":
                guard = (p.full["y"].shape[0] - p.base["y"].shape[0]) // 2
                p.full["y"].view(-1)[(guard + int(mapped[-1]) + 1) * D:(guard + int(mapped[-1]) + 1) * D + 8] = 0
            at_mapped = bug == "y2, mean and rstd written at the mapped row"
            for nm, val in (("y2", t), ("mean", mu), ("rstd", rs)):
                if not p.has(nm):
                    continue
                if at_mapped:
                    f = p.full[nm]
                    guard = (f.shape[0] - p.base[nm].shape[0]) // 2
                    if val.dim() == 2:
                        f[guard + mapped] = val.to(f.dtype)
                    else:
                        f.view(-1)[guard * f.shape[1] + mapped] = val
                else:
                    p.put(nm, val)
            return
        # backward
        rms = c.op == "rms"
        cols = _own(D, C.coalesced_bwd(D, c.xdt, c.dydt, c.dxdt))
        dy = p.get("dy").float()
        rs = p.get("rstd").float()
        mu = torch.zeros(rows, dtype=F32) if rms else p.get("mean").float()
        t = (x - mu[:, None]) * rs[:, None]
        if rms and bug != "RMS without round_to":
            t = _round_to(t, c.xdt)
        gg = dy * p.get("gamma").float()[None, :] if p.has("gamma") else dy
        Df = torch.tensor(float(D), dtype=F32)
        if c.need_dx:
            m1 = _wave_sum(_by_lane(gg, cols)) / Df
            if rms and bug != "RMS with m1 != 0":
                m1 = torch.zeros(rows, dtype=F32)
            m2 = _wave_sum(_by_lane(gg * t, cols)) / Df
            u = (gg - m1[:, None] - t * m2[:, None]) * rs[:, None]
            pre = u
            if p.has("dres") and bug != "dres dropped":
                u = u + p.get("dres").float()
            p.put("dx", u)
            if p.has("dx_bf16"):
                p.put("dx_bf16", pre if bug == "dx_bf16 taken before dres" else u)
        if c.need_dw:
            term = dy if bug == "dgamma taken without x^" else dy * t
            p.put("dgamma", _col_reduce(term, rows, bug, p.get("dgamma") if c.accumulate else None))
            if c.need_dbeta:
                p.put("dbeta", _col_reduce(dy, rows, bug, p.get("dbeta") if c.accumulate else None))
    return step


def _run(family, kw, step):
    return C.run_case(C.make(family, kw), step)


# ------------------------------------------------------------------------------------------------------------------ the steps that are right

@pytest.mark.parametrize("D", C.D_LIST)
def test_row_kernel_cases_build_and_pass(D):
    """Every forward and backward case of the GPU file at this D: the builder conditions hold (the builders assert them), the plain fp64
    step and the kernel-shaped fp32 step give the exact answers, frames intact."""
    for kw in C.fwd_cases(D):
        c = C.make_fwd(**kw)
        C.run_case(c, plain_step)
        C.run_case(c, kernel_step())
    for kw in C.bwd_cases(D):
        c = C.make_bwd(**kw)
        C.run_case(c, plain_step)
        C.run_case(c, kernel_step())


@pytest.mark.parametrize("rows", C.SMALL_ROWS)
def test_few_rows_cases_build_and_pass(rows):
    for D in C.SMALL_ROWS_D:
        for family, cases in (("fwd", C.fwd_cases(D, rows)), ("bwd", C.bwd_cases(D, rows))):
            for kw in cases:
                c = C.make(family, kw)
                C.run_case(c, plain_step)
                C.run_case(c, kernel_step())


@pytest.mark.parametrize("rows", C.EDGE_ROWS)
def test_row_chunk_edge_cases_build_and_pass(rows):
    """dgamma / dbeta and colsum on both sides of every pick_rch edge; the one-hot form covers every row of row_edges() in one case."""
    for family, cases in (("bwd", C.edge_row_cases(rows)), ("colsum", C.edge_colsum_cases(rows))):
        for kw in cases:
            c = C.make(family, kw)
            if c.form == "onehot":
                assert c.edges_covered and set(C.row_edges(rows)) <= set(c.rstars.tolist())
            C.run_case(c, plain_step)
            if rows < 4096 or c.form in ("count", "onehot"):
                C.run_case(c, kernel_step())


def test_row_edges_name_the_chunk_boundaries():
    assert C.pick_rch(63) == 1 and C.pick_rch(64) == 2 and C.pick_rch(8191) == 255 and C.pick_rch(8192) == 256 == C.pick_rch(8193)
    assert C.row_edges(65) == [0, 1, 2, 3, 32, 33, 61, 62, 63, 64]           # per = 33: chunks [0, 33) and [33, 65)
    e = C.row_edges(8193)                                                        # per = 33: 248 full chunks, one of 9 rows, 7 empty ones
    assert 8184 in e and 8192 in e and 8183 in e and len(e) <= 512


def test_general_cases_build_and_pass_and_hf_share_is_inside_the_cap():
    """The toleranced kind: both steps lie inside the per-element bounds; the HF RMSNorm seeds leave out at most 1 % (from the reference
    alone: the builder asserts it) and not nothing at all over the seeds together -- the window is real."""
    left = []
    for family, kw in C.general_cases():
        c = C.make(family, kw)
        _, w0 = C.run_case(c, plain_step)
        _, w1 = C.run_case(c, kernel_step())
        assert w0 <= 1.0 and w1 <= 1.0
        if family == "fwd" and c.exp.left_out is not None:
            assert c.left_out_share <= C.HF_CAP
            left.append(c.left_out_share)
    assert len(left) >= 4 and max(left) < 8 * 2.0 ** -10
    print("\nHF shares left out: %s\n%s" % (["%.5f" % s for s in left], C.worst_table()))


# ------------------------------------------------------------------------------------------------------------------ the steps that are wrong

LN_MAP = dict(op="ln", rows=6, xdt=F32, ydt=BF16, ymap=C.default_map(6), y2=True)
BWD = dict(op="ln", rows=6, D=520, xdt=F32, dydt=F32, dxdt=F32, dres=True, dx_bf16=True)
WRONG = [
    ("last lane's columns left out of the mean", "fwd", dict(D=520, **LN_MAP), C.MEAN_NOT_EXACT),
    ("last lane's columns left out of the mean", "fwd", dict(D=4096, **LN_MAP), C.MEAN_NOT_EXACT),
    ("the two 256-column halves swapped for gamma", "fwd", dict(D=512, **LN_MAP), C.Y_NOT_EXACT),
    ("statistics of a chunk taken past D", "fwd", dict(D=520, **LN_MAP), C.READ_OUTSIDE),
    ("stores a chunk past D", "fwd", dict(D=520, **LN_MAP), C.FRAME_WRITTEN),
    ("y2, mean and rstd written at the mapped row", "fwd", dict(LN_MAP, D=520, ymap=(3, 4, 1)), C.FRAME_WRITTEN),
    ("y written at the plain row", "fwd", dict(D=520, **LN_MAP), C.FRAME_WRITTEN),
    ("truncating bf16 store", "fwd", dict(D=520, **LN_MAP), C.Y_NOT_EXACT),
    ("truncating bf16 store", "fwd", dict(op="rms", rows=6, D=8, xdt=F32, ydt=BF16, entry="add_rmsnorm_fwd"), C.Y_NOT_EXACT),
    ("xsum not rounded to the stream dtype", "fwd", dict(op="ln", rows=6, D=520, xdt=BF16, ydt=BF16, ddt=BF16), C.MEAN_NOT_EXACT),
    ("statistics taken before the add", "fwd", dict(op="ln", rows=6, D=1032, xdt=F32, ydt=F32, ddt=BF16), C.MEAN_NOT_EXACT),
    ("statistics taken before the add", "fwd", dict(op="rms", rows=6, D=1032, xdt=F32, ydt=F32, ddt=BF16), C.RSTD_NOT_EXACT),
    ("dres dropped", "bwd", BWD, C.DX_NOT_EXACT),
    ("dx_bf16 taken before dres", "bwd", BWD, C.DXB_NOT_EXACT),
    ("RMS with m1 != 0", "bwd", dict(BWD, op="rms"), C.DX_NOT_EXACT),
    ("RMS without round_to", "bwd", dict(BWD, op="rms", xdt=BF16, dydt=BF16, dxdt=BF16, dx_bf16=False), C.DX_NOT_EXACT),
    ("last row of a row chunk lost", "bwd", dict(BWD, rows=65, form="count", dres=False, dx_bf16=False), C.DGAMMA_NOT_EXACT),
    ("last row of a row chunk lost", "bwd", dict(BWD, rows=65, form="onehot"), C.DGAMMA_NOT_EXACT),
    ("last row of a row chunk lost", "bwd", dict(BWD, rows=65, form="onerow", rstar=32, need_dx=False), C.DGAMMA_NOT_EXACT),
    ("wave 3's rows lost", "bwd", dict(BWD, rows=33, form="count", dres=False, dx_bf16=False), C.DGAMMA_NOT_EXACT),
    ("wave 3's rows lost", "bwd", dict(BWD, rows=33, form="onerow", rstar=3, need_dx=False), C.DGAMMA_NOT_EXACT),
    ("empty trailing chunks left unwritten", "bwd", dict(BWD, rows=8193, form="count", need_dx=False), C.DGAMMA_NOT_EXACT),
    ("final reduction rounds rch down to a multiple of 4", "bwd", dict(BWD, rows=200, form="count", need_dx=False), C.DGAMMA_NOT_EXACT),
    ("accumulate ignored", "bwd", dict(BWD, rows=65, accumulate=True), C.DGAMMA_NOT_EXACT),
    ("dgamma taken without x^", "bwd", dict(BWD, rows=65), C.DGAMMA_NOT_EXACT),
    ("last row of a row chunk lost", "colsum", dict(rows=65, D=520, form="count"), C.OUT_NOT_EXACT),
    ("wave 3's rows lost", "colsum", dict(rows=33, D=520, sdt=BF16, form="onehot"), C.OUT_NOT_EXACT),
    ("empty trailing chunks left unwritten", "colsum", dict(rows=8193, D=520, sdt=BF16, form="count"), C.OUT_NOT_EXACT),
    ("final reduction rounds rch down to a multiple of 4", "colsum", dict(rows=200, D=520, form="random"), C.OUT_NOT_EXACT),
    ("accumulate ignored", "colsum", dict(rows=65, D=520, accumulate=True), C.OUT_NOT_EXACT),
]


@pytest.mark.parametrize("bug,family,kw,reason", WRONG, ids=["%s | %s %d" % (w[0], w[1], i) for i, w in enumerate(WRONG)])
def test_wrong_step_fails_its_named_check(bug, family, kw, reason):
    c = C.make(family, kw)
    C.run_case(c, kernel_step())                              # the same step without the fault passes
    with pytest.raises(C.CheckFailure) as e:
        C.run_case(c, kernel_step(bug))
    assert e.value.reason == reason, str(e.value)


def test_general_bounds_reject_a_lost_lane_and_a_wrong_gamma_column():
    """The per-element bounds see what relmax < 1e-2 on a bf16 y does not: a mean without one lane's eight elements at D = 4096 and one
    column scaled by its neighbour's gamma."""
    kw = dict(op="ln", rows=9, D=4096, xdt=F32, ydt=BF16, kind="general")
    c = C.make_fwd(**kw)
    C.run_case(c, kernel_step())
    with pytest.raises(C.CheckFailure) as e:
        C.run_case(c, kernel_step("last lane's columns left out of the mean"))
    assert e.value.reason == C.BEYOND_BOUND

    def neighbour_gamma(p):
        kernel_step()(p)
        y = p.get("y").float()
        g = p.case.gamma.double()
        y[:, 7] = ((y[:, 7].double() - p.case.beta.double()[7]) / g[7] * g[8] + p.case.beta.double()[7]).float()
        p.put("y", y)

    with pytest.raises(C.CheckFailure) as e:
        C.run_case(c, neighbour_gamma)
    assert e.value.reason == C.BEYOND_BOUND


def test_rmsnorm_bwd_rejects_a_dy_of_another_dtype():
    """ops.rmsnorm_bwd hands the C function x's dtype for dy: a dy of another dtype must raise before anything is launched."""
    from otter_amd import _capi, ops

    x, w, rstd = torch.zeros(4, 8), torch.ones(8), torch.ones(4)
    with pytest.raises(_capi.OtterHipError, match="dy must have the dtype of x"):
        ops.rmsnorm_bwd(torch.zeros(4, 8, dtype=BF16), x, w, rstd)
    with pytest.raises(_capi.OtterHipError, match="dy must have the dtype of x"):
        ops.rmsnorm_bwd(torch.zeros(4, 8), x.to(BF16), w, rstd)
