"""The kernels of csrc/norm.hip on inputs whose answer is known exactly -- tests/_norm_cases.py builds, places and checks them,
tests/test_norm_cases_cpu.py shows that the checks fail on a step that loses a lane, a row, a wave or a chunk, swaps gamma columns, rounds
by truncation, skips round_to, drops dres or accumulate, or writes at the wrong row.  Every check but the `general` kind is torch.equal;
that kind is per element, with the bounds derived in _norm_cases.

  D edges        8, 504, 512, 520, 1024, 1032, 2048, 2056, 3584, 4096, 4104, 4608, 8184, 8192 (generic NCH 1 .. 16 with dead lanes in the last
                 live chunk, coalesced NCH 1 .. 8) x the four dtype routes x fp32 / bf16 weights, 5 or 6 rows
  entry points   layernorm_fwd / add_layernorm_fwd / rmsnorm_fwd / add_rmsnorm_fwd (with and without delta) / layernorm_bwd / rmsnorm_bwd /
                 rmsnorm_bwd_ex / colsum through the C ABI on framed buffers, and through the ops wrappers
  options        gamma, beta, y2, ymap, dymap, delta, dres, dx_bf16, need_dx = False, need_dw = False, need_dbeta = False, accumulate,
                 mean / rstd not wanted: each present and absent
  rows           1 .. 5 (waves that return early); 31 .. 8193 on both sides of every pick_rch edge for dgamma / dbeta and colsum
  generic kernels at coalescable shapes   a fresh child process with OTTER_NORM_VARIANT=0 (read once per process)

Every output (mean, rstd, dgamma, dbeta and the row-mapped y with its gaps included) lies in a sentinel frame, every input in a NaN
frame (_norm_cases.Placed); the dgamma / dbeta / colsum workspace is handed over holding stale values."""
import gc
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import _norm_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = C.BF16, C.F32
COALESCABLE_D = [512, 1024, 2048, 3584, 4096]


@pytest.fixture(scope="module")
def ops():
    from otter_amd import _capi, ops as _ops

    assert _capi.lib().otter_device_check() > 0, _capi.lib().otter_last_error()
    yield _ops
    print("\n" + C.worst_table())
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _rowmap(m):
    from otter_amd._capi import RowMap

    return RowMap(*m) if m else RowMap(0, 0, 0)


def _stale_ws(K, rows, D):
    n = K.lib().otter_layernorm_bwd_workspace_bytes(rows, D)
    assert n == C.pick_rch(rows) * 2 * D * 4
    return torch.full((n // 4,), 7.0, dtype=F32, device=DEV)               # what another call left behind


def capi_step(p):
    """The C ABI on the framed buffers themselves: every output pointer is the first logical (physical, under a row map) row of its frame."""
    from otter_amd import _capi as K

    c, L, st = p.case, K.lib(), K.stream()
    rows, D = c.rows, c.D
    if c.family == "fwd":
        wdt = K.dt_of(c.wdt)
        if c.entry == "layernorm_fwd":
            rc = L.otter_layernorm_fwd(p.ptr("x"), K.dt_of(c.xdt), p.ptr("gamma"), p.ptr("beta"), wdt, p.ptr("y"), K.dt_of(c.ydt), _rowmap(c.ymap),
                                       p.ptr("y2"), p.ptr("mean"), p.ptr("rstd"), rows, D, c.eps, st)
        elif c.entry == "add_layernorm_fwd":
            rc = L.otter_add_layernorm_fwd(p.ptr("x"), K.dt_of(c.xdt), p.ptr("delta"), K.dt_of(c.ddt), p.ptr("xsum"), p.ptr("gamma"), p.ptr("beta"),
                                           wdt, p.ptr("y"), K.dt_of(c.ydt), p.ptr("mean"), p.ptr("rstd"), rows, D, c.eps, st)
        elif c.entry == "rmsnorm_fwd":
            rc = L.otter_rmsnorm_fwd(p.ptr("x"), K.dt_of(c.xdt), p.ptr("gamma"), wdt, p.ptr("y"), p.ptr("rstd"), rows, D, c.eps, st)
        else:
            rc = L.otter_add_rmsnorm_fwd(p.ptr("x"), K.dt_of(c.xdt), p.ptr("delta"), K.dt_of(c.ddt) if c.ddt is not None else K.F32, p.ptr("xsum"),
                                         p.ptr("gamma"), wdt, p.ptr("y"), K.dt_of(c.ydt), p.ptr("rstd"), rows, D, c.eps, st)
    elif c.family == "bwd":
        ws = _stale_ws(K, rows, D) if c.need_dw else None
        wdt, acc = K.dt_of(c.wdt), 1 if c.accumulate else 0
        if c.entry == "layernorm_bwd":
            rc = L.otter_layernorm_bwd(p.ptr("dy"), K.dt_of(c.dydt), _rowmap(c.dymap), p.ptr("x"), K.dt_of(c.xdt), p.ptr("gamma"), wdt, p.ptr("mean"),
                                       p.ptr("rstd"), p.ptr("dres"), p.ptr("dx"), K.dt_of(c.dxdt), p.ptr("dx_bf16"), p.ptr("dgamma"), p.ptr("dbeta"),
                                       acc, K.ptr(ws), rows, D, st)
        elif c.entry == "rmsnorm_bwd":
            rc = L.otter_rmsnorm_bwd(p.ptr("dy"), p.ptr("x"), K.dt_of(c.xdt), p.ptr("gamma"), wdt, p.ptr("rstd"), p.ptr("dx"), p.ptr("dgamma"), acc,
                                     K.ptr(ws), rows, D, st)
        else:
            rc = L.otter_rmsnorm_bwd_ex(p.ptr("dy"), K.dt_of(c.dydt), p.ptr("x"), K.dt_of(c.xdt), p.ptr("gamma"), wdt, p.ptr("rstd"), p.ptr("dres"),
                                        p.ptr("dx"), K.dt_of(c.dxdt), p.ptr("dx_bf16"), p.ptr("dgamma"), acc, K.ptr(ws), rows, D, st)
    else:
        ws = _stale_ws(K, rows, D)
        rc = L.otter_colsum(p.ptr("src"), K.dt_of(c.sdt), _rowmap(c.smap), p.ptr("out"), 1 if c.accumulate else 0, ws.data_ptr(), rows, D, st)
    K.check(rc, c.entry if c.family != "colsum" else "colsum")
    torch.cuda.synchronize()


def ops_step(ops):
    """The ops wrappers: what they allocate themselves is copied into the frames, what they take preallocated (y, y2, dx_bf16, out) IS the frame."""
    def step(p):
        c = p.case
        t = lambda nm: p.get(nm) if p.has(nm) else None                    # noqa: E731
        if c.family == "fwd":
            if c.entry == "layernorm_fwd":
                _, mean, rstd = ops.layernorm_fwd(p.base["x"], t("gamma"), t("beta"), c.ydt, eps=c.eps, y=p.base["y"], ymap=_rowmap(c.ymap) if c.ymap else None,
                                                  y2=p.base["y2"] if p.has("y2") else None, need_stats=c.stats)
                outs = dict(mean=mean, rstd=rstd)
            elif c.entry == "add_layernorm_fwd":
                xsum, y, mean, rstd = ops.add_layernorm_fwd(p.base["x"], p.base["delta"], t("gamma"), t("beta"), c.ydt, eps=c.eps, need_stats=c.stats)
                outs = dict(xsum=xsum, y=y, mean=mean, rstd=rstd)
            elif c.entry == "rmsnorm_fwd":
                y, rstd = ops.rmsnorm_fwd(p.base["x"], t("gamma"), eps=c.eps)
                outs = dict(y=y, rstd=rstd)
            else:
                xsum, y, rstd = ops.add_rmsnorm_fwd(p.base["x"], p.base["delta"] if p.has("delta") else None, t("gamma"), c.ydt, eps=c.eps)
                outs = dict(xsum=xsum, y=y, rstd=rstd)
        elif c.family == "bwd":
            dxb = p.base["dx_bf16"] if p.has("dx_bf16") else None
            if c.entry == "layernorm_bwd":
                dx, dg, db = ops.layernorm_bwd(p.base["dy"], p.base["x"], t("gamma"), t("mean"), t("rstd"), c.dxdt, dres=p.base["dres"] if p.has("dres") else None,
                                               dymap=_rowmap(c.dymap) if c.dymap else None, need_dw=c.need_dw, need_dbeta=c.need_dbeta, need_dx=c.need_dx,
                                               dx_bf16=dxb)
                outs = dict(dx=dx, dgamma=dg, dbeta=db)
            elif c.entry == "rmsnorm_bwd":
                dx, dw = ops.rmsnorm_bwd(p.base["dy"], p.base["x"], t("gamma"), t("rstd"))
                outs = dict(dx=dx, dgamma=dw)
            else:
                dx, dw = ops.rmsnorm_bwd_ex(p.base["dy"], p.base["x"], t("gamma"), t("rstd"), c.dxdt, dres=p.base["dres"] if p.has("dres") else None,
                                            need_dw=c.need_dw, dx_bf16=dxb)
                outs = dict(dx=dx, dgamma=dw)
        else:
            ops.colsum(p.base["src"], _rowmap(c.smap) if c.smap else None, c.rows, out=p.base["out"][0], accumulate=c.accumulate)
            outs = {}
        torch.cuda.synchronize()
        for nm, v in outs.items():
            if v is not None and nm in p.outputs:
                p.put(nm, v)
    return step


def run(c, step=capi_step):
    try:
        return C.run_case(c, step, DEV)
    except C.CheckFailure as e:
        raise AssertionError(str(e)) from e


def _through_ops(c):
    """What the ops wrappers can express: no accumulate, statistics only where the wrapper returns them."""
    if getattr(c, "accumulate", False) and c.family == "bwd":
        return False
    return not (c.family == "fwd" and c.op == "rms" and not c.stats)


# ------------------------------------------------------------------------------------------------------------------ D edges x routes

@pytest.mark.parametrize("D", C.D_LIST)
def test_forward_at_chunk_edges_every_route_and_option(ops, D):
    """LayerNorm (plain, row-mapped with y2, fused add, without gamma / beta / statistics) and RMSNorm (both entry points, with and without
    delta, +-a and the 15 : 1 form) at one D: mean, rstd, xsum and fp32 y bit-equal, bf16 y the nearest-even cast, y2 the bits of y."""
    for kw in C.fwd_cases(D):
        run(C.make_fwd(**kw))


@pytest.mark.parametrize("D", C.D_LIST)
def test_backward_at_chunk_edges_every_route_and_option(ops, D):
    """dx = h rstd + dres with sum g = D m1 and sum g x^ = D m2 exact at every D; dx_bf16 the nearest-even cast of dx AFTER dres; RMSNorm with
    sum g != 0 and, for a bf16 x, an x rstd on a bf16 tie; dgamma / dbeta exact, with and without accumulate, dbeta, dx, a dy row map."""
    for kw in C.bwd_cases(D):
        run(C.make_bwd(**kw))


@pytest.mark.parametrize("D", [520, 1024])
def test_ops_wrappers_every_optional_argument(ops, D):
    """The same cases through ops.*: every optional argument present and absent reaches the C function as the wrapper documents."""
    n = 0
    for family, cases in (("fwd", C.fwd_cases(D)), ("bwd", C.bwd_cases(D))):
        for kw in cases:
            c = C.make(family, kw)
            if _through_ops(c):
                run(c, ops_step(ops))
                n += 1
    for kw in C.edge_colsum_cases(65)[:3] + C.edge_colsum_cases(65)[-3:]:
        run(C.make_colsum(**kw), ops_step(ops))
    assert n > 40


def test_ops_rmsnorm_bwd_rejects_a_dy_of_another_dtype(ops):
    from otter_amd._capi import OtterHipError

    x = torch.ones(4, 8, device=DEV)
    with pytest.raises(OtterHipError, match="dy must have the dtype of x"):
        ops.rmsnorm_bwd(torch.ones(4, 8, dtype=BF16, device=DEV), x, torch.ones(8, device=DEV), torch.ones(4, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ rows

@pytest.mark.parametrize("rows", C.SMALL_ROWS)
def test_blocks_with_waves_that_return_early(ops, rows):
    """rows < 4 (and 5: a full block and a block of one wave) at D = 520 (generic) and 1024 (coalesced for fp32 -> bf16)."""
    for D in C.SMALL_ROWS_D:
        for family, cases in (("fwd", C.fwd_cases(D, rows)), ("bwd", C.bwd_cases(D, rows))):
            for kw in cases:
                run(C.make(family, kw))


@pytest.mark.parametrize("rows", C.EDGE_ROWS)
def test_dgamma_dbeta_at_row_chunk_edges(ops, rows):
    """pick_rch edges 63 / 64 / 65 (one chunk becomes two, a short last chunk) and 8191 / 8192 / 8193 (the cap: per = 33, empty trailing chunks
    that must still write zeros over a stale workspace): random rows with dx (generic D = 520 and coalesced D = 512), the count form
    (dgamma = dbeta = rows), the one-hot form (every row of row_edges() in one launch) and, below the cap, one launch per r*."""
    for kw in C.edge_row_cases(rows):
        run(C.make_bwd(**kw))


@pytest.mark.parametrize("rows", C.EDGE_ROWS)
def test_colsum_at_row_chunk_edges(ops, rows):
    for kw in C.edge_colsum_cases(rows):
        run(C.make_colsum(**kw))


# ------------------------------------------------------------------------------------------------------------------ general kind

def test_general_data_within_per_element_bounds(ops):
    """Seeded normal data at the default eps against the fp64 reference per element (bounds: _norm_cases docstring), HF's RMSNorm rounding
    (bf16 x, fp32 y through add_rmsnorm_fwd, y = w bf16(x rstd)) included.  The worst error / bound per check is printed."""
    for family, kw in C.general_cases():
        c = C.make(family, kw)
        _, worst = run(c)
        assert worst <= 1.0
        if family != "colsum" and _through_ops(c):
            run(c, ops_step(ops))                                        # (the table is printed once, when the module's fixture ends)


# ------------------------------------------------------------------------------------------------------------------ OTTER_NORM_VARIANT=0

def _coalescable(kw, family):
    if family == "fwd":
        return C.coalesced_fwd(kw["D"], kw["xdt"], kw["ydt"])
    return C.coalesced_bwd(kw["D"], kw["xdt"], kw["dydt"], kw["dxdt"]) and kw.get("need_dx", True) and kw.get("form") != "onehot"


@pytest.mark.parametrize("D", COALESCABLE_D)
def test_coalescable_cases_forward_and_backward(ops, D):
    """The cases of this file whose shape and dtypes the coalesced kernels take.  Under the default OTTER_NORM_VARIANT they run those; the
    test below runs this selection again in a process of its own with OTTER_NORM_VARIANT=0, where the generic kernels meet them."""
    n = 0
    for family, cases in (("fwd", C.fwd_cases(D) + (C.fwd_cases(D, 3) if D == 1024 else [])),
                          ("bwd", C.bwd_cases(D) + (C.bwd_cases(D, 3) if D == 1024 else []) + (C.edge_row_cases(65) if D == 512 else []))):
        for kw in cases:
            if _coalescable(kw, family):
                run(C.make(family, kw))
                n += 1
    assert n >= 8
    print("\n[norm-exact] OTTER_NORM_VARIANT=%s: %d coalescable cases at D = %d" % (os.environ.get("OTTER_NORM_VARIANT", "(default 1)"), n, D))


def test_generic_kernels_meet_the_coalesced_shapes_in_a_fresh_process():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OTTER_NORM_VARIANT="0")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_norm_exact.py"), "-m", "gpu", "-k", "coalescable_cases", "-q",
                          "-s", "-p", "no:cacheprovider"], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert out.stdout.count("OTTER_NORM_VARIANT=0:") == len(COALESCABLE_D), out.stdout[-3000:]
    m = re.search(r"(\d+) passed", out.stdout)
    assert m and int(m.group(1)) == len(COALESCABLE_D) and "skipped" not in out.stdout.splitlines()[-1], out.stdout[-1000:]
