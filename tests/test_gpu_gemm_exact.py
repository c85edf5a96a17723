"""The GEMM kernels (csrc/gemm.hip and gemm_*.hip, gemm_tail.h, gemm_t4_ktile.inc) on inputs whose answer is known exactly -- tests/_gemm_cases.py builds, places and
checks them, tests/test_gemm_cases_cpu.py shows that the checks fail on a step that loses, doubles or shifts a k, misplaces a tile, writes
past an edge, miscounts a partial, ignores accumulate or a leading dimension, or rounds by truncation.  Every check but the gated forms, the
GELU value and the stashed derivative is torch.equal; those three are per element, with the constants of _gemm_cases.

  forced variants   1, 2, 3, 13, 25, 26 (default and plain K order, cross-tile form on and off), 30 at M x N pairs on both sides of every
                    tile edge and the K list for which a Python mirror of pick_cfg says the forced kernel really runs
  epilogue matrix   every epilogue form, both output dtypes, at an all-full and a ragged shape per variant
  wide switch       N = 264 bf16: ldc / ldc2 / ldr / ldaux at N + 4 one at a time (4-wide tail) against all at N + 8 (8-wide)
  fp32 parity       gemm_f32_kernel at its 64 x 64 x 32 edges, every epilogue form
  k=                operands wider than the reduction, NaN behind column k
  several tiles per workgroup   CU budget 8 at 520 x 772; variant 26 also one workgroup per tile (OTTER_GRID_PER_TILE), same bits
  default dispatch  >= 192 tiles of 256 x 256: variant 26 on K-contiguous and K-major operands (nt, a, b, ab; ab at any K)

Every output view lies in a sentinel-filled frame and every input in a NaN-filled one (_gemm_cases.Placed)."""
import gc
from contextlib import contextmanager, nullcontext

import pytest
import torch

from tests import _gemm_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
GATE = 0.37
BF16, F32 = C.BF16, C.F32


@pytest.fixture(scope="module")
def ops():
    from otter_amd import _capi, ops as _ops

    assert _capi.lib().otter_device_check() > 0, _capi.lib().otter_last_error()
    yield _ops
    _ops.set_gemm_variant(0)
    _capi.gemm_set_debug(0)
    _ops.set_gemm_cu_budget(0)
    print("\n" + C.worst_table())
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@contextmanager
def forced(ops, variant=0, debug=0, budget=0, grid=None):
    from otter_amd import _capi as K

    prev = K.gemm_set_debug(debug)
    try:
        ops.set_gemm_variant(variant)
        if budget:
            ops.set_gemm_cu_budget(budget)
        with (ops.gemm_grid_mode(grid) if grid is not None else nullcontext()):
            yield
    finally:
        ops.set_gemm_variant(0)
        K.gemm_set_debug(prev)
        ops.set_gemm_cu_budget(0)


def mirror_pick(v, M, N, K):
    """pick_cfg of csrc/gemm.hip for bf16 operands below 4 GB (plus gemm_impl's 25 -> 30 for few tiles and no partials under auto)."""
    if v == 0:
        if C.cdiv(M, 256) * C.cdiv(N, 256) >= 192:
            v = 26 if K % 128 == 0 else 13
        elif K % 256 == 0 and K >= 512 and C.cdiv(M, 128) * C.cdiv(N, 128) <= 512:
            v = 25
        else:
            v = 1
    if v == 13 and K % 64:
        v = 2
    if v == 26 and K % 128:
        v = 13 if K % 64 == 0 else 2
    if v in (25, 30) and K % 256:
        v = 1
    if v == 3 and K % 64:
        v = 2
    return v


KIND = {"store": 0, "gelu": 1, "scale_res": 2, "gate_bwd": 3}


def gpu_step(ops):
    def step(p):
        c = p.case
        gate = torch.tensor([c.gate], dtype=F32, device=DEV) if c.gate is not None else None
        if c.epi == "gelu":
            auxg = "stash" if c.stash else False
        else:
            auxg = c.aux_mode if c.aux_mode in ("sqrelu", "stash") else False
        if p.partial is not None:
            assert p.partial.numel() == ops.gemm_num_partials(c.M, c.N, c.in_dtype), "%s: tile rule %r" % (c.name, c.tile)
        kw = dict(out=p.view["C"], kind=KIND[c.epi], gate=gate, R=p.view.get("R"), C2=p.view.get("C2"), aux=p.view.get("aux"), aux_gelu=auxg,
                  partial=p.partial, accumulate=c.accumulate, k=c.K if c.kw else None)
        if c.a_kmajor or c.b_kmajor:
            ops.gemm(p.view["A"], p.view["B"], c.a_kmajor, c.b_kmajor, **kw)
        else:
            ops.gemm_nt(p.view["A"], p.view["B"], **kw)
        torch.cuda.synchronize()
    return step


def reducer(ops):
    def reduce(partial, gate):
        g = torch.tensor([gate], dtype=F32, device=DEV) if gate is not None else None
        return float(ops.reduce_partials(partial, g))
    return reduce


def run(ops, c, s_dev=None, tag=""):
    try:
        return C.run_case(c, gpu_step(ops), DEV, s_dev=s_dev, reduce=reducer(ops))
    except C.CheckFailure as e:
        raise AssertionError("%s: %s" % (tag, e)) from e


def get_s_dev(ops, M, N, K, tag, in_dtype=BF16):
    """The kernel's own s = tanhf(gate), from the elements of a gated fp32 STORE whose accumulator is exactly 1; checked against fp64 tanh."""
    c = C.make_case("onehot", M, N, K, in_dtype=in_dtype, out_dtype=F32, gate=GATE)
    p = C.Placed(c, DEV)
    gpu_step(ops)(p)
    s = C.read_s_dev(c, p.result())
    d = C.check_s_dev(s, GATE)
    print("[gemm-exact] %s: s_dev = %r, %.2f ulp from tanh(%r) (bound %d; measured: the device library's accuracy is not documented here)"
          % (tag, s, d, GATE, C.TANH_ULPS))
    run(ops, c, s, tag)
    return s


# ------------------------------------------------------------------------------------------------------------------ forced variants

SHAPES = [(1, 4), (1, 264), (33, 12), (33, 132), (64, 64), (64, 260), (65, 68), (65, 264), (129, 132), (129, 12), (257, 260), (257, 68)]
VARIANT_K = {1: [8, 56, 64, 72, 136, 200], 2: [8, 56, 64, 72, 136, 200], 3: [64, 192], 13: [64, 192, 320], 25: [512, 768, 1024],
             30: [512, 768, 1024], 26: [128, 256, 384, 512, 640]}
XT_OFF, PLAIN_ORDER = 1 << 14, 1 << 23
MODES = [(v, 0, "") for v in (1, 2, 3, 13, 25, 30, 26)] + [(26, PLAIN_ORDER, "plain K order"), (26, XT_OFF, "cross-tile off")]


def store_cases(M, N, K, pads=None, **kw):
    mk = C.make_case
    return [mk("onehot", M, N, K, out_dtype=F32, pads=pads, **kw), mk("onehot", M, N, K, out_dtype=BF16, mirrored=True, pads=pads, **kw),
            mk("count", M, N, K, out_dtype=BF16, pads=pads, **kw), mk("ints", M, N, K, out_dtype=F32, pads=pads, **kw),
            mk("ints", M, N, K, out_dtype=BF16, pads=pads, **kw)]


@pytest.mark.parametrize("variant,debug,what", MODES, ids=["v%d%s" % (m[0], "-" + m[2].replace(" ", "_") if m[2] else "") for m in MODES])
def test_forced_variant_at_tile_and_k_tile_edges(ops, variant, debug, what):
    n = 0
    with forced(ops, variant, debug):
        for K in VARIANT_K[variant]:
            for i, (M, N) in enumerate(SHAPES):
                if mirror_pick(variant, M, N, K) != variant:
                    continue                                   # the forced kernel would fall back: not this test's subject
                pads = {"A": 8 * (i % 3), "B": 8 * ((i + 1) % 3), "C": 4 * (i % 3)}
                for c in store_cases(M, N, K, pads):
                    run(ops, c, tag="variant %d %s" % (variant, what))
                    n += 1
    assert n >= 5 * len(SHAPES) * len(VARIANT_K[variant])
    print("[gemm-exact] variant %d %s: %d exact cases" % (variant, what, n))


def test_the_harness_fails_on_a_kernel_without_its_mfmas(ops):
    """Debug bit 1 (a roofline ablation of variants 1 - 3: the K loop without its MFMAs, results wrong by construction): the exact check
    must say so -- this harness reaches the kernel and can fail on it."""
    c = C.make_case("ints", 129, 132, 72, out_dtype=F32)
    with forced(ops, 1, 2):
        with pytest.raises(AssertionError) as e:
            run(ops, c, tag="variant 1 without MFMAs")
    assert C.C_NOT_EXACT in str(e.value)
    with forced(ops, 1):
        run(ops, c, tag="variant 1")


# ------------------------------------------------------------------------------------------------------------------ epilogue matrix

def epilogue_cases(M, N, K, od, tile, pads, in_dtype=BF16, gated=True):
    mk = lambda kind, **kw: C.make_case(kind, M, N, K, in_dtype=in_dtype, out_dtype=od, pads=pads, **kw)      # noqa: E731
    out = [mk("ints"), mk("count")]
    if od == F32:
        out += [mk("ints", accumulate=True), mk("count", want_partial=True, tile=tile), mk("count", accumulate=True, want_partial=True, tile=tile)]
    out += [mk("ints", epi="scale_res", r_dtype=F32), mk("ints", epi="scale_res", r_dtype=BF16)]
    for adt in (BF16, F32):
        out += [mk("ints", epi="gate_bwd", aux_dtype=adt), mk("ints", epi="gate_bwd", aux_mode="sqrelu", aux_dtype=adt),
                mk("ints", epi="gate_bwd", aux_mode="stash", aux_dtype=adt)]
    out += [mk("count", epi="gate_bwd", want_partial=True, tile=tile), mk("count", epi="gate_bwd", aux_mode="sqrelu", want_partial=True, tile=tile),
            mk("onehot", epi="gate_bwd", aux_dtype=F32, want_partial=True, tile=tile)]
    out += [mk("ints", epi="gelu", want_c2=True), mk("gelu", epi="gelu", want_c2=True), mk("gelu", epi="gelu"), mk("gelu", epi="gelu", stash=True)]
    if gated:
        out += [mk("ints", gate=GATE), mk("ints", epi="scale_res", gate=GATE), mk("ints", epi="scale_res", r_dtype=BF16, gate=GATE),
                mk("ints", epi="gate_bwd", gate=GATE), mk("ints", epi="gate_bwd", aux_mode="sqrelu", gate=GATE),
                mk("ints", epi="gate_bwd", aux_mode="stash", gate=GATE), mk("count", epi="gate_bwd", gate=GATE, want_partial=True, tile=tile)]
        if od == F32:
            out += [mk("ints", accumulate=True, gate=GATE)]
    return out


EPI_K = {1: 72, 2: 136, 3: 192, 13: 192, 25: 512, 30: 768, 26: 256}
EPI_MODES = [(v, 0) for v in (1, 2, 3, 13, 25, 30, 26)] + [(26, XT_OFF)]


@pytest.mark.parametrize("od", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("variant,debug", EPI_MODES, ids=["v%d%s" % (v, "-xt_off" if d else "") for v, d in EPI_MODES])
def test_every_epilogue_form(ops, variant, debug, od):
    K = EPI_K[variant]
    tag = "variant %d debug %#x" % (variant, debug)
    with forced(ops, variant, debug):
        assert mirror_pick(variant, 512, 768, K) == variant
        s = get_s_dev(ops, 65, 68, K, tag)
        for (M, N), pads in (((512, 768), None), ((257, 260), {"C": 8, "C2": 4, "R": 8, "aux": 4, "A": 8})):
            cases = epilogue_cases(M, N, K, od, C.TILE_OF[variant], pads)
            for c in cases:
                run(ops, c, s, tag)
    print("[gemm-exact] %s -> %s: %d epilogue cases at 512 x 768 and 257 x 260, K = %d" % (tag, str(od)[6:], 2 * len(cases), K))


# ------------------------------------------------------------------------------------------------------------------ the wide switch

@pytest.mark.parametrize("variant", [1, 2, 3, 13, 25, 30, 26])
def test_wide_tail_switch_one_leading_dimension_at_a_time(ops, variant):
    """bf16 out, N = 264: every tensor of the tail at N + 8 takes the 8-wide tail; ldc, ldc2, ldr or ldaux at N + 4 in turn the 4-wide one.
    Both are exact where the form is, and the GELU value (the packed polynomial in both) keeps its bits."""
    K, N = EPI_K[variant], 264
    forms = [("scale_res", dict(r_dtype=BF16), ("C", "R")), ("scale_res", dict(r_dtype=F32), ("C", "R")),
             ("gate_bwd", dict(aux_mode="sqrelu"), ("C", "aux")), ("gate_bwd", dict(aux_mode="stash", aux_dtype=F32), ("C", "aux")),
             ("gelu", dict(want_c2=True), ("C", "C2")), ("gelu", dict(stash=True), ("C", "C2")), ("store", {}, ("C",))]
    n = 0
    with forced(ops, variant):
        for M in (257, 512):
            for epi, kw, tensors in forms:
                kind = "gelu" if epi == "gelu" else "ints"
                wide = C.make_case(kind, M, N, K, epi=epi, pads={t: 8 for t in tensors}, **kw)
                ref, _ = run(ops, wide, tag="variant %d wide" % variant)
                for t in tensors:
                    narrow = C.make_case(kind, M, N, K, epi=epi, pads={u: (4 if u == t else 8) for u in tensors}, **kw)
                    got, _ = run(ops, narrow, tag="variant %d, ld of %s at N + 4" % (variant, t))
                    C.check_same_bits(narrow, ref.C, got.C, "the 4-wide and the 8-wide tail differ")
                    if ref.C2 is not None:
                        C.check_same_bits(narrow, ref.C2, got.C2, "the 4-wide and the 8-wide tail differ", "C2")
                    n += 1
    print("[gemm-exact] variant %d: %d narrow launches against their wide twin" % (variant, n))


# ------------------------------------------------------------------------------------------------------------------ fp32 parity kernel

@pytest.mark.parametrize("M,N", [(1, 4), (63, 68), (65, 60), (130, 132)])
def test_fp32_kernel_at_its_tile_edges(ops, M, N):
    s = get_s_dev(ops, 65, 68, 36, "fp32 kernel", in_dtype=F32)
    n = 0
    for K in (4, 28, 32, 36, 100):
        pads = {"A": 4, "B": 8, "C": 4, "R": 4, "aux": 8, "C2": 4}
        for od in (F32, BF16):
            cases = epilogue_cases(M, N, K, od, (64, 64), pads, in_dtype=F32)
            cases += [C.make_case("onehot", M, N, K, in_dtype=F32, out_dtype=od, pads=pads),
                      C.make_case("onehot", M, N, K, in_dtype=F32, out_dtype=od, pads=pads, mirrored=True)]
            for c in cases:
                run(ops, c, s, "fp32 kernel")
                n += 1
    print("[gemm-exact] fp32 kernel %d x %d: %d cases" % (M, N, n))


# ------------------------------------------------------------------------------------------------------------------ k=

@pytest.mark.parametrize("variant,M,N,K,kw", [(1, 65, 68, 72, 56), (1, 129, 132, 200, 8), (0, 129, 132, 512, 256), (0, 65, 264, 136, 64),
                                              (0, 130, 132, 36, 28)])
def test_k_argument_reduces_over_the_first_k_columns(ops, variant, M, N, K, kw):
    with forced(ops, variant):
        for in_dtype in ((F32,) if K % 8 else (BF16, F32)):
            for c in store_cases(M, N, K, {"A": 8, "B": 16}, kw=kw, in_dtype=in_dtype):
                run(ops, c, tag="k= under variant %d" % variant)


# ------------------------------------------------------------------------------------------------------------------ several tiles per workgroup

MULTI_MODES = [(v, 0, None) for v in (1, 2, 3, 13, 25, 30, 26)] + [(26, XT_OFF, None), (26, 0, "per_tile"), (26, XT_OFF, "per_tile")]


def multi_cases(K, tile):
    M, N = C.MULTI_SHAPE
    out = []
    for kind in ("onehot", "count", "ints"):
        for od in (BF16, F32):
            pads = {"C": 4, "R": 8, "aux": 4}
            out += [C.make_case(kind, M, N, K, out_dtype=od, pads=pads), C.make_case(kind, M, N, K, out_dtype=od, pads=pads, epi="scale_res", r_dtype=od),
                    C.make_case(kind, M, N, K, out_dtype=od, pads=pads, epi="gate_bwd", aux_mode=None if od == BF16 else "sqrelu", aux_dtype=od,
                                want_partial=True, tile=tile)]
    return out


@pytest.mark.parametrize("variant,debug,grid", MULTI_MODES,
                         ids=["v%d%s%s" % (v, "-xt_off" if d else "", "-per_tile" if g else "") for v, d, g in MULTI_MODES])
def test_several_tiles_per_workgroup(ops, variant, debug, grid):
    """CU budget 8: the persistent grids are 8 workgroups (16 of the 128-tile kernels) for 12 tiles of 256 x 256, 35 of 128 x 128 or 63 of
    64 x 128, all edges ragged.  Variant 26 with one workgroup per tile must give the bits of the persistent launch."""
    from otter_amd import _capi as K_

    M, N = C.MULTI_SHAPE
    n = 0
    for K in C.MULTI_K[variant]:
        assert mirror_pick(variant, M, N, K) == variant
        for c in multi_cases(K, C.TILE_OF[variant]):
            with forced(ops, variant, debug, budget=8, grid=K_.GRID_PER_TILE if grid else None):
                got, _ = run(ops, c, tag="variant %d debug %#x grid %s, budget 8" % (variant, debug, grid))
            if grid:
                with forced(ops, variant, debug, budget=8):
                    ref, _ = run(ops, c, tag="variant %d persistent" % variant)
                C.check_same_bits(c, ref.C, got.C, "one workgroup per tile and the persistent grid differ")
            n += 1
    print("[gemm-exact] variant %d debug %#x grid %s: %d cases at %d x %d under a budget of 8" % (variant, debug, grid, n, M, N))


# ------------------------------------------------------------------------------------------------------------------ default dispatch, large grid

LAYOUTS = {"nt": (False, False), "b": (False, True), "a": (True, False), "ab": (True, True)}


def large_case(kind, M, N, K, layout, **kw):
    ta, tb = LAYOUTS[layout]
    pads = {"C": 8, "R": 8, "aux": 8}
    if ta:
        pads["A"] = 8
    if tb:
        pads["B"] = 24
    c = C.make_case(kind, M, N, K, a_kmajor=ta, b_kmajor=tb, pads=pads, tile=(256, 256) if kw.get("want_partial") else None,
                    with_acc=(kind == "onehot"), **kw)
    if c.acc is None:
        c.acc = c.A.to(DEV).double() @ c.B.to(DEV).double().T        # the fp64 reference of the count cases, on the device
        C.finish(c)
    return c


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("M,N", C.LARGE_SHAPES)
def test_default_dispatch_large_grid_and_k_major(ops, M, N, layout):
    ta, tb = LAYOUTS[layout]
    n = 0
    for K in C.LARGE_K:
        if K % 128 and layout != "ab":
            continue
        if ta or tb:
            assert ops.gemm_kmajor_supported(M, N, K, M + 8 if ta else K, N + 24 if tb else K, ta, tb, BF16)
        else:
            assert mirror_pick(0, M, N, K) == 26
        todo = [("onehot", dict(out_dtype=F32)), ("onehot", dict(out_dtype=BF16, mirrored=True)),
                ("count", dict(out_dtype=F32, accumulate=True, want_partial=True)), ("count", dict(out_dtype=BF16))]
        if layout in ("nt", "b"):
            todo += [("count", dict(out_dtype=BF16, epi="gate_bwd", want_partial=True)),
                     ("count", dict(out_dtype=F32, epi="gate_bwd", aux_mode="sqrelu", aux_dtype=F32, want_partial=True))]
        if layout == "nt":
            todo += [("count", dict(out_dtype=F32, epi="scale_res"))]
        for kind, kw in todo:
            c = large_case(kind, M, N, K, layout, **kw)
            run(ops, c, tag="default dispatch, %s" % layout)
            del c
            n += 1
    print("[gemm-exact] default dispatch %d x %d %s: %d exact cases" % (M, N, layout, n))
