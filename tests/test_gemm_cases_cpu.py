"""tests/_gemm_cases.py judged on the CPU: its checkers pass on a plain fp64 step and on a tiled step that mimics a kernel (128 x 128 tiles,
64-wide K-tiles, an edge mask, fp32 tail), every builder condition holds at every shape tests/test_gpu_gemm_exact.py visits, and each of
fourteen deliberately wrong steps makes the checker NAMED beside it fail -- an arithmetic fault by an arithmetic check, never by the frames."""
import math

import pytest
import torch

from tests import _gemm_cases as C

G = C.GUARD
BM = BN = 128


# ------------------------------------------------------------------------------------------------------------------ steps

def _epilogue(c, p, v, bug):
    """fp32 tail on the accumulator v [M, N] (fp32), as epilogue4 does it."""
    s = torch.tensor(math.tanh(c.gate), dtype=torch.float32) if c.gate is not None else torch.tensor(1.0)
    part = None
    if c.epi == "store":
        o = s * v
        if c.accumulate and bug != "ignores accumulate":
            o = p.view["C"].float() + o
        if c.out_dtype == C.F32:
            part = o.double() ** 2
    elif c.epi == "scale_res":
        R = p.view["R"]
        if bug == "R with ldc":
            R = torch.as_strided(p.full["R"], (c.M, c.N), (p.full["C"].stride(0), 1), G * p.full["R"].stride(0))
        o = v * s + R.float()
    elif c.epi == "gate_bwd":
        a = p.view["aux"].float()
        if c.aux_mode == "stash":
            o = s * v * a
        elif c.aux_mode == "sqrelu":
            r = a.clamp(min=0)
            o, part = s * v * (2 * r), v.double() * (r * r).double()
        else:
            o, part = s * v, v.double() * a.double()
    else:
        u = v.double()
        o = C.gelu64(u).float()
        if c.want_c2:
            p.view["C2"].copy_((C.gelu_grad64(u) if c.stash else u).float())
    return o, part


def _operand(p, nm, kmajor, extra):
    c = p.case
    rows = c.M if nm == "A" else c.N
    if kmajor:
        return p.full[nm][G:G + c.K + extra, :rows].T.double()
    return p.full[nm][G:G + rows, :c.K + extra].double()


def plain_step(p):
    c = p.case
    acc = _operand(p, "A", c.a_kmajor, 0) @ _operand(p, "B", c.b_kmajor, 0).T
    o, part = _epilogue(c, p, acc.float(), None)
    p.view["C"].copy_(o)
    if p.partial is not None:
        p.partial.copy_(C.tile_sums(part, *c.tile).float())


def tiled_step(bug=None):
    def step(p):
        c = p.case
        M, N, K = c.M, c.N, c.K
        A = _operand(p, "A", c.a_kmajor, 1 if bug in ("reads column k", "reads the row behind K") else 0)
        B = _operand(p, "B", c.b_kmajor, 1 if bug in ("reads column k", "reads the row behind K") else 0)
        gm, gn, nk = C.cdiv(M, BM), C.cdiv(N, BN), C.cdiv(A.shape[1], 64)
        Ap = torch.zeros(gm * BM, (nk + 1) * 64, dtype=torch.float64)
        Bp = torch.zeros(gn * BN, (nk + 1) * 64, dtype=torch.float64)
        Ap[:M, :A.shape[1]], Bp[:N, :B.shape[1]] = A, B                        # the edge mask: out-of-range rows and k read as zeros
        if bug == "counts masked elements":                                     # ... or as the last row, by a clamped address
            Ap[M:, :] = Ap[M - 1]
            Bp[N:, :] = Bp[N - 1]
        kts = list(range(nk))
        t1 = min(1, nk - 1)
        if bug == "loses the last k of a K-tile":
            Ap[:, 64 * t1 + 63] = 0
        if bug == "doubles a K-tile":
            kts.append(t1)
        if bug == "K rotation one off":
            kts = list(range(1, nk + 1))
        acc = torch.zeros(gm * BM, gn * BN, dtype=torch.float64)
        for i in range(gm):
            for j in range(gn):
                for t in kts[(i + j) % len(kts):] + kts[:(i + j) % len(kts)]:   # rotated by the tile, as variant 26 does
                    acc[i * BM:(i + 1) * BM, j * BN:(j + 1) * BN] += Ap[i * BM:(i + 1) * BM, 64 * t:64 * t + 64] @ Bp[j * BN:(j + 1) * BN, 64 * t:64 * t + 64].T
        if bug == "swaps two tiles":
            acc[:BM, :2 * BN] = torch.cat([acc[:BM, BN:2 * BN], acc[:BM, :BN]], 1)
        if bug == "transposes a 32 x 32 block":
            acc[:32, :32] = acc[:32, :32].T.clone()
        o, part = _epilogue(c, p, acc[:M, :N].float(), bug)
        if bug == "truncates to bf16":
            o = (o.contiguous().view(torch.int32) & -65536).view(torch.float32)
        p.view["C"].copy_(o)
        if bug == "stores 4 columns past N":
            p.full["C"][G:G + M, N:N + 4] = 0
        if bug == "stores a row past M":
            p.full["C"][G + M, :N] = 0
        if p.partial is not None:
            if bug == "counts masked elements":
                full = torch.nn.functional.pad(part[None, None], (0, gn * BN - N, 0, gm * BM - M), mode="replicate")[0, 0]
                sums = full.view(gm, BM, gn, BN).sum((1, 3))
            else:
                sums = C.tile_sums(part, BM, BN).view(gm, gn)
            flat = sums.T.reshape(-1).float()                                   # column-major slots: the order is not part of the contract
            if bug == "drops a tile's partial":
                flat[1] = float("nan")
            p.partial.copy_(flat)
    return step


def _reduce(partial, gate):
    t = partial.sum(dtype=torch.float32)
    if gate is not None:
        th = torch.tensor(math.tanh(gate), dtype=torch.float32)
        t = t * (1.0 - th * th)
    return float(t)


GATE = 0.37


def _s_cpu():
    return float(torch.tensor(math.tanh(GATE), dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------ the checkers pass

def small_cases():
    T = (BM, BN)
    mk = C.make_case
    out = []
    for kind in ("onehot", "count", "ints"):
        for od in (C.BF16, C.F32):
            out.append(mk(kind, 129, 132, 200, out_dtype=od, pads={"A": 8, "B": 16, "C": 4}))
            out.append(mk(kind, 65, 68, 136, out_dtype=od, epi="scale_res", r_dtype=C.BF16 if od == C.BF16 else C.F32, pads={"R": 8, "C": 4}))
            for am in (None, "sqrelu", "stash"):
                out.append(mk(kind, 129, 260, 72, out_dtype=od, epi="gate_bwd", aux_mode=am, aux_dtype=od, pads={"aux": 4}))
            out.append(mk(kind, 33, 12, 64, out_dtype=od, epi="gelu", want_c2=True, pads={"C2": 8}))
        if kind != "ints":                                                      # squares of dense integer products do not fit a tile
            out.append(mk(kind, 257, 260, 192, out_dtype=C.F32, accumulate=True, want_partial=True, tile=T))
        out.append(mk(kind, 257, 260, 192, out_dtype=C.BF16, epi="gate_bwd", want_partial=True, tile=T))
        out.append(mk(kind, 130, 264, 128, out_dtype=C.F32, epi="gate_bwd", aux_mode="sqrelu", want_partial=True, tile=T, gate=GATE))
        out.append(mk(kind, 64, 64, 128, kw=64))
        out.append(mk(kind, 136, 264, 200, a_kmajor=True, b_kmajor=True, pads={"A": 8, "B": 24}))
        out.append(mk(kind, 65, 68, 72, in_dtype=C.F32, out_dtype=C.F32))
    out.append(mk("onehot", 65, 132, 136, mirrored=True))
    for od in (C.BF16, C.F32):
        out.append(mk("gelu", 65, 68, 200, out_dtype=od, epi="gelu", want_c2=True))
        out.append(mk("gelu", 65, 68, 200, out_dtype=od, epi="gelu", stash=True))
        for epi, kw in (("store", {}), ("scale_res", {}), ("gate_bwd", {}), ("gate_bwd", {"aux_mode": "sqrelu"}), ("gate_bwd", {"aux_mode": "stash"})):
            out.append(mk("ints", 65, 68, 200, out_dtype=od, epi=epi, gate=GATE, **kw))
    out.append(mk("ints", 65, 68, 200, out_dtype=C.F32, accumulate=True, gate=GATE))
    return out


@pytest.mark.parametrize("step", [plain_step, tiled_step()], ids=["plain", "tiled"])
def test_checkers_pass_on_a_right_step(step):
    c0 = C.make_case("onehot", 65, 68, 200, out_dtype=C.F32, gate=GATE)
    res, _ = C.run_case(c0, step, s_dev=_s_cpu())
    s_dev = C.read_s_dev(c0, res)
    assert s_dev == _s_cpu()
    assert C.check_s_dev(s_dev, GATE) <= 1.0
    for c in small_cases():
        C.run_case(c, step, s_dev=s_dev, reduce=_reduce)
    print("\n" + C.worst_table())


# ------------------------------------------------------------------------------------------------------------------ the checkers fail

def _mut_case(kind, **kw):
    a = dict(M=257, N=260, K=200, out_dtype=C.F32, pads={"C": 8})
    a.update(kw)
    return C.make_case(kind, a.pop("M"), a.pop("N"), a.pop("K"), **a)


MUTANTS = [
    # bug, the case it is shown on, the reason the checker must give
    ("loses the last k of a K-tile", lambda: _mut_case("onehot"), C.C_NOT_EXACT),
    ("loses the last k of a K-tile", lambda: _mut_case("count", out_dtype=C.BF16), C.C_NOT_EXACT),
    ("doubles a K-tile", lambda: _mut_case("onehot"), C.C_NOT_EXACT),
    ("doubles a K-tile", lambda: _mut_case("ints", out_dtype=C.BF16), C.C_NOT_EXACT),
    ("K rotation one off", lambda: _mut_case("onehot"), C.C_NOT_EXACT),
    ("K rotation one off", lambda: _mut_case("onehot", mirrored=True), C.C_NOT_EXACT),
    ("swaps two tiles", lambda: _mut_case("count"), C.C_NOT_EXACT),
    ("swaps two tiles", lambda: _mut_case("onehot"), C.C_NOT_EXACT),
    ("transposes a 32 x 32 block", lambda: _mut_case("count", out_dtype=C.BF16), C.C_NOT_EXACT),
    ("stores 4 columns past N", lambda: _mut_case("ints"), C.FRAME_WRITTEN),
    ("stores a row past M", lambda: _mut_case("ints", out_dtype=C.BF16), C.FRAME_WRITTEN),
    ("counts masked elements", lambda: _mut_case("count", want_partial=True, tile=(BM, BN)), C.PARTIAL_MULTISET),
    ("counts masked elements", lambda: _mut_case("count", epi="gate_bwd", want_partial=True, tile=(BM, BN), out_dtype=C.BF16), C.PARTIAL_MULTISET),
    ("drops a tile's partial", lambda: _mut_case("count", epi="gate_bwd", aux_mode="sqrelu", want_partial=True, tile=(BM, BN)), C.PARTIAL_MULTISET),
    ("ignores accumulate", lambda: _mut_case("ints", accumulate=True), C.C_NOT_EXACT),
    ("R with ldc", lambda: _mut_case("ints", epi="scale_res", pads={"R": 8}), C.READ_OUTSIDE),
    ("reads column k", lambda: _mut_case("count", kw=8), C.READ_OUTSIDE),
    ("reads the row behind K", lambda: _mut_case("count", M=264, N=264, a_kmajor=True, b_kmajor=True, pads={"A": 8, "B": 24}), C.READ_OUTSIDE),
    ("truncates to bf16", lambda: _mut_case("ints", K=520, out_dtype=C.BF16), C.C_NOT_EXACT),
]


@pytest.mark.parametrize("bug,case,reason", MUTANTS, ids=["%s-%d" % (m[0].replace(" ", "_"), i) for i, m in enumerate(MUTANTS)])
def test_each_wrong_step_fails_its_named_check(bug, case, reason):
    c = case()
    C.run_case(c, tiled_step(), reduce=_reduce)                     # the same case passes on the right step
    with pytest.raises(C.CheckFailure) as e:
        C.run_case(c, tiled_step(bug), reduce=_reduce)
    print("\n%s -> %s" % (bug, e.value))
    assert e.value.reason == reason, str(e.value)


def test_a_wrong_s_or_a_third_rounding_fails_the_gated_bound():
    c = C.make_case("ints", 65, 68, 200, out_dtype=C.F32, epi="scale_res", gate=GATE)
    s = _s_cpu()
    C.run_case(c, tiled_step(), s_dev=s)
    with pytest.raises(C.CheckFailure) as e:
        C.run_case(c, tiled_step(), s_dev=float(torch.nextafter(torch.tensor(s), torch.tensor(1.0))))
    assert e.value.reason == C.C_BEYOND_BOUND
    with pytest.raises(C.CheckFailure) as e:
        C.check_s_dev(s * (1 + 6 * 2.0 ** -23), GATE)
    assert e.value.reason == C.S_DEV


def test_total_and_bit_identity_checks_can_fail():
    c = _mut_case("count", want_partial=True, tile=(BM, BN))
    with pytest.raises(C.CheckFailure) as e:
        C.run_case(c, tiled_step(), reduce=lambda p, g: _reduce(p, g) + 1.0)
    assert e.value.reason == C.PARTIAL_TOTAL

    def flips(p):
        tiled_step()(p)
        if p.partial is not None:
            p.view["C"][3, 5] += 1.0
    with pytest.raises(C.CheckFailure) as e:
        C.run_case(c, flips, reduce=_reduce)
    assert e.value.reason in (C.PARTIAL_CHANGES_C, C.C_NOT_EXACT)


# ------------------------------------------------------------------------------------------------------------------ builder conditions

def test_km_covers_every_k_tile_edge():
    for K in (8, 56, 64, 72, 136, 200, 192, 320, 512, 768, 1024, 128, 256, 384, 640, 129, 333):
        edges = C.k_edges(K)
        want = {0, K - 1} | {64 * t for t in range(C.cdiv(K, 64))} | {min(64 * t + 63, K - 1) for t in range(C.cdiv(K, 64))}
        want |= {128 * t for t in range(C.cdiv(K, 128))} | {min(128 * t + 127, K - 1) for t in range(C.cdiv(K, 128))}
        if K % 64 and K > 64:
            want |= {K // 64 * 64 - 1, K // 64 * 64}
        assert set(edges) == want
        rows = max(len(edges), 65)
        for mirrored in (False, True):
            c = C.make_case("onehot", rows if not mirrored else 33, 68 if not mirrored else C.cdiv(rows, 4) * 4, K, mirrored=mirrored)
            assert set(edges) <= set(c.km.tolist()), (K, mirrored)
            hot = c.B if mirrored else c.A
            assert bool(((hot != 0).sum(1) == 1).all()) and float(c.acc[0, 0]) == 1.0
            assert torch.equal(c.acc, c.A.double() @ c.B.double().T)             # the closed form against the product


def test_builder_caps_at_every_gpu_shape():
    """The count cap and the per-tile cap at the shapes tests/test_gpu_gemm_exact.py visits: on the exact product at the small ones, from
    the operands alone (count_bound, tile_bound: no product formed) at the 3072 x 4096 and 2824 x 4040 ones."""
    LARGE_K, LARGE_SHAPES, MULTI_K, MULTI_SHAPE, TILE_OF = C.LARGE_K, C.LARGE_SHAPES, C.MULTI_K, C.MULTI_SHAPE, C.TILE_OF
    worst_count, worst_tile = 0, 0
    for v, Ks in MULTI_K.items():
        for K in Ks:
            for kind in ("onehot", "count", "ints"):
                for epi, od, am in (("store", C.F32, None), ("gate_bwd", C.BF16, None), ("gate_bwd", C.F32, "sqrelu")):
                    if epi == "store" and kind != "count":
                        continue
                    c = C.make_case(kind, MULTI_SHAPE[0], MULTI_SHAPE[1], K, out_dtype=od, epi=epi, aux_mode=am, want_partial=True, tile=TILE_OF[v])
                    worst_tile = max(worst_tile, c.tile_max)
                    if kind == "count":
                        assert c.tile_max <= c.tile_bound
                        worst_count = max(worst_count, c.count_max)
    for (M, N) in LARGE_SHAPES:
        for K in LARGE_K:
            for partial in (False, True):
                c = C.make_case("count", M, N, K, out_dtype=C.F32, accumulate=partial, want_partial=partial, tile=(256, 256), with_acc=False)
                assert c.count_bound <= C.COUNT_CAP and (not partial or c.tile_bound < C.LIMIT)
                worst_count = max(worst_count, c.count_bound)
                worst_tile = max(worst_tile, c.tile_bound if partial else 0)
                mu = c.pa * c.pb * K
                assert not partial or (mu * mu + 1.25 * mu + 0.125) * M * N < C.LIMIT      # the whole-output total of otter_reduce_partials
    print("\n[gemm-cases] largest count (bound at the large shapes) %d of %d; largest per-tile sum (bound at the large shapes) %d of 2^24 = %d"
          % (worst_count, C.COUNT_CAP, worst_tile, C.LIMIT))
    assert worst_count <= C.COUNT_CAP and worst_tile < C.LIMIT


def test_bounds_stay_under_the_old_ceiling_and_ints_fit():
    for K in (8, 1024, 16384):
        assert K * 16 < C.LIMIT
    with pytest.raises(AssertionError):
        C.make_case("ints", 8, 8, 2 ** 20)
    u = torch.linspace(-8, 8, 4001, dtype=torch.float64)
    ref = C.gelu64(u)
    for cdf in (C.CDF_F32, C.CDF_BF16):
        b = u.abs() * cdf + 2 * C.H32 * ref.abs()
        b = b + C.HBF * (ref.abs() + b)
        assert bool((b <= C.GELU_CEILING * float(ref.abs().max())).all())
