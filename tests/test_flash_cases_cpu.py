"""tests/_flash_cases.py on the CPU: fed the plain fp64 step, every checker passes and every builder condition holds (no count above 32, one
owner dim per key, ramp growth as stated) at the narrow, padded and Sq != Sk cases that tests/test_gpu_flash_exact.py visits; fed the same
step with the kernels' bf16 roundings, the bounds' rounding counts suffice; at the long shapes the closed-form answers equal the plain step on
a subset of rows; fed each deliberately wrong step, the named checker fails for the stated reason.  That is what shows the GPU tests can fail."""
import math

import pytest
import torch

from tests import _flash_cases as C


@pytest.fixture(scope="module", autouse=True)
def worst_per_kind():
    yield
    print("\n" + C.worst_table())       # over the plain and the rounded steps (only checks that pass are recorded)


def _run(cases, rounded=False):
    worst = 0.0
    for c in cases:
        worst = max(worst, C.check(c, C.plain_step(c, rounded=rounded)))
    return worst


@pytest.mark.parametrize("hd", [128, 64])
def test_plain_step_passes_every_narrow_case(hd):
    worst = rnd = 0.0
    for S in C.ALL_S:
        cases = C.narrow_cases(S, hd)
        worst = max(worst, _run(cases))
        if S in (1, 33, 129, 321):
            rnd = max(rnd, _run(cases, rounded=True))
    print("[flash-cases] narrow hd %d: worst error / bound of the fp64 step %.3g, with the kernels' bf16 roundings %.3f" % (hd, worst, rnd))
    assert worst < 1e-6 and 0.05 < rnd <= 1.0


@pytest.mark.parametrize("mask", ["left", "holes", "right"])
def test_plain_step_passes_every_padded_case(mask):
    cases = C.padded_cases(mask, 128)
    dead = sum(int((C.forward_reference(c).n == 0).sum()) for c in cases[:1])
    worst, rnd = _run(cases), _run(cases[::3], rounded=True)
    print("[flash-cases] padded %s: %d cases, %d dead rows, fp64 step %.3g, rounded step %.3f" % (mask, len(cases), dead, worst, rnd))
    assert worst < 1e-6 and rnd <= 1.0
    assert (dead > 0) == (mask != "right")          # left padding leaves whole waves (pad 32, 64) and a whole block (pad 128, 129, 200) dead


@pytest.mark.parametrize("Sq,Sk", C.SQSK)
def test_plain_step_passes_every_sq_ne_sk_case(Sq, Sk):
    cases = C.sqsk_cases(Sq, Sk, 128) + C.sqsk_cases(Sq, Sk, 64)
    worst, rnd = _run(cases), _run(cases[::2], rounded=True)
    print("[flash-cases] Sq %d Sk %d: %d cases, fp64 step %.3g, rounded step %.3f" % (Sq, Sk, len(cases), worst, rnd))
    assert worst < 1e-6 and rnd <= 1.0
    if Sq > Sk:                                      # rows i < Sq - Sk see no key under the causal mask
        c = [c for c in cases if c.causal and c.kind == "count"][0]
        assert bool((C.forward_reference(c).n[:, :, :Sq - Sk] == 0).all()) and bool((C.forward_reference(c).n[:, :, Sq - Sk:] > 0).any())


def test_ramps_grow_as_stated_and_both_walks_of_the_forward_pass():
    """The builder asserts the growth; here the plain step, the rounded step and the tile-by-tile walk with the lazy rescale all pass, and the
    walk takes the stale-maximum path where it should."""
    worst = 0.0
    for c in C.ramp_cases():
        worst = max(worst, C.check(c, C.plain_step(c)), C.check(c, C.plain_step(c, rounded=True)))
        o, lse = C.online_forward(c)
        worst = max(worst, C.check_forward(c, C.Result(o=o, lse=lse)))
        if c.ramp == "up5.0":
            assert 7.0 < float(c.growth_log2.min()) and float(c.growth_log2.max()) < C.RESCALE_LOG2
        if c.ramp == "up5.6":
            assert C.RESCALE_LOG2 < float(c.growth_log2.min()) and float(c.growth_log2.max()) < 8.1
    print("[flash-cases] ramps: worst error / bound %.3f" % worst)
    assert worst <= 1.0


def row_step(case):
    """The plain step at the rows that a long one-query case reads (o = 0, lse = 0 elsewhere: never read)."""
    rows = torch.unique(torch.cat([case.rows_fwd, case.rows_bwd]))
    f = C.ref_forward(case, rows)
    o = torch.zeros(case.B, case.H, case.Sq, case.hd, dtype=torch.float64)
    lse = torch.zeros(case.B, case.H, case.Sq, dtype=torch.float64)
    o[:, :, rows], lse[:, :, rows] = f.o, f.lse
    g = C.ref_backward(case, C.sbh(o), lse, case.rows_bwd)
    return C.Result(o=C.sbh(o), lse=lse, dq=C.sbh(g.dq), dk=C.sbh(g.dk), dv=C.sbh(g.dv))


LONG = [(64, 8256, False), (8256, 8256, True), (8192, 8192, True), (4096, 4096, True), (4097, 4097, True), (4224, 4224, True)]


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("Sq,Sk,backward", LONG)
def test_long_cases_build_and_their_closed_forms_equal_the_plain_step(Sq, Sk, backward, hd):
    cases = C.long_cases(Sq, Sk, hd, backward=backward) + ([] if backward else C.long_cases(Sq, Sk, hd, backward=False, causal=False))
    kinds = [c.kind for c in cases]
    assert "count" in kinds and ("onequery" in kinds) == backward and all(c.long for c in cases)
    rows = torch.tensor(sorted({0, 1, 31, 32, 199 % Sq, 200 % Sq, 201 % Sq, Sq // 2, Sq - 2, Sq - 1}))
    worst = 0.0
    for c in cases:
        if c.kind == "onequery":
            worst = max(worst, C.check(c, row_step(c)))
            continue
        closed, plain = C.zero_score_forward(c), C.ref_forward(c, rows)
        assert float((closed.o[:, :, rows] - plain.o).abs().max()) < 1e-12 and bool((closed.n[:, :, rows] == plain.n).all())
        live = plain.n > 0
        assert float((closed.lse[:, :, rows][live] - plain.lse[live]).abs().max()) < 1e-12
        assert bool(torch.isinf(closed.lse[:, :, rows][~live]).all())
        worst = max(worst, C.check(c, C.closed_step(c), backward=backward))
        if c.kind == "count":
            assert c.top <= C.COUNT_LIMIT
    print("[flash-cases] long Sq %d Sk %d hd %d: %d cases (%s), worst error / bound %.3g" % (Sq, Sk, hd, len(cases), ", ".join(sorted(set(kinds))), worst))
    assert worst < 1e-6


# ------------------------------------------------------------------------------------------------------------- wrong steps

def _vis(extra):
    def fn(case, rows):
        return extra(case, rows, C.visible(case, rows))
    return fn


def drops_last_key_of_every_tile(c):
    return C.plain_step(c, _vis(lambda c, rows, v: v & (torch.arange(c.Sk) % C.TILE != C.TILE - 1)))


def _causal(c, rows, shift):
    v = torch.ones(c.B, 1, len(rows), c.Sk, dtype=torch.bool) if c.key_valid is None else c.key_valid.bool()[:, None, None, :].expand(-1, -1, len(rows), -1)
    return v & (torch.arange(c.Sk)[None, :] <= (rows + shift)[:, None])[None, None]


def admits_the_key_behind_the_diagonal(c):
    return C.plain_step(c, lambda c, rows: _causal(c, rows, c.Sk - c.Sq + 1))


def ignores_off(c):
    return C.plain_step(c, lambda c, rows: _causal(c, rows, 0))


def ignores_the_mask_from_tile_1_on(c):
    return C.plain_step(c, _vis(lambda c, rows, v: v | (_causal(C.SimpleNamespace(**{**c.__dict__, "key_valid": None}), rows, c.Sk - c.Sq)
                                                      & (torch.arange(c.Sk) >= C.TILE))))


def ignores_mask_bit_31(c):
    assert (c.Sk + 127) // 128 == 32
    r = row_step(c)
    r.dk[:, 31 * 128:], r.dv[:, 31 * 128:] = 0.0, 0.0       # the lane's bit of block 31 read as 0: its keys count as padded
    return r


def dead_rows_get_the_average_of_v(c):
    r = C.plain_step(c)
    dead = torch.isinf(r.lse)
    assert bool(dead.any())
    r.o = torch.where(dead.permute(0, 2, 1)[..., None], C.sbh(C.bh(c.v).mean(2, keepdim=True).expand(-1, -1, c.Sq, -1)), r.o)
    r.lse = torch.where(dead, torch.full_like(r.lse, math.log(c.Sk)), r.lse)
    return r


def lse_over_one_key_less_at_512(c):
    r = C.closed_step(c)
    n = torch.exp(r.lse)
    assert bool((n >= 512).any())
    r.lse = torch.where(n >= 511.5, torch.log(n - 1.0), r.lse)
    return r


def rescales_o_but_not_the_row_sum(c):
    o, lse = C.online_forward(c, "sum_not_rescaled")
    return C.Result(o=o, lse=lse)


def never_rescales_after_tile_0(c):
    o, lse = C.online_forward(c, "stale_forever")
    return C.Result(o=o, lse=lse)


def dkv_miss_the_last_query_tile(c):
    r = C.plain_step(c)
    g = C.ref_backward(c, r.o, r.lse, torch.arange((c.Sq - 1) // 32 * 32))
    r.dk, r.dv = C.sbh(g.dk), C.sbh(g.dv)
    return r


def dv_nonzero_at_a_masked_key(c):
    r = C.plain_step(c)
    b, j = (int(x) for x in torch.nonzero(c.key_valid == 0)[-1])
    r.dv[b, j, 0, 3] = 2.0 ** -20
    return r


def delta_from_another_head(c):
    r = C.plain_step(c)
    g = C.ref_backward(c, r.o.roll(1, 2), r.lse)
    r.dq, r.dk = C.sbh(g.dq), C.sbh(g.dk)
    return r


def _first(cases, kind, pred=lambda c: True):
    return [c for c in cases if c.kind == kind and pred(c)][0]


WRONG = [
    # wrong step, the case it is fed, the checker that must fail, the reason it must give
    (drops_last_key_of_every_tile, lambda: _first(C.narrow_cases(129, 128), "count"), C.check_forward, "count.lse"),
    (admits_the_key_behind_the_diagonal, lambda: _first(C.narrow_cases(129, 128), "onekey", lambda c: c.causal), C.check_forward, "onekey.zero"),
    (ignores_off, lambda: _first(C.sqsk_cases(33, 200, 128), "count", lambda c: c.causal), C.check_forward, "count.lse"),
    (ignores_the_mask_from_tile_1_on, lambda: _first(C.padded_cases("right", 128), "count"), C.check_forward, "count.lse"),
    (ignores_mask_bit_31, lambda: _first(C.long_cases(4096, 4096), "onequery", lambda c: int(c.istar.max()) == 4095), C.check_backward, "bwd.dk"),
    (dead_rows_get_the_average_of_v, lambda: _first(C.padded_cases("left", 128), "count"), C.check_forward, "dead.o"),
    (lse_over_one_key_less_at_512, lambda: _first(C.long_cases(4096, 4096), "count"), C.check_forward, "count.lse"),
    (rescales_o_but_not_the_row_sum, lambda: C.ramp_case("jump60", 128, False, False), C.check_forward, "ramp.o"),
    (never_rescales_after_tile_0, lambda: C.ramp_case("up30", 128, False, False), C.check_forward, "ramp.o"),
    (dkv_miss_the_last_query_tile, lambda: _first(C.narrow_cases(129, 128), "oracle", lambda c: not c.causal), C.check_backward, "bwd.dk"),
    (dv_nonzero_at_a_masked_key, lambda: _first(C.padded_cases("holes", 128), "oracle"), C.check_backward, "bwd.dv.zero"),
    (delta_from_another_head, lambda: _first(C.narrow_cases(64, 128), "oracle"), C.check_backward, "bwd.dq"),
]


@pytest.mark.parametrize("wrong,case,checker,reason", WRONG, ids=[w[0].__name__ for w in WRONG])
def test_wrong_step_is_rejected_by_its_checker(wrong, case, checker, reason):
    c = case()
    with pytest.raises(C.CheckFailure) as e:
        checker(c, wrong(c))
    print("[flash-cases] %s -> %s" % (wrong.__name__, e.value))
    assert e.value.reason == reason


def test_one_lost_key_is_far_outside_the_count_bounds():
    """What the old 2e-3 / fraction-of-the-maximum tolerances let through: at n = 8256 a lost key moves lse by 1.2e-4 (bound: a quarter of that)
    and an owned element of o by at least 1 / 32 of its value (bound: 2^-8 of it)."""
    n = 8256.0
    assert math.log(n / (n - 1)) > 3.9 * (0.25 / n)
    assert 1.0 / C.COUNT_LIMIT > 7.9 * C.BF16
