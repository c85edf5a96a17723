"""tests/_decode_cases.py on the CPU: fed a plain fp64 attention step, every checker passes and every builder condition holds (each key owned
exactly once, counts within their limit, needle margin >= 32) at the shapes and positions tests/test_gpu_decode_key_accounting.py visits; fed
each deliberately wrong step, the matching checker fails.  That is what shows the GPU tests can fail."""
import pytest
import torch

from tests import _decode_cases as C

POOLS = {}


def pool(N, H, HD):
    key = (N, H, HD)
    if key not in POOLS:
        POOLS[key] = (C.random_pool(N, H, HD, C.CAPACITY, 77 + N + H), C.ownership_values(N, H, HD, C.CAPACITY))
    return POOLS[key]


@pytest.mark.parametrize("name", list(C.FAMILIES))
def test_count_inputs_hold_their_conditions_and_the_plain_step_passes(name):
    """Every (shape, position, variant) of the GPU file is built (the builder asserts ownership and the count limit); the fp64 step is checked
    at every narrow case and at the wide shape's 129 and 1350."""
    fam = C.FAMILIES[name]
    worst, top = 0.0, 0
    for (N, H) in C.shapes(fam):
        rnd, own = pool(N, H, fam.HD)
        for pos in C.positions(fam, (N, H)):
            kps = C._base(fam, N, H, pos, C.CAPACITY, C.CUS).kps
            for variant in C.variants(N, pos, kps):
                c = C.count_case(fam, N, H, pos, variant, rnd.k, own)
                top = max(top, int(c.count.max()))
                assert c.count_limit == 32 or (name[0] == "P" and (N, H, pos, variant) == (1, 2, 4100, "a")), (N, H, pos, variant)
                if (N, H) != fam.wide or pos < 4100:
                    worst = max(worst, C.check_counts(c, C.reference_step(c)))
    print("[decode-cases] %s count: largest count %d, worst error / bound of the fp64 step %.3f" % (name, top, worst))
    assert top <= 33


def test_only_one_listed_case_needs_a_count_above_32():
    """4101 keys over the 128 (pair, dim) slots of head_dim 64 at (1, 2): some element owns 33 whatever the rule.  Everything else is <= 32."""
    fam = C.FAMILIES["P2"]
    rnd, own = pool(1, 2, 64)
    c = C.count_case(fam, 1, 2, 4100, "a", rnd.k, own)
    assert int(c.count.max()) == 33 and c.count_limit == 33
    assert 1.0 / 33 - 1.0 / 4101 > 7.5 * C.TOL_COUNT          # a lost key still moves an element by more than 7.5 times the tolerance


@pytest.mark.parametrize("name", ["P1", "P2"])
def test_oracle_and_new_key_checkers_pass_on_the_plain_step(name):
    fam = C.FAMILIES[name]
    worst_o = worst_k = 0.0
    for (N, H) in C.NARROW:
        rnd, _ = pool(N, H, 64)
        for i, pos in enumerate(C.FULL):
            kps = C._base(fam, N, H, pos, C.CAPACITY, C.CUS).kps
            for variant in [v for v in C.variants(N, pos, kps) if v in "bc"]:
                rot = C.ROTS[(i + (variant == "c")) % 4]
                c = C.oracle_case(fam, N, H, pos, rot, variant, rnd)
                r = C.reference_step(c)
                worst_o = max(worst_o, C.check_oracle(c, r))
                worst_k = max(worst_k, C.check_new_key(c, r))
                c2 = C.oracle_case(fam, N, H, pos, rot, variant, rnd, quadrant=False)
                worst_k = max(worst_k, C.check_new_key(c2, C.reference_step(c2)))
    print("[decode-cases] %s oracle: worst error / bound of the fp64 step: o %.3f, k' %.3f" % (name, worst_o, worst_k))


@pytest.mark.parametrize("name", ["P2", "D2"])
@pytest.mark.parametrize("N,H", C.NARROW)
def test_needle_inputs_hold_their_margin_and_the_plain_step_passes(N, H, name):
    fam = C.FAMILIES[name]
    rnd, _ = pool(N, H, fam.HD)
    seen, lowest, through_table = set(), 1e30, False
    for pos in C.FULL:
        for kinds in C.needle_kind_schedule(fam, N, H, pos):
            for masked in (False, True):
                c = C.needle_case(fam, N, H, pos, kinds, rnd, masked=masked)
                lowest = min(lowest, c.margin)
                through_table |= getattr(c, "through_table", False)
                C.check_needle(c, C.reference_step(c))
            seen.update(kinds)
    assert lowest >= C.NEEDLE_MARGIN and through_table == (N > 1)
    assert {"first", "edge0", "edge127", "edge128", "iter_last", "key31", "key32", "prev", "new", "padded"} <= seen, seen


def test_needle_schedule_of_the_wide_shape_builds():
    fam = C.FAMILIES["P2"]
    N, H = fam.wide
    rnd = C.random_pool(N, H, 64, C.CAPACITY, 5)
    for kinds in C.needle_kind_schedule(fam, N, H, 1350):
        c = C.needle_case(fam, N, H, 1350, kinds, rnd)
        assert c.margin >= C.NEEDLE_MARGIN


def _count(N, H, pos, variant, name="P2"):
    fam = C.FAMILIES[name]
    rnd, own = pool(N, H, fam.HD)
    return C.count_case(fam, N, H, pos, variant, rnd.k, own), C.check_counts


def _oracle(N, H, pos, rot, variant, quadrant=True):
    rnd, _ = pool(N, H, 64)
    return C.oracle_case(C.FAMILIES["P2"], N, H, pos, rot, variant, rnd, quadrant=quadrant)


def _needle(N, H, pos, kind, name="P2"):
    fam = C.FAMILIES[name]
    rnd, _ = pool(N, H, fam.HD)
    return C.needle_case(fam, N, H, pos, [kind] * H, rnd), C.check_needle


# mutant -> the (case, checker) pairs that must reject it
REJECTED_BY = {
    "drop_range_last": lambda: [_count(3, 2, 300, "a"), _count(1, 2, 127, "a", "D2"), _needle(3, 2, 300, "edge127"), (_oracle(3, 2, 300, 32, "c"), C.check_oracle)],
    "drop_lonely_new": lambda: [_count(1, 2, 128, "a"), _count(3, 2, 256, "a", "D3"), _needle(1, 2, 128, "new"), _needle(3, 2, 256, "new", "D2")],
    "double_key": lambda: [_count(1, 2, 129, "a"), _count(3, 2, 4100, "a", "D2"), _count(3, 2, 64, "a", "D3")],
    "own_row": lambda: [_count(3, 2, 300, "b"), _count(3, 2, 33, "b", "D3"), _needle(3, 2, 300, "edge128"), (_oracle(3, 2, 64, 32, "b"), C.check_oracle)],
    "mask_shift": lambda: [_count(3, 2, 300, "b"), _count(1, 2, 31, "b", "D2"), (_oracle(3, 2, 300, 32, "c"), C.check_oracle)],
    "masked_range_weight1": lambda: [_count(3, 2, 300, "c"), _count(3, 2, 1350, "c", "D3"), (_oracle(3, 2, 300, 32, "c"), C.check_oracle)],
    "kv_shift": lambda: [_needle(3, 2, 300, "edge127"), _needle(3, 2, 129, "edge128", "D2"), _needle(1, 2, 33, "key31"), _needle(1, 2, 1, "first"), (_oracle(3, 2, 129, 32, "b"), C.check_oracle)],
    "rot_half_plus8": lambda: [(_oracle(3, 2, 300, r, "b", quadrant=False), C.check_new_key) for r in (16, 32, 48)]
    + [(_oracle(3, 2, 300, 32, "b"), C.check_oracle)],
    "rot_half_minus8": lambda: [(_oracle(3, 2, 300, r, "b", quadrant=False), C.check_new_key) for r in (32, 48, 64)]
    + [(_oracle(3, 2, 300, 48, "b"), C.check_oracle)],
}


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_every_wrong_step_is_rejected(mutant):
    pairs = REJECTED_BY[mutant]()
    assert pairs
    for c, check in pairs:
        check(c, C.reference_step(c))                                  # the plain step passes on the very same case
        with pytest.raises(AssertionError):
            check(c, C.reference_step(c, mutant))


def test_split_rule_restates_the_headers_static_asserts():
    assert C.split_rule(4096, 32, 256, 32) == (256, 16) and C.split_rule(4100, 32, 256, 32) == (288, 15)
    assert C.split_rule(4100, 32, 256, 64) == (320, 13) and C.split_rule(100, 32, 256, 32) == (128, 1)
    assert C.split_rule(4101, 2, 256, 64) == (128, 33) and C.split_rule(129, 6, 256, 64) == (128, 2)
