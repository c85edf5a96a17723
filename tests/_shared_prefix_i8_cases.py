"""The shared-prefix table of tests/_shared_prefix_cases.py over an int8 cache, for the grouped kernel of csrc/decode_cache_shared_i8.hip.
Pure torch, device-agnostic; everything about the table, the shapes, the positions and the count inputs is that module's and
tests/_decode_cases.py's, reused by import.

The kernel's geometry is 16 lanes per key, two keys per group in flight: 32 keys per iteration (`KPI`), so the ranges of a position are
those of split_rule(pos + 1, (N / group) * H, cus, 32) -- the same as the bf16 grouped kernel's -- and the 31 / 32 / 33 triple of
`shared_lens` already is KPI - 1, KPI, KPI + 1: an iteration and a group's pair of keys straddle it.
"""
import contextlib
from types import SimpleNamespace

import torch

from tests import _decode_cases as C
from tests import _shared_prefix_cases as S

KPI = 32
# the int8 family of _decode_cases.py (check_counts: what a slot holds of a 0 / 1 vector) with this kernel's keys per iteration
FAM = SimpleNamespace(**{**vars(C.FAMILIES["D3"]), "name": "D3s", "kpi": KPI})
H, SHAPES, WIDE_SHAPE, POSITIONS, WIDE_POSITIONS = S.H, S.SHAPES, S.WIDE_SHAPE, S.POSITIONS, S.WIDE_POSITIONS


@contextlib.contextmanager
def family():
    """Within it the builders of _shared_prefix_cases.py build for FAM."""
    saved = S.FAM
    S.FAM = FAM
    try:
        yield
    finally:
        S.FAM = saved


def positions(shape):
    return POSITIONS + (WIDE_POSITIONS if shape == WIDE_SHAPE else [])


def kps_of(N, group, pos, cus):
    return C.split_rule(pos + 1, (N // group) * H, cus, KPI)[0]


def shared_lens(pos, kps):
    """_shared_prefix_cases.shared_lens with its 31 / 32 / 33 read as KPI - 1, KPI, KPI + 1 (they are the same numbers)."""
    lens = S.shared_lens(pos, kps)
    assert all(min(max(s, 1), pos) in lens for s in (KPI - 1, KPI, KPI + 1))
    return lens


def count_case(N, group, pos, shared_len, variant, pool_k, own_v, cus, S_max=C.CAPACITY):
    """_shared_prefix_cases.count_case for FAM.  Its own assertion count.max() <= count_limit holds whatever KPI is: an element owns at most
    ceil((pos + 1) / (N H 128)) <= 9 keys."""
    with family():
        c = S.count_case(N, group, pos, shared_len, variant, pool_k, own_v, cus, S_max)
    assert c.fam is FAM and c.kps == kps_of(N, group, pos, cus)
    return c


def logical_table(N, group, pos, shared_len, S_max):
    return S.shared_table(N, group, pos, shared_len, S_max)


def poisoned(group, shared_len, kc, vc, ks, vs, src):
    """Clones with everything the grouped kernel must not read spoiled: the non-leader rows' slots [0, shared_len) hold NaN scales and 0x5A
    codes, and the table's first shared_len columns point at the row itself (whose slots there are spoiled)."""
    N = kc.shape[0]
    kc, vc, ks, vs = kc.clone(), vc.clone(), ks.clone(), vs.clone()
    others = [n for n in range(N) if n % group]
    for codes, scales in ((kc, ks), (vc, vs)):
        codes[others, :, :shared_len] = 0x5A
        scales[others, :, :shared_len] = float("nan")
    if src is not None:
        src = src.clone()
        src[:, :shared_len] = torch.arange(N, dtype=torch.int32, device=src.device)[:, None]
    return kc, vc, ks, vs, src
