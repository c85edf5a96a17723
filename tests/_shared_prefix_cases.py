"""A shared-prefix beam table laid over the inputs of tests/_decode_cases.py (family D2: csrc/decode_cache.hip's), for the grouped kernel of
csrc/decode_cache_shared.hip.  Pure torch, device-agnostic.

The N rows are N / group sentences x `group` contiguous beams.  The LOGICAL table of a case is

    columns [0, shared_len)      the leader, (n // group) * group
    columns [shared_len, pos)    a sibling beam: a rotation within the group on the first half of them, a repeated ancestor on the second
    columns >= pos               the row's own index

and the builders of _decode_cases.py see that table (`shared_layout` puts it in the place of their `full_table`), so their counts, needles and
fp64 answers are those of otter_decode_attn_cached over it -- which is what the grouped entry points must return.  The grouped kernel itself
never reads the first `shared_len` columns; `poisoned` fills them, and the non-leader rows' cache slots below shared_len, with values that
give the game away if they are read.
"""
import contextlib

import torch

from tests import _decode_cases as C

FAM = C.FAMILIES["D2"]
SHAPES = [(2, 2), (3, 3), (6, 3), (8, 4)]          # (N, group), H = 2
H = 2
WIDE_SHAPE = (6, 3)                                # the one shape that visits positions 1 350 and 4 100
POSITIONS = [p for p in C.FULL if p <= 300]
WIDE_POSITIONS = [1350, 4100]


def shared_table(N, group, pos, shared_len, S_max):
    """int32 [N, S_max - 1]: the logical table of the module docstring."""
    n = torch.arange(N, dtype=torch.int32)
    leader, i = n // group * group, n % group
    src = n[:, None].repeat(1, S_max - 1)
    src[:, :shared_len] = leader[:, None]
    half = shared_len + (pos - shared_len) // 2
    src[:, shared_len:half] = (leader + (i + 1) % group)[:, None]                       # a rotation of the group's rows
    src[:, half:pos] = (leader + torch.where(i == group - 1, 0, 1).int())[:, None]     # a repeated ancestor (the group's row 1, and row 0)
    return src


@contextlib.contextmanager
def shared_layout(group, shared_len):
    """Within it the builders of _decode_cases.py lay the shared-prefix table instead of their own beam table."""
    saved = C.full_table
    C.full_table = lambda N, pos, S_max: shared_table(N, group, pos, shared_len, S_max)
    try:
        yield
    finally:
        C.full_table = saved


def shared_lens(pos, kps):
    """The prefix lengths at which the key loop changes path: 1, around a 32-key iteration, around a range edge, and up to the position."""
    return sorted({min(max(s, 1), pos) for s in (1, 31, 32, 33, kps - 1, kps, kps + 1, pos - 1, pos)})


def kps_of(N, group, pos, cus):
    """Keys per range of the grouped kernel: the split rule over (N / group) * H workgroups per range."""
    return C.split_rule(pos + 1, (N // group) * H, cus, FAM.kpi)[0]


def _finish(c, N, group, shared_len, cus):
    c.group, c.shared_len = group, shared_len
    c.kps, c.nsplit = C.split_rule(c.pos + 1, (N // group) * H, cus, FAM.kpi)
    return c


def count_case(N, group, pos, shared_len, variant, pool_k, own_v, cus, S_max=C.CAPACITY):
    """_decode_cases.count_case over the shared-prefix table.  Variant 'a': no mask, and the kernel gets src = NULL (the own part is the row's
    own); 'b' / 'z': the mask of make_mask, with its range edges those of the grouped kernel, and the sibling table."""
    gen = torch.Generator().manual_seed(1000 * pos + 10 * N + shared_len)
    c = C.count_case(FAM, N, H, pos, "a", pool_k, own_v, cus, S_max)
    _finish(c, N, group, shared_len, cus)
    c.variant = variant
    table = shared_table(N, group, pos, shared_len, S_max)
    if variant == "a":
        table[:, shared_len:] = torch.arange(N, dtype=torch.int32)[:, None]
    else:
        c.src = table
        c.valid = C.make_mask(variant, N, pos, S_max, c.kps, gen)
    # the counts, by the rule of _decode_cases.count_case, from the logical table and the mask
    j = torch.arange(pos + 1)
    cc = j % (N * H * FAM.HD)
    pair, d = cc // FAM.HD, cc % FAM.HD
    count = torch.zeros(N, H, FAM.HD, dtype=torch.int64)
    admitted = torch.zeros(N, dtype=torch.int64)
    for n in range(N):
        rows = torch.full((pos + 1,), n, dtype=torch.int64)
        rows[:pos] = table[n, :pos].long()
        ok = torch.ones(pos + 1, dtype=torch.bool) if c.valid is None else c.valid[n, :pos + 1].bool()
        h = pair - rows * H
        sel = ok & (h >= 0) & (h < H)
        count[n].index_put_((h[sel], d[sel]), torch.ones(int(sel.sum()), dtype=torch.int64), accumulate=True)
        admitted[n] = int(ok.sum())
    c.count, c.admitted = count, admitted
    c.new_admitted = torch.ones(N, dtype=torch.bool) if c.valid is None else c.valid[:, pos].bool()
    c.count_limit = max(32, -(-int(admitted.max()) // (N * H * FAM.HD)))
    assert int(count.max()) <= c.count_limit, (N, group, pos, shared_len, variant, int(count.max()))
    return c


def needle_case(N, group, pos, shared_len, kinds, pool, cus, masked=False):
    """_decode_cases.needle_case over the shared-prefix table: a needle below shared_len sits in the leader's row, one above it in a
    sibling's."""
    with shared_layout(group, shared_len):
        c = C.needle_case(FAM, N, H, pos, kinds, pool, cus, masked=masked)
    return _finish(c, N, group, shared_len, cus)


def needle_kinds(N, group, pos, shared_len, cus):
    """Per-head kind lists: key 0 and the edges of the grouped kernel's ranges, keys 31 / 32 / 63, the keys on both sides of shared_len, pos - 1,
    then the new token.  (No "padded" kind: its needles lie at another key in every row, which rows that share a prefix cannot have.)"""
    c = _finish(C._base(FAM, N, H, pos, C.CAPACITY, cus), N, group, shared_len, cus)
    cand = {k: j for k, j in C.needle_candidates(c, [0] * N).items() if k != "new" and j < pos}
    kinds = list(cand)
    return [[kinds[(i + h) % len(kinds)] for h in range(H)] for i in range(0, len(kinds), H)] + [["new"] * H]


def oracle_case(N, group, pos, shared_len, variant, pool, cus, rotary, alibi, S_max=C.CAPACITY):
    """Random K and V (the pool's, not written) behind the shared-prefix table, mask 'b' or 'c', and an exactly known query: with `rotary` the
    tables hold only (1, 0), (0, 1), (-1, 0), (0, -1) pairs, so q' is plus or minus an element of q (c.q: what the checker takes, c.q_in:
    what the kernel is given); `alibi`: slopes [H].  k' is taken from the written slot."""
    gen = torch.Generator().manual_seed(7000 * pos + 10 * N + shared_len)
    c = _finish(C._base(FAM, N, H, pos, S_max, cus), N, group, shared_len, cus)
    c.test, c.variant, c.rot, c.exact = "oracle", variant, 128 if rotary else 0, True
    c.kc, c.vc = pool.k, pool.v
    c.src = shared_table(N, group, pos, shared_len, S_max)
    c.valid = C.make_mask(variant, N, pos, S_max, c.kps, gen)
    c.q_in, c.k_new, c.v_new = (torch.randn(N, H, FAM.HD, generator=gen).bfloat16() for _ in range(3))
    c.q, c.cos_table, c.sin_table = c.q_in, None, None
    if rotary:
        c.cos_table, c.sin_table = C.quadrant_tables(128, S_max, gen)
        cs, sn = c.cos_table[pos].double(), c.sin_table[pos].double()
        x = c.q_in.double()
        c.q = (x * cs + torch.cat((-x[..., 64:], x[..., :64]), -1) * sn).bfloat16()      # exact: every term is 0 or plus / minus an element
        assert torch.equal(c.q.double(), x * cs + torch.cat((-x[..., 64:], x[..., :64]), -1) * sn)
    c.slopes = torch.tensor([0.25, 2.0 ** -5]) if alibi else None
    return c


def check_oracle(c, res):
    """_decode_cases.check_oracle; with ALiBi slopes the same bound against the same fp64 softmax with slope * (j - pos) added to every score."""
    if c.slopes is None:
        return C.check_oracle(c, res)
    pos, dev = c.pos, res.o.device
    q = c.q.double()
    K = torch.cat([C.gather_logical(c.kc, c.src, pos).double(), res.k_slot[:, :, None].double()], 2)
    V = torch.cat([C.gather_logical(c.vc, c.src, pos).double(), c.v_new[:, :, None].double()], 2)
    s = torch.einsum("nhd,nhkd->nhk", q, K) * c.scale
    s = s + c.slopes.double().to(dev)[None, :, None] * torch.arange(-pos, 1, device=dev, dtype=torch.float64)[None, None, :]
    ok = c.valid[:, :pos + 1].bool()
    s = s.masked_fill(~ok[:, None, :], float("-inf"))
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = p.sum(-1, keepdim=True)
    ref = torch.einsum("nhk,nhkd->nhd", p, V) / torch.where(l > 0, l, torch.ones_like(l))
    o = res.o.double().reshape(c.N, c.H, c.HD)
    err, bound = (o - ref).abs().amax(-1), C.TOL_ORACLE * ref.abs().amax(-1)
    dead = ~ok.any(1)
    assert bool((o[dead] == 0).all()), ("a fully masked row", c.N, c.group, c.pos, c.shared_len)
    ratio = err[~dead] / bound[~dead]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        raise AssertionError(("oracle (alibi)", c.N, c.group, c.pos, c.shared_len, c.variant, worst, (err / bound).tolist()))
    return worst


def poisoned(c, value=float("nan")):
    """Clones of the caches and of the table with everything the grouped kernel must not read spoiled: the non-leader rows' slots
    [0, shared_len) hold `value`, and the table's first shared_len columns point at the row itself (whose slots there are spoiled)."""
    kc, vc = c.kc.clone(), c.vc.clone()
    others = [n for n in range(c.N) if n % c.group]
    kc[others, :, :c.shared_len] = value
    vc[others, :, :c.shared_len] = value
    src = None
    if c.src is not None:
        src = c.src.clone()
        src[:, :c.shared_len] = torch.arange(c.N, dtype=torch.int32, device=src.device)[:, None]
    return kc, vc, src
