"""Inputs with exactly known answers for the split-key decode kernels (csrc/decode_split.h and its four includers, csrc/decode.hip), and the
checkers that go with them.  Pure torch, device-agnostic: tests/test_gpu_decode_key_accounting.py feeds the checkers with the HIP entry points,
tests/test_decode_cases_cpu.py with a plain fp64 attention step and with deliberately wrong ones.

A *case* is a SimpleNamespace: the physical caches kc / vc [N, H, S_max, HD] bf16, the beam table src [N, S_max - 1] int32 or None, the mask
valid [N, S_max] uint8 or None, the position `pos` (the step attends over keys 0 .. pos, key pos being the new token), the new token, and
what the builder knows about the answer.  A *step* is a callable case -> Result(o [N, H, HD], k_slot [N, H, HD], v_slot [N, H, HD]): the output
and what slot `pos` of the caller's own row holds afterwards.

Three kinds of input:
  count   every score is exactly 0 and V holds only 0 and 1, one 1 per key: o[n, h, d] = (keys that (n, h, d) owns) / (admitted keys), exact
          in fp32 in any summation order.  One lost, doubled or misplaced key moves an element by 1 / count, not by 1 / S.
  needle  the query is known exactly and one key per (row, head) outscores every other by >= 32: o = V[needle] to one bf16 rounding.
  oracle  the same exact query against an fp64 softmax over the gathered keys, at every position where the kernels change path.
"""
from types import SimpleNamespace

import numpy as np
import torch

CUS = 256                      # MI355X; the GPU tests pass the device's own count
MIN_KEYS_PER_SPLIT = 128
CAPACITY = 4224
FULL = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 300, 1350, 4100]
WIDE = [129, 1350, 4100]
DYN_ORDER = [4100, 129, 1350, 128, 1, 257, 127, 300, 64]
EPS, SCALE = 1e-5, 0.125
ROTS = [16, 32, 48, 64]

# kpi: keys per iteration of the kernel (GROUPS * UNROLL); D1 (csrc/decode.hip) has no ranges, 128 stands in for the mask's edges
FAMILIES = {
    "P1": SimpleNamespace(name="P1", kind="P", HD=64, kpi=64, ranges=True, table=False, i8=False, max_keys=65536, wide=(3, 64)),
    "P2": SimpleNamespace(name="P2", kind="P", HD=64, kpi=64, ranges=True, table=True, i8=False, max_keys=65536, wide=(3, 64)),
    "D1": SimpleNamespace(name="D1", kind="D", HD=128, kpi=32, ranges=False, table=False, i8=False, max_keys=16384, wide=(3, 32)),
    "D2": SimpleNamespace(name="D2", kind="D", HD=128, kpi=32, ranges=True, table=True, i8=False, max_keys=65536, wide=(3, 32)),
    "D3": SimpleNamespace(name="D3", kind="D", HD=128, kpi=64, ranges=True, table=True, i8=True, max_keys=65536, wide=(3, 32)),
}
NARROW = [(1, 2), (3, 2)]

TOL_COUNT = 2.0 ** -8 + 2.0 ** -16     # one bf16 rounding of an exact quotient + the fp32 division
TOL_ORACLE = 2.0 ** -8 + 2.0 ** -12    # one bf16 rounding + fp32 scores, __expf and the merges
NEEDLE_MARGIN = 32.0


class Result(SimpleNamespace):
    pass


def split_rule(Sk, NH, cus, kpi):
    """(kps, nsplit) of csrc/decode_split.h's split_rule."""
    want = max((2 * cus + NH - 1) // NH, 1)
    kps = max((Sk + want - 1) // want, MIN_KEYS_PER_SPLIT)
    kps = (kps + kpi - 1) // kpi * kpi
    return kps, (Sk + kps - 1) // kps


def positions(fam, shape):
    """The positions that a family visits at a shape: the full list at the narrow shapes, WIDE at its wide one, within its key limit."""
    ps = WIDE if shape == fam.wide else FULL
    return [p for p in ps if p + 1 <= fam.max_keys]


def shapes(fam):
    return NARROW + [fam.wide]


def beam_table(N, cols):
    """tests/test_gpu_fuyu_static_cache.beam_table, on the CPU: a permutation of the rows on the first half of the positions, a repeated
    ancestor (row 1, twice) on the second."""
    src = torch.empty(N, cols, dtype=torch.int32)
    half = cols // 2
    src[:, :half] = torch.tensor([2, 0, 1], dtype=torch.int32)[:N, None] % N
    src[:, half:] = torch.tensor([1, 1, 0], dtype=torch.int32)[:N, None] % N
    return src


def full_table(N, pos, S_max):
    """beam_table(N, pos) in a table of the capacity's width (the columns from pos on are never read: the row's own)."""
    src = torch.arange(N, dtype=torch.int32)[:, None].repeat(1, S_max - 1)
    src[:, :pos] = beam_table(N, pos)
    return src


def range_edges(pos, kps):
    """First and last key of every range of keys 0 .. pos."""
    out = []
    for j0 in range(0, pos + 1, kps):
        out += [j0, min(j0 + kps - 1, pos)]
    return sorted(set(out))


def make_mask(variant, N, pos, S_max, kps, gen):
    """uint8 [N, S_max] or None.  'a': none.  'b': left padding of 3 + 8 n keys, random holes at 30 %, and one masked key at the first and the
    last slot of every range.  'c' (N = 3): row 1 padded by kps + 72 keys (200 with ranges of 128), so that its first range is entirely masked
    and its second partly.  'z': 'b' with the last row masked entirely.  A row left without an admitted key (other than z's) gets key pos."""
    if variant == "a":
        return None
    valid = torch.ones(N, S_max, dtype=torch.uint8)
    if variant in ("b", "z"):
        holes = torch.rand(N, S_max, generator=gen) < 0.3
        valid[holes] = 0
        for n in range(N):
            valid[n, :min(3 + 8 * n, pos)] = 0
        valid[:, range_edges(pos, kps)] = 0
    elif variant == "c":
        assert N == 3 and pos >= kps + 72 + 57
        valid[1, :kps + 72] = 0
    else:
        raise ValueError(variant)
    for n in range(N):
        if not valid[n, :pos + 1].any():
            valid[n, pos] = 1
    if variant == "z":
        valid[N - 1] = 0
    return valid


def variants(N, pos, kps):
    return ["a", "b", "z"] + (["c"] if N == 3 and pos >= max(257, kps + 72 + 57) else [])


def rotary_tables(rot, S_max):
    inv = 1.0 / (25000.0 ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    fr = torch.arange(S_max, dtype=torch.float32)[:, None] * inv[None, :]
    emb = torch.cat([fr, fr], -1)
    return emb.cos().contiguous(), emb.sin().contiguous()


def quadrant_tables(rot, S_max, gen):
    """(cos, sin) [S_max, rot] with every entry pair one of (1, 0), (0, 1), (-1, 0), (0, -1), varied over dims and positions: every
    rotated element is plus or minus one of the inputs, exact in every number format."""
    q = torch.randint(0, 4, (S_max, rot), generator=gen)          # (independently per dim: the kernel must take cs[d], not its partner's)
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[q]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[q]
    return cos.contiguous(), sin.contiguous()


def random_pool(N, H, HD, S_max, seed):
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(k=torch.randn(N, H, S_max, HD, generator=g).bfloat16(), v=torch.randn(N, H, S_max, HD, generator=g).bfloat16())


def ownership_values(N, H, HD, S_max):
    """V [N, H, S_max, HD] bf16 of the count inputs: physical row r, head h, key j holds 1 at dim d exactly when key j's owner
    c = j mod (N H HD) is pair c // HD = r H + h, dim c % HD = d."""
    v = torch.zeros(N, H, S_max, HD)
    j = torch.arange(S_max)
    c = j % (N * H * HD)
    pair, d = c // HD, c % HD
    v[pair // H, pair % H, j, d] = 1.0
    assert bool((v.sum((0, 1, 3)) == 1).all())                    # every key is owned by exactly one (pair, dim)
    return v.bfloat16()


def _base(fam, N, H, pos, S_max, cus):
    kps, nsplit = split_rule(pos + 1, N * H, cus, fam.kpi) if fam.ranges else (MIN_KEYS_PER_SPLIT, 1)
    return SimpleNamespace(fam=fam, N=N, H=H, HD=fam.HD, pos=pos, S_max=S_max, kps=kps, nsplit=nsplit, scale=SCALE, eps=EPS, src=None, valid=None)


def _persimmon_token(c, gen, rot, exact_q, quadrant, tables=None):
    """The new token of a P case.  exact_q: gamma_q = 0 and beta_q = b (random bf16 values), so q' is the rotation of b whatever qkv holds."""
    c.rot = rot
    c.qkv = (torch.randn(c.N, c.H, 3, 64, generator=gen) * 2 + 0.3).bfloat16()
    c.gk, c.bk = 1 + 0.3 * torch.randn(64, generator=gen), 0.1 * torch.randn(64, generator=gen)
    c.gq = torch.zeros(64)
    c.bq = torch.randn(64, generator=gen).bfloat16().float() if exact_q else torch.zeros(64)
    if tables is None:
        tables = quadrant_tables(rot, c.S_max, gen) if quadrant else rotary_tables(rot, c.S_max)
    c.cos_table, c.sin_table = tables


def to_device(c, device):
    for k, v in list(vars(c).items()):
        if torch.is_tensor(v):
            setattr(c, k, v.to(device))
    return c


# ---- the count inputs (Test 1) --------------------------------------------------------------------------------------------------------------


def count_case(fam, N, H, pos, variant, pool_k, own_v, cus=CUS, S_max=CAPACITY, seed=0):
    """pool_k: random bf16 keys [N, H, S_max, HD]; own_v = ownership_values(N, H, HD, S_max).  Neither is written."""
    gen = torch.Generator().manual_seed(1000 * pos + 10 * N + H + seed)
    c = _base(fam, N, H, pos, S_max, cus)
    c.test, c.variant = "count", variant
    c.kc, c.vc = pool_k, own_v
    if variant != "a":
        c.src = full_table(N, pos, S_max)
        c.valid = make_mask(variant, N, pos, S_max, c.kps, gen)
    c.v_new = own_v[:, :, pos].clone()                                  # the same rule for j = pos, the row's own
    if fam.kind == "P":
        _persimmon_token(c, gen, 32, False, False)
        c.qkv[:, :, 2] = c.v_new
    else:
        c.q = torch.zeros(N, H, fam.HD, dtype=torch.bfloat16)
        c.k_new = torch.randn(N, H, fam.HD, generator=gen).bfloat16()
    # the counts, from the table and the mask
    j = torch.arange(pos + 1)
    cc = j % (N * H * fam.HD)
    pair, d = cc // fam.HD, cc % fam.HD
    count = torch.zeros(N, H, fam.HD, dtype=torch.int64)
    admitted = torch.zeros(N, dtype=torch.int64)
    for n in range(N):
        rows = torch.full((pos + 1,), n, dtype=torch.int64)
        if c.src is not None:
            rows[:pos] = c.src[n, :pos].long()
        ok = torch.ones(pos + 1, dtype=torch.bool) if c.valid is None else c.valid[n, :pos + 1].bool()
        h = pair - rows * H
        sel = ok & (h >= 0) & (h < H)
        count[n].index_put_((h[sel], d[sel]), torch.ones(int(sel.sum()), dtype=torch.int64), accumulate=True)
        admitted[n] = int(ok.sum())
    c.count, c.admitted = count, admitted
    c.new_admitted = torch.ones(N, dtype=torch.bool) if c.valid is None else c.valid[:, pos].bool()
    # one lost key moves an element by 1 / count - 1 / admitted: 32 keeps that at eight times the tolerance.  Some element owns
    # at least ceil(admitted keys / (N H HD)) keys, whatever the rule: 33 for 4101 keys over 128 (pair, dim) slots, the one listed case above 32.
    c.count_limit = max(32, -(-int(admitted.max()) // (N * H * fam.HD)))
    assert int(count.max()) <= c.count_limit, (fam.name, N, H, pos, variant, int(count.max()))
    return c


def check_counts(c, res):
    """o == 0 bit for bit where no admitted key is owned, |o - count / admitted| <= (2^-8 + 2^-16) count / admitted elsewhere; a fully masked
    row is all zeros; the appended slot is the new token.  Returns the worst error / bound."""
    dev = res.o.device
    o = res.o.double().reshape(c.N, c.H, c.HD)
    v_new = c.v_new.to(dev).double()
    if c.fam.i8:                                                      # code 127, scale fp32(1 / 127): the value the slot now holds
        one = float(np.float32(127.0) * (np.float32(1.0) / np.float32(127.0)))
        stored = v_new * one
    else:
        stored = v_new
    assert torch.equal(res.v_slot.double(), stored), ("v slot", c.fam.name, c.N, c.H, c.pos, c.variant)
    count, adm = c.count.to(dev), c.admitted.to(dev).double()[:, None, None]
    new_adm = c.new_admitted.to(dev)[:, None, None]
    hist = count.double() - torch.where(new_adm, v_new, torch.zeros_like(v_new))       # v_new is the 0 / 1 indicator of the new key's owner
    want = (hist + torch.where(new_adm, stored, torch.zeros_like(stored))) / adm.clamp(min=1)
    zero = count == 0
    tag = (c.fam.name, c.N, c.H, c.pos, c.variant)
    assert bool((o[zero] == 0).all()), ("o != 0 where no key is owned", tag, float(o[zero].abs().max()))
    dead = (c.admitted == 0).to(dev)
    assert bool((o[dead] == 0).all()) and bool(zero[dead].all()), ("a fully masked row", tag)
    ratio = ((o - want).abs() / (TOL_COUNT * want))[~zero]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        idx = ((o - want).abs() > TOL_COUNT * want).nonzero()[0].tolist()
        raise AssertionError(("count", tag, idx, float(o[tuple(idx)]), float(want[tuple(idx)]), int(count[tuple(idx)]), worst))
    return worst


# ---- the fp64 side ------------------------------------------------------------------------------------------------------------------------


def rotate_half64(y, cos, sin, rot, half=None):
    """y [..., 64] fp64: the first `rot` dims rotated, y1 = x1 c - x2 s, y2 = x2 c + x1 s (x1 / x2 the two halves of the rotated part)."""
    half = rot // 2 if half is None else half
    d = torch.arange(rot, device=y.device)
    first = d < half
    partner = torch.where(first, d + half, d - half) % 64
    out = y.clone()
    sign = torch.where(first, -1.0, 1.0).double()
    out[..., :rot] = y[..., :rot] * cos.double() + sign * y[..., partner] * sin.double()
    return out


def persimmon_qk64(c, half=None):
    """fp64 LayerNorm + rotate-half of the new token's q and k, before any rounding: (q' [N, H, 64], k' [N, H, 64])."""
    x = c.qkv[:, :, :2].double()
    mean = x.mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + c.eps)
    y = y * torch.stack([c.gq, c.gk]).double() + torch.stack([c.bq, c.bk]).double()
    y = rotate_half64(y, c.cos_table[c.pos], c.sin_table[c.pos], c.rot, half)
    return y[:, :, 0], y[:, :, 1]


def bf16_round(t):
    return t.float().bfloat16().double()       # (fp64 -> fp32 -> bf16: two roundings; the reference's own rounding, not a bound on anything)


def gather_logical(t, src, upto):
    """t [N, H, S, HD] -> [N, H, upto, HD]: position j of row n from physical row src[n, j]."""
    if src is None:
        return t[:, :, :upto]
    idx = src[:, :upto].long()
    return t[idx, :, torch.arange(upto, device=t.device)[None]].permute(0, 2, 1, 3)


def new_token64(c, half=None):
    """(q', k', v) of the new token as the kernels hold them: bf16-rounded q' and k', v raw; fp64 tensors [N, H, HD]."""
    if c.fam.kind == "P":
        q, k = persimmon_qk64(c, half)
        return bf16_round(q), bf16_round(k), c.qkv[:, :, 2].double()
    return c.q.double(), c.k_new.double(), c.v_new.double()


def attention64(c, q, k_slot, v_slot, src="table", valid=None, weights=None, v_shift=False):
    """fp64 softmax attention of q [N, H, HD] over the logical keys 0 .. pos (key pos = k_slot / v_slot).  weights [N, pos + 1]: a factor on
    every key's p (the mutants').  Rows without an admitted key give 0."""
    pos = c.pos
    table = c.src if src == "table" else None
    K = torch.cat([gather_logical(c.kc, table, pos).double(), k_slot[:, :, None].double()], 2)
    V = torch.cat([gather_logical(c.vc, table, pos).double(), v_slot[:, :, None].double()], 2)
    if v_shift:
        V = torch.cat([V[:, :, 1:], V[:, :, :1]], 2)
    s = torch.einsum("nhd,nhkd->nhk", q, K) * c.scale
    valid = c.valid if valid is None else valid
    ok = torch.ones(c.N, pos + 1, dtype=torch.bool, device=q.device) if valid is None else valid[:, :pos + 1].bool()
    s = s.masked_fill(~ok[:, None, :], float("-inf"))
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    if weights is not None:
        p = p * weights[:, None, :].double()
    l = p.sum(-1, keepdim=True)
    return torch.einsum("nhk,nhkd->nhd", p, V) / torch.where(l > 0, l, torch.ones_like(l))


MUTANTS = ["drop_range_last", "drop_lonely_new", "double_key", "own_row", "mask_shift", "masked_range_weight1", "kv_shift", "rot_half_plus8",
           "rot_half_minus8"]


def reference_step(c, mutant=None):
    """The plain fp64 attention step (bf16-rounded o, q', k' as the kernels round them), or one of the deliberately wrong ones:
      drop_range_last       the last key of every full range is lost
      drop_lonely_new       the new token is lost when it is alone in its range
      double_key            key pos - 1 is counted twice
      own_row               the row's own cache row is read instead of src[n, j]
      mask_shift            key j is admitted by key_valid[j - 1]
      masked_range_weight1  a range whose keys are all masked is merged as if none were
      kv_shift              K[j] is paired with V[j + 1]
      rot_half_plus8 / rot_half_minus8   the new token is rotated with half = rot / 2 +- 8"""
    assert mutant is None or mutant in MUTANTS, mutant
    half = None
    if mutant in ("rot_half_plus8", "rot_half_minus8"):
        half = c.rot // 2 + (8 if mutant == "rot_half_plus8" else -8)
    q, k_new, v_new = new_token64(c, half)
    dev = q.device
    pos, kps = c.pos, c.kps
    j = torch.arange(pos + 1, device=dev)
    w = torch.ones(c.N, pos + 1, device=dev)
    valid = c.valid
    if mutant == "drop_range_last":
        w[:, (j + 1) % kps == 0] = 0
    elif mutant == "drop_lonely_new" and pos % kps == 0:
        w[:, pos] = 0
    elif mutant == "double_key":
        w[:, pos - 1] = 2
    elif mutant == "mask_shift" and valid is not None:
        valid = torch.cat([torch.ones_like(valid[:, :1]), valid[:, :-1]], 1)
    elif mutant == "masked_range_weight1" and valid is not None:
        valid = valid.clone()
        for j0 in range(0, pos + 1, kps):
            j1 = min(j0 + kps, pos + 1)
            dead = ~valid[:, j0:j1].bool().any(1) & valid[:, :pos + 1].bool().any(1)
            valid[dead, j0:j1] = 1
    o = attention64(c, q, k_new, v_new, src="own" if mutant == "own_row" else "table", valid=valid, weights=w, v_shift=mutant == "kv_shift")
    v_slot = v_new
    if c.fam.i8:                                                      # what an int8 slot holds of a 0 / 1 vector: 127 * fp32(1 / 127) per 1
        v_slot = v_new * float(np.float32(127.0) * (np.float32(1.0) / np.float32(127.0)))
    return Result(o=bf16_round(o), k_slot=k_new, v_slot=v_slot)


# ---- the exact query: oracle (Test 3) and needle (Test 2) inputs ------------------------------------------------------------------------------


def exact_query(c):
    """q' of an exact-query case in fp64.  P: every element plus or minus an element of beta_q (the quadrant tables), which it asserts.
    D: the bf16 query itself."""
    if c.fam.kind == "D":
        return c.q.double()
    q, _ = persimmon_qk64(c)
    assert torch.equal(bf16_round(q), q) and bool((q.abs()[..., None] == c.bq.double().abs()).any(-1).all())
    return q


def oracle_case(fam, N, H, pos, rot, variant, pool, cus=CUS, S_max=CAPACITY, seed=0, quadrant=True, tables=None):
    """Random K and V (the pool's, not written), an exactly known query, ordinary gamma_k / beta_k, mask 'b' or 'c', the beam table.
    quadrant=False: ordinary rotary tables, for the check of the stored k' alone (the query is then known only to rounding)."""
    gen = torch.Generator().manual_seed(7000 * pos + 100 * rot + 10 * N + H + seed)
    c = _base(fam, N, H, pos, S_max, cus)
    c.test, c.variant = "oracle", variant
    c.kc, c.vc = pool.k, pool.v
    c.src = full_table(N, pos, S_max)
    c.valid = make_mask(variant, N, pos, S_max, c.kps, gen)
    _persimmon_token(c, gen, rot, True, quadrant, tables)
    c.v_new = c.qkv[:, :, 2].clone()
    c.exact = quadrant
    return c


def check_oracle(c, res):
    """Per (row, head): max_d |o - ref| <= (2^-8 + 2^-12) max_d |ref|, ref the fp64 softmax of the exactly known q' over the gathered keys with
    k' of the new token taken from the written slot.  A row without an admitted key must be exactly 0.  Returns the worst error / bound."""
    q = exact_query(c)
    ref = attention64(c, q, res.k_slot.double(), c.v_new.double())
    o = res.o.double().reshape(c.N, c.H, c.HD)
    err, bound = (o - ref).abs().amax(-1), TOL_ORACLE * ref.abs().amax(-1)
    dead = ~c.valid[:, :c.pos + 1].bool().any(1) if c.valid is not None else torch.zeros(c.N, dtype=torch.bool, device=o.device)
    assert bool((o[dead] == 0).all()), ("a fully masked row", c.fam.name, c.N, c.H, c.pos)
    live = ~dead
    ratio = err[live] / bound[live]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        raise AssertionError(("oracle", c.fam.name, c.N, c.H, c.pos, c.rot, c.variant, worst, (err / bound).tolist()))
    return worst


def check_new_key(c, res):
    """The stored k' against fp64 LayerNorm + rotate-half of the bf16 k: |k'_slot - k_ref| <= (2^-8 + 2^-12) |k_ref| + 2^-18 max |k_ref|,
    elementwise (dims >= rot are unrotated in the reference); v stored raw, bit for bit.  Returns the worst error / bound."""
    _, k_ref = persimmon_qk64(c)
    assert torch.equal(res.v_slot.double(), c.qkv[:, :, 2].double()), ("v slot", c.fam.name, c.pos)
    err = (res.k_slot.double() - k_ref).abs()
    bound = TOL_ORACLE * k_ref.abs() + 2.0 ** -18 * k_ref.abs().max()
    worst = float((err / bound).max())
    if not worst <= 1.0:
        idx = (err > bound).nonzero()[0].tolist()
        raise AssertionError(("new key", c.fam.name, c.N, c.H, c.pos, c.rot, idx, float(res.k_slot[tuple(idx)]), float(k_ref[tuple(idx)]), worst))
    return worst


def needle_candidates(c, pads):
    """{kind: logical key} of the needle positions of a case: 0 (or the first key every row admits), the first and the last key of every range,
    the last key of a 64-key iteration, keys 31 and 32, pos - 1, and pos itself."""
    pos, lo = c.pos, max(pads)
    out = {"first": lo}
    for e in range_edges(pos, c.kps):
        out["edge%d" % e] = e
    out["iter_last"] = 63 if pos > 127 else None
    if pos > 191:
        out["iter_last2"] = 191
    out["key31"], out["key32"], out["prev"], out["new"] = 31, 32, pos - 1, pos
    return {k: j for k, j in out.items() if j is not None and lo <= j <= pos}


def needle_case(fam, N, H, pos, kinds, pool, cus=CUS, S_max=CAPACITY, seed=0, masked=False):
    """kinds: one needle kind per head (needle_candidates), or "padded" for every head (each row left-padded, the needle its first admitted
    key), or "new" for every head (the new token: gamma_k / beta_k are shared).  Every row of a head has its needle at the same logical key -- rows that
    share an ancestor then share the slot -- except for "padded", which lies where the table is a permutation.  masked: key_valid hides the
    needle; the answer is then the fp64 oracle's without it (check_oracle).  The caches are clones: the needle is written into them."""
    gen = torch.Generator().manual_seed(9000 * pos + 10 * N + H + seed)
    c = _base(fam, N, H, pos, S_max, cus)
    c.test, c.variant, c.masked_needle = "needle", "pad", masked
    c.kc, c.vc = pool.k.clone(), pool.v.clone()
    c.src = full_table(N, pos, S_max)
    assert "padded" not in kinds or all(k == "padded" for k in kinds)
    pads = [min(2 + 3 * n, max(pos // 2 - 1, 0)) if "padded" in kinds else 0 for n in range(N)]
    valid = torch.ones(N, S_max, dtype=torch.uint8)
    valid[torch.rand(N, S_max, generator=gen) < 0.3] = 0
    for n in range(N):
        valid[n, :pads[n]] = 0
    if fam.kind == "P":
        _persimmon_token(c, gen, 32, True, True)
        c.v_new = c.qkv[:, :, 2].clone()
    else:                                                             # head_dim 128: the query is an input, exact as it stands
        c.rot = 0
        c.q, c.k_new, c.v_new = (torch.randn(N, H, fam.HD, generator=gen).bfloat16() for _ in range(3))
        c.q = c.q[:1].expand(N, H, fam.HD).contiguous()              # one query per head: rows that share an ancestor share its needle
    c.exact = True
    cand = needle_candidates(c, pads)
    new = "new" in kinds
    assert not new or all(k == "new" for k in kinds)
    jn = torch.empty(N, H, dtype=torch.int64)
    for h, kind in enumerate(kinds):
        for n in range(N):
            jn[n, h] = pads[n] if kind == "padded" else cand[kind]
    c.needle, c.kinds = jn, list(kinds)
    for n in range(N):
        valid[n, jn[n]] = 1
    c.valid = valid
    dev = pool.k.device
    to_device(c, dev)
    jn, valid = c.needle, c.valid
    q = exact_query(c)
    qn = (q ** 2).sum(-1)                                              # [N, H] (P: the same query for every pair)
    # the largest other score of every pair, in fp64 (for "new": over the cache; the new token's own k' becomes the needle)
    _, k_plain, _ = new_token64(c)
    K = torch.cat([gather_logical(c.kc, c.src, pos).double(), k_plain[:, :, None]], 2)
    s = torch.einsum("nhd,nhkd->nhk", q, K) * c.scale
    s = s.masked_fill(~valid[:, None, :pos + 1].bool(), float("-inf"))
    s.scatter_(2, jn[:, :, None], float("-inf"))
    other = s.amax(-1)                                                 # [N, H]; -inf when the needle is the only admitted key
    other = torch.where(torch.isfinite(other), other, torch.zeros_like(other))
    if new:
        if fam.kind == "P":
            alpha = float(other.max() + NEEDLE_MARGIN * 1.05 + 1) / (c.scale * float(qn[0, 0]))
            c.gk = torch.zeros(64, device=dev)
            c.bk = (alpha * c.bq.double()).float()                   # k' = bf16(rot(alpha b)) = bf16(alpha q')
        else:
            c.k_new = (((other + NEEDLE_MARGIN * 1.05 + 1) / (c.scale * qn))[:, :, None] * q).float().bfloat16()
        _, k_needle, _ = new_token64(c)
        margin = torch.einsum("nhd,nhd->nh", q, k_needle) * c.scale - other
        c.needle_v = c.v_new.double()
    else:
        alpha = ((other + NEEDLE_MARGIN * 1.05 + 1) / (c.scale * qn)).amax(0, keepdim=True).expand(N, H)   # per head: a slot may be shared
        k_needle = (alpha[:, :, None] * q).float().bfloat16()
        rows = torch.gather(c.src.long(), 1, jn.clamp(max=pos - 1))     # the physical row of every needle
        c.needle_v = torch.empty(N, H, fam.HD, dtype=torch.float64, device=dev)
        for n in range(N):
            for h in range(H):
                r, j = int(rows[n, h]), int(jn[n, h])
                # every row that reads this slot has its needle there too
                assert all(int(jn[m, h]) == j for m in range(N) if int(c.src[m, j]) == r), (n, h, r, j)
                if any(int(jn[m, h]) == j and int(c.src[m, j]) == r for m in range(n)):
                    k_needle[n, h] = c.kc[r, h, j]                  # the slot is already another row's needle (a shared ancestor)
                c.kc[r, h, j] = k_needle[n, h]
                c.needle_v[n, h] = c.vc[r, h, j].double()
        K = gather_logical(c.kc, c.src, pos).double()
        sn = torch.einsum("nhd,nhd->nh", q, torch.gather(K, 2, jn[:, :, None, None].expand(N, H, 1, fam.HD))[:, :, 0]) * c.scale
        margin = sn - other
        c.through_table = bool((rows != torch.arange(N, device=dev)[:, None]).any())
    c.margin = float(margin.min())
    assert c.margin >= NEEDLE_MARGIN, (fam.name, N, H, pos, kinds, c.margin)
    if masked:
        for n in range(N):
            c.valid[n, jn[n]] = 0
        for n in range(N):
            if not c.valid[n, :pos + 1].any():                        # (pos 1: the needle was the only admitted key)
                c.valid[n, [k for k in (0, pos) if k not in jn[n].tolist()][:1] or [pos]] = 1
    return c


def check_needle(c, res):
    """|o - V[needle]| <= 2^-8 |V[needle]| + 2^-30, elementwise; with the needle masked, the fp64 oracle's bound without it."""
    if c.masked_needle:
        return check_oracle(c, res)
    o = res.o.double().reshape(c.N, c.H, c.HD)
    want = c.needle_v.to(o.device)
    err, bound = (o - want).abs(), 2.0 ** -8 * want.abs() + 2.0 ** -30
    worst = float((err / bound).max())
    if not worst <= 1.0:
        idx = (err > bound).nonzero()[0].tolist()
        raise AssertionError(("needle", c.fam.name, c.N, c.H, c.pos, c.kinds, idx, float(o[tuple(idx)]), float(want[tuple(idx)]), worst))
    return worst


def needle_kind_schedule(fam, N, H, pos, cus=CUS):
    """The lists of per-head kinds that make every needle position of (shape, pos) hit: the cached kinds cycled over the heads, then "new"."""
    c = _base(fam, N, H, pos, CAPACITY, cus)
    cand = needle_candidates(c, [0] * N)
    kinds = [k for k in cand if k != "new" and cand[k] < pos]
    out = [[kinds[(i + h) % len(kinds)] for h in range(H)] for i in range(0, len(kinds), H)]
    return out + ([["padded"] * H] if pos // 2 - 1 > 0 else []) + [["new"] * H]
