"""The split-key decode kernels (csrc/decode_split.h through persimmon_decode.hip, persimmon_decode_cache.hip, decode_cache.hip,
decode_cache_i8.hip; csrc/decode.hip beside them) on inputs whose answer is known exactly -- tests/_decode_cases.py builds them and checks
them, tests/test_decode_cases_cpu.py shows that the checks fail on a step that loses, doubles or misplaces one key.

  Test 1 (all five families)  every score 0, V of 0 / 1 with one owner per key: o = count / admitted to one bf16 rounding, bit-exact zeros
                              where nothing is owned, at every position where a kernel changes path, without and with table and mask.
  Test 2 (P1, P2, D2)         one needle key per (row, head) outscoring the rest by >= 32, at every range and iteration edge, behind the
                              table, as the new token: o = V[needle]; with the needle masked, the fp64 answer without it.
  Test 3 (P1, P2)             an exactly known query against an fp64 softmax, rot 16 / 32 / 48 / 64; the stored k' against fp64 LayerNorm +
                              rotate-half on its own.

P1 = persimmon_decode_attn, P2 = persimmon_decode_attn_cached (+ _dyn), D1 = decode_attn, D2 = decode_attn_cached (+ _dyn),
D3 = decode_attn_cached_i8 (+ _dyn).  The dyn entry points keep one cache of capacity 4224 and one workspace and are walked down as well as
up (4100, 129, 1350, 128, 1, 257, 127, 300, 64), so a combine meets the stale records of ranges that are no longer live."""
import gc
from types import SimpleNamespace

import pytest
import torch

from tests import _decode_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
WORST = {}


def note(family, test, ratio, local=None):
    """Keeps the worst error / bound per (family, test) for the report, and per test function in `local`."""
    WORST[(family, test)] = max(WORST.get((family, test), 0.0), ratio)
    if local is not None:
        local[test] = max(local.get(test, 0.0), ratio)


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(scope="module")
def pools():
    """(random K / V pool, ownership V) per (N, H, HD), on the device; never left modified."""
    made = {}

    def get(N, H, HD):
        if (N, H, HD) not in made:
            p = C.random_pool(N, H, HD, C.CAPACITY, 77 + N + H)
            p.k, p.v = p.k.to(DEV), p.v.to(DEV)
            made[(N, H, HD)] = (p, C.ownership_values(N, H, HD, C.CAPACITY).to(DEV))
        return made[(N, H, HD)]

    yield get
    made.clear()
    gc.collect()
    torch.cuda.empty_cache()


def order(fam, shape):
    """The dyn order first (range counts go down as well as up), then the rest of the family's list."""
    ps = C.positions(fam, shape)
    return [p for p in C.DYN_ORDER if p in ps] + [p for p in ps if p not in C.DYN_ORDER]


# ---- the entry points as steps: case -> Result(o, k_slot, v_slot) ---------------------------------------------------------------------------


def _past(c, layout):
    K, V = C.gather_logical(c.kc, c.src, c.pos), C.gather_logical(c.vc, c.src, c.pos)
    if layout == "contiguous":
        return K.contiguous(), V.contiguous()
    k = K.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)                          # [N, S, H, 64] seen as [N, H, S, 64]
    v3 = torch.zeros(c.N, c.pos, c.H, 3, 64, dtype=torch.bfloat16, device=K.device)     # v inside a qkv projection
    v3[:, :, :, 2] = V.permute(0, 2, 1, 3)
    return k, v3[:, :, :, 2].permute(0, 2, 1, 3)


def step_p1(layout):
    def step(c):
        from otter_amd import ops

        pos = c.pos
        K, V = _past(c, layout)
        K0, V0 = K.clone(), V.clone()
        valid = None if c.valid is None else c.valid[:, :pos + 1].contiguous()
        o, kn, vn = ops.persimmon_decode_attn(c.qkv, c.gq, c.bq, c.gk, c.bk, c.cos_table[pos].contiguous(), c.sin_table[pos].contiguous(), K, V,
                                              valid, c.rot, c.eps, c.scale)
        torch.cuda.synchronize()
        assert torch.equal(K, K0) and torch.equal(V, V0)                                # the past is never written
        assert torch.equal(kn[:, :, :pos], K) and torch.equal(vn[:, :, :pos], V)        # copied rows: bit-equal
        return C.Result(o=o.view(c.N, c.H, 64), k_slot=kn[:, :, pos], v_slot=vn[:, :, pos])

    return step


def _in_place(c, tensors, call):
    """Run `call` over caches that it appends to in place; returns (o, the slot of every tensor); restores the slot and asserts that every
    other byte is as before."""
    before = [t.clone() for t in tensors]
    o = call()
    torch.cuda.synchronize()
    slots = [t[:, :, c.pos].clone() for t in tensors]
    for t, b in zip(tensors, before):
        t[:, :, c.pos] = b[:, :, c.pos]
        assert torch.equal(t, b), ("a cache byte outside the slot changed", c.fam.name, c.N, c.H, c.pos)
    return o, slots


def step_p2(dyn, pos_dev=None):
    def step(c):
        from otter_amd import ops

        pos = c.pos
        ln = (c.gq, c.bq, c.gk, c.bk)
        if dyn:
            pos_dev.fill_(pos)
            call = lambda: ops.persimmon_decode_attn_cached_dyn(c.qkv, *ln, c.cos_table, c.sin_table, c.kc, c.vc, pos_dev, c.rot, c.eps, c.scale,
                                                                src=c.src, key_valid=c.valid)
        else:
            call = lambda: ops.persimmon_decode_attn_cached(c.qkv, *ln, c.cos_table[pos], c.sin_table[pos], c.kc, c.vc, pos, c.rot, c.eps, c.scale,
                                                            src=c.src, key_valid=c.valid)
        o, (ks, vs) = _in_place(c, [c.kc, c.vc], call)
        return C.Result(o=o.view(c.N, c.H, 64), k_slot=ks, v_slot=vs)

    return step


def step_d1(c):
    from otter_amd import ops

    pos = c.pos
    K = torch.cat([C.gather_logical(c.kc, c.src, pos), c.k_new[:, :, None]], 2).contiguous()
    V = torch.cat([C.gather_logical(c.vc, c.src, pos), c.v_new[:, :, None]], 2).contiguous()
    valid = None if c.valid is None else c.valid[:, :pos + 1].contiguous()
    o = ops.decode_attn(c.q, K, V, None, valid, c.scale)
    torch.cuda.synchronize()
    return C.Result(o=o, k_slot=c.k_new, v_slot=c.v_new)                                # (no append: the keys are the caller's)


def step_d2(dyn, pos_dev=None):
    def step(c):
        from otter_amd import ops

        if dyn:
            pos_dev.fill_(c.pos)
            call = lambda: ops.decode_attn_cached_dyn(c.q, c.k_new, c.v_new, c.kc, c.vc, pos_dev, c.scale, src=c.src, key_valid=c.valid)
        else:
            call = lambda: ops.decode_attn_cached(c.q, c.k_new, c.v_new, c.kc, c.vc, c.pos, c.scale, src=c.src, key_valid=c.valid)
        o, (ks, vs) = _in_place(c, [c.kc, c.vc], call)
        assert torch.equal(ks, c.k_new)                                                 # no rotary: the key is stored as given
        return C.Result(o=o.view(c.N, c.H, 128), k_slot=ks, v_slot=vs)

    return step


def int8_cache(pool_k, own_v):
    """The int8 form of a count case's caches: V codes in {0, 1} with every scale 1.0 (stored values exactly 0 and 1); K random codes."""
    N, H, S = own_v.shape[:3]
    return SimpleNamespace(kq=(pool_k.float() * 40).round().clamp(-127, 127).to(torch.int8), vq=own_v.to(torch.int8),
                           ks=torch.full((N, H, S), 1.0 / 40, device=DEV), vs=torch.ones(N, H, S, device=DEV))


def step_d3(q8, dyn, pos_dev=None):
    def step(c):
        from otter_amd import ops

        kw = dict(src=c.src, key_valid=c.valid)
        if dyn:
            pos_dev.fill_(c.pos)
            call = lambda: ops.decode_attn_cached_i8_dyn(c.q, c.k_new, c.v_new, q8.kq, q8.vq, q8.ks, q8.vs, pos_dev, c.scale, **kw)
        else:
            call = lambda: ops.decode_attn_cached_i8(c.q, c.k_new, c.v_new, q8.kq, q8.vq, q8.ks, q8.vs, c.pos, c.scale, **kw)
        o, (kq, vq, ks, vs) = _in_place(c, [q8.kq, q8.vq, q8.ks[..., None], q8.vs[..., None]], call)     # (views: a scale's slot is [:, :, pos] too)
        k_slot, v_slot = kq.float() * ks, vq.float() * vs
        amax = c.k_new.float().abs().amax(-1, keepdim=True)
        assert torch.equal(ks, torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, 127.0)))   # a true division
        assert bool(((k_slot - c.k_new.float()).abs() <= ks * 0.5 * (1 + 2.0 ** -14)).all())
        return C.Result(o=o.view(c.N, c.H, 128), k_slot=k_slot, v_slot=v_slot)

    return step


def steps_of(fam, pool_k, own_v):
    """[(label, step)] of a family: the scalar entry point(s), then the dyn one."""
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    if fam.name == "P1":
        return [("contiguous", step_p1("contiguous")), ("prefill_view", step_p1("prefill_view"))]
    if fam.name == "P2":
        return [("scalar", step_p2(False)), ("dyn", step_p2(True, pos_dev))]
    if fam.name == "D1":
        return [("scalar", step_d1)]
    if fam.name == "D2":
        return [("scalar", step_d2(False)), ("dyn", step_d2(True, pos_dev))]
    q8 = int8_cache(pool_k, own_v)
    return [("scalar", step_d3(q8, False)), ("dyn", step_d3(q8, True, pos_dev))]


def dyn_workspace(fam, N, H):
    from otter_amd import ops

    nbytes = {"P2": ops.persimmon_decode_cached_dyn_workspace_bytes, "D2": ops.decode_attn_cached_dyn_workspace_bytes,
              "D3": ops.decode_attn_cached_i8_dyn_workspace_bytes}[fam.name](N, H, C.CAPACITY)
    return ops._ws.get(nbytes, torch.device(DEV, torch.cuda.current_device()))


def test_the_helper_restates_the_static_cache_tests_beam_table():
    from tests.test_gpu_fuyu_static_cache import beam_table

    for N, cols in ((1, 7), (3, 300), (3, 4100), (3, 1)):
        assert torch.equal(beam_table(N, cols).cpu(), C.beam_table(N, cols))


# ---- Test 1 ---------------------------------------------------------------------------------------------------------------------------------

FAMILY_SHAPES = [(name, shape) for name, fam in C.FAMILIES.items() for shape in C.shapes(fam)]
IDS = ["%s-N%dH%d" % (name, s[0], s[1]) for name, s in FAMILY_SHAPES]


@pytest.mark.parametrize("name,shape", FAMILY_SHAPES, ids=IDS)
def test_every_admitted_key_is_counted_exactly_once(pools, name, shape):
    """o == 0 bit for bit where no admitted key is owned and |o - count / admitted| <= (2^-8 + 2^-16) count / admitted elsewhere (one bf16
    rounding of an exact quotient, the fp32 division); a fully masked row is all zeros; the appended slot is the new token; every other cache
    byte is unchanged.  Variants: no table and no mask; the beam table with left padding, 30 % holes and a masked key at both ends of every
    range; that with one row masked entirely; (N = 3, pos >= 257) one row padded past its whole first range.  The count of an element is at
    most 32 -- a lost key moves it by eight tolerances -- except at head_dim 64, (1, 2), pos 4100 without a mask, where 4101 keys over 128
    (pair, dim) slots force a 33 (7.7 tolerances)."""
    fam = C.FAMILIES[name]
    N, H = shape
    pool, own = pools(N, H, fam.HD)
    steps, w = steps_of(fam, pool.k, own), {}
    ws = dyn_workspace(fam, N, H) if len(steps) > 1 and fam.table else None
    if ws is not None:                                                 # the dyn entry point alone, down and up, over one workspace
        dyn = steps[1][1]
        for pos in [p for p in C.DYN_ORDER if p in C.positions(fam, shape)]:
            c = C.to_device(C.count_case(fam, N, H, pos, "b", pool.k, own, cus()), DEV)
            note(name, "count", C.check_counts(c, dyn(c)), w)
            assert dyn_workspace(fam, N, H) is ws
    for pos in order(fam, shape):
        kps = C._base(fam, N, H, pos, C.CAPACITY, cus()).kps
        for variant in C.variants(N, pos, kps):
            c = C.to_device(C.count_case(fam, N, H, pos, variant, pool.k, own, cus()), DEV)
            for _, step in steps:
                note(name, "count", C.check_counts(c, step(c)), w)
    if ws is not None:
        assert dyn_workspace(fam, N, H) is ws
    print("[key-accounting] %s N%d H%d count: worst error / bound %.3f" % (name, N, H, w["count"]), flush=True)


# ---- Test 2 ---------------------------------------------------------------------------------------------------------------------------------

P_SHAPES = [(name, shape) for name in ("P1", "P2") for shape in C.shapes(C.FAMILIES[name])]
P_IDS = ["%s-N%dH%d" % (name, s[0], s[1]) for name, s in P_SHAPES]


NEEDLE_SHAPES = P_SHAPES + [("D2", shape) for shape in C.shapes(C.FAMILIES["D2"])]


@pytest.mark.parametrize("name,shape", NEEDLE_SHAPES, ids=P_IDS + ["D2-N%dH%d" % s for s in C.shapes(C.FAMILIES["D2"])])
def test_the_needle_key_goes_with_its_value(pools, name, shape):
    """|o - V[needle]| <= 2^-8 |V[needle]| + 2^-30 elementwise, the needle at key 0 (or the first key every row admits), the first and the last
    key of every range, keys 63 / 191 (the last of a 64-key iteration), 31, 32, pos - 1, the first admitted key after each row's left padding,
    behind a table entry of another physical row (N = 3: every needle of rows 0 and 2), and as the new token; then with the needle's slot masked,
    against the fp64 softmax without it under Test 3's bound (a masked needle that is still seen gives V[needle], far from that).  The Persimmon
    query is exact through gamma_q = 0, beta_q = b and quadrant rotary tables; D2's is its bf16 input, with no rotary."""
    fam = C.FAMILIES[name]
    N, H = shape
    pool, own = pools(N, H, fam.HD)
    steps, w = steps_of(fam, pool.k, own), {}
    seen = set()
    for pos in order(fam, shape):
        for kinds in C.needle_kind_schedule(fam, N, H, pos, cus()):
            seen.update(kinds)
            for masked in (False, True):
                c = C.needle_case(fam, N, H, pos, kinds, pool, cus(), masked=masked)
                for _, step in steps:
                    note(name, "needle masked" if masked else "needle", C.check_needle(c, step(c)), w)
    assert {"first", "edge0", "iter_last", "key31", "key32", "prev", "new", "padded"} <= seen and (shape == fam.wide or {"edge127", "edge128"} <= seen)
    print("[key-accounting] %s N%d H%d needle: worst error / bound %.3f, masked %.3f" % (name, N, H, w["needle"], w["needle masked"]), flush=True)


# ---- Test 3 ---------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,shape", P_SHAPES, ids=P_IDS)
def test_exact_query_against_the_fp64_oracle_at_every_edge(pools, name, shape):
    """Per (row, head): max_d |o - ref| <= (2^-8 + 2^-12) max_d |ref| (one bf16 rounding; fp32 scores, __expf and the merges), the query known
    exactly (gamma_q = 0, quadrant rotary tables), k' of the new token taken from the written slot, every position of the list, rot 16 / 32 /
    48 / 64, mask variants b and c, the beam table.  The stored k' is held to |k' - ref| <= (2^-8 + 2^-12) |ref| + 2^-18 max |ref| elementwise
    against fp64 LayerNorm + rotate-half, with these tables and with ordinary ones; v is stored raw."""
    fam = C.FAMILIES[name]
    N, H = shape
    pool, own = pools(N, H, 64)
    steps, w = steps_of(fam, pool.k, own), {}
    for pos in order(fam, shape):
        kps = C._base(fam, N, H, pos, C.CAPACITY, cus()).kps
        for rot in C.ROTS:
            for variant in [v for v in C.variants(N, pos, kps) if v in "bc"]:
                c = C.to_device(C.oracle_case(fam, N, H, pos, rot, variant, pool, cus()), DEV)
                for _, step in steps:
                    r = step(c)
                    note(name, "oracle", C.check_oracle(c, r), w)
                    note(name, "new key", C.check_new_key(c, r), w)
            c = C.to_device(C.oracle_case(fam, N, H, pos, rot, "b", pool, cus(), quadrant=False), DEV)
            for _, step in steps:
                note(name, "new key", C.check_new_key(c, step(c)), w)
    print("[key-accounting] %s N%d H%d oracle: worst error / bound: o %.3f, k' %.3f" % (name, N, H, w["oracle"], w["new key"]), flush=True)


def test_zz_report():
    """The worst error / bound per family and test of this run (profiles/decode_key_accounting.txt records them)."""
    for (family, test), r in sorted(WORST.items()):
        print("[key-accounting] worst %s %s %.4f" % (family, test, r))
        assert r <= 1.0
