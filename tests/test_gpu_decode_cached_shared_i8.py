"""GPU: the grouped cached-decode kernel over the int8 cache, csrc/decode_cache_shared_i8.hip (ops.decode_attn_cached_shared_i8 / _dyn), on
inputs with exactly known answers and against the fp64 oracle on the stored operands (tests/_shared_prefix_i8_cases.py: the shared-prefix
table of tests/_shared_prefix_cases.py over the int8 caches of tests/test_gpu_decode_key_accounting.py and tests/test_gpu_kv_cache_int8.py),
and generate(share_prompt=True, kv_cache_dtype="int8")'s pieces on 2-layer full-width hosts.

H = 2, (N, group) in {(2, 2), (3, 3), (6, 3), (8, 4)}; positions: _decode_cases.FULL up to 300 at every shape, 1 350 and 4 100 at (6, 3);
shared_len: 1, 31 / 32 / 33 (the kernel has 32 keys per iteration: an iteration and a group's pair of keys straddle it), kps - 1 / kps /
kps + 1 (a range edge), pos - 1, pos, clipped to [1, pos].  Both entry points everywhere.

Figures of the run that introduced it are in DESIGN.md section 4.20."""
import copy
import gc
import itertools
from types import SimpleNamespace

import pytest
import torch

from tests import _decode_cases as C
from tests import _shared_prefix_i8_cases as S8

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0x5A5A                                    # bf16 bit pattern of an untouched output
FLOOR = 2.0 ** -8                                # tests/test_gpu_kv_cache_int8.py: one bf16 rounding of the output
IDS = ["N%dg%d" % s for s in S8.SHAPES]
ENTRIES = ["scalar", "dyn"]


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def same(a, b):
    """Bit equality of two tuples of tensors (a NaN or a sentinel pattern is a value like any other)."""
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def call(a, dyn, caches=None, src="own", pos_dev=None, out=None):
    """One call of the grouped entry point on the inputs `a` (its own caches and table, or the ones given)."""
    from otter_amd import ops

    kc, vc, ks, vs = a.caches if caches is None else caches
    src = a.src if isinstance(src, str) else src
    if dyn:
        pos_dev = torch.empty(1, dtype=torch.int32, device=DEV) if pos_dev is None else pos_dev
        pos_dev.fill_(a.pos)
        return ops.decode_attn_cached_shared_i8_dyn(a.q, a.kn, a.vn, kc, vc, ks, vs, pos_dev, a.scale, a.group, a.sl, cos_table=a.cos_table,
                                                    sin_table=a.sin_table, src=src, key_valid=a.valid, slopes=a.slopes, out=out)
    rows = dict(cos=a.cos_table[a.pos], sin=a.sin_table[a.pos]) if a.cos_table is not None else {}
    return ops.decode_attn_cached_shared_i8(a.q, a.kn, a.vn, kc, vc, ks, vs, a.pos, a.scale, a.group, a.sl, src=src, key_valid=a.valid,
                                            slopes=a.slopes, **rows)


def existing(a, caches):
    """ops.decode_attn_cached_i8 (the parent's kernel) on the same inputs through the logical table."""
    from otter_amd import ops

    rows = dict(cos=a.cos_table[a.pos], sin=a.sin_table[a.pos]) if a.cos_table is not None else {}
    return ops.decode_attn_cached_i8(a.q, a.kn, a.vn, *caches, a.pos, a.scale, src=a.logical, key_valid=a.valid, slopes=a.slopes, **rows)


def slot(caches, pos):
    return tuple(t[:, :, pos].clone() for t in caches)


def restored(caches, orig, pos):
    """Slot `pos` put back: then every byte of the four tensors must be as before."""
    for t, t0 in zip(caches, orig):
        t[:, :, pos] = t0[:, :, pos]
    return same(caches, orig)


# ---- 1. count inputs --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def count_pools():
    """(int8 form of the count caches, their clones to compare against) per N: V codes in {0, 1} with every scale 1.0, K random codes."""
    from tests.test_gpu_decode_key_accounting import int8_cache

    made = {}

    def get(N):
        if N not in made:
            pool_k = C.random_pool(N, S8.H, 128, C.CAPACITY, 77 + N + S8.H).k.to(DEV)
            own = C.ownership_values(N, S8.H, 128, C.CAPACITY).to(DEV)
            q8 = int8_cache(pool_k, own)
            caches = (q8.kq, q8.vq, q8.ks.to(DEV), q8.vs.to(DEV))
            made[N] = (pool_k, own, caches, tuple(t.clone() for t in caches))
        return made[N]

    yield get
    made.clear()
    gc.collect()
    torch.cuda.empty_cache()


def count_step(c, caches, orig, dyn, pos_dev):
    """count case -> Result(o, k_slot, v_slot) with the slots dequantised; the appended slot holds the new token's codes and scales (the
    torch quantiser's), and no other byte of the four tensors changes."""
    from otter_amd.kv_cache import quantize_kv_int8

    a = SimpleNamespace(q=c.q, kn=c.k_new, vn=c.v_new, caches=caches, pos=c.pos, scale=c.scale, group=c.group, sl=c.shared_len, cos_table=None,
                        sin_table=None, src=c.src, valid=c.valid, slopes=None)
    o = call(a, dyn, pos_dev=pos_dev)
    torch.cuda.synchronize()
    kq, vq, ks, vs = slot(caches, c.pos)
    tag = (c.N, c.group, c.pos, c.shared_len, c.variant, dyn)
    assert same((kq, ks), quantize_kv_int8(c.k_new)) and same((vq, vs), quantize_kv_int8(c.v_new)), ("slot", tag)
    assert restored(caches, orig, c.pos), ("a byte outside the slot changed", tag)
    return C.Result(o=o.view(c.N, c.H, 128), k_slot=kq.float() * ks[..., None], v_slot=vq.float() * vs[..., None])


@pytest.mark.parametrize("shape", S8.SHAPES, ids=IDS)
def test_every_admitted_key_is_counted_exactly_once(count_pools, shape):
    """check_counts (bounds TOL_COUNT): o == 0 bit for bit where no admitted key is owned, |o - count / admitted| <= (2^-8 + 2^-16) count /
    admitted elsewhere, a fully masked row all zeros, the appended slot the new token's codes and scales, no other byte of the four tensors
    changed -- at every position and every shared_len of the module docstring, both entry points.  The masks a (none, src = NULL) / b / z take
    turns over the (position, shared_len) pairs, so that each meets every kind of shared_len."""
    N, group = shape
    pool_k, own, caches, orig = count_pools(N)
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst, turn, seen = 0.0, 0, set()
    for pos in S8.positions(shape):
        for sl in S8.shared_lens(pos, S8.kps_of(N, group, pos, cus())):
            variant = "abz"[turn % 3]
            turn += 1
            seen.add((variant, "1" if sl == 1 else "pos" if sl == pos else "mid"))
            c = C.to_device(S8.count_case(N, group, pos, sl, variant, pool_k, own, cus()), DEV)
            for dyn in (False, True):
                worst = max(worst, C.check_counts(c, count_step(c, caches, orig, dyn, pos_dev)))
    assert len(seen) == 9, seen
    print("[shared-prefix-i8] N%d group %d count: worst error / bound %.3f" % (N, group, worst), flush=True)


# ---- random int8 caches behind the shared-prefix table (tests 2 - 6) -----------------------------------------------------------------------

COMBOS = list(itertools.product([False, True], repeat=4))          # rotary, ALiBi, mask (with one fully masked row), fused q / k / v views


def make_inputs(N, group, pos, sl, g, rotary, alibi, masked, fused, S_max=None):
    """Random codes and scales (tests/test_gpu_kv_cache_int8._cache: slots >= pos hold sentinels), the logical shared-prefix table, that file's
    new tokens (zero, exact-tie and negative-amax vectors among them)."""
    from tests.test_gpu_kv_cache_int8 import _cache, _inputs

    H = S8.H
    S_max = pos + 3 if S_max is None else S_max
    caches = _cache(N, H, S_max, pos, g)
    q, kn, vn, zero = _inputs(N, H, fused, g)
    valid = None
    if masked:
        valid = (torch.rand(N, S_max, generator=g, device=DEV) > 0.3).to(torch.uint8)
        valid[:, pos] = 1
        valid[N // 2] = 0                                              # a fully masked row
    cos_table = sin_table = None
    if rotary:
        cos_table, sin_table = (torch.rand(S_max, 128, generator=g, device=DEV) * 2 - 1 for _ in range(2))
    slopes = (2.0 ** -(8.0 * torch.arange(1, H + 1, device=DEV, dtype=torch.float32) / H)).contiguous() if alibi else None
    logical = S8.logical_table(N, group, pos, sl, S_max).to(DEV)
    return SimpleNamespace(N=N, H=H, group=group, pos=pos, sl=sl, scale=128 ** -0.5, S_max=S_max, q=q, kn=kn, vn=vn, zero=zero, caches=caches,
                           orig=tuple(t.clone() for t in caches), valid=valid, cos_table=cos_table, sin_table=sin_table, slopes=slopes,
                           logical=logical, src=logical, rotary=rotary, masked=masked)


def oracle_case(a, stats):
    """One set of inputs, both entry points, against tests/test_gpu_kv_cache_int8._oracle_i8 over the logical table:
    err_grouped <= max(1.25 err_existing, 2^-8 max|ref|), err_existing the parent kernel's (ops.decode_attn_cached_i8) error against the same
    oracle on the same inputs through the logical table -- 1.25 and the floor are that file's.  Slot pos (codes and both scales) bit-equal to
    the existing kernel's and to the torch quantiser's for every row; a second call gives the same bits; a fully masked row is all zeros; no
    other byte of the four tensors changes."""
    from tests.test_gpu_kv_cache_int8 import _oracle_i8

    N, pos = a.N, a.pos
    tag = (N, a.group, pos, a.sl, a.rotary, a.slopes is not None, a.masked)
    cos, sin = (a.cos_table[pos], a.sin_table[pos]) if a.rotary else (None, None)
    ref, want_slot = _oracle_i8(a.q, a.kn, a.vn, *a.orig, pos, a.scale, cos, sin, a.logical, a.valid, a.slopes)
    theirs = tuple(t.clone() for t in a.orig)
    o_existing = existing(a, theirs).view(N, a.H, 128)
    their_slot = slot(theirs, pos)
    mag = float(ref.abs().max())
    err_existing = float((o_existing.double() - ref).abs().max())
    bound = max(1.25 * err_existing, FLOOR * mag)
    kq, ksc, vq, vsc = want_slot
    assert same(their_slot, (kq, vq, ksc, vsc)), ("the existing kernel's slot", tag)
    for dyn in (False, True):
        o = call(a, dyn).view(N, a.H, 128)
        torch.cuda.synchronize()
        got_slot = slot(a.caches, pos)
        assert same(got_slot, their_slot), ("slot", tag, dyn)
        o2 = call(a, dyn).view(N, a.H, 128)
        assert same((o,), (o2,)) and same(slot(a.caches, pos), their_slot), ("not deterministic", tag, dyn)
        assert restored(a.caches, a.orig, pos), ("a byte outside the slot changed", tag, dyn)
        if a.masked:
            assert float(o[N // 2].float().abs().max()) == 0.0, ("fully masked row", tag, dyn)
        err = float((o.double() - ref).abs().max())
        stats["worst"], stats["n"] = max(stats["worst"], err / bound), stats["n"] + 1
        assert err <= bound, ("o", tag, dyn, err, err_existing, mag)
    # the special vectors reached the quantisers (the value's always, the key's when nothing rotates it)
    kq8, vq8, ks8, vs8 = their_slot
    for codes, scales in ((vq8, vs8),) if a.rotary else ((kq8, ks8), (vq8, vs8)):
        assert not a.zero or (float(scales[0, 0]) == 1.0 and not bool(codes[0, 0].any())), ("zero vector", tag)
        assert float(scales[0, 1]) == 2.0 ** -7 and bool((codes[0, 1] % 2 == 0)[:-1].all()), ("tie vector", tag)
        assert int(codes[N - 1, 0, 5]) == -127, ("negative amax", tag)


# ---- 3. the fp64 oracle on the stored operands ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", S8.SHAPES, ids=IDS)
def test_kernel_against_fp64_oracle_on_the_stored_operands(shape):
    """oracle_case at every position and shared_len of the module docstring; {rotary} x {ALiBi} x {mask with one fully masked row} x {fused /
    separate q, k, v views} take turns over the (position, shared_len) pairs, all sixteen at every shape."""
    N, group = shape
    g = torch.Generator(device=DEV).manual_seed(5000 + 10 * N + group)
    stats, turn, seen = dict(worst=0.0, n=0), 0, set()
    for pos in S8.positions(shape):
        for sl in S8.shared_lens(pos, S8.kps_of(N, group, pos, cus())):
            combo = COMBOS[turn % len(COMBOS)]
            turn += 1
            seen.add(combo)
            oracle_case(make_inputs(N, group, pos, sl, g, *combo), stats)
    assert len(seen) == len(COMBOS)
    print("[shared-prefix-i8] N%d group %d oracle: %d runs, worst err_grouped / bound %.3f" % (N, group, stats["n"], stats["worst"]), flush=True)


# ---- 2. poison ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", S8.SHAPES, ids=IDS)
def test_shared_keys_are_read_from_the_leaders_row_only(shape):
    """The non-leader rows' slots [0, shared_len) hold NaN scales and 0x5A codes, and the table's first shared_len columns point at the row
    itself: o is finite and bit-equal to the run over clean caches.  (The existing kernel cannot pass this: it reads those columns.)"""
    N, group = shape
    g = torch.Generator(device=DEV).manual_seed(6000 + 10 * N + group)
    for pos in [p for p in S8.positions(shape) if p in (1, 33, 129, 257, 300, 4100)]:
        for sl in S8.shared_lens(pos, S8.kps_of(N, group, pos, cus())):
            a = make_inputs(N, group, pos, sl, g, False, True, False, True)
            *spoiled, src = S8.poisoned(group, sl, *a.orig, a.src)
            for dyn in (False, True):
                clean = call(a, dyn, caches=tuple(t.clone() for t in a.orig))
                got = call(a, dyn, caches=tuple(t.clone() for t in spoiled), src=src)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(got.float()).all()), (N, group, pos, sl, dyn)
                assert same((got,), (clean,)), (N, group, pos, sl, dyn)


# ---- 4. guard frames --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dyn", [False, True], ids=ENTRIES)
def test_nothing_outside_the_slot_and_the_workspace_is_written(dyn):
    """Through the C entry points, as tests/test_gpu_kv_cache_int8._raw does: o and a workspace of exactly the published size, each inside a
    sentinel frame.  The frames and every byte of the four tensors other than slot pos are untouched, o is the binding's, and one byte less of
    workspace is refused before anything is launched."""
    from otter_amd import _capi as K
    from otter_amd import ops
    from tests.test_gpu_decode_cached import _frame

    N, group = 6, 3
    g = torch.Generator(device=DEV).manual_seed(7000)
    name = "decode_attn_cached_shared_i8" + ("_dyn" if dyn else "")
    for pos, sl in ((129, 128), (300, 33), (4100, 1350)):
        a = make_inputs(N, group, pos, sl, g, True, True, True, False)
        want = call(a, dyn).clone()
        assert restored(a.caches, a.orig, pos)
        kc, vc, ks, vs = a.caches
        obuf, o16 = _frame(N * a.H * 128)
        need = (ops.decode_attn_cached_shared_i8_dyn_workspace_bytes(N, a.H, a.S_max) if dyn
                else ops.decode_attn_cached_shared_i8_workspace_bytes(N, a.H, pos + 1))
        wbuf, w16 = _frame(need // 2)
        pos_dev = torch.full((1,), pos, dtype=torch.int32, device=DEV)
        rotary = (a.cos_table.data_ptr(), a.sin_table.data_ptr(), a.cos_table.stride(0)) if dyn else \
                 (a.cos_table[pos].data_ptr(), a.sin_table[pos].data_ptr(), 0)
        args = [a.q.data_ptr(), a.q.stride(0), a.q.stride(1), a.kn.data_ptr(), a.kn.stride(0), a.kn.stride(1), a.vn.data_ptr(), a.vn.stride(0),
                a.vn.stride(1), *rotary, kc.data_ptr(), kc.stride(0), kc.stride(1), vc.data_ptr(), vc.stride(0), vc.stride(1), ks.data_ptr(),
                ks.stride(0), ks.stride(1), vs.data_ptr(), vs.stride(0), vs.stride(1), a.src.data_ptr(), a.src.stride(0), a.valid.data_ptr(),
                a.valid.stride(0), a.slopes.data_ptr(), o16.data_ptr(), w16.data_ptr(), need, N, a.H, pos_dev.data_ptr() if dyn else pos, a.S_max,
                128, float(a.scale), group, sl, K.stream()]
        fn = getattr(K.lib(), "otter_" + name)
        K.check(fn(*args), name)
        torch.cuda.synchronize()
        for b in (obuf, wbuf):
            assert bool((b[:256] == SENT).all()) and bool((b[-256:] == SENT).all()), ("frame", pos, sl)
        assert torch.equal(o16, want.view(torch.int16).reshape(-1)), (pos, sl)
        assert restored(a.caches, a.orig, pos), ("a byte outside the slot changed", pos, sl)
        args[31] = need - 1
        assert fn(*args) == -1 and b"%d needed" % need in K.lib().otter_last_error()


# ---- 5. the dyn entry -------------------------------------------------------------------------------------------------------------------------

def test_dyn_entry_is_bit_identical_to_the_scalar_entry_at_every_position():
    """One capacity-sized launch configuration (the same tensors, the same arguments, only the value in pos_dev moves), the positions of
    DYN_ORDER -- range counts go down as well as up: o and the appended slots are the scalar entry's bits, and a second call gives the same
    bits again."""
    N, group = S8.WIDE_SHAPE
    sl = 33
    g = torch.Generator(device=DEV).manual_seed(8000)
    a = make_inputs(N, group, C.CAPACITY - 1, sl, g, True, True, True, True, S_max=C.CAPACITY)
    a.src[:, sl:] = torch.randint(0, N, (N, C.CAPACITY - 1 - sl), generator=g, device=DEV, dtype=torch.int32)          # any ancestry
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.empty((N, a.H * 128), dtype=torch.bfloat16, device=DEV)
    dyn_caches = tuple(t.clone() for t in a.orig)
    for pos in [p for p in C.DYN_ORDER if p >= sl]:
        a.pos = pos
        theirs = tuple(t.clone() for t in a.orig)
        want = call(a, False, caches=theirs)
        again = call(a, False, caches=tuple(t.clone() for t in a.orig))
        for t, t0 in zip(dyn_caches, a.orig):
            t.copy_(t0)
        got = call(a, True, caches=dyn_caches, pos_dev=pos_dev, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert same((want,), (again,)), pos
        assert same((got,), (want,)), (pos, float((got.float() - want.float()).abs().max()))
        assert same(dyn_caches, theirs), pos
        got2 = call(a, True, caches=dyn_caches, pos_dev=pos_dev).clone()
        assert same((got2,), (want,)), pos


@pytest.mark.parametrize("bad", ["0", "shared_len - 1", "S_max"])
def test_dyn_entry_ignores_a_position_it_cannot_serve(bad):
    """pos_dev outside [1, S_max), or below shared_len (the in-place invariant needs shared_len <= pos): o, the codes and the scales are
    untouched."""
    from otter_amd import ops

    N, group, sl = 6, 3, 33
    g = torch.Generator(device=DEV).manual_seed(8100)
    a = make_inputs(N, group, 300, sl, g, True, True, True, True)
    out = torch.full((N, a.H * 128), SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    pos_dev = torch.full((1,), {"0": 0, "shared_len - 1": sl - 1, "S_max": a.S_max}[bad], dtype=torch.int32, device=DEV)
    ops.decode_attn_cached_shared_i8_dyn(a.q, a.kn, a.vn, *a.caches, pos_dev, a.scale, group, sl, cos_table=a.cos_table, sin_table=a.sin_table,
                                         src=a.src, key_valid=a.valid, slopes=a.slopes, out=out)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == SENT).all()) and same(a.caches, a.orig)


# ---- 6. groups of 5 and 6 -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(5, 5), (6, 6)], ids=["N5g5", "N6g6"])
def test_other_group_sizes(shape):
    """The remaining instances: oracle_case at a straddling shared_len, every option on."""
    N, group = shape
    g = torch.Generator(device=DEV).manual_seed(9000 + group)
    stats = dict(worst=0.0, n=0)
    for pos, sl in ((300, 33), (129, 128)):
        oracle_case(make_inputs(N, group, pos, sl, g, True, True, True, True), stats)
    print("[shared-prefix-i8] N%d group %d oracle: worst err_grouped / bound %.3f" % (N, group, stats["worst"]), flush=True)


# ---- 7. hosts (the schedule of tests/test_gpu_decode_cached_shared.py) ---------------------------------------------------------------------------

from tests.test_gpu_decode_cached_shared import (B, NB, NEW, P_LEN, PAD, ROWS, _Count, _ctx, _drift, _prompt_pass, _quantised_pair, _run,  # noqa: E402
                                                 _schedule, hosts)  # noqa: F401


@pytest.mark.parametrize("decoder", ["bf16", "w8"])
@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_share_prompt_int8_steps_stay_within_twice_the_unshared_int8_drift(hosts, kind, decoder, monkeypatch):
    """2-layer full-width host, B = 2 x 3 beams, a 40-token prompt (row 1 left-padded by 9), 11 cached steps with per-beam tokens and
    reorders, kv_cache_dtype="int8".  With OTTER_SHARED_PREFIX_I8=1 every step of every layer runs on the grouped int8 op, and its logits'
    drift from an fp32-compute run of the same model is at most twice the unshared int8-KV static path's own drift from that run.  With
    OTTER_SHARED_PREFIX_I8=0 the same run goes through ops.decode_attn_cached_i8 and picks the same token wherever the top-2 margin exceeds
    twice the difference of the two paths' logits."""
    from otter_amd import ops

    model, bench = hosts(kind)
    run_model, model = _quantised_pair(model) if decoder == "w8" else (model, model)
    grouped, i8_k = _Count(monkeypatch, ops, "decode_attn_cached_shared_i8"), _Count(monkeypatch, ops, "decode_attn_cached_i8")
    layers = 2
    monkeypatch.delenv("OTTER_SHARED_PREFIX", raising=False)
    monkeypatch.setenv("OTTER_SHARED_PREFIX_I8", "1")
    ref = _run(model, bench, False, False)
    assert (grouped.n, i8_k.n) == (0, 0)                                                 # fp32 compute: the restatement
    d_plain = _drift(_run(run_model, bench, True, False, "int8"), ref)
    assert (grouped.n, i8_k.n) == (0, layers * (NEW - 1))
    shared = _run(run_model, bench, True, True, "int8")
    assert (grouped.n, i8_k.n) == (layers * (NEW - 1), layers * (NEW - 1))                # every step of every layer on the grouped int8 op
    d_shared = _drift(shared, ref)
    monkeypatch.setenv("OTTER_SHARED_PREFIX_I8", "0")
    table = _run(run_model, bench, True, True, "int8")
    assert (grouped.n, i8_k.n) == (layers * (NEW - 1), 2 * layers * (NEW - 1))            # the existing int8 op, through the table
    top2 = shared.topk(2, dim=-1).values
    decided = (top2[..., 0] - top2[..., 1]) > 2 * (shared - table).abs().amax(-1)
    print("[shared-prefix-i8] %s %s: drift vs fp32: int8 KV unshared %.3e, share_prompt grouped %.3e (ratio %.2f), table path %.3e; %.0f %% of "
          "the steps decided" % (kind, decoder, d_plain, d_shared, d_shared / d_plain, _drift(table, ref), 100 * float(decided.float().mean())),
          flush=True)
    assert bool(decided.any()) and bool((shared.argmax(-1) == table.argmax(-1))[decided].all())
    assert d_plain > 0 and d_shared <= 2 * d_plain, (d_shared, d_plain)


# ---- 8. replay ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_replayed_shared_int8_steps_equal_the_eager_ones(hosts, kind, monkeypatch):
    """The steps after a shared prompt pass into an int8 cache under a captured graph (2 eager warm-up steps, 1 capture, 9 replays in 11 cached
    steps) against the same replay-mode steps issued eagerly over a second pair of caches: every step's logits torch.equal, in bf16 and
    with the int8 decoder.  The captured step runs the grouped int8 dyn op."""
    from otter_amd import ops
    from otter_amd.graph_decode import GraphDecodeStep

    model, bench = hosts(kind)
    monkeypatch.delenv("OTTER_SHARED_PREFIX", raising=False)
    monkeypatch.setenv("OTTER_SHARED_PREFIX_I8", "1")                  # (the grouped kernel at 2 sentences x 40 shared keys)
    grouped, i8_k = _Count(monkeypatch, ops, "decode_attn_cached_shared_i8_dyn"), _Count(monkeypatch, ops, "decode_attn_cached_i8_dyn")
    cont, reorders = _schedule()
    for tag in ("bf16", "w8"):
        if tag == "w8":
            model = copy.deepcopy(model)
            assert model.quantize_decoder_int8()["replaced"] > 0
        with torch.no_grad(), _ctx(True):
            cache, mc, full, logits = _prompt_pass(model, bench, True, True, "int8")
            c2, m2 = copy.copy(cache), copy.copy(mc)
            c2.k, c2.v, c2.k_scale, c2.v_scale, c2.src = (t.clone() for t in (cache.k, cache.v, cache.k_scale, cache.v_scale, cache.src))
            m2.seen, m2.kv = mc.seen.clone(), list(mc.kv)
            cache.enable_replay(full[:, :P_LEN], beams=True)
            c2.enable_replay(full[:, :P_LEN], beams=True)
            graph, eager = GraphDecodeStep(model.lang_encoder, cache, mc), GraphDecodeStep(model.lang_encoder, c2, m2)
            assert graph.use_graph
            eager.use_graph = False
            try:
                for t in range(NEW - 1):
                    for c, m in ((cache, mc), (c2, m2)):
                        c.reorder(reorders[t])
                        m.reorder(reorders[t])
                    lg = graph(cont[:, t:t + 1]).clone()
                    le = eager(cont[:, t:t + 1])
                    assert torch.equal(lg, le), (kind, tag, t, float((lg.float() - le.float()).abs().max()))
                assert same((cache.k, cache.v, cache.k_scale, cache.v_scale, cache.src), (c2.k, c2.v, c2.k_scale, c2.v_scale, c2.src))
                assert (graph.captures, graph.replays) == (1, NEW - 1 - 2) and graph.replays == 9
            finally:
                graph.release()
                eager.release()
                model.lang_encoder.clear_conditioned_layers()
    assert grouped.n > 0 and i8_k.n == 0


# ---- 9. generate --------------------------------------------------------------------------------------------------------------------------------

def test_generate_share_prompt_int8_with_graph_decode(hosts, monkeypatch):
    """generate(num_beams=3, no_repeat_ngram_size=3, cache_implementation="static", kv_cache_dtype="int8", cross_attention_cache=True,
    graph_decode=True, share_prompt=True) on the 2-layer MPT host: the prompt pass has B rows, one capture and 9 replays serve the 11 cached
    steps on the grouped int8 dyn op, and the tokens are those of the same call without the graph."""
    from otter_amd import ops
    from otter_amd.graph_decode import GraphDecodeStep

    model, bench = hosts("mpt")
    monkeypatch.delenv("OTTER_SHARED_PREFIX", raising=False)
    monkeypatch.setenv("OTTER_SHARED_PREFIX_I8", "1")                  # (the grouped kernel at 2 sentences x 40 shared keys)
    grouped, i8_k = _Count(monkeypatch, ops, "decode_attn_cached_shared_i8_dyn"), _Count(monkeypatch, ops, "decode_attn_cached_i8_dyn")
    vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN, DEV, seed=99, frames=1)
    mask[1, :PAD] = 0
    counts, rows, release = [], [], GraphDecodeStep.release

    def spy_release(self):
        counts.append((self.steps, self.captures, self.replays, self.use_graph))
        return release(self)

    monkeypatch.setattr(GraphDecodeStep, "release", spy_release)
    h = model.lang_encoder.register_forward_hook(lambda _m, _a, k, _o: rows.append(tuple(k["input_ids"].shape)), with_kwargs=True)
    kw = dict(max_new_tokens=NEW, eos_token_id=-1, num_beams=NB, no_repeat_ngram_size=3, cache_implementation="static", kv_cache_dtype="int8",
              cross_attention_cache=True, share_prompt=True)
    try:
        with torch.no_grad(), _ctx(True):
            got = model.generate(vision_x=vx.to(torch.bfloat16), lang_x=ids, attention_mask=mask, graph_decode=True, **kw)
            n_graph = len(rows)
            assert 2 * 3 <= grouped.n < 2 * (NEW - 1)              # two layers x (2 warm-up steps + the captured one): the rest are replays
            want = model.generate(vision_x=vx.to(torch.bfloat16), lang_x=ids, attention_mask=mask, **kw)
    finally:
        h.remove()
    assert i8_k.n == 0
    assert counts == [(NEW - 1, 1, NEW - 3, True)], counts
    assert rows[0] == (B, P_LEN) and rows[n_graph] == (B, P_LEN) and set(rows[n_graph + 1:]) == {(ROWS, 1)}
    assert got.shape == (B, P_LEN + NEW) and torch.equal(got, want), (got[:, P_LEN:].tolist(), want[:, P_LEN:].tolist())
    assert not model.lang_encoder.is_conditioned()
