"""GPU: the grouped cached-decode kernel of csrc/decode_cache_shared.hip (ops.decode_attn_cached_shared / _dyn) on inputs with exactly known
answers (tests/_decode_cases.py under the shared-prefix table of tests/_shared_prefix_cases.py), and generate(share_prompt=True)'s pieces on
2-layer full-width hosts.

H = 2, (N, group) in {(2, 2), (3, 3), (6, 3), (8, 4)}: at most 4 (sentence, head) pairs, so ranges are 128 keys and every position >= 128 has
several.  Positions: _decode_cases.FULL up to 300 at every shape, 1 350 and 4 100 at (6, 3).  shared_len: 1, 31 / 32 / 33 (a 32-key iteration
and a group's pair of keys straddle it), kps - 1 / kps / kps + 1 (a range edge), pos - 1, pos, clipped to [1, pos]."""
import copy
import gc

import pytest
import torch

from tests import _decode_cases as C
from tests import _shared_prefix_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x5A5A                                    # bf16 bit pattern of an untouched output
IDS = ["N%dg%d" % s for s in S.SHAPES]


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(scope="module")
def pools():
    """(random K / V pool, ownership V) per N, on the device; never left modified."""
    made = {}

    def get(N):
        if N not in made:
            p = C.random_pool(N, S.H, 128, C.CAPACITY, 77 + N + S.H)
            p.k, p.v = p.k.to(DEV), p.v.to(DEV)
            made[N] = (p, C.ownership_values(N, S.H, 128, C.CAPACITY).to(DEV))
        return made[N]

    yield get
    made.clear()
    gc.collect()
    torch.cuda.empty_cache()


def positions(shape):
    return S.POSITIONS + (S.WIDE_POSITIONS if shape == S.WIDE_SHAPE else [])


def launch(c, dyn, pos_dev=None, kc=None, vc=None, src="case", out=None):
    """One call of the grouped entry point on a case (its own caches, or the ones given)."""
    from otter_amd import ops

    kc, vc = (c.kc if kc is None else kc), (c.vc if vc is None else vc)
    src = c.src if isinstance(src, str) else src
    q, cos, sin, slopes = getattr(c, "q_in", c.q), getattr(c, "cos_table", None), getattr(c, "sin_table", None), getattr(c, "slopes", None)
    if dyn:
        pos_dev.fill_(c.pos)
        return ops.decode_attn_cached_shared_dyn(q, c.k_new, c.v_new, kc, vc, pos_dev, c.scale, c.group, c.shared_len, cos_table=cos, sin_table=sin,
                                                 src=src, key_valid=c.valid, slopes=slopes, out=out)
    rows = dict(cos=cos[c.pos], sin=sin[c.pos]) if cos is not None else {}
    return ops.decode_attn_cached_shared(q, c.k_new, c.v_new, kc, vc, c.pos, c.scale, c.group, c.shared_len, src=src, key_valid=c.valid,
                                         slopes=slopes, **rows)


def step(c, dyn, pos_dev=None):
    """case -> Result(o, k_slot, v_slot); the caches are restored, and every byte outside slot `pos` must be as before."""
    before = [c.kc.clone(), c.vc.clone()]
    o = launch(c, dyn, pos_dev)
    torch.cuda.synchronize()
    slots = [t[:, :, c.pos].clone() for t in (c.kc, c.vc)]
    for t, b in zip((c.kc, c.vc), before):
        t[:, :, c.pos] = b[:, :, c.pos]
        assert torch.equal(t, b), ("a cache byte outside the slot changed", c.N, c.group, c.pos, c.shared_len)
    return C.Result(o=o.view(c.N, c.H, 128), k_slot=slots[0], v_slot=slots[1])


def entries():
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    return [("scalar", lambda c: step(c, False)), ("dyn", lambda c: step(c, True, pos_dev))]


# ---- 1. count inputs --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_every_admitted_key_is_counted_exactly_once(pools, shape):
    """check_counts: o == 0 bit for bit where no admitted key is owned, |o - count / admitted| <= (2^-8 + 2^-16) count / admitted elsewhere, a
    fully masked row all zeros, the appended slot the new token, no other cache byte changed -- at every position and every shared_len of the
    module docstring, both entry points.  The masks a (none, src = NULL) / b / z take turns over the (position, shared_len) pairs, so that each
    meets every kind of shared_len."""
    N, group = shape
    pool, own = pools(N)
    worst, turn, seen = 0.0, 0, set()
    for pos in positions(shape):
        for sl in S.shared_lens(pos, S.kps_of(N, group, pos, cus())):
            variant = "abz"[turn % 3]
            turn += 1
            seen.add((variant, "1" if sl == 1 else "pos" if sl == pos else "mid"))
            c = C.to_device(S.count_case(N, group, pos, sl, variant, pool.k, own, cus()), DEV)
            for _, run in entries():
                worst = max(worst, C.check_counts(c, run(c)))
    assert len(seen) == 9, seen
    print("[shared-prefix] N%d group %d count: worst error / bound %.3f" % (N, group, worst), flush=True)


# ---- 2. needles -------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_the_needle_key_goes_with_its_value(pools, shape):
    """check_needle: |o - V[needle]| <= 2^-8 |V[needle]| + 2^-30, the needle in the shared prefix (the leader's row: key 0, keys 31 / 32 / 63,
    range edges below shared_len), in the own part behind a table entry that points at a sibling beam (pos - 1, range edges above
    shared_len), and as the new token; then with the needle masked, against the fp64 softmax without it."""
    N, group = shape
    pool, _ = pools(N)
    worst, shared, sibling, new = 0.0, 0, 0, 0
    for pos in [p for p in positions(shape) if p in (1, 33, 129, 257, 300, 1350)]:
        for sl in S.shared_lens(pos, S.kps_of(N, group, pos, cus())):
            for kinds in S.needle_kinds(N, group, pos, sl, cus()):
                for masked in (False, True):
                    c = S.needle_case(N, group, pos, sl, kinds, pool, cus(), masked=masked)
                    j = c.needle[0]
                    shared += int((j < sl).sum())
                    new += int((j == pos).sum())
                    if kinds[0] != "new":
                        rows = torch.gather(c.src.long(), 1, c.needle.clamp(max=pos - 1))
                        sibling += int(((c.needle >= sl) & (rows != torch.arange(N, device=DEV)[:, None])).sum())
                    for _, run in entries():
                        worst = max(worst, C.check_needle(c, run(c)))
    assert shared > 0 and sibling > 0 and new > 0, (shared, sibling, new)
    print("[shared-prefix] N%d group %d needle: worst error / bound %.3f (%d shared, %d behind a sibling, %d new)" % (
        N, group, worst, shared, sibling, new), flush=True)


# ---- 3. the fp64 oracle, and the appended slot against the existing kernel ------------------------------------------------------------------


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_exact_query_against_the_fp64_oracle(pools, shape):
    """check_oracle: per (row, head) max_d |o - ref| <= (2^-8 + 2^-12) max_d |ref|, ref the fp64 softmax of the exactly known query over the
    keys gathered through the shared-prefix table, with ALiBi slopes and with a rotary embedding (quadrant tables: the rotated query is exact),
    masks b and c.  The appended k and v slots are torch.equal to those otter_decode_attn_cached writes for the same new token."""
    from otter_amd import ops

    N, group = shape
    pool, _ = pools(N)
    worst = {}
    for pos in positions(shape):
        kps = S.kps_of(N, group, pos, cus())
        for i, sl in enumerate(S.shared_lens(pos, kps)):
            rotary = bool(i % 2)
            for variant in [v for v in C.variants(N, pos, kps) if v in "bc"]:
                c = C.to_device(S.oracle_case(N, group, pos, sl, variant, pool, cus(), rotary, not rotary), DEV)
                for name, run in entries():
                    r = run(c)
                    key = "rotary" if rotary else "alibi"
                    worst[key] = max(worst.get(key, 0.0), S.check_oracle(c, r))
                # the slot the existing kernel appends for this token
                kc, vc = c.kc.clone(), c.vc.clone()
                rows = dict(cos=c.cos_table[pos], sin=c.sin_table[pos]) if rotary else {}
                ops.decode_attn_cached(c.q_in, c.k_new, c.v_new, kc, vc, pos, c.scale, src=c.src, key_valid=c.valid, slopes=c.slopes, **rows)
                torch.cuda.synchronize()
                assert torch.equal(r.k_slot, kc[:, :, pos]) and torch.equal(r.v_slot, vc[:, :, pos]), (N, group, pos, sl)
    assert set(worst) == {"rotary", "alibi"}
    print("[shared-prefix] N%d group %d oracle: worst error / bound %s" % (N, group, {k: round(v, 3) for k, v in worst.items()}), flush=True)


def test_ordinary_rotary_tables_store_the_existing_kernels_key(pools):
    """Ordinary cos / sin tables ([N, 128] rows at the scalar entry, the whole table at the dyn one): the stored key is bit-equal to the one
    otter_decode_attn_cached stores, and o agrees with that kernel's to two bf16 roundings of the larger."""
    from otter_amd import ops

    N, group = 6, 3
    pool, _ = pools(N)
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    cos_t, sin_t = (t.to(DEV) for t in C.rotary_tables(128, C.CAPACITY))
    for pos, sl in ((40, 33), (300, 129)):
        c = C.to_device(S.oracle_case(N, group, pos, sl, "b", pool, cus(), False, True), DEV)
        kc, vc = c.kc.clone(), c.vc.clone()
        want = ops.decode_attn_cached(c.q_in, c.k_new, c.v_new, kc, vc, pos, c.scale, cos=cos_t[pos], sin=sin_t[pos], src=c.src, key_valid=c.valid,
                                      slopes=c.slopes)
        c.cos_table, c.sin_table = cos_t, sin_t
        for dyn in (False, True):
            r = step(c, dyn, pos_dev)
            assert torch.equal(r.k_slot, kc[:, :, pos]) and torch.equal(r.v_slot, vc[:, :, pos])
            err = (r.o.reshape(N, -1).float() - want.float()).abs()
            assert bool((err <= 2.0 ** -7 * want.float().abs().amax(-1, keepdim=True)).all()), float(err.max())


# ---- 4. leader-only reads -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", S.SHAPES, ids=IDS)
def test_shared_keys_are_read_from_the_leaders_row_only(pools, shape):
    """The non-leader rows' slots [0, shared_len) hold NaN and the table's first shared_len columns point at the row itself: o is finite and
    bit-equal to the run over clean caches.  (The existing kernel cannot pass this: it reads those columns.)"""
    N, group = shape
    pool, _ = pools(N)
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    for pos in [p for p in positions(shape) if p in (1, 33, 129, 257, 300, 4100)]:
        kps = S.kps_of(N, group, pos, cus())
        for sl in S.shared_lens(pos, kps):
            c = C.to_device(S.oracle_case(N, group, pos, sl, "b", pool, cus(), False, True), DEV)
            kc, vc, src = S.poisoned(c)
            for dyn in (False, True):
                clean = launch(c, dyn, pos_dev, kc=c.kc.clone(), vc=c.vc.clone())
                got = launch(c, dyn, pos_dev, kc=kc, vc=vc, src=src)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(got.float()).all()), (N, group, pos, sl, dyn)
                assert torch.equal(got, clean), (N, group, pos, sl, dyn)


# ---- 5. guard frames ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dyn", [False, True], ids=["scalar", "dyn"])
def test_nothing_outside_the_slot_and_the_workspace_is_written(pools, dyn):
    """Through the C entry points with a workspace of exactly the bytes asked for inside a sentinel frame: the frame, every cache slot other
    than [n, :, pos, :] and the table are untouched; o is fully written."""
    from otter_amd import _capi, ops

    N, group = 6, 3
    pool, _ = pools(N)
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    name = "decode_attn_cached_shared" + ("_dyn" if dyn else "")
    for pos, sl in ((129, 128), (300, 33), (4100, 1350)):
        c = C.to_device(S.oracle_case(N, group, pos, sl, "b", pool, cus(), False, True), DEV)
        kc, vc, src0 = c.kc.clone(), c.vc.clone(), c.src.clone()
        pos_dev.fill_(pos)
        keys = C.CAPACITY if dyn else pos + 1
        need = ops.decode_attn_cached_shared_workspace_bytes(N, S.H, keys)
        frame = 4096
        buf = torch.full((need + 2 * frame,), 0xA5, dtype=torch.uint8, device=DEV)
        out = torch.full((N, S.H * 128), SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        args, _ = ops._decode_cached_args(name, dyn, c.q_in, c.k_new, c.v_new, kc, vc, None, pos_dev if dyn else pos, c.scale, None, None, c.src,
                                          c.valid, c.slopes, out)
        args = list(args)
        assert args[-8] == ops._ws.get(0, out.device).data_ptr()
        args[-8], args[-7] = buf.data_ptr() + frame, need
        fn = getattr(_capi.lib(), "otter_" + name)
        _capi.check(fn(*args, group, sl, _capi.stream()), name)
        torch.cuda.synchronize()
        assert bool((buf[:frame] == 0xA5).all()) and bool((buf[frame + need:] == 0xA5).all()), (pos, sl)
        assert not bool((out.view(torch.int16) == SENT).all(dim=1).any())
        assert torch.equal(c.src, src0)
        for t, b in ((kc, c.kc), (vc, c.vc)):
            t[:, :, pos] = b[:, :, pos]
            assert torch.equal(t, b), ("a cache byte outside the slot changed", pos, sl)
        args[-7] = need - 1                                            # one byte less is refused before anything is launched
        assert fn(*args, group, sl, _capi.stream()) == -1


# ---- 6. scalar against dyn ------------------------------------------------------------------------------------------------------------------


def test_dyn_entry_is_bit_identical_to_the_scalar_entry_at_every_position(pools):
    """One capacity-sized launch configuration (the same tensors, the same arguments, only the value in pos_dev moves), the positions of
    DYN_ORDER -- range counts go down as well as up: o and the appended slots are the scalar entry's bits, and a second call gives the same
    bits again."""
    N, group = S.WIDE_SHAPE
    pool, _ = pools(N)
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.empty((N, S.H * 128), dtype=torch.bfloat16, device=DEV)
    cos_t, sin_t = (t.to(DEV) for t in C.rotary_tables(128, C.CAPACITY))
    sl = 33
    kd, vd = pool.k.clone(), pool.v.clone()
    base = C.to_device(S.oracle_case(N, group, 4100, sl, "b", pool, cus(), False, True), DEV)
    base.src[:, sl:] = torch.randint(0, N, (N, C.CAPACITY - 1 - sl), generator=torch.Generator().manual_seed(3)).int().to(DEV)   # any ancestry
    base.cos_table, base.sin_table = cos_t, sin_t
    for pos in [p for p in C.DYN_ORDER if p >= sl]:
        c = copy.copy(base)
        c.pos = pos
        ks, vs = pool.k.clone(), pool.v.clone()
        want = launch(c, False, kc=ks, vc=vs)
        again = launch(c, False, kc=pool.k.clone(), vc=pool.v.clone())
        kd[:, :, :] = pool.k
        vd[:, :, :] = pool.v
        got = launch(c, True, pos_dev, kc=kd, vc=vd, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert torch.equal(want, again), pos
        assert torch.equal(got, want), (pos, float((got.float() - want.float()).abs().max()))
        assert torch.equal(kd, ks) and torch.equal(vd, vs), pos
        got2 = launch(c, True, pos_dev, kc=kd, vc=vd).clone()
        assert torch.equal(got2, want), pos


@pytest.mark.parametrize("bad", [0, -3, C.CAPACITY, 1 << 30, 32])
def test_dyn_entry_ignores_a_position_it_cannot_serve(pools, bad):
    """pos_dev outside [1, S_max), or below shared_len = 33 (the in-place invariant needs shared_len <= pos): the call writes nothing."""
    from otter_amd import ops

    N, group = 6, 3
    pool, _ = pools(N)
    c = C.to_device(S.oracle_case(N, group, 300, 33, "b", pool, cus(), False, True), DEV)
    kc, vc = c.kc.clone(), c.vc.clone()
    out = torch.full((N, S.H * 128), SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    pos_dev = torch.full((1,), bad, dtype=torch.int32, device=DEV)
    ops.decode_attn_cached_shared_dyn(c.q_in, c.k_new, c.v_new, kc, vc, pos_dev, c.scale, group, 33, src=c.src, key_valid=c.valid, slopes=c.slopes,
                                      out=out)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == SENT).all()) and torch.equal(kc, c.kc) and torch.equal(vc, c.vc)


def test_other_group_sizes(pools):
    """Groups of 5 and 6 rows (the remaining instances): the count inputs at a straddling shared_len, both entry points."""
    for N, group in ((5, 5), (6, 6)):
        pool = C.random_pool(N, S.H, 128, C.CAPACITY, 5)
        own = C.ownership_values(N, S.H, 128, C.CAPACITY).to(DEV)
        for pos, sl, variant in ((300, 33, "b"), (129, 128, "a"), (257, 1, "z")):
            c = C.to_device(S.count_case(N, group, pos, sl, variant, pool.k.to(DEV), own, cus()), DEV)
            for _, run in entries():
                C.check_counts(c, run(c))


# ---- 7. hosts -----------------------------------------------------------------------------------------------------------------------------

P_LEN, NEW, B, NB = 40, 12, 2, 3
ROWS = B * NB
PAD = 9                                           # row 1 is left-padded


class _Count:
    def __init__(self, monkeypatch, mod, name):
        self.n, orig = 0, getattr(mod, name)

        def f(*a, **k):
            self.n += 1
            return orig(*a, **k)

        monkeypatch.setattr(mod, name, f)


def _schedule():
    """Per-beam continuations and within-sentence reorders, the same for every run."""
    g = torch.Generator().manual_seed(5)
    cont = torch.randint(1, 1000, (ROWS, NEW), generator=g).to(DEV)
    reorders = [torch.cat([torch.randint(0, NB, (NB,), generator=g) + b * NB for b in range(B)]).to(DEV) for _ in range(NEW)]
    return cont, reorders


def _prompt_pass(model, bench, bf16, share, kv_dtype=None):
    """(cache, media cache, the repeated mask [ROWS, P_LEN + NEW], last-position logits [ROWS, V]) after the prompt pass: one row per sentence
    into a shared cache, or the repeated prompt into an unshared one."""
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache

    vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN, DEV, seed=99, frames=1)
    mask[1, :PAD] = 0
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    cache = StaticKVCache(n_layers, ROWS, n_kv, hd, P_LEN + NEW, DEV, torch.bfloat16 if bf16 else torch.float32, kv_dtype=kv_dtype)
    v = vx.to(torch.bfloat16) if bf16 else vx
    rep = (lambda t: t) if share else (lambda t: t.repeat_interleave(NB, dim=0))
    mc = MediaCache(B if share else ROWS, model.media_token_id, rows_per_media=1 if share else NB)
    if share:
        cache.share_prompt(NB)
    out = model(vision_x=rep(v), lang_x=rep(ids), attention_mask=rep(mask), past_key_values=cache, use_cache=True, clear_conditioned_layers=False,
                media_cache=mc)
    logits = out.logits[:, -1].float()
    if share:
        mc.expand(NB)
        logits = logits.repeat_interleave(NB, dim=0)
    full = torch.cat([mask.repeat_interleave(NB, dim=0), torch.ones(ROWS, NEW, dtype=mask.dtype, device=DEV)], 1)
    return cache, mc, full, logits


def _ctx(bf16):
    return torch.autocast("cuda", dtype=torch.bfloat16) if bf16 else torch.autocast("cuda", enabled=False)


def _run(model, bench, bf16, share, kv_dtype=None):
    """The prompt pass and NEW - 1 cached steps with per-beam tokens and a within-sentence reorder before each: logits [ROWS, NEW, V] fp32."""
    cont, reorders = _schedule()
    with torch.no_grad(), _ctx(bf16):
        cache, mc, full, logits = _prompt_pass(model, bench, bf16, share, kv_dtype)
        steps = [logits]
        for t in range(NEW - 1):
            cache.reorder(reorders[t])
            mc.reorder(reorders[t])
            out = model(vision_x=None, lang_x=cont[:, t:t + 1], attention_mask=full[:, :P_LEN + t + 1], use_cached_vision_x=True,
                        past_key_values=cache, use_cache=True, clear_conditioned_layers=False, media_cache=mc)
            steps.append(out.logits[:, -1].float())
        model.lang_encoder.clear_conditioned_layers()
    assert cache.length == P_LEN + NEW - 1 and (not share or (cache.group, cache.shared_len) == (NB, P_LEN))
    return torch.stack(steps, dim=1)


def _drift(got, ref):
    """tests/test_gpu_w8._drift: max over rows and steps of max_v |got - ref| / max_v |ref|."""
    return float(((got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)).max())


@pytest.fixture(scope="module")
def hosts():
    """The 2-layer full-width hosts of tests/test_gpu_media_cache.py, built once per kind and never modified (a test that quantises works on
    a copy)."""
    from tests.test_gpu_media_cache import _build

    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = _build(kind)
        return made[kind]

    yield get
    made.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _quantised_pair(model):
    """(a copy with the int8 decoder, a copy with the dequantised weights: its fp32 reference)."""
    from otter_amd.quant import Int8FrozenLinear, dequantize_weight_int8

    qmodel, ref = copy.deepcopy(model), copy.deepcopy(model)
    assert qmodel.quantize_decoder_int8()["replaced"] > 0
    fq = dict(ref.named_modules())
    with torch.no_grad():
        for name, m in qmodel.named_modules():
            if isinstance(m, Int8FrozenLinear):
                fq[name].weight.copy_(dequantize_weight_int8(m.qweight, m.scale, torch.float32))
    return qmodel, ref


@pytest.mark.parametrize("decoder", ["bf16", "w8"])
@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_share_prompt_steps_stay_within_twice_the_unshared_bf16_drift(hosts, kind, decoder, monkeypatch):
    """2-layer full-width host, B = 2 x 3 beams, a 40-token prompt (row 1 left-padded by 9), 11 cached steps with per-beam tokens and
    reorders.  Every step's logits on the share_prompt path against an fp32-compute run of the same model: the drift is at most twice the
    unshared bf16 static path's own drift from that run.  The steps run on the grouped kernel; with OTTER_SHARED_PREFIX=0 they run on the
    existing kernel through the table, hold the same bound, and pick the same token wherever the top-2 margin exceeds twice the difference
    of the two paths' logits; with kv_cache_dtype="int8" they run on the existing int8 kernel.  (OTTER_SHARED_PREFIX=1: 2 sentences x 40
    shared keys are below the count from which `attend` takes the grouped kernel by itself, which the last lines check.)"""
    from otter_amd import ops

    model, bench = hosts(kind)
    run_model, model = _quantised_pair(model) if decoder == "w8" else (model, model)
    grouped, plain_k, i8_k = (_Count(monkeypatch, ops, n) for n in ("decode_attn_cached_shared", "decode_attn_cached", "decode_attn_cached_i8"))
    layers = 2
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "1")
    ref = _run(model, bench, False, False)
    assert (grouped.n, plain_k.n, i8_k.n) == (0, 0, 0)                                   # fp32 compute: the restatement
    d_plain = _drift(_run(run_model, bench, True, False), ref)
    assert (grouped.n, plain_k.n) == (0, layers * (NEW - 1))
    shared = _run(run_model, bench, True, True)
    assert (grouped.n, plain_k.n) == (layers * (NEW - 1), layers * (NEW - 1))             # every step of every layer on the grouped kernel
    d_shared = _drift(shared, ref)
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "0")
    table = _run(run_model, bench, True, True)
    assert (grouped.n, plain_k.n) == (layers * (NEW - 1), 2 * layers * (NEW - 1))         # the existing kernel, through the table
    monkeypatch.delenv("OTTER_SHARED_PREFIX")
    auto = _run(run_model, bench, True, True)                                            # left to itself at this size: the table path again
    assert (grouped.n, plain_k.n) == (layers * (NEW - 1), 3 * layers * (NEW - 1)) and torch.equal(auto, table)
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "1")
    d_table = _drift(table, ref)
    top2 = shared.topk(2, dim=-1).values
    decided = (top2[..., 0] - top2[..., 1]) > 2 * (shared - table).abs().amax(-1)
    assert bool((shared.argmax(-1) == table.argmax(-1))[decided].all()) and float(decided.float().mean()) > 0.5
    d_i8_plain = _drift(_run(run_model, bench, True, False, "int8"), ref)
    n_i8 = i8_k.n
    d_i8 = _drift(_run(run_model, bench, True, True, "int8"), ref)
    assert i8_k.n - n_i8 == n_i8 == layers * (NEW - 1) and grouped.n == layers * (NEW - 1)
    print("[shared-prefix] %s %s: drift vs fp32: unshared bf16 %.3e, share_prompt %.3e (ratio %.2f), table path %.3e (ratio %.2f); int8 KV unshared "
          "%.3e, shared %.3e (ratio %.2f)" % (kind, decoder, d_plain, d_shared, d_shared / d_plain, d_table, d_table / d_plain, d_i8_plain, d_i8,
                                              d_i8 / d_i8_plain), flush=True)
    assert d_plain > 0 and d_shared <= 2 * d_plain, (d_shared, d_plain)
    assert d_table <= 2 * d_plain, (d_table, d_plain)
    assert d_i8 <= 2 * d_i8_plain, (d_i8, d_i8_plain)


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_replayed_shared_steps_equal_the_eager_ones(hosts, kind, monkeypatch):
    """The steps after a shared prompt pass under a captured graph (2 eager warm-up steps, 1 capture, 9 replays in 11 cached steps) against
    the same replay-mode steps issued eagerly over a second pair of caches: every step's logits torch.equal, in bf16 and with the int8
    decoder.  The captured step runs the grouped dyn kernel."""
    from otter_amd import ops
    from otter_amd.graph_decode import GraphDecodeStep

    model, bench = hosts(kind)
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "1")                     # (the grouped kernel at 2 sentences x 40 shared keys)
    grouped, plain_k = _Count(monkeypatch, ops, "decode_attn_cached_shared_dyn"), _Count(monkeypatch, ops, "decode_attn_cached_dyn")
    cont, reorders = _schedule()
    for tag in ("bf16", "w8"):
        if tag == "w8":
            model = copy.deepcopy(model)
            assert model.quantize_decoder_int8()["replaced"] > 0
        with torch.no_grad(), _ctx(True):
            cache, mc, full, logits = _prompt_pass(model, bench, True, True)
            c2, m2 = copy.copy(cache), copy.copy(mc)
            c2.k, c2.v, c2.src = cache.k.clone(), cache.v.clone(), cache.src.clone()
            m2.seen, m2.kv = mc.seen.clone(), list(mc.kv)
            table = cache.src
            cache.enable_replay(full[:, :P_LEN], beams=True)
            c2.enable_replay(full[:, :P_LEN], beams=True)
            assert cache.src is table                                  # found, not created: its address was fixed by the prompt pass
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
                assert torch.equal(cache.k, c2.k) and torch.equal(cache.v, c2.v) and torch.equal(cache.src, c2.src)
                assert (graph.captures, graph.replays) == (1, NEW - 1 - 2) and graph.replays == 9
            finally:
                graph.release()
                eager.release()
                model.lang_encoder.clear_conditioned_layers()
    assert grouped.n > 0 and plain_k.n == 0


def test_generate_share_prompt_with_graph_decode(hosts, monkeypatch):
    """generate(num_beams=3, share_prompt=True, graph_decode=True) on the 2-layer MPT host: the prompt pass has B rows, one capture and 9
    replays serve the 11 cached steps, and the tokens are those of the same call without the graph."""
    from otter_amd.graph_decode import GraphDecodeStep

    from otter_amd import ops

    model, bench = hosts("mpt")
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "1")                     # (the grouped kernel at 2 sentences x 40 shared keys)
    grouped = _Count(monkeypatch, ops, "decode_attn_cached_shared_dyn")
    vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN, DEV, seed=99, frames=1)
    mask[1, :PAD] = 0
    counts, rows, release = [], [], GraphDecodeStep.release

    def spy_release(self):
        counts.append((self.steps, self.captures, self.replays, self.use_graph))
        return release(self)

    monkeypatch.setattr(GraphDecodeStep, "release", spy_release)
    h = model.lang_encoder.register_forward_hook(lambda _m, _a, k, _o: rows.append(tuple(k["input_ids"].shape)), with_kwargs=True)
    kw = dict(max_new_tokens=NEW, eos_token_id=-1, num_beams=NB, cache_implementation="static", cross_attention_cache=True, share_prompt=True)
    try:
        with torch.no_grad(), _ctx(True):
            got = model.generate(vision_x=vx.to(torch.bfloat16), lang_x=ids, attention_mask=mask, graph_decode=True, **kw)
            n_graph = len(rows)
            assert 2 * 3 <= grouped.n < 2 * (NEW - 1)              # two layers x (2 warm-up steps + the captured one): the rest are replays
            want = model.generate(vision_x=vx.to(torch.bfloat16), lang_x=ids, attention_mask=mask, **kw)
    finally:
        h.remove()
    assert counts == [(NEW - 1, 1, NEW - 3, True)], counts
    assert rows[0] == (B, P_LEN) and rows[n_graph] == (B, P_LEN) and set(rows[n_graph + 1:]) == {(ROWS, 1)}
    assert got.shape == (B, P_LEN + NEW) and torch.equal(got, want), (got[:, P_LEN:].tolist(), want[:, P_LEN:].tolist())
    assert not model.lang_encoder.is_conditioned()
