"""CPU, fp32, tiny models: the int8 form of the static KV cache (otter_amd/kv_cache.py, `kv_dtype="int8"`) -- the quantiser's rule, `fill`
against the quantiser applied to an unquantised cache, `attend_reference`'s int8 branch against plain attention over the dequantised
tensors, the append, replay mode against scalar mode, generate(kv_cache_dtype="int8") on both hosts, the error paths, and that nothing
changes without the keyword.  The cached step runs the documented plain-torch branch here; the kernel (csrc/decode_cache_i8.hip) is
tests/test_gpu_kv_cache_int8.py's.  Models and batches are those of tests/test_static_kv_cache.py."""
import itertools

import pytest
import torch

import tests.test_static_kv_cache as ts
from otter_amd import kv_cache
from otter_amd.kv_cache import StaticKVCache, cache_geometry, dequantize_kv_int8, quantize_kv_int8, rotate_half
from tests._cpu_backend import oracle_backend

P_LEN, STEPS = ts.P_LEN, ts.STEPS


# ---- the quantiser ---------------------------------------------------------------------------------------------------------------------

def test_zero_vector_has_scale_one_and_zero_codes():
    x = torch.randn(3, 16)
    x[1] = 0
    q, s = quantize_kv_int8(x)
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and q.shape == x.shape and s.shape == (3,)
    assert float(s[1]) == 1.0 and not bool(q[1].any())
    assert torch.equal(dequantize_kv_int8(q, s)[1], torch.zeros(16))


def test_amax_on_a_negative_element_gives_minus_127_and_minus_128_never_occurs():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 128, generator=g)
    x[:, 5] = -x.abs().amax(dim=-1) * 1.5
    q, s = quantize_kv_int8(x)
    assert bool((q[:, 5] == -127).all()) and int(q.min()) == -127
    assert torch.equal(s, x[:, 5].abs() / torch.full((64,), 127.0))
    for dtype in (torch.bfloat16, torch.float16):                     # the compute dtypes a cache may be created with
        q, _ = quantize_kv_int8((torch.randn(256, 128, generator=g) * 100).to(dtype))
        assert int(q.min()) >= -127 and int(q.max()) <= 127


def test_exact_ties_round_to_even():
    """Values (j + 0.5) * 2^-7 with amax 127 * 2^-7: the scale is exactly 2^-7, every quotient an exact tie."""
    j = torch.arange(-126, 126, dtype=torch.float32)
    x = torch.cat([(j + 0.5) * 2.0 ** -7, torch.tensor([127 * 2.0 ** -7])])
    q, s = quantize_kv_int8(x[None].bfloat16())                       # (all exactly representable in bf16)
    assert float(s) == 2.0 ** -7
    want = torch.where(j.long() % 2 == 0, j.long(), j.long() + 1)     # j + 0.5 -> the even neighbour
    assert torch.equal(q[0, :-1].long(), want) and int(q[0, -1]) == 127


def test_the_rule_is_quantize_weight_int8_over_the_last_dim():
    from otter_amd.quant import dequantize_weight_int8, quantize_weight_int8

    x = torch.randn(5, 7, 32, generator=torch.Generator().manual_seed(1)).bfloat16()
    q, s = quantize_kv_int8(x)
    qw, sw = quantize_weight_int8(x.reshape(35, 32))
    assert torch.equal(q.reshape(35, 32), qw) and torch.equal(s.reshape(35), sw)
    assert torch.equal(dequantize_kv_int8(q, s).reshape(35, 32), dequantize_weight_int8(qw, sw))


def test_unknown_kv_dtype_is_rejected_by_the_constructor():
    with pytest.raises(ValueError, match="kv_dtype"):
        StaticKVCache(1, 1, 1, 8, 4, "cpu", torch.float32, kv_dtype="fp8")
    c = StaticKVCache(1, 2, 2, 8, 4, "cpu", torch.float32)
    assert c.k.dtype == torch.float32 and c.kv_dtype is None and not c.int8 and c.k_scale is None and len(c.data_ptrs()) == 2
    assert c.nbytes() == 2 * 2 * 2 * 4 * 8 * 4


# ---- fill: the prompt pass ---------------------------------------------------------------------------------------------------------------

def _caches(model, rows, max_len):
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    return (StaticKVCache(n_layers, rows, n_kv, hd, max_len, "cpu", torch.float32),
            StaticKVCache(n_layers, rows, n_kv, hd, max_len, "cpu", torch.float32, kv_dtype="int8"))


@pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
def test_prompt_pass_fills_the_quantised_contents_of_the_unquantised_cache(llama):
    """The prompt pass never reads the cache, so this is exact.  nbytes: 132 / 256 of the 16-bit cache at head_dim 128; stated for any
    head_dim and compute dtype as (d + 4) bytes against d * itemsize."""
    model = ts._model(llama)
    vx, ids, mask = ts._batch(3, (0, 2, 3))
    plain, quant = _caches(model, 3, P_LEN + STEPS)
    with torch.no_grad(), oracle_backend():
        for c in (plain, quant):
            model(vision_x=vx, lang_x=ids[:, :P_LEN], attention_mask=mask[:, :P_LEN], past_key_values=c, use_cache=True)
            assert c.length == P_LEN
    assert quant.k.dtype == quant.v.dtype == torch.int8 and quant.k_scale.dtype == quant.v_scale.dtype == torch.float32
    assert quant.dtype == torch.float32 and quant.k.shape == plain.k.shape and quant.k_scale.shape == plain.k.shape[:-1]
    for i in range(plain.n_layers):
        for codes, scales, t in ((quant.k, quant.k_scale, plain.k), (quant.v, quant.v_scale, plain.v)):
            q, s = quantize_kv_int8(t[i, :, :, :P_LEN])
            assert torch.equal(codes[i, :, :, :P_LEN], q) and torch.equal(scales[i, :, :, :P_LEN], s), i
            assert not bool(codes[i, :, :, P_LEN:].any())
    d = plain.head_dim
    assert quant.nbytes() * d * 4 == plain.nbytes() * (d + 4)
    full = StaticKVCache(2, 3, 4, 128, 40, "cpu", torch.bfloat16), StaticKVCache(2, 3, 4, 128, 40, "cpu", torch.bfloat16, kv_dtype="int8")
    assert full[1].nbytes() <= 0.52 * full[0].nbytes() and full[1].nbytes() * 256 == full[0].nbytes() * 132


# ---- attend_reference ------------------------------------------------------------------------------------------------------------------

def _filled(N, H, d, S0, max_len, g, dtype=torch.float32):
    c = StaticKVCache(1, N, H, d, max_len, "cpu", dtype, kv_dtype="int8")
    k, v = torch.randn(N, H, S0, d, generator=g), torch.randn(N, H, S0, d, generator=g)
    k[0, 0, 1] = 0                                                    # a zero vector among the cached keys
    c.fill(0, k, v)
    c.length = S0
    return c


def _manual_dequantised(c, layer, upto):
    """[N,H,upto,d] fp32 keys and values, gathered through the table by explicit loops."""
    N = c.rows
    K = torch.zeros(N, c.n_heads, upto, c.head_dim)
    V = torch.zeros_like(K)
    for n in range(N):
        for j in range(upto):
            r = int(c.src[n, j]) if c.src is not None else n
            K[n, :, j] = c.k[layer, r, :, j].float() * c.k_scale[layer, r, :, j, None]
            V[n, :, j] = c.v[layer, r, :, j].float() * c.v_scale[layer, r, :, j, None]
    return K, V


@pytest.mark.parametrize("gqa", [False, True], ids=["mha", "gqa"])
def test_attend_reference_is_plain_attention_over_the_dequantised_cache(gqa):
    """Every combination of {table, mask with a fully masked row, slopes, rotary}: the output against an fp64 softmax attention over the
    dequantised gathered tensors (slot pos included) to fp32 rounding -- 1e-5 max|ref| is some hundred fp32 ulps for sums of <= 16 x 8
    terms, and three orders below the quantisation step -- the slot written, and every other byte of the four tensors unchanged."""
    N, H, Hkv, d, S0 = 4, 4, (2 if gqa else 4), 8, 5
    for seed, (tabled, masked, alibi, rotary) in enumerate(itertools.product([False, True], repeat=4)):
        g = torch.Generator().manual_seed(100 + seed)
        c = _filled(N, Hkv, d, S0, 16, g)
        if tabled:
            c.reorder(torch.tensor([1, 1, 3, 0]))
        q, k, v = torch.randn(N, H, d, generator=g), torch.randn(N, Hkv, d, generator=g), torch.randn(N, Hkv, d, generator=g)
        v[1, 0] = 0                                                   # a zero vector as the new token
        cos, sin = (torch.rand(d, generator=g), torch.rand(d, generator=g)) if rotary else (None, None)
        slopes = torch.tensor([0.5, 0.25, 0.125, 0.0625]) if alibi else None
        valid = None
        if masked:
            valid = torch.ones(N, S0 + 1, dtype=torch.uint8)
            valid[0, :2] = 0
            valid[2] = 0
        before = [t.clone() for t in (c.k, c.v, c.k_scale, c.v_scale)]
        o = c.attend_reference(0, q, k, v, 0.35, cos=cos, sin=sin, key_valid=valid, slopes=slopes).view(N, H, d)
        # the append: slot S0 holds the quantised new token (k after rotary, in fp32 = the compute dtype), nothing else moved
        kr = k * cos + rotate_half(k) * sin if rotary else k
        for t, s_, x, b in ((c.k, c.k_scale, kr, before[:3:2]), (c.v, c.v_scale, v, before[1::2])):
            qx, sx = quantize_kv_int8(x)
            assert torch.equal(t[0, :, :, S0], qx) and torch.equal(s_[0, :, :, S0], sx)
            b[0][0, :, :, S0], b[1][0, :, :, S0] = qx, sx
            assert torch.equal(t, b[0]) and torch.equal(s_, b[1])
        K, V = _manual_dequantised(c, 0, S0 + 1)
        K, V = K.double().repeat_interleave(H // Hkv, dim=1), V.double().repeat_interleave(H // Hkv, dim=1)
        qr = (q * cos + rotate_half(q) * sin if rotary else q).double()
        sc = torch.einsum("nhd,nhjd->nhj", qr, K) * 0.35
        if alibi:
            sc = sc + slopes.double().view(1, H, 1) * torch.arange(-S0, 1, dtype=torch.float64)
        rows = [0, 1, 3] if masked else [0, 1, 2, 3]
        if masked:
            sc = sc.masked_fill(valid[:, None, :] == 0, float("-inf"))
            assert float(o[2].abs().max()) == 0.0
        want = torch.einsum("nhj,nhjd->nhd", torch.softmax(sc[rows], -1), V[rows])
        err = float((o[rows].double() - want).abs().max())
        assert err <= 1e-5 * float(want.abs().max()), (tabled, masked, alibi, rotary, err)


def test_keys_are_rounded_to_the_compute_dtype_before_they_are_quantised():
    g = torch.Generator().manual_seed(3)
    c = _filled(2, 2, 8, 3, 8, g, dtype=torch.bfloat16)
    q, k, v = (torch.randn(2, 2, 8, generator=g).bfloat16() for _ in range(3))
    cos, sin = torch.rand(8, generator=g), torch.rand(8, generator=g)
    c.attend_reference(0, q, k, v, 0.3, cos=cos, sin=sin)
    kr = (k.float() * cos + rotate_half(k.float()) * sin).bfloat16()
    qk, sk = quantize_kv_int8(kr)
    assert torch.equal(c.k[0, :, :, 3], qk) and torch.equal(c.k_scale[0, :, :, 3], sk)
    leg = c.to_legacy("llama")[0]
    assert leg[0].dtype == torch.bfloat16 and leg[0].shape == (2, 2, 3, 8)


# ---- replay mode == scalar mode -----------------------------------------------------------------------------------------------------------

def test_replay_mode_equals_the_position_scalar_mode():
    """tests/test_graph_decode.py's scenario over int8 caches: six consecutive steps, rotary and ALiBi, a left-padded mask with a row
    without a valid prompt key, a table reordered before some steps.  Outputs and all four cache tensors are torch.equal."""
    import tests.test_graph_decode as tg

    ROWS, H, D, MAX_LEN, S0, LAYERS = tg.ROWS, tg.H, tg.D, tg.MAX_LEN, tg.S0, tg.LAYERS

    def prefilled(g):
        c = StaticKVCache(LAYERS, ROWS, H, D, MAX_LEN, "cpu", torch.float32, kv_dtype="int8")
        for i in range(LAYERS):
            c.fill(i, torch.randn(ROWS, H, S0, D, generator=g), torch.randn(ROWS, H, S0, D, generator=g))
        c.length = S0
        return c

    g = torch.Generator().manual_seed(0)
    a, b = prefilled(g), prefilled(torch.Generator().manual_seed(0))
    mask = torch.ones(ROWS, S0, dtype=torch.long)
    mask[1, :2] = 0
    mask[2, :] = 0
    cos_t, sin_t = tg._tables()
    slopes = torch.tensor([0.5, 0.125])
    same = lambda: all(torch.equal(x, y) for x, y in ((a.k, b.k), (a.v, b.v), (a.k_scale, b.k_scale), (a.v_scale, b.v_scale)))
    assert same()
    with torch.no_grad():
        b.enable_replay(mask, beams=True)
        ptrs = (b.pos_dev.data_ptr(), b.valid.data_ptr(), b.src.data_ptr()) + b.data_ptrs()
        assert len(b.data_ptrs()) == 4
        for step in range(6):
            pos = a.length
            if step in (1, 2, 4):
                beam_idx = torch.randint(0, ROWS, (ROWS,), generator=g)
                a.reorder(beam_idx)
                b.reorder(beam_idx)
            mask = torch.cat([mask, torch.ones(ROWS, 1, dtype=torch.long)], dim=1)
            b.check_step(ROWS, 1)
            for layer in range(LAYERS):
                q, k, v = (torch.randn(ROWS, H, D, generator=g) for _ in range(3))
                oa = a.attend_reference(layer, q, k, v, 0.3, cos=cos_t[pos], sin=sin_t[pos], key_valid=mask.to(torch.uint8), slopes=slopes)
                ob = b.attend(layer, q, k, v, 0.3, cos=cos_t, sin=sin_t, slopes=slopes)
                assert torch.equal(oa, ob), (step, layer)
            a.length = pos + 1
            b.advance()
            assert b.length == a.length == int(b.pos_dev) == S0 + step + 1 and same()
        assert not b.kernel_steps                                    # (the restatement ran: such a step is never captured)
        assert ptrs == (b.pos_dev.data_ptr(), b.valid.data_ptr(), b.src.data_ptr()) + b.data_ptrs()
        b.note_replay()
        assert b.length == S0 + 7


# ---- generate ---------------------------------------------------------------------------------------------------------------------------

GEN_CASES = {"greedy": dict(), "beams3": dict(num_beams=3), "sample": dict(do_sample=True, top_k=20, temperature=0.9)}
STATIC_I8 = dict(cache_implementation="static", kv_cache_dtype="int8")


class _Spy:
    """Records the StaticKVCache objects generate() creates."""

    def __init__(self, monkeypatch):
        self.made = made = []

        class Recorded(StaticKVCache):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                made.append(self)

        monkeypatch.setattr(kv_cache, "StaticKVCache", Recorded)


@pytest.mark.parametrize("case", list(GEN_CASES))
@pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
def test_generate_runs_over_an_int8_cache(llama, case, monkeypatch):
    """Left-padded batch of two.  The call is deterministic, composes with the media cache and the replay-mode step (token for token the
    plain int8 call's), and after beam search to_legacy() is a manual gather + dequantise of the cache."""
    model = ts._model(llama)
    vx, ids, mask = ts._batch(2, (0, 2), seed=21)
    lx, mask = ids[:, :P_LEN], mask[:, :P_LEN]
    spy = _Spy(monkeypatch)
    got, _ = ts._generate(model, vx, lx, mask, GEN_CASES[case], **STATIC_I8)
    again, _ = ts._generate(model, vx, lx, mask, GEN_CASES[case], **STATIC_I8)
    assert got.shape == (2, P_LEN + ts.NEW) and torch.equal(got[:, :P_LEN], lx) and torch.equal(got, again)
    assert len(spy.made) == 2 and all(c.int8 and c.k.dtype == torch.int8 and c.dtype == torch.float32 for c in spy.made)
    c = spy.made[0]
    assert c.length == P_LEN + ts.NEW - 1 and c.rows == 2 * GEN_CASES[case].get("num_beams", 1) and (c.src is not None) == (case == "beams3")
    K, V = _manual_dequantised(c, 1, c.length)
    leg = c.to_legacy("llama")
    assert torch.equal(leg[1][0], K) and torch.equal(leg[1][1], V)
    assert torch.equal(c.to_legacy("mpt")[1][0], K.transpose(2, 3))
    media, _ = ts._generate(model, vx, lx, mask, GEN_CASES[case], cross_attention_cache=True, **STATIC_I8)
    graph, _ = ts._generate(model, vx, lx, mask, GEN_CASES[case], cross_attention_cache=True, graph_decode=True, **STATIC_I8)
    assert torch.equal(graph, media) and spy.made[-1].replay and spy.made[-1].int8
    assert not model.lang_encoder.is_conditioned()


# ---- drift sanity ---------------------------------------------------------------------------------------------------------------------------

# the worst relative logit error max_v |int8 - plain| / max_v |plain| over the prompt's last position and the 8 teacher-forced steps of
# tests/test_static_kv_cache.py's batches (seed 5; unpadded and left-padded), measured on the CPU in fp32 when this test was written
MEASURED_DRIFT = {"mpt": 8.830e-04, "llama": 2.986e-03}


def _steps(model, vx, ids, mask, cache):
    am = (lambda t: None) if mask is None else (lambda t: mask[:, :t])
    out = model(vision_x=vx, lang_x=ids[:, :P_LEN], attention_mask=am(P_LEN), past_key_values=cache, use_cache=True, clear_conditioned_layers=False)
    logits = [out.logits[:, -1]]
    for t in range(P_LEN, P_LEN + STEPS):
        out = model(vision_x=None, lang_x=ids[:, t:t + 1], attention_mask=am(t + 1), use_cached_vision_x=True, past_key_values=cache, use_cache=True,
                    clear_conditioned_layers=False)
        logits.append(out.logits[:, -1])
    model.lang_encoder.clear_conditioned_layers()
    assert cache.length == P_LEN + STEPS
    return torch.stack(logits, dim=1)


@pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
def test_int8_cache_steps_stay_near_the_unquantised_static_steps(llama):
    """A guard against a wrong scale or sign, not a quality claim: at most twice the drift measured when the test was written."""
    model = ts._model(llama)
    worst = 0.0
    for pads in (None, (0, 2, 3)):
        vx, ids, mask = ts._batch(3, pads)
        plain, quant = _caches(model, 3, P_LEN + STEPS)
        with torch.no_grad(), oracle_backend():
            ref, got = _steps(model, vx, ids, mask, plain), _steps(model, vx, ids, mask, quant)
        assert torch.equal(got[:, 0], ref[:, 0])                      # the prompt pass does not read the cache
        worst = max(worst, float(((got - ref).abs().amax(-1) / ref.abs().amax(-1)).max()))
    name = "llama" if llama else "mpt"
    print("[kv-int8] %s: worst relative logit error of int8-cache steps against unquantised static steps %.3e" % (name, worst))
    assert 0 < worst <= 2 * MEASURED_DRIFT[name], (worst, MEASURED_DRIFT[name])


# ---- errors, and the default ------------------------------------------------------------------------------------------------------------------

def test_generate_rejects_a_bad_kv_cache_dtype():
    model = ts._model(False)
    vx, ids, _ = ts._batch(1, None)
    kw = dict(vision_x=vx, lang_x=ids[:, :P_LEN], max_new_tokens=2)
    with pytest.raises(ValueError, match="kv_cache_dtype must be None or 'int8'"):
        model.generate(cache_implementation="static", kv_cache_dtype="fp8", **kw)
    for extra in (dict(), dict(use_cache=True), dict(cache_implementation="dynamic")):
        with pytest.raises(ValueError, match="needs cache_implementation='static'"):
            model.generate(kv_cache_dtype="int8", **extra, **kw)
    assert not model.lang_encoder.is_conditioned()


def test_fuyu_and_persimmon_hosts_do_not_take_kv_cache_dtype():
    from oracle.gen_golden_fuyu import tiny_fuyu_config
    from otter_amd.fuyu import FuyuForCausalLM, PersimmonForCausalLM

    cfg = tiny_fuyu_config()
    ids = torch.randint(1, 100, (1, 5), generator=torch.Generator().manual_seed(0))
    for model in (FuyuForCausalLM(cfg).eval(), PersimmonForCausalLM(cfg.text_config).eval()):
        with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
            model.generate(input_ids=ids, max_new_tokens=2, kv_cache_dtype="int8")
    with pytest.raises(NotImplementedError, match="kv_cache_dtype"):
        FuyuForCausalLM(cfg).eval().generate(input_ids=ids, max_new_tokens=2, cache_implementation="static", kv_cache_dtype="int8")
    with pytest.raises(NotImplementedError, match="static"):         # (the existing raise is as it was)
        FuyuForCausalLM(cfg).eval().generate(input_ids=ids, max_new_tokens=2, cache_implementation="static")


@pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
def test_without_the_keyword_nothing_changes(llama, monkeypatch):
    """The same tokens as the legacy cache's (tests/test_static_kv_cache.py's criterion, on its seeds) with and without an explicit None,
    over a cache that stores the compute dtype and has no scales."""
    model = ts._model(llama)
    vx, ids, mask = ts._batch(2, (0, 2), seed=21)
    lx, mask = ids[:, :P_LEN], mask[:, :P_LEN]
    spy = _Spy(monkeypatch)
    for kw in (dict(), dict(num_beams=3, no_repeat_ngram_size=3)):
        want, _ = ts._generate(model, vx, lx, mask, kw, use_cache=True)
        absent, _ = ts._generate(model, vx, lx, mask, kw, cache_implementation="static")
        none, _ = ts._generate(model, vx, lx, mask, kw, cache_implementation="static", kv_cache_dtype=None)
        assert torch.equal(absent, want) and torch.equal(none, want)
    assert len(spy.made) == 4
    for c in spy.made:
        assert c.kv_dtype is None and c.k.dtype == c.v.dtype == c.dtype == torch.float32 and c.k_scale is None and c.v_scale is None
        assert len(c.data_ptrs()) == 2
