"""CPU: the host side of `generate(..., graph_decode=True)` -- StaticKVCache in replay mode (the position, the padding mask and the beam
table in device buffers: otter_amd/kv_cache.py) against the position-scalar mode it restates, tiny generate() calls against the eager
static + media-cache path, the argument errors, and the argument validation of otter_decode_attn_cached_dyn (no GPU needed: nothing is
launched).  On the CPU there is no graph: the same replay-mode step runs eagerly (otter_amd/graph_decode.py), so the bookkeeping a captured
step relies on is exercised end to end here.  The tiny models and batches are those of tests/test_media_cache.py."""
import os
import re

import pytest
import torch

import tests.test_media_cache as tm
from otter_amd.kv_cache import StaticKVCache

# ---- replay mode == position-scalar mode ----------------------------------------------------------------------------------------------

ROWS, H, D, MAX_LEN, S0, LAYERS, STEPS = 4, 2, 8, 16, 5, 2, 6


def _tables():
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    fr = torch.arange(MAX_LEN, dtype=torch.float32)[:, None] * inv[None, :]
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().contiguous(), emb.sin().contiguous()


def _prefilled(dtype, g):
    c = StaticKVCache(LAYERS, ROWS, H, D, MAX_LEN, "cpu", dtype)
    for i in range(LAYERS):
        c.fill(i, torch.randn(ROWS, H, S0, D, generator=g).to(dtype), torch.randn(ROWS, H, S0, D, generator=g).to(dtype))
    c.length = S0
    return c


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_replay_mode_equals_the_position_scalar_mode(dtype):
    """Six consecutive steps with rotary AND ALiBi, a left-padded mask whose row 2 has no valid prompt key, and a table reordered before
    some steps: outputs and caches of the two modes are torch.equal, and the device position follows the host length."""
    g = torch.Generator().manual_seed(0)
    a = _prefilled(dtype, g)                                        # position-scalar mode: the existing attend_reference, host `length`
    b = _prefilled(dtype, torch.Generator().manual_seed(0))         # replay mode
    assert torch.equal(a.k, b.k) and torch.equal(a.v, b.v)
    mask = torch.ones(ROWS, S0, dtype=torch.long)
    mask[1, :2] = 0
    mask[2, :] = 0                                                  # every prompt key of row 2 is padding
    cos_t, sin_t = _tables()
    slopes = torch.tensor([0.5, 0.125])
    with torch.no_grad():
        b.enable_replay(mask, beams=True)
        assert b.replay and not a.replay and b.src is not None and b.pos_dev.dtype == torch.int32 and int(b.pos_dev) == S0
        assert b.valid.dtype == torch.uint8 and torch.equal(b.valid[:, :S0].long(), mask) and bool(b.valid[:, S0:].all())
        with pytest.raises(ValueError, match="already"):
            b.enable_replay(mask)
        ptrs = (b.pos_dev.data_ptr(), b.valid.data_ptr(), b.src.data_ptr()) + b.data_ptrs()
        for step in range(STEPS):
            pos = a.length
            if step in (1, 2, 4):
                beam_idx = torch.randint(0, ROWS, (ROWS,), generator=g)
                a.reorder(beam_idx)
                b.reorder(beam_idx)
            if step == STEPS - 1:                                   # a row with NO valid key at all, the new one included -> o = 0
                b.valid[3] = 0
            mask = torch.cat([mask, torch.ones(ROWS, 1, dtype=torch.long)], dim=1)
            key_valid = mask.to(torch.uint8)
            if step == STEPS - 1:
                key_valid[3] = 0
            b.check_step(ROWS, 1)
            for layer in range(LAYERS):
                q, k, v = (torch.randn(ROWS, H, D, generator=g).to(dtype) for _ in range(3))
                oa = a.attend_reference(layer, q, k, v, 0.3, cos=cos_t[pos], sin=sin_t[pos], key_valid=key_valid, slopes=slopes)
                ob = b.attend(layer, q, k, v, 0.3, cos=cos_t, sin=sin_t, slopes=slopes)
                assert torch.equal(oa, ob), (step, layer)
                assert int(b.pos_dev) == pos                        # one advance per forward, after the last layer
            a.length = pos + 1
            b.advance()
            assert b.length == a.length == int(b.pos_dev) == S0 + step + 1
            assert torch.equal(a.k, b.k) and torch.equal(a.v, b.v) and torch.equal(a.src if a.src is not None else a._own_rows(), b.src)
            if step == STEPS - 1:
                assert float(ob[3].abs().max()) == 0.0
        assert ptrs == (b.pos_dev.data_ptr(), b.valid.data_ptr(), b.src.data_ptr()) + b.data_ptrs()      # nothing a graph points at moved


def test_replay_mode_reads_the_device_position_not_the_host_length():
    """attend_reference in replay mode follows pos_dev: with the host length left behind, the slot written is the device position's."""
    g = torch.Generator().manual_seed(1)
    c = _prefilled(torch.float32, g)
    with torch.no_grad():
        c.enable_replay(None)
        assert c.src is None
        c.pos_dev.fill_(9)
        q, k, v = (torch.randn(ROWS, H, D, generator=g) for _ in range(3))
        before = c.k[0].clone()
        c.attend(0, q, k, v, 0.3)
        assert torch.equal(c.k[0, :, :, 9], k) and torch.equal(c.k[0, :, :, :9], before[:, :, :9]) and c.length == S0
        c.pos_dev.fill_(MAX_LEN)                                    # outside [1, max_len): refused, never an index
        with pytest.raises(ValueError, match="1 <= length < max_len"):
            c.attend(0, q, k, v, 0.3)
        with pytest.raises(ValueError, match="key_valid=None"):
            c.attend(0, q, k, v, 0.3, key_valid=torch.ones(ROWS, S0 + 1, dtype=torch.uint8))
        with pytest.raises(ValueError, match="without beams"):
            c.reorder(torch.arange(ROWS))
    fresh = StaticKVCache(1, 2, H, D, MAX_LEN, "cpu", torch.float32)
    with pytest.raises(ValueError, match="empty"):
        fresh.enable_replay(None)
    with pytest.raises(ValueError, match="replay mode only"):
        fresh.advance()


# ---- generate -------------------------------------------------------------------------------------------------------------------------

GRAPH_CASES = {"greedy": dict(), "beams3": dict(num_beams=3), "sample": dict(do_sample=True, top_k=20, temperature=0.9)}
STATIC_MEDIA = dict(cache_implementation="static", cross_attention_cache=True)


@pytest.mark.parametrize("case", list(GRAPH_CASES))
@pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
def test_graph_decode_generate_returns_the_eager_static_tokens(llama, case):
    """Left-padded batch of two.  The steps of the two calls run the same arithmetic (attend_reference with the same position, mask and
    table), so the tokens are equal exactly -- no margin rule is needed."""
    model = tm._model(llama)
    vx, ids, mask = tm._batch(2, (0, 2), seed=tm.GEN_SEED)
    lx, mask = ids[:, :tm.P_LEN], mask[:, :tm.P_LEN]
    want, _ = tm._generate(model, vx, lx, mask, GRAPH_CASES[case], **STATIC_MEDIA)
    got, _ = tm._generate(model, vx, lx, mask, GRAPH_CASES[case], graph_decode=True, **STATIC_MEDIA)
    assert want.shape[1] == tm.P_LEN + tm.NEW
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert not model.lang_encoder.is_conditioned()
    got2, _ = tm._generate(model, vx, lx, None, GRAPH_CASES[case], graph_decode=True, **STATIC_MEDIA)      # no mask at all
    want2, _ = tm._generate(model, vx, lx, None, GRAPH_CASES[case], **STATIC_MEDIA)
    assert torch.equal(got2, want2)


def test_graph_decode_steps_run_in_replay_mode(monkeypatch):
    """The cached steps of graph_decode=True really take the replay branch: every attend after the prompt pass sees a cache in replay mode
    and no key_valid, and the device position ends level with the host length."""
    model = tm._model(False)
    vx, ids, mask = tm._batch(2, (0, 2), seed=tm.GEN_SEED)
    seen = []
    real = StaticKVCache.attend

    def spy(self, layer, q, k_new, v_new, scale, cos=None, sin=None, key_valid=None, slopes=None):
        seen.append((self.replay, key_valid is None, int(self.pos_dev) if self.replay else -1, self.length))
        return real(self, layer, q, k_new, v_new, scale, cos=cos, sin=sin, key_valid=key_valid, slopes=slopes)

    monkeypatch.setattr(StaticKVCache, "attend", spy)
    tm._generate(model, vx, ids[:, :tm.P_LEN], mask[:, :tm.P_LEN], dict(), graph_decode=True, **STATIC_MEDIA)
    assert seen and all(r and kv_none and p == n for r, kv_none, p, n in seen)
    assert sorted({n for _, _, _, n in seen}) == list(range(tm.P_LEN, tm.P_LEN + tm.NEW - 1))


# ---- argument errors ------------------------------------------------------------------------------------------------------------------

def test_graph_decode_needs_the_static_cache_and_the_media_cache():
    model = tm._model(False)
    vx, ids, _ = tm._batch(1, None)
    lx = ids[:, :tm.P_LEN]
    for kw in (dict(use_cache=True, cross_attention_cache=True), dict(cache_implementation="static"), dict(),
               dict(cache_implementation="dynamic", cross_attention_cache=True)):
        with pytest.raises(ValueError, match=r"graph_decode.*cache_implementation='static'.*cross_attention_cache=True"):
            model.generate(vision_x=vx, lang_x=lx, max_new_tokens=2, graph_decode=True, **kw)
        assert not model.lang_encoder.is_conditioned()


def test_position_ids_over_a_replay_cache_are_rejected():
    from transformers import LlamaConfig

    from otter_amd.llama import LlamaModel

    cfg = LlamaConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=50,
                      max_position_embeddings=32, rms_norm_eps=1e-6)
    torch.manual_seed(0)
    lm = LlamaModel(cfg).eval()
    ids = torch.randint(1, 50, (2, 4), generator=torch.Generator().manual_seed(0))
    cache = StaticKVCache(2, 2, 4, 8, 12, "cpu", torch.float32)
    with torch.no_grad():
        lm(input_ids=ids, past_key_values=cache, use_cache=True)
        lm(input_ids=ids[:, :1], past_key_values=cache, use_cache=True, position_ids=torch.full((2, 1), 4))      # fine without replay mode
        cache.enable_replay(None)
        with pytest.raises(ValueError, match="position_ids"):
            lm(input_ids=ids[:, :1], past_key_values=cache, use_cache=True, position_ids=torch.full((2, 1), 5))
        assert cache.length == 5 == int(cache.pos_dev)
        lm(input_ids=ids[:, :1], past_key_values=cache, use_cache=True)
        assert cache.length == 6 == int(cache.pos_dev)


def test_grouped_key_value_heads_step_in_replay_mode_and_report_no_kernel_step():
    """A host with fewer key / value heads than query heads: the replay-mode step is the restatement's (never the kernel's), equal to the
    position-scalar static step, and the cache says so (`kernel_steps`), which is what keeps generate(graph_decode=True) from capturing it."""
    from transformers import LlamaConfig

    from otter_amd.llama import LlamaModel

    cfg = LlamaConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=50,
                      max_position_embeddings=32, rms_norm_eps=1e-6)
    torch.manual_seed(0)
    lm = LlamaModel(cfg).eval()
    ids = torch.randint(1, 50, (2, 7), generator=torch.Generator().manual_seed(0))
    a, b = StaticKVCache(2, 2, 2, 8, 12, "cpu", torch.float32), StaticKVCache(2, 2, 2, 8, 12, "cpu", torch.float32)
    with torch.no_grad():
        for c in (a, b):
            lm(input_ids=ids[:, :4], past_key_values=c, use_cache=True)
        b.enable_replay(None)
        assert b.kernel_steps
        for t in range(4, 7):
            want = lm(input_ids=ids[:, t:t + 1], past_key_values=a, use_cache=True)[0]
            got = lm(input_ids=ids[:, t:t + 1], past_key_values=b, use_cache=True)[0]
            assert torch.equal(got, want), t
    assert not b.kernel_steps and a.length == b.length == 7 == int(b.pos_dev)
    assert torch.equal(a.k, b.k) and torch.equal(a.v, b.v)


def test_fuyu_host_does_not_take_graph_decode():
    from oracle.gen_golden_fuyu import tiny_fuyu_config
    from otter_amd.fuyu import FuyuForCausalLM

    model = FuyuForCausalLM(tiny_fuyu_config()).eval()
    ids = torch.randint(1, 100, (1, 5), generator=torch.Generator().manual_seed(0))
    with pytest.raises(NotImplementedError, match="graph_decode=True replays a step over the static cache"):
        model.generate(input_ids=ids, max_new_tokens=2, graph_decode=True)
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=ids, max_new_tokens=2, graph_decode=True, cache_implementation="static", cross_attention_cache=True)


def test_side_streams_report_disabled_inside_a_single_chain():
    from otter_amd import functional as OF

    dev = torch.device("cuda", 0)                       # (only the device TYPE is read: no GPU is touched while the flag is set)
    with OF.single_chain():
        assert OF._single_chain and not OF._SideStream(dev).enabled
        with OF.single_chain():
            pass
        assert OF._single_chain
    assert not OF._single_chain


# ---- otter_decode_attn_cached_dyn: argument validation, nothing launched ----------------------------------------------------------------

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
S_MAX = 64


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, **over):
    a = dict(q=P, q_rs=3 * H * 128, q_hs=128, kn=P + 2 * H * 128, kn_rs=3 * H * 128, kn_hs=128, vn=P + 4 * H * 128, vn_rs=3 * H * 128, vn_hs=128,
             cos=None, sin=None, tab_rs=0, kc=P, kc_rs=H * S_MAX * 128, kc_hs=S_MAX * 128, vc=P, vc_rs=H * S_MAX * 128, vc_hs=S_MAX * 128,
             src=None, src_rs=0, kvalid=None, kv_rs=0, slopes=None, o=P, ws=P, ws_bytes=1 << 20, N=3, H=H, pos_dev=P, S_max=S_MAX, head_dim=128,
             scale=0.0884)
    a.update(over)
    return lib.otter_decode_attn_cached_dyn(a["q"], a["q_rs"], a["q_hs"], a["kn"], a["kn_rs"], a["kn_hs"], a["vn"], a["vn_rs"], a["vn_hs"], a["cos"],
                                            a["sin"], a["tab_rs"], a["kc"], a["kc_rs"], a["kc_hs"], a["vc"], a["vc_rs"], a["vc_hs"], a["src"],
                                            a["src_rs"], a["kvalid"], a["kv_rs"], a["slopes"], a["o"], a["ws"], a["ws_bytes"], a["N"], a["H"],
                                            a["pos_dev"], a["S_max"], a["head_dim"], a["scale"], None)


@pytest.mark.parametrize("name", ["q", "kn", "vn", "kc", "vc", "o", "ws", "pos_dev"])
def test_dyn_null_pointers_are_rejected(lib, name):
    assert call(lib, **{name: None}) == -1
    assert b"decode_attn_cached_dyn: null pointer" in lib.otter_last_error()


def test_dyn_cos_without_sin_is_rejected(lib):
    assert call(lib, cos=P, tab_rs=128) == -1
    assert b"both be given or both be NULL" in lib.otter_last_error()
    assert call(lib, sin=P, tab_rs=128) == -1
    assert b"both be given or both be NULL" in lib.otter_last_error()


@pytest.mark.parametrize("name", ["q", "kn", "vn", "kc", "vc"])
def test_dyn_misaligned_pointers_are_rejected(lib, name):
    assert call(lib, **{name: P + 2}) == -1
    assert b"16-byte alignment" in lib.otter_last_error()


def test_dyn_misaligned_position_pointer_is_rejected(lib):
    assert call(lib, pos_dev=P + 2) == -1
    assert b"4-byte alignment" in lib.otter_last_error()


@pytest.mark.parametrize("name", ["q_rs", "q_hs", "kn_rs", "kn_hs", "vn_rs", "vn_hs", "kc_rs", "vc_rs"])
def test_dyn_strides_that_are_not_multiples_of_8_are_rejected(lib, name):
    assert call(lib, **{name: 3 * H * 128 + 4}) == -1
    assert b"multiples of 8" in lib.otter_last_error()


def test_dyn_cache_table_and_mask_stride_rules(lib):
    assert call(lib, kc_hs=S_MAX * 128 - 8) == -1                  # the slots of two heads would overlap
    assert b"overlap" in lib.otter_last_error()
    assert call(lib, vc_hs=S_MAX * 128 - 8) == -1
    assert b"overlap" in lib.otter_last_error()
    assert call(lib, src=P, src_rs=S_MAX - 2) == -1                # any pos < S_max may come up: S_max - 1 entries per row
    assert b"src one >= S_max - 1" in lib.otter_last_error()
    assert call(lib, kvalid=P, kv_rs=S_MAX - 1) == -1              # S_max keys per row
    assert b"key_valid one >= S_max" in lib.otter_last_error()
    assert call(lib, cos=P, sin=P, tab_rs=64) == -1                # rows of 128
    assert b"row stride >= 128" in lib.otter_last_error()


def test_dyn_head_dim_and_capacity_rules(lib):
    assert call(lib, head_dim=64) == -1
    assert b"head_dim 64" in lib.otter_last_error()
    assert call(lib, S_max=1) == -1
    assert b"S_max=1" in lib.otter_last_error()
    big = 65536 + 1
    assert call(lib, S_max=big, kc_hs=big * 128, vc_hs=big * 128, kc_rs=H * big * 128, vc_rs=H * big * 128, ws_bytes=1 << 40) == -1
    assert b"S_max=65537" in lib.otter_last_error()
    assert call(lib, N=0) == -1
    assert b"bad shape" in lib.otter_last_error()


def test_dyn_workspace_one_byte_short_is_rejected(lib):
    need = 3 * H * 1 * 130 * 4                                     # N * H * ceil(64 / 128) records of 130 floats: sized by the CAPACITY
    assert call(lib, ws_bytes=need - 1) == -1
    assert b"%d needed" % need in lib.otter_last_error()
    need = 3 * H * 3 * 130 * 4                                     # S_max = 257: three records, whatever the position
    assert call(lib, S_max=257, kc_hs=264 * 128, vc_hs=264 * 128, kc_rs=H * 264 * 128, vc_rs=H * 264 * 128, ws_bytes=need - 1) == -1
    assert b"%d needed" % need in lib.otter_last_error()


def test_dyn_workspace_formula_matches_the_header():
    from otter_amd import ops

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    m = re.search(r"#define OTTER_DECODE_CACHED_DYN_WORKSPACE_BYTES\(N, H, S_max\) (.*)", hdr)
    expr = m.group(1).replace("(int64_t)", "").replace("/", "//")
    for N, H_, S in [(1, 32, 513), (12, 32, 2), (3, 2, 65536), (1, 32, 4352)]:
        assert eval(expr, {"N": N, "H": H_, "S_max": S}) == ops.decode_attn_cached_dyn_workspace_bytes(N, H_, S)
    assert ops.decode_attn_cached_dyn_workspace_bytes(1, 32, 4352) == 32 * 34 * 130 * 4
    # the scalar entry point's need at the last position of the same cache is the same: one workspace serves both
    assert ops.decode_attn_cached_dyn_workspace_bytes(3, 2, 4352) == ops.decode_attn_cached_workspace_bytes(3, 2, 4352)
