"""GPU: the graph-replayed decode step (otter_amd/graph_decode.py).  The kernel with the position in device memory
(otter_decode_attn_cached_dyn, csrc/decode_cache.hip) against the position-scalar kernel it shares its arithmetic with -- bit for bit --;
one launch serving two positions; a captured step of 2-layer full-width hosts against the same step run eagerly; generate(graph_decode=True)
against the eager static + media-cache path, its capture / replay counts, its single chain and what it leaves allocated."""
import copy
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S_MAX = 4352
POSITIONS = (1, 127, 128, 129, 1000, 4351)      # one range, the range boundaries, many ranges, the last slot
SENT = 0x5A5A                                    # bf16 bit pattern of an untouched output


# ---- kernel ---------------------------------------------------------------------------------------------------------------------------

def _inputs(N, H, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    qkv = r(N, 3, H, 128).bfloat16()
    k0, v0 = r(N, H, S_MAX, 128).bfloat16(), r(N, H, S_MAX, 128).bfloat16()
    inv = 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32, device=DEV) / 128))
    fr = torch.arange(S_MAX, dtype=torch.float32, device=DEV)[:, None] * inv[None, :]
    emb = torch.cat((fr, fr), dim=-1)
    valid = (torch.rand(N, S_MAX, device=DEV, generator=g) > 0.2).to(torch.uint8)
    valid[:, :40] = 0                                                    # left padding
    valid[N - 1] = 0 if N > 1 else valid[N - 1]                          # N > 1: the last row has no valid key at all -> o = 0
    src = torch.randint(0, N, (N, S_MAX), device=DEV, generator=g, dtype=torch.int32)
    slopes = (2.0 ** -(8.0 * torch.arange(1, H + 1, device=DEV, dtype=torch.float32) / H)).contiguous()
    return dict(q=qkv[:, 0], k=qkv[:, 1], v=qkv[:, 2], k0=k0, v0=v0, cos=emb.cos().contiguous(), sin=emb.sin().contiguous(), valid=valid, src=src,
                slopes=slopes)


OPTIONS = {                     # (alibi, rotary, key_valid, table)
    "plain": (False, False, False, False),
    "alibi_mask": (True, False, True, False),
    "rotary_table": (False, True, False, True),
    "all": (True, True, True, True),
}


def _scalar(ops, a, kc, vc, pos, opt):
    alibi, rot, mask, table = OPTIONS[opt]
    return ops.decode_attn_cached(a["q"], a["k"], a["v"], kc, vc, pos, 0.0884, cos=a["cos"][pos] if rot else None, sin=a["sin"][pos] if rot else None,
                                  src=a["src"] if table else None, key_valid=a["valid"] if mask else None, slopes=a["slopes"] if alibi else None)


def _dyn(ops, a, kc, vc, pos_dev, opt, out=None):
    alibi, rot, mask, table = OPTIONS[opt]
    return ops.decode_attn_cached_dyn(a["q"], a["k"], a["v"], kc, vc, pos_dev, 0.0884, cos_table=a["cos"] if rot else None,
                                      sin_table=a["sin"] if rot else None, src=a["src"] if table else None, key_valid=a["valid"] if mask else None,
                                      slopes=a["slopes"] if alibi else None, out=out)


@pytest.mark.parametrize("N,H", [(1, 2), (3, 2), (1, 32), (3, 32)])
def test_dyn_kernel_is_bit_identical_to_the_position_scalar_kernel(N, H):
    """At every position and option set: o and the written K / V slot torch.equal to otter_decode_attn_cached at the same pos, no other
    slot changed, two calls the same bits.  No tolerance: equality with the merged kernel inherits its fp64-oracle bound."""
    from otter_amd import ops

    a = _inputs(N, H, 7 * N + H)
    ka, va, kb, vb = a["k0"].clone(), a["v0"].clone(), a["k0"].clone(), a["v0"].clone()
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    for opt in OPTIONS:
        for pos in POSITIONS:
            want = _scalar(ops, a, ka, va, pos, opt)
            pos_dev.fill_(pos)
            got = _dyn(ops, a, kb, vb, pos_dev, opt)
            assert torch.equal(got, want), (opt, pos, float((got.float() - want.float()).abs().max()))
            assert torch.equal(kb[:, :, pos], ka[:, :, pos]) and torch.equal(vb[:, :, pos], va[:, :, pos]), (opt, pos)
            assert not torch.equal(kb[:, :, pos], a["k0"][:, :, pos])                      # (the slot was written)
            again = _dyn(ops, a, kb, vb, pos_dev, opt)
            assert torch.equal(again, got) and torch.equal(kb[:, :, pos], ka[:, :, pos]), (opt, pos)
            if OPTIONS[opt][2] and N > 1:
                assert float(got[N - 1].float().abs().max()) == 0.0                        # the fully masked row
            for c, c0 in ((ka, a["k0"]), (va, a["v0"]), (kb, a["k0"]), (vb, a["v0"])):     # put the slot back: every OTHER slot is as it was
                c[:, :, pos] = c0[:, :, pos]
            assert torch.equal(kb, a["k0"]) and torch.equal(vb, a["v0"]), (opt, pos)
    assert int(pos_dev) == POSITIONS[-1]                                                   # the kernel only reads the position


@pytest.mark.parametrize("bad", [0, S_MAX, -3, 1 << 30])
def test_dyn_kernel_ignores_a_position_outside_the_cache(bad):
    from otter_amd import ops

    N, H = 3, 32
    a = _inputs(N, H, 5)
    kb, vb = a["k0"].clone(), a["v0"].clone()
    out = torch.full((N, H * 128), SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    pos_dev = torch.full((1,), bad, dtype=torch.int32, device=DEV)
    got = _dyn(ops, a, kb, vb, pos_dev, "all", out=out)
    torch.cuda.synchronize()
    assert got is out and bool((out.view(torch.int16) == SENT).all())
    assert torch.equal(kb, a["k0"]) and torch.equal(vb, a["v0"])


def test_a_position_with_more_ranges_than_the_capacity_has():
    """The range count is not monotone in the key count, so the grid is sized by the rule's upper bound, not by its value at the capacity.
    N H = 32 on 256 CUs wants 16 ranges: 4096 keys (pos 4095) split into 16 of 256, but the 4100 keys of a cache of S_max = 4100 split
    into 15 of 288 (the range length is rounded up to 32).  A grid sized by the count at the capacity would drop the sixteenth range at pos
    4095.  Positions: the last with 16 ranges, the first with 15, the last slot; the cache is a view of S_max = 4100 keys per head."""
    from otter_amd import ops

    N, H, s_max = 1, 32, 4100
    a = _inputs(N, H, 23)
    ka, va, kb, vb = a["k0"].clone(), a["v0"].clone(), a["k0"].clone(), a["v0"].clone()
    pos_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    for pos in (4095, 4096, s_max - 1):
        want = _scalar(ops, a, ka, va, pos, "all")
        pos_dev.fill_(pos)
        got = _dyn(ops, a, kb[:, :, :s_max], vb[:, :, :s_max], pos_dev, "all")
        assert torch.equal(got, want), (pos, float((got.float() - want.float()).abs().max()))
        assert torch.equal(kb, ka) and torch.equal(vb, va), pos
    pos_dev.fill_(s_max)                                                                   # the view's capacity, not the buffer's
    out = torch.full((N, H * 128), SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    _dyn(ops, a, kb[:, :, :s_max], vb[:, :, :s_max], pos_dev, "all", out=out)
    assert bool((out.view(torch.int16) == SENT).all()) and torch.equal(kb, ka) and torch.equal(vb, va)


def test_one_launch_serves_two_positions():
    """What replay relies on, without a graph: the wrapper is called twice with IDENTICAL Python arguments; between the calls only the
    device position changes (5 -> 3000, by a device op)."""
    from otter_amd import ops

    N, H = 3, 32
    a = _inputs(N, H, 11)
    ka, va, kb, vb = a["k0"].clone(), a["v0"].clone(), a["k0"].clone(), a["v0"].clone()
    pos_dev = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    out = torch.empty((N, H * 128), dtype=torch.bfloat16, device=DEV)
    args = dict(ops=ops, a=a, kc=kb, vc=vb, pos_dev=pos_dev, opt="all", out=out)
    first = _dyn(**args).clone()
    pos_dev.add_(2995)
    second = _dyn(**args).clone()
    assert torch.equal(first, _scalar(ops, a, ka, va, 5, "all"))
    assert torch.equal(second, _scalar(ops, a, ka, va, 3000, "all"))
    assert torch.equal(kb, ka) and torch.equal(vb, va)
    assert not torch.equal(first, second)


def test_wrapper_rejects_what_the_kernel_cannot_take():
    from otter_amd import ops
    from otter_amd._capi import OtterHipError

    a = _inputs(2, 2, 3)
    kb, vb = a["k0"].clone(), a["v0"].clone()
    pos_dev = torch.full((1,), 9, dtype=torch.int32, device=DEV)
    base = dict(q=a["q"], k=a["k"], v=a["v"], kc=kb, vc=vb, pos=pos_dev, cos=a["cos"], sin=a["sin"], src=a["src"], valid=a["valid"])
    for bad in (dict(pos=pos_dev.long()), dict(pos=pos_dev.cpu()), dict(pos=torch.zeros(2, dtype=torch.int32, device=DEV)), dict(cos=a["cos"][:100]),
                dict(sin=None), dict(cos=a["cos"][9]), dict(src=a["src"][:, :100]), dict(valid=a["valid"][:, :S_MAX - 1]), dict(q=a["q"].float()),
                dict(kc=kb[:, :, :-1])):
        x = dict(base)
        x.update(bad)
        with pytest.raises(OtterHipError):
            ops.decode_attn_cached_dyn(x["q"], x["k"], x["v"], x["kc"], x["vc"], x["pos"], 0.0884, cos_table=x["cos"], sin_table=x["sin"], src=x["src"],
                                       key_valid=x["valid"])
    torch.cuda.synchronize()
    assert torch.equal(kb, a["k0"])


# ---- a captured step of 2-layer full-width hosts ----------------------------------------------------------------------------------------

P_LEN, NEW, B = 40, 12, 2
PADS = (0, 9)


def _prefilled(model, bench, rows_total):
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache

    vx, ids, mask, _, _ = bench.synth_batch(model, B, rows_total, DEV, seed=99, frames=1)
    for r, n in enumerate(PADS):
        mask[r, :n] = 0
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    cache, mc = StaticKVCache(n_layers, B, n_kv, hd, rows_total, DEV), MediaCache(B, model.media_token_id)
    out = model(vision_x=vx.to(torch.bfloat16), lang_x=ids[:, :P_LEN], attention_mask=mask[:, :P_LEN], past_key_values=cache, use_cache=True,
                clear_conditioned_layers=False, media_cache=mc)
    return cache, mc, mask[:, :P_LEN], out.logits[:, -1]


def _twin(cache, mc):
    """A second pair of caches holding what the first pair holds: the projected media are shared (read only), everything a step writes is
    copied."""
    c2, m2 = copy.copy(cache), copy.copy(mc)
    c2.k, c2.v = cache.k.clone(), cache.v.clone()
    m2.seen, m2.kv = mc.seen.clone(), list(mc.kv)
    return c2, m2


def _graph_against_eager(model, bench, tag):
    from otter_amd.graph_decode import GraphDecodeStep

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        cache, mc, mask, logits = _prefilled(model, bench, P_LEN + NEW)
        c2, m2 = _twin(cache, mc)
        cache.enable_replay(mask)
        c2.enable_replay(mask)
        graph, eager = GraphDecodeStep(model.lang_encoder, cache, mc), GraphDecodeStep(model.lang_encoder, c2, m2)
        assert graph.use_graph
        eager.use_graph = False                         # the same replay-mode step, every launch issued from Python
        try:
            nxt = logits.float().argmax(-1)
            for t in range(NEW - 1):
                lg = graph(nxt[:, None]).clone()
                le = eager(nxt[:, None])
                assert lg.shape == le.shape == (B, model.lang_encoder.config.vocab_size)
                assert torch.equal(lg, le), (tag, t, float((lg.float() - le.float()).abs().max()))
                assert cache.length == c2.length == P_LEN + t + 1 == int(cache.pos_dev) == int(c2.pos_dev)
                nxt = lg.float().argmax(-1)
            assert torch.equal(cache.k, c2.k) and torch.equal(cache.v, c2.v) and torch.equal(mc.seen, m2.seen)
            assert (graph.captures, graph.replays) == (1, NEW - 1 - 2) and (eager.captures, eager.replays) == (0, 0)
            print("[graph-decode] %s: %d steps bit-equal, capture %.1f ms" % (tag, NEW - 1, graph.capture_seconds * 1e3), flush=True)
        finally:
            graph.release()
            eager.release()
            model.lang_encoder.clear_conditioned_layers()


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_replayed_steps_equal_the_eager_replay_mode_steps(kind):
    """2-layer full-width host, bf16 autocast, then the same model with quantize_decoder_int8(): 40-token left-padded prompt, B = 2, 12 new
    tokens.  The logits of every step of the graph path (two eager warm-up steps on the capture stream, the captured step, 8 replays) are
    torch.equal to the eager replay-mode step over a second pair of caches holding the same prefill: the kernels are deterministic and the
    launches are the same."""
    from tests.test_gpu_media_cache import _build

    model, bench = _build(kind)
    _graph_against_eager(model, bench, kind + " bf16")
    assert model.quantize_decoder_int8()["replaced"] > 0
    _graph_against_eager(model, bench, kind + " int8")
    del model
    gc.collect()
    torch.cuda.empty_cache()


# ---- generate ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mpt2():
    from tests.test_gpu_media_cache import _build

    model, bench = _build("mpt")
    yield model, bench
    del model
    gc.collect()
    torch.cuda.empty_cache()


def _gen(model, bench, graph, **kw):
    vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN, DEV, seed=99, frames=1)
    for r, n in enumerate(PADS):
        mask[r, :n] = 0
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        return model.generate(vision_x=vx.to(torch.bfloat16), lang_x=ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=-1,
                              cache_implementation="static", cross_attention_cache=True, **(dict(graph_decode=True) if graph else {}), **kw)


@pytest.mark.parametrize("case", ["greedy", "beams3", "sample"])
def test_generate_captures_once_replays_the_rest_and_forks_nothing(mpt2, case, monkeypatch):
    """12 new tokens = the prompt pass + 11 cached steps = 2 eager warm-up steps + 1 capture + 9 replays (the captured step's own included).
    No side stream is forked while the step is captured.  The tokens are those of the eager static + media-cache path."""
    from otter_amd import functional as OF
    from otter_amd.graph_decode import GraphDecodeStep

    model, bench = mpt2
    kw = dict(greedy=dict(), beams3=dict(num_beams=3), sample=dict(do_sample=True, top_k=20, temperature=0.9))[case]
    counts, forks = [], []
    release, fork = GraphDecodeStep.release, OF._SideStream.fork

    def spy_release(self):
        counts.append((self.steps, self.captures, self.replays, self.use_graph))
        return release(self)

    def spy_fork(self):
        if torch.cuda.is_current_stream_capturing():
            forks.append(self.enabled)
        return fork(self)

    monkeypatch.setattr(GraphDecodeStep, "release", spy_release)
    monkeypatch.setattr(OF._SideStream, "fork", spy_fork)
    gen = lambda: dict(generator=torch.Generator(device=DEV).manual_seed(1234)) if case == "sample" else {}
    got = _gen(model, bench, True, **kw, **gen())
    assert counts == [(NEW - 1, 1, NEW - 3, True)], counts
    assert counts[0][2] >= 9 and not any(forks), forks
    want = _gen(model, bench, False, **kw, **gen())
    assert got.shape == want.shape and got.shape[1] == P_LEN + NEW
    assert torch.equal(got, want), (got[:, P_LEN:].tolist(), want[:, P_LEN:].tolist())
    assert not model.lang_encoder.is_conditioned() and not OF._single_chain


def test_grouped_key_value_heads_fall_back_to_the_eager_replay_step(monkeypatch):
    """A LLaMA host with head_dim 128 in bf16 but fewer key / value heads than query heads: the cache's step is the plain-torch restatement
    (StaticKVCache.uses_kernel), which reads the position back to the host and so cannot be captured.  generate(graph_decode=True) must
    notice that over its warm-up steps and go on eagerly -- no capture, every cached step run, the tokens of the eager static path."""
    import bench
    from oracle import synth
    from otter_amd.configuration_otter import OtterConfig
    from otter_amd.graph_decode import GraphDecodeStep
    from otter_amd.modeling_otter import OtterForConditionalGeneration

    text, vis = dict(bench.LLAMA7B_TEXT), dict(bench.CLIP_L14)
    text.update(num_hidden_layers=2, num_key_value_heads=8)
    vis["num_hidden_layers"] = 2
    with torch.device(DEV):
        model = OtterForConditionalGeneration(OtterConfig(vision_config=vis, text_config=text, cross_attn_every_n_layers=1, max_num_frames=8))
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.from_numpy(synth.param_for(1234, name, tuple(p.shape))).to(DEV))
    model.eval()
    counts, release = [], GraphDecodeStep.release

    def spy_release(self):
        counts.append((self.steps, self.captures, self.replays, self.use_graph, self.cache.kernel_steps))
        return release(self)

    monkeypatch.setattr(GraphDecodeStep, "release", spy_release)
    got = _gen(model, bench, True)
    assert counts == [(NEW - 1, 0, 0, False, False)], counts
    want = _gen(model, bench, False)
    assert got.shape == want.shape and got.shape[1] == P_LEN + NEW and torch.equal(got, want)
    del model
    gc.collect()
    torch.cuda.empty_cache()


GEMM_WORKSPACE = 76 << 20     # the library GEMM's workspace: one per stream it has run on, kept by the library for the life of the process


def test_generate_releases_the_graph_pool(mpt2):
    """memory_allocated around graph_decode generate() calls, against the footprint of the model after an eager static + media-cache call
    (which has warmed what that path keeps by design: the main stream's workspaces, ALiBi slopes).  The first graph call may leave ONE
    thing behind: the library GEMM's workspace of the capture stream (at most 76 MiB, the size this library takes; the stream is one per
    device for the life of the process, so it is left once -- nothing, if an earlier test of this process has used the stream).  A second call leaves nothing at all: the graph,
    its private pool, the static ids / logits, the replay buffers of the cache and this project's workspace of the capture stream are
    gone."""
    from otter_amd import ops

    model, bench = mpt2

    def allocated():
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()

    _gen(model, bench, False)
    footprint, n_ws = allocated(), len(ops._ws.bufs)
    _gen(model, bench, True)
    first = allocated()
    _gen(model, bench, True)
    second = allocated()
    print("[graph-decode] memory_allocated: footprint %d, after the first graph call +%d, after the second +%d"
          % (footprint, first - footprint, second - footprint), flush=True)
    assert 0 <= first - footprint <= GEMM_WORKSPACE, (footprint, first)
    assert second == first, (first, second)
    assert len(ops._ws.bufs) == n_ws


def test_tiny_generate_with_beams_equals_the_eager_static_path():
    """The tiny MPT-host Otter (head_dim 16: the step is the plain-torch restatement, so no graph -- the same replay-mode step, eagerly, on
    the GPU) in bf16 autocast with num_beams=3: token for token the eager static + media-cache path."""
    from oracle import synth
    from tests.test_gpu_w8 import _tiny

    model, m = _tiny(DEV)
    vision_x, ids, _, _ = synth.tiny_batch(m["seed"])
    vx, lx = torch.from_numpy(vision_x).to(DEV).to(torch.bfloat16), torch.from_numpy(ids[:, :8]).to(DEV)
    kw = dict(max_new_tokens=8, eos_token_id=-1, num_beams=3, cache_implementation="static", cross_attention_cache=True)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        want = model.generate(vision_x=vx, lang_x=lx, **kw)
        got = model.generate(vision_x=vx, lang_x=lx, graph_decode=True, **kw)
    assert got.shape == want.shape == (lx.shape[0], 16) and torch.equal(got, want), (got.tolist(), want.tolist())
    assert not model.lang_encoder.is_conditioned()
