"""Cached generation at Fuyu-8B shape: ms per decode step over a StaticKVCache passed as `past_key_values` (in-place append on
csrc/persimmon_decode_cache.hip), eager and graph-replayed (otter_amd/graph_decode.py), against the default growing tuple cache
(csrc/persimmon_decode.hip: the whole past copied every step), alternated in one process.

Random-init PersimmonForCausalLM at Fuyu-8B's shape (hidden 4096, 64 heads x 64, partial_rotary_factor 0.5, 36 layers, FFN 16384, untied
vocabulary 262144), stored in bf16; the int8 model is a deep copy of it after quantize_decoder_int8(); both stay resident.  A PROMPT-token
prompt (HIP prefill, not timed, last position un-embedded only), then STEPS greedy tokens (no end token) fed back one at a time.  Points:
B = 1, B = 4, and "3 beams": 3 rows whose cache is reordered before every step by a fixed beam_idx -- index_select of every layer's past for
the default cache, `StaticKVCache.reorder` (the int32 table) for the static one; the beam scoring itself is not in the clock.  Three paths:

    default   the tuple cache, every launch from Python
    static    StaticKVCache, position-scalar step, every launch from Python
    graph     StaticKVCache in replay mode through GraphDecodeStep: 2 eager warm-up steps, 1 capture, the rest replays

Clock: torch.cuda.synchronize() + perf_counter around the cached steps only; the graph path's one-off capture time (measured inside
GraphDecodeStep: synchronize, capture, synchronize) is taken out and printed beside.  Per point: one untimed run of each path (warm-up; it
also records the tokens), then ROUNDS rounds alternating the three paths.  Reported: median ms per cached step, spread (max - min) /
median over the rounds, launches per step (torch.profiler kernel events over 4 eager steps of each path; the graph holds the launches of the
replay-mode step, counted on that step run eagerly), peak memory above the resident models over one run of each path, and where the greedy
tokens of the static and graph paths first part from the default cache's, if they do.
Condition (DESIGN.md sections 4.10 / 4.11): at every point static <= 1.03 x default and graph <= 1.03 x default, in the same run; a point
that misses prints MISS.

  python tools/fuyu_static_decode_bench.py [--rounds 3] [--steps 128] [--prompt 1350] [--layers 36] [--out profiles/r15_fuyu_static_decode_ab.txt]"""
from __future__ import annotations

import argparse
import copy
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

VOCAB = 262144
PATHS = ("default", "static", "graph")
THRESHOLD = 1.03
POINTS = (("B=1", 1, False), ("B=4", 4, False), ("3 beams", 3, True))


def build_model(layers: int):
    from transformers import PersimmonConfig

    from otter_amd.fuyu import PersimmonForCausalLM

    cfg = PersimmonConfig(vocab_size=VOCAB, hidden_size=4096, intermediate_size=16384, num_hidden_layers=layers, num_attention_heads=64,
                          max_position_embeddings=16384, qk_layernorm=True, partial_rotary_factor=0.5, hidden_act="relu2", layer_norm_eps=1e-5,
                          rope_theta=25000.0, tie_word_embeddings=False, use_cache=True)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = PersimmonForCausalLM(cfg)
    return model.to(torch.bfloat16).eval()


def beam_idx_for(step: int, rows: int, device):
    """A fixed reordering per step: every row continues its left neighbour or itself, rows 0 and 1 sometimes the same ancestor."""
    pat = ((1, 0, 2), (0, 0, 1), (2, 1, 1), (0, 2, 2))[step % 4]
    return torch.tensor(pat[:rows], dtype=torch.long, device=device)


@torch.no_grad()
def decode(model, path, ids, steps, beams, cache=None, count_launches=0):
    """prompt pass + `steps` greedy cached steps on `path`; returns (ms per step without the capture, capture ms, tokens [rows, steps]).
    `count_launches` > 0: that many steps run under torch.profiler instead of the clock; returns kernel events per step."""
    from otter_amd.graph_decode import GraphDecodeStep

    rows, dev = ids.shape[0], ids.device
    if path == "default":
        out = model(input_ids=ids, use_cache=True, _last_position_only=True)
        past = out.past_key_values
    else:
        cache.reset()
        out = model(input_ids=ids, past_key_values=cache, _last_position_only=True)
        past = cache
    graph = None
    if path == "graph":
        cache.enable_replay(None, beams=beams)
        graph = GraphDecodeStep(model, cache, None, step_fn=lambda i: model(input_ids=i, past_key_values=cache).logits[:, -1, :],
                                kernel_head_dim=64)
        if count_launches:
            graph.use_graph = False         # the replay-mode step with every launch from Python: the launches the graph holds
    nxt = out.logits[:, -1].argmax(-1, keepdim=True)
    toks = [nxt]

    def one(s, nxt, past):
        if beams:
            bi = beam_idx_for(s, rows, dev)
            nxt = nxt.index_select(0, bi)
            if path == "default":
                past = tuple(tuple(t.index_select(0, bi) for t in layer) for layer in past)
            else:
                cache.reorder(bi)
        if path == "graph":
            lg = graph(nxt)
        else:
            o = model(input_ids=nxt, past_key_values=past, use_cache=True)
            past, lg = o.past_key_values, o.logits[:, -1]
        return lg.argmax(-1, keepdim=True), past

    try:
        if count_launches:
            from torch.profiler import ProfilerActivity, profile

            for s in range(3):              # (past the warm-up steps of the graph path's bookkeeping)
                nxt, past = one(s, nxt, past)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for s in range(3, 3 + count_launches):
                    nxt, past = one(s, nxt, past)
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                    and "memset" not in e.name.lower())
            return n / count_launches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            nxt, past = one(s, nxt, past)
            toks.append(nxt)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        cap = graph.capture_seconds if graph is not None else 0.0
        if graph is not None:
            assert (graph.captures, graph.replays) == (1, steps - 2), (graph.captures, graph.replays)
        return (sec - cap) * 1e3 / steps, cap * 1e3, torch.cat(toks, 1)[:, :steps].cpu()
    finally:
        if graph is not None:
            graph.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--prompt", type=int, default=1350)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fuyu_static_decode_bench: no GPU visible (this tool measures; it has no CPU mode)")
    if a.rounds < 3:
        raise SystemExit("fuyu_static_decode_bench: at least three rounds (the spread over rounds is part of the result)")
    from otter_amd.kv_cache import StaticKVCache

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def write_out():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    dev = torch.cuda.get_device_properties(0)
    say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
    say("model: Persimmon at Fuyu-8B shape, %d layers, vocabulary %d, bf16, random init; prompt %d tokens; %d greedy cached steps; paths: "
        "default (tuple cache) | static (StaticKVCache as past_key_values) | graph (static + graph replay, capture taken out)"
        % (a.layers, VOCAB, a.prompt, a.steps))
    plain = build_model(a.layers)
    int8 = copy.deepcopy(plain)
    int8.quantize_decoder_int8()
    gc.collect()
    torch.cuda.empty_cache()
    models = {"bf16": plain, "int8": int8}
    result, misses, n_points = {}, 0, 0
    g = torch.Generator().manual_seed(1)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for name, rows, beams in POINTS:
        ids = torch.randint(0, VOCAB, (1 if beams else rows, a.prompt), generator=g).cuda()
        if beams:
            ids = ids.repeat_interleave(rows, dim=0)
        for quant, model in models.items():
            tag = "%s %s" % (name, quant)
            cache = StaticKVCache.for_model(model, rows=rows, max_len=a.prompt + a.steps + 1)
            gc.collect()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            tok, peak = {}, {}
            for p in PATHS:                  # warm-up (allocator, library handles, kernel loads, workspaces) + tokens + peak memory
                torch.cuda.reset_peak_memory_stats()
                _, _, tok[p] = decode(model, p, ids, a.steps, beams, cache)
                peak[p] = torch.cuda.max_memory_allocated() - base + (0 if p == "default" else cache.nbytes())
            t, caps = {p: [] for p in PATHS}, []
            for r in range(a.rounds):
                for p in PATHS:
                    ms, cap, out = decode(model, p, ids, a.steps, beams, cache)
                    t[p].append(ms)
                    if p == "graph":
                        caps.append(cap)
                    say("%s round %d %-7s %.3f ms/step%s" % (tag, r, p, ms, " (capture %.1f ms taken out)" % cap if p == "graph" else ""))
                    if not torch.equal(out, tok[p]):
                        say("NOTE: %s round %d %s: tokens differ from the path's own first run" % (tag, r, p))
            m = {p: med(v) for p, v in t.items()}
            spread = {p: (max(v) - min(v)) / m[p] for p, v in t.items()}
            part = {}
            for p in ("static", "graph"):
                d = (tok[p] != tok["default"]).any(0).nonzero()
                part[p] = int(d[0]) if len(d) else None
            launches = {}
            if not a.no_launch_count:
                for p in PATHS:
                    try:
                        launches[p] = decode(model, p, ids, a.steps, beams, cache, count_launches=4)
                    except Exception as e:      # (a profiler that does not work here is not a result)
                        launches[p] = None
                        say("NOTE: %s %s: launches not counted (%s: %s)" % (tag, p, type(e).__name__, str(e)[:120]))
            ratio = {p: m[p] / m["default"] for p in ("static", "graph")}
            say("%s: median ms per cached step default %.3f (spread %.2f%%) | static %.3f (%.2f%%) = x%.3f | graph %.3f (%.2f%%) = x%.3f of default "
                "(condition <= %.2f); capture %.1f ms; launches per step %s; peak memory above the models (cache included) %s MB; tokens first part "
                "from the default cache's at step: %s"
                % (tag, m["default"], 100 * spread["default"], m["static"], 100 * spread["static"], ratio["static"], m["graph"],
                   100 * spread["graph"], ratio["graph"], THRESHOLD, med(caps), json.dumps(launches),
                   json.dumps({p: round(v / 1e6, 1) for p, v in peak.items()}), json.dumps(part)))
            for p in ("static", "graph"):
                n_points += 1
                if ratio[p] > THRESHOLD:
                    misses += 1
                    say("MISS: %s: the %s step is more than %.0f %% slower than the default-cache step" % (tag, p, (THRESHOLD - 1) * 100))
            result[tag] = {"ms_per_step": t, "median": m, "spread": spread, "over_default": ratio, "capture_ms": caps, "launches_per_step": launches,
                           "peak_bytes_above_models": peak, "tokens_first_part": part}
            del cache
            write_out()
    say("comparisons with a MISS: %d of %d" % (misses, n_points))
    say(json.dumps(result))
    write_out()


if __name__ == "__main__":
    main()
