"""Cached generation at OTTER-MPT7B shape: generate(cache_implementation="static") (otter_amd/kv_cache.py, csrc/decode_cache.hip) against the
legacy growing cache (two torch.cat per layer per step, index_select of every cache tensor under beam search), alternated in one process.

Full 32-layer OTTER-MPT7B with synthetic weights (bench.build_model: frozen weights bf16, trainable ones fp32, bf16 autocast -- the
production mode), one 224 x 224 image per sentence.  Every timing is a whole `model.generate` call (vision encoder, prompt pass, NEW tokens,
no end token), so the beam reorder and the cache allocation are inside the clock; the same call with ONE new token is timed too, and
(t[NEW] - t[1]) / (NEW - 1) is the cost of one cached step.  Clock: torch.cuda.synchronize() + perf_counter; one warm-up call per path and
case; the median of ROUNDS alternating rounds, the spread (max - min) between the rounds of the same path, and
torch.cuda.max_memory_allocated() of a call above what was allocated before it.  A case prints MISS when the static path's median is slower
than the legacy median by more than the spread between the legacy path's own rounds.  Cases: greedy at B = 1 and 4, num_beams = 3 at B = 1;
prompts of 512 and 1536 tokens; the unquantised and the int8 decoder.

  python tools/kv_cache_decode_bench.py [--rounds 3] [--new 64] [--prompts 512 1536] [--layers 32] [--no-int8] [--out profiles/r09_static_cache_ab.txt]
  python tools/kv_cache_decode_bench.py --trace-one static|legacy [--beams 3]    (one warm call + one call, for rocprofv3 --kernel-trace --stats)"""
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

PATHS = {"static": dict(cache_implementation="static"), "legacy": dict(use_cache=True)}


@torch.no_grad()
def timed_generate(model, vx, ids, new, beams, path):
    """(seconds, peak bytes above the start, tokens) of one generate call."""
    kw = dict(PATHS[path], max_new_tokens=new, eos_token_id=-1)
    if beams > 1:
        kw["num_beams"] = beams
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        toks = model.generate(vision_x=vx, lang_x=ids, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base, toks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--prompts", type=int, nargs="+", default=[512, 1536])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--no-int8", action="store_true")
    ap.add_argument("--trace-one", choices=list(PATHS), default=None)
    ap.add_argument("--beams", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_cache_decode_bench: no GPU visible (this tool measures; it has no CPU mode)")
    import bench

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.cuda.get_device_properties(0)
    say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
    say("model: OTTER-MPT7B shape, %d decoder layers, synthetic weights, bf16 autocast; 1 image per sentence; %d new tokens, no end token; "
        "times are whole generate() calls" % (a.layers, a.new))
    plain = bench.build_model("cuda:0", seed=0, debug_layers=0 if a.layers == 32 else a.layers).eval()
    if a.trace_one:
        vx, ids, _, _, _ = bench.synth_batch(plain, 1, a.prompts[0], "cuda:0", seed=17)
        for _ in range(2):
            s, _, _ = timed_generate(plain, vx.to(torch.bfloat16), ids, a.new, a.beams, a.trace_one)
        say("trace-one %s beams=%d prompt=%d: %.3f s for %d new tokens" % (a.trace_one, a.beams, a.prompts[0], s, a.new))
        return
    models = {"bf16": plain}
    if not a.no_int8:
        models["int8"] = copy.deepcopy(plain)
        models["int8"].quantize_decoder_int8()
    result, misses = {}, 0
    for wname, model in models.items():
        for prompt in a.prompts:
            for B, beams in ((1, 1), (4, 1), (1, 3)):
                vx, ids, _, _, _ = bench.synth_batch(plain, B, prompt, "cuda:0", seed=17)
                vx = vx.to(torch.bfloat16)
                tag = "%s prompt=%d B=%d beams=%d" % (wname, prompt, B, beams)
                for p in PATHS:                          # warm-up: allocator, kernel loads, workspaces
                    timed_generate(model, vx, ids, 4, beams, p)
                t = {p: {"full": [], "one": [], "peak": 0} for p in PATHS}
                toks = {}
                for r in range(a.rounds):
                    for p in PATHS:
                        s1, _, _ = timed_generate(model, vx, ids, 1, beams, p)
                        s, peak, out = timed_generate(model, vx, ids, a.new, beams, p)
                        t[p]["full"].append(s)
                        t[p]["one"].append(s1)
                        t[p]["peak"] = max(t[p]["peak"], peak)
                        toks.setdefault(p, out.cpu())
                        say("%s round %d %-6s %.1f ms (1 new token: %.1f ms)" % (tag, r, p, s * 1e3, s1 * 1e3))
                med = {p: sorted(t[p]["full"])[len(t[p]["full"]) // 2] for p in PATHS}
                med1 = {p: sorted(t[p]["one"])[len(t[p]["one"]) // 2] for p in PATHS}
                spread = {p: max(t[p]["full"]) - min(t[p]["full"]) for p in PATHS}
                step = {p: (med[p] - med1[p]) / max(a.new - 1, 1) for p in PATHS}
                same = toks["static"].shape == toks["legacy"].shape and bool((toks["static"] == toks["legacy"]).all())
                n_eq = 0
                if toks["static"].shape == toks["legacy"].shape:
                    eq = (toks["static"] == toks["legacy"]).all(dim=0).tolist()
                    n_eq = eq.index(False) if False in eq else len(eq)
                say("%s median: static %.1f ms, legacy %.1f ms (x%.3f); spread between rounds static %.1f ms, legacy %.1f ms; per cached step static "
                    "%.3f ms, legacy %.3f ms; peak memory above the model static %.3f GB, legacy %.3f GB; tokens equal: %s (first %d columns of %d)" % (
                        tag, med["static"] * 1e3, med["legacy"] * 1e3, med["legacy"] / med["static"], spread["static"] * 1e3, spread["legacy"] * 1e3,
                        step["static"] * 1e3, step["legacy"] * 1e3, t["static"]["peak"] / 1e9, t["legacy"]["peak"] / 1e9, same, n_eq,
                        toks["legacy"].shape[1]))
                if med["static"] > med["legacy"] + spread["legacy"]:
                    misses += 1
                    say("MISS: %s: the static path is slower than the legacy path by more than the legacy path's own spread" % tag)
                result[tag] = {"seconds": {p: t[p]["full"] for p in PATHS}, "seconds_one_token": {p: t[p]["one"] for p in PATHS}, "median": med,
                               "spread": spread, "ms_per_step": {p: step[p] * 1e3 for p in PATHS}, "peak_bytes": {p: t[p]["peak"] for p in PATHS},
                               "tokens_equal": same}
    say("cases with a MISS: %d of %d" % (misses, len(result)))
    say(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
