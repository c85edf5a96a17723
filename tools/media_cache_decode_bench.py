"""Cached generation that sees the image, at OTTER-MPT7B shape: generate(cross_attention_cache=True) (otter_amd/media_cache.py,
csrc/xattn_decode.hip) against the legacy cached step (which ignores the image after the prompt and still projects the media and runs the
64-row-tile attention kernel in every gated block) and against use_cache=False (the full re-forward, the only path that attended to the image
before), alternated in one process.

Full 32-layer OTTER-MPT7B with synthetic weights (bench.build_model: frozen weights bf16, trainable ones fp32, bf16 autocast -- the
production mode), one 224 x 224 image per sentence.  Every timing is a whole `model.generate` call (vision encoder, prompt pass, NEW tokens,
no end token); the same call with ONE new token is timed too, and (t[NEW] - t[1]) / (NEW - 1) is the cost of one step.  The re-forward mode
runs --new-full tokens (it is quadratic; its step is the mean over a shorter run).  Clock: torch.cuda.synchronize() + perf_counter; one
warm-up call per mode and case; the median of ROUNDS alternating rounds and the spread (max - min) between the rounds of the same mode.
Condition: ms per step with the media cache <= 1.03 x the legacy cached step of the same process and cache implementation (3 %: the
box-noise threshold of tools/regress.sh); a case that misses prints MISS.  The ratio to use_cache=False is recorded, not judged.

  python tools/media_cache_decode_bench.py [--rounds 3] [--new 64] [--new-full 8] [--prompt 512] [--layers 32] [--out profiles/r10_media_cache_ab.txt]"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

CACHES = {"tuple": dict(use_cache=True), "static": dict(cache_implementation="static")}
MODES = ("legacy", "media", "reforward")
THRESHOLD = 1.03


def mode_kwargs(mode, cache):
    if mode == "reforward":
        return dict(use_cache=False)
    return dict(CACHES[cache], cross_attention_cache=(mode == "media"))


@torch.no_grad()
def timed_generate(model, vx, ids, new, kw):
    """(seconds, tokens) of one generate call."""
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        toks = model.generate(vision_x=vx, lang_x=ids, max_new_tokens=new, eos_token_id=-1, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, toks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--new-full", type=int, default=8)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("media_cache_decode_bench: no GPU visible (this tool measures; it has no CPU mode)")
    import bench

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.cuda.get_device_properties(0)
    say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
    say("model: OTTER-MPT7B shape, %d decoder layers, synthetic weights, bf16 autocast; 1 image per sentence; prompt %d; greedy, no end token; "
        "%d new tokens (re-forward: %d); times are whole generate() calls" % (a.layers, a.prompt, a.new, a.new_full))
    model = bench.build_model("cuda:0", seed=0, debug_layers=0 if a.layers == 32 else a.layers).eval()
    result, misses = {}, 0
    for B in a.batches:
        vx, ids, _, _, _ = bench.synth_batch(model, B, a.prompt, "cuda:0", seed=17)
        vx = vx.to(torch.bfloat16)
        for cache in CACHES:
            tag = "prompt=%d B=%d %s" % (a.prompt, B, cache)
            new = {m: (a.new_full if m == "reforward" else a.new) for m in MODES}
            for m in MODES:                              # warm-up: allocator, kernel loads, workspaces
                timed_generate(model, vx, ids, 3, mode_kwargs(m, cache))
            t = {m: {"full": [], "one": []} for m in MODES}
            toks = {}
            for r in range(a.rounds):
                for m in MODES:
                    s1, _ = timed_generate(model, vx, ids, 1, mode_kwargs(m, cache))
                    s, out = timed_generate(model, vx, ids, new[m], mode_kwargs(m, cache))
                    t[m]["full"].append(s)
                    t[m]["one"].append(s1)
                    toks.setdefault(m, out.cpu())
                    say("%s round %d %-9s %.1f ms for %d new tokens (1 new token: %.1f ms)" % (tag, r, m, s * 1e3, new[m], s1 * 1e3))
            med = {m: sorted(t[m]["full"])[len(t[m]["full"]) // 2] for m in MODES}
            med1 = {m: sorted(t[m]["one"])[len(t[m]["one"]) // 2] for m in MODES}
            spread = {m: max(t[m]["full"]) - min(t[m]["full"]) for m in MODES}
            step = {m: (med[m] - med1[m]) / max(new[m] - 1, 1) * 1e3 for m in MODES}
            nf = a.new_full
            eq_full = bool((toks["media"][:, :a.prompt + nf] == toks["reforward"]).all())
            eq_legacy = bool((toks["legacy"][:, :a.prompt + nf] == toks["reforward"]).all())
            ratio = step["media"] / step["legacy"]
            say("%s: ms per step legacy %.3f, media cache %.3f (x%.3f of legacy; condition <= %.2f), re-forward %.3f (media cache is x%.3f of it); "
                "spread between rounds of whole calls legacy %.1f ms, media %.1f ms, re-forward %.1f ms; first %d new tokens equal to the re-forward's: "
                "media cache %s, legacy %s" % (tag, step["legacy"], step["media"], ratio, THRESHOLD, step["reforward"], step["media"] / step["reforward"],
                                                spread["legacy"] * 1e3, spread["media"] * 1e3, spread["reforward"] * 1e3, nf, eq_full, eq_legacy))
            if ratio > THRESHOLD:
                misses += 1
                say("MISS: %s: the media-cache step is more than %.0f %% slower than the legacy cached step" % (tag, (THRESHOLD - 1) * 100))
            result[tag] = {"seconds": {m: t[m]["full"] for m in MODES}, "seconds_one_token": {m: t[m]["one"] for m in MODES}, "ms_per_step": step,
                           "media_over_legacy": ratio, "media_over_reforward": step["media"] / step["reforward"],
                           "tokens_equal_to_reforward": {"media": eq_full, "legacy": eq_legacy}}
    say("cases with a MISS: %d of %d" % (misses, len(result)))
    say(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
