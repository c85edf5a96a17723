"""Whole cached step of the int8 OTTER-MPT7B at 72 to 192 rows with and without `wide_steps` (the panel kernel of csrc/w8_panel.hip against
the dequantising route).

Full 32-layer OTTER-MPT7B with synthetic weights (bench.build_model), `quantize_decoder_int8(gated_blocks=True, lm_head=True)`, static KV
cache + cross-attention cache + graph replay, 3 beams, a 512-token prompt, 64 new tokens.  Contenders, alternated in one process on ONE
int8 model: `panel_rows` set to `quant.PANEL_MAX_ROWS` on every Int8FrozenLinear (what `wide_steps=True` does: "on") against 0 ("off"); the
unquantised model, for information.  Points: 24, 32 and 64 sentences (72, 96 and 192 rows); --kv int8 runs the KV cache in int8 where the bf16
cache does not fit.  ms per generated position = (t[NEW] - t[1] - capture) / (NEW - 1) of whole generate() calls
(tools/graph_decode_bench.py: timed_generate), the median and the spread (max - min) of --rounds rounds; tokens per second = sentences /
that.  Condition, per point: on <= 1.03 x off; a point that misses prints MISS.

  python tools/w8_panel_decode_bench.py [--sentences 24 32 64] [--rounds 3] [--new 64] [--prompt 512] [--layers 32] [--kv bf16|int8]
                                        [--no-bf16] [--out profiles/r23_w8_panel_decode_ab.txt]"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.graph_decode_bench import THRESHOLD, mode_kwargs, timed_generate  # noqa: E402

BEAMS = 3
med = lambda xs: sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, nargs="+", default=[24, 32, 64])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--kv", choices=["bf16", "int8"], default="bf16")
    ap.add_argument("--no-bf16", action="store_true", help="leave out the unquantised model")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w8_panel_decode_bench: no GPU visible (this tool measures; it has no CPU mode)")
    import bench
    from otter_amd.quant import PANEL_MAX_ROWS, set_wide_steps

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    dev = torch.cuda.get_device_properties(0)
    say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
    say("OTTER-MPT7B shape, %d decoder layers, synthetic weights, bf16 autocast; 1 image per sentence; %d beams; prompt %d; no end token; %d new "
        "tokens; static KV cache (%s) + media cache + graph replay; PANEL_MAX_ROWS = %d; times are whole generate() calls" % (
            a.layers, BEAMS, a.prompt, a.new, a.kv, PANEL_MAX_ROWS))
    with torch.no_grad():
        q = bench.build_model("cuda:0", seed=0, debug_layers=0 if a.layers == 32 else a.layers).eval()
        models = {}
        if not a.no_bf16:
            import copy

            models["bf16"] = copy.deepcopy(q)
        say("quantize_decoder_int8(gated_blocks=True, lm_head=True, wide_steps=True): %s" % json.dumps(
            q.quantize_decoder_int8(gated_blocks=True, lm_head=True, wide_steps=True)))
        gc.collect()
        torch.cuda.empty_cache()
        models["off"] = models["on"] = q
        kw = dict(mode_kwargs("graph"), num_beams=BEAMS)
        if a.kv == "int8":
            kw["kv_cache_dtype"] = "int8"
        result, misses = {}, 0
        for B in a.sentences:
            tag = "%d sentences x %d beams (%d rows)" % (B, BEAMS, B * BEAMS)
            vx, ids, _, _, _ = bench.synth_batch(q, B, a.prompt, "cuda:0", seed=17)
            vx = vx.to(torch.bfloat16)

            def run(who, new):
                if who != "bf16":
                    set_wide_steps(q, PANEL_MAX_ROWS if who == "on" else 0)
                return timed_generate(models[who], vx, ids, new, kw)

            toks = {}
            for _ in range(2):                                      # warm-up, twice: allocator, kernel loads, workspaces, and the library's
                for who in models:                                  # choice of algorithm for this point's prompt pass (the step time below is
                    run(who, 1)                                     # a difference of two calls that must spend the same time in it)
                    toks[who] = run(who, 4)[2]
            t = {who: [] for who in models}
            for r in range(a.rounds):
                for who in models:
                    s1, c1, _ = run(who, 1)
                    s, cap, toks[who] = run(who, a.new)
                    t[who].append((s - cap - (s1 - c1)) / (a.new - 1) * 1e3)
                    say("%s round %d %-4s %.1f ms for %d new tokens (1 new token: %.1f ms; capture %.1f ms)" % (tag, r, who, s * 1e3, a.new, s1 * 1e3,
                                                                                                              cap * 1e3))
            step = {who: med(v) for who, v in t.items()}
            spread = {who: max(v) - min(v) for who, v in t.items()}
            ratio = step["on"] / step["off"]
            differ = (toks["on"][:, a.prompt:] != toks["off"][:, a.prompt:]).any(dim=0).nonzero()
            first = int(differ[0]) if differ.numel() else None
            say("%s: median ms per generated position %s = on x%.3f of off (condition <= %.2f); sentence-tokens per second %s; beam tokens of on / "
                "off first part at new token %s of %d" % (
                    tag, " | ".join("%s %.3f (spread %.3f)" % (w, step[w], spread[w]) for w in models), ratio, THRESHOLD,
                    " | ".join("%s %.0f" % (w, B / step[w] * 1e3) for w in models), first, a.new))
            if ratio > THRESHOLD:
                misses += 1
                say("MISS: %s: wide_steps on is more than %.0f %% slower than off" % (tag, (THRESHOLD - 1) * 100))
            result[tag] = {"ms_per_position": step, "spread": spread, "all": t, "tokens_first_part": first}
            del vx, ids, toks
            gc.collect()
            torch.cuda.empty_cache()
        say("conditions missed: %d of %d" % (misses, len(a.sentences)))
    say(json.dumps(result))


if __name__ == "__main__":
    main()
