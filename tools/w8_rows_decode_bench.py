"""The cached step of the int8 decoder at 17 to 64 rows, at OTTER-MPT7B shape: int8 on otter_gemm_w8_rows against the int8 step that
dequantises every weight (OTTER_W8_ROWS=0: the step before that kernel existed) and against the unquantised model, alternated in one
process.

Full 32-layer OTTER-MPT7B with synthetic weights (bench.build_model: frozen weights bf16, trainable ones fp32, bf16 autocast) and a copy of
it after quantize_decoder_int8(); one 224 x 224 image per sentence, a 512-token prompt, no end token, static KV cache + cross-attention
cache; eager and graph_decode=True.  Row counts: 24 (8 sentences x num_beams=3), 32 and 64 (greedy).  Every timing is a whole
`model.generate` call; the same call with ONE new token (the prompt pass alone) is timed too.  ms per step = (t[NEW] - t[1] - capture) /
(NEW - 1), where `capture` is the one-off cost of capturing the step (0 for the eager path).  Clock: torch.cuda.synchronize() +
perf_counter; one warm-up call per contender and mode; the median of ROUNDS alternating rounds.
Conditions, per row count and mode: rows < dequant, and rows <= 1.03 x bf16 (3 %: the pool's box-to-box and run-to-run spread); a case
that misses prints MISS.

  python tools/w8_rows_decode_bench.py [--rounds 3] [--new 64] [--prompt 512] [--layers 32] [--out profiles/r12_w8_rows_decode_ab.txt]"""
from __future__ import annotations

import argparse
import copy
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.graph_decode_bench import MODES, THRESHOLD, mode_kwargs, timed_generate  # noqa: E402

CASES = [("24 rows (8 x 3 beams)", 8, dict(num_beams=3)), ("32 rows", 32, {}), ("64 rows", 64, {})]
CONTENDERS = ("rows", "dequant", "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w8_rows_decode_bench: no GPU visible (this tool measures; it has no CPU mode)")
    import bench

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
    say("model: OTTER-MPT7B shape, %d decoder layers, synthetic weights, bf16 autocast; 1 image per sentence; prompt %d; no end token; %d new "
        "tokens; static KV cache + media cache; times are whole generate() calls" % (a.layers, a.prompt, a.new))
    plain = bench.build_model("cuda:0", seed=0, debug_layers=0 if a.layers == 32 else a.layers).eval()
    quant = copy.deepcopy(plain)
    quant.quantize_decoder_int8()
    gc.collect()
    torch.cuda.empty_cache()

    def run(who, vx, ids, new, kw):
        os.environ["OTTER_W8_ROWS"] = "0" if who == "dequant" else "1"
        try:
            return timed_generate(plain if who == "bf16" else quant, vx, ids, new, kw)
        finally:
            os.environ.pop("OTTER_W8_ROWS", None)

    result, misses = {}, 0
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for tag, B, extra in CASES:
        vx, ids, _, _, _ = bench.synth_batch(plain, B, a.prompt, "cuda:0", seed=17)
        vx = vx.to(torch.bfloat16)
        for m in MODES:
            kw = dict(mode_kwargs(m), **extra)
            for who in CONTENDERS:                          # warm-up: allocator, kernel loads, workspaces
                run(who, vx, ids, 4, kw)
            t = {who: [] for who in CONTENDERS}
            for r in range(a.rounds):
                for who in CONTENDERS:
                    s1, c1, _ = run(who, vx, ids, 1, kw)
                    s, cap, _ = run(who, vx, ids, a.new, kw)
                    t[who].append((s - cap - (s1 - c1)) / (a.new - 1) * 1e3)
                    say("%s %-5s round %d %-7s %.1f ms for %d new tokens (1 new token: %.1f ms; capture %.1f ms)" % (
                        tag, m, r, who, s * 1e3, a.new, s1 * 1e3, cap * 1e3))
            step = {who: med(t[who]) for who in CONTENDERS}
            say("%s %-5s: median ms per step int8 rows %.3f | int8 dequant %.3f (x%.2f of rows) | bf16 %.3f (rows = x%.3f of bf16; condition <= %.2f)" % (
                tag, m, step["rows"], step["dequant"], step["dequant"] / step["rows"], step["bf16"], step["rows"] / step["bf16"], THRESHOLD))
            if step["rows"] >= step["dequant"]:
                misses += 1
                say("MISS: %s %s: the rows step is not faster than the dequantising step" % (tag, m))
            if step["rows"] > THRESHOLD * step["bf16"]:
                misses += 1
                say("MISS: %s %s: the rows step is more than %.0f %% slower than the unquantised step" % (tag, m, (THRESHOLD - 1) * 100))
            result["%s %s" % (tag, m)] = {"ms_per_step": step, "all": t}
            write_out()
    say("conditions missed: %d of %d" % (misses, 2 * len(result)))
    say(json.dumps(result))
    write_out()


if __name__ == "__main__":
    main()
