"""The int8 gated-block FFNs and un-embedding (quantize_decoder_int8(gated_blocks=True, lm_head=True)), measured
twice: the two products alone against the bf16 products they replace, and the whole cached step of OTTER-MPT7B against the plain int8
configuration.

Kernel alone (--kernels).  (N, K) = (4096, 16384), the second FFN product with its tanh-gate residual tail (otter_gemv_w8_gated /
otter_gemm_w8_rows_gated against ops.gemm_nt with EPI_SCALE_RES on the bf16 weight), and (16384, 4096), the first with its GELU
(otter_gemv_w8 / otter_gemm_w8_rows with act 1 against ops.gemm_nt with EPI_GELU), at M in {1, 4, 24, 64}.  Cold weights: every timed call
reads its own copy of the weight out of a ring of copies larger than the 256 MB Infinity Cache, as a step of the model reads each weight
once.  Device events around ITERS calls, the median of --rounds alternating rounds, us per call.

Whole step (--steps).  Full 32-layer OTTER-MPT7B with synthetic weights (bench.build_model), a 512-token prompt, static KV cache +
cross-attention cache + graph replay; `quantize_decoder_int8()` against `quantize_decoder_int8(gated_blocks=True, lm_head=True)`, both
models resident and alternated in one process.  Points: B = 1 and B = 4 greedy, B = 8 x 3 beams.  ms per step = (t[NEW] - t[1] - capture) /
(NEW - 1) of whole generate() calls (tools/graph_decode_bench.py: timed_generate), the median and the spread (max - min) of --rounds
rounds; torch.cuda.memory_allocated() after each model is built; the first position at which the two configurations' greedy tokens part.
Condition, per point: the new configuration's step <= 1.03 x the plain int8 configuration's; a point that misses prints MISS.

  python tools/w8_gated_decode_bench.py [--kernels] [--steps] [--rounds 3] [--new 64] [--prompt 512] [--layers 32] [--out profiles/r21_w8_gated_ab.txt]"""
from __future__ import annotations

import argparse
import copy
import gc
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.graph_decode_bench import THRESHOLD, mode_kwargs, timed_generate  # noqa: E402

KERNEL_SHAPES = [("FF down + gate residual", 4096, 16384), ("FF up + GELU", 16384, 4096)]
KERNEL_MS = (1, 4, 24, 64)
ITERS = 40
RING_BYTES = 768 << 20                      # of weight copies per contender: three times the Infinity Cache
CASES = [("B=1 greedy", 1, {}), ("B=4 greedy", 4, {}), ("B=8 x 3 beams", 8, dict(num_beams=3))]

med = lambda xs: sorted(xs)[len(xs) // 2]


def kernels(a, say):
    from otter_amd import functional as OF
    from otter_amd import ops
    from otter_amd.quant import quantize_weight_int8

    dev, result = "cuda:0", {}
    for tag, N, K in KERNEL_SHAPES:
        g = torch.Generator(device=dev).manual_seed(N + K)
        w = torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)
        q, scale = quantize_weight_int8(w)
        n8, n16 = max(2, RING_BYTES // (N * K)), max(2, RING_BYTES // (2 * N * K))
        q_ring = [q.clone() for _ in range(n8)]
        w_ring = [w.to(torch.bfloat16) for _ in range(n16)]
        gate = torch.tensor([0.7], device=dev)
        down = N < K
        for M in KERNEL_MS:
            x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            R = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
            y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            if down:
                i8 = ops.gemv_w8_gated if M <= 16 else ops.gemm_w8_rows_gated
                run8 = lambda i: i8(x, q_ring[i % n8], scale, gate, R, out=y)
                run16 = lambda i: ops.gemm_nt(x, w_ring[i % n16], out=y, kind=OF.EPI_SCALE_RES, gate=gate, R=R)
            else:
                i8 = ops.gemv_w8 if M <= 16 else ops.gemm_w8_rows
                run8 = lambda i: i8(x, q_ring[i % n8], scale, None, 1, out=y)
                run16 = lambda i: ops.gemm_nt(x, w_ring[i % n16], out=y, kind=OF.EPI_GELU)

            def timed(run):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(ITERS):
                    run(i)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / ITERS * 1e3

            for run in (run8, run16):                       # warm-up: code objects, workspaces
                run(0)
            t = {"int8": [], "bf16": []}
            for _ in range(a.rounds):
                t["int8"].append(timed(run8))
                t["bf16"].append(timed(run16))
            us = {k: med(v) for k, v in t.items()}
            say("%-24s N=%5d K=%5d M=%2d: int8 %7.1f us (%.0f GB/s of int8 weight) | bf16 %7.1f us (%.0f GB/s of bf16 weight) | int8 = x%.2f of bf16" % (
                tag, N, K, M, us["int8"], N * K / us["int8"] / 1e3, us["bf16"], 2 * N * K / us["bf16"] / 1e3, us["int8"] / us["bf16"]))
            result["%s M=%d" % (tag, M)] = {"us": us, "all": t}
        del q_ring, w_ring
        gc.collect()
        torch.cuda.empty_cache()
    return result


def steps(a, say):
    import bench

    base = torch.cuda.memory_allocated()
    plain = bench.build_model("cuda:0", seed=0, debug_layers=0 if a.layers == 32 else a.layers).eval()
    full = copy.deepcopy(plain)
    say("quantize_decoder_int8(): %s" % json.dumps(plain.quantize_decoder_int8()))
    say("quantize_decoder_int8(gated_blocks=True, lm_head=True): %s" % json.dumps(full.quantize_decoder_int8(gated_blocks=True, lm_head=True)))
    gc.collect()
    torch.cuda.empty_cache()
    mem = {}
    for who, m in (("int8", plain), ("int8+gated+head", full)):
        mem[who] = sum(t.numel() * t.element_size() for t in list(m.parameters()) + list(m.buffers()))
    say("parameters + buffers: int8 %.3f GB | int8+gated+head %.3f GB (both resident: %.3f GB allocated)" % (
        mem["int8"] / 1e9, mem["int8+gated+head"] / 1e9, (torch.cuda.memory_allocated() - base) / 1e9))
    models = {"int8": plain, "int8+gated+head": full}
    kw = mode_kwargs("graph")
    result, misses = {"memory_bytes": mem}, 0
    for tag, B, extra in CASES:
        vx, ids, _, _, _ = bench.synth_batch(plain, B, a.prompt, "cuda:0", seed=17)
        vx = vx.to(torch.bfloat16)
        k = dict(kw, **extra)
        toks = {}
        for who, m in models.items():                       # warm-up: allocator, kernel loads, workspaces
            toks[who] = timed_generate(m, vx, ids, 4, k)[2]
        t = {who: [] for who in models}
        for r in range(a.rounds):
            for who, m in models.items():
                s1, c1, _ = timed_generate(m, vx, ids, 1, k)
                s, cap, toks[who] = timed_generate(m, vx, ids, a.new, k)
                t[who].append((s - cap - (s1 - c1)) / (a.new - 1) * 1e3)
                say("%s round %d %-16s %.1f ms for %d new tokens (1 new token: %.1f ms; capture %.1f ms)" % (tag, r, who, s * 1e3, a.new, s1 * 1e3, cap * 1e3))
        step = {who: med(v) for who, v in t.items()}
        spread = {who: max(v) - min(v) for who, v in t.items()}
        ratio = step["int8+gated+head"] / step["int8"]
        differ = (toks["int8"][:, a.prompt:] != toks["int8+gated+head"][:, a.prompt:]).any(dim=0).nonzero()
        first = int(differ[0]) if differ.numel() else None
        say("%s: median ms per step int8 %.3f (spread %.3f) | int8+gated+head %.3f (spread %.3f) = x%.3f of int8 (condition <= %.2f); "
            "tokens first part at new token %s of %d" % (tag, step["int8"], spread["int8"], step["int8+gated+head"], spread["int8+gated+head"],
                                                          ratio, THRESHOLD, first, a.new))
        if ratio > THRESHOLD:
            misses += 1
            say("MISS: %s: the new configuration's step is more than %.0f %% slower than the plain int8 step" % (tag, (THRESHOLD - 1) * 100))
        result[tag] = {"ms_per_step": step, "spread": spread, "all": t, "tokens_first_part": first}
    say("conditions missed: %d of %d" % (misses, len(CASES)))
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w8_gated_decode_bench: no GPU visible (this tool measures; it has no CPU mode)")
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
    result = {}
    both = not (a.kernels or a.steps)
    with torch.no_grad():
        if a.kernels or both:
            say("kernel alone: cold weights (a ring of %d MB of copies per contender), bf16 x / R / y, gate 0.7; us per call, device events around %d "
                "calls, median of %d rounds" % (RING_BYTES >> 20, ITERS, a.rounds))
            result["kernels"] = kernels(a, say)
        if a.steps or both:
            say("whole step: OTTER-MPT7B shape, %d decoder layers, synthetic weights, bf16 autocast; 1 image per sentence; prompt %d; no end token; %d "
                "new tokens; static KV cache + media cache + graph replay; times are whole generate() calls" % (a.layers, a.prompt, a.new))
            result["steps"] = steps(a, say)
    say(json.dumps(result))


if __name__ == "__main__":
    main()
