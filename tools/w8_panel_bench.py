"""otter_gemm_w8_panel (csrc/w8_panel.hip) at the decode shapes of MPT-7B and 72 to 256 rows: microseconds per call on COLD weights, against
what a one-token step of that many rows could run instead, and the dispatch threshold that follows.

For each of the four decoder shapes (N, K) and M in {72, 96, 128, 192, 256}, four contenders in the same process, in alternating rounds:
  (a) dequant  ops.dequant_w8 into one bf16 scratch, then F.linear on it, then the activation pass (the GELU of up_proj): the step without
               `wide_steps`;
  (b) rows     ceil(M / 64) slices of ops.gemm_w8_rows (each streams the whole weight);
  (c) bf16     F.linear on the bf16 weight (+ the activation pass): the unquantised layer, for information;
  (d) panel    ops.gemm_w8_panel on the int8 weight (the Python wrapper the model calls, its checks and workspace look-up included).
A decode step never sees a warm weight, so every call of a round reads a DIFFERENT weight buffer: enough distinct buffers that their total
exceeds the 256 MB last-level cache (the bf16 set and the int8 set are each sized that way).  Clock: one pair of hipEvents around LAUNCHES
back-to-back calls, after a warm-up pass over every buffer; median and spread (max - min) of ROUNDS rounds.  Bytes per call = N K + 4 N (the
int8 weight and its scales); the fraction is of the 8 TB/s nominal HBM bandwidth.
Threshold: the largest measured M such that at it and at every smaller measured M, on all four shapes, (d) <= 1.03 x min((a), (b)); 64 if
that already fails at 72 rows.

  python tools/w8_panel_bench.py [--launches 48] [--rounds 3] [--out profiles/r23_w8_panel.txt]"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [("Wqkv", 12288, 4096, 0), ("out_proj", 4096, 4096, 0), ("up_proj", 16384, 4096, 1), ("down_proj", 4096, 16384, 0)]     # (.., act)
MS = [72, 96, 128, 192, 256]
NOMINAL = 8.0e12
LLC = 256 << 20
MARGIN = 1.03


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w8_panel_bench: no GPU visible (this tool measures; it has no CPU mode)")
    from otter_amd import functional as OF
    from otter_amd import ops
    from otter_amd.quant import quantize_weight_int8

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.cuda.get_device_properties(0)
    say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
    say("cold weights: every call of a timed window reads another buffer, each set > 256 MB; %d launches per window, median (max - min) of %d "
        "alternating rounds; us per call" % (a.launches, a.rounds))
    say("%-9s %6s %6s %3s | %16s %6s %6s | %16s %16s %7s | %16s" % ("layer", "N", "K", "M", "(d) panel", "TB/s", "of 8", "(a) dequant", "(b) rows slices",
                                                                 "d/best", "(c) bf16"))
    g = torch.Generator(device="cuda").manual_seed(0)
    ok_at = {M: True for M in MS}
    for name, N, K, act in SHAPES:
        nbuf8 = LLC // (N * K) + 2
        nbuf16 = LLC // (2 * N * K) + 2
        w16 = [torch.randn(N, K, device="cuda", generator=g).mul_(K ** -0.5).to(torch.bfloat16) for _ in range(nbuf16)]
        q8 = []
        for i in range(nbuf8):
            q, s = quantize_weight_int8(w16[i % nbuf16])
            if i >= nbuf16:
                q = q.roll(i, dims=0).contiguous()                      # distinct contents, same statistics
            q8.append((q, s))
        scratch = torch.empty(N, K, dtype=torch.bfloat16, device="cuda")
        for M in MS:
            x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
            y8 = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
            ref = F.linear(x.float(), (q8[0][0].float() * q8[0][1][:, None]))
            ref = F.gelu(ref) if act else ref
            ops.gemm_w8_panel(x, q8[0][0], q8[0][1], None, act, out=y8)
            err = float((y8.float() - ref).abs().max() / ref.abs().max())
            assert err < 1e-2, err                     # (parity proper: tests/test_gpu_w8_panel.py)

            def f_panel(i):
                q, s = q8[i % nbuf8]
                ops.gemm_w8_panel(x, q, s, None, act, out=y8)

            def f_rows(i):
                q, s = q8[i % nbuf8]
                for r in range(0, M, 64):
                    ops.gemm_w8_rows(x[r:r + 64], q, s, None, act, out=y8[r:r + 64])

            def f_deq(i):
                q, s = q8[i % nbuf8]
                y = F.linear(x, ops.dequant_w8(q, s, out=scratch))
                return OF.gelu(y) if act else y

            def f16(i):
                y = F.linear(x, w16[i % nbuf16])
                return OF.gelu(y) if act else y

            fns = [f_panel, f_deq, f_rows, f16]
            with torch.no_grad():
                for f in fns:                          # warm-up: code objects, library algorithm choice, allocator
                    timed(f, max(nbuf8, nbuf16))
                t = [[] for _ in fns]
                for _ in range(a.rounds):
                    for k, f in enumerate(fns):
                        t[k].append(timed(f, a.launches))
            med = [sorted(v)[len(v) // 2] for v in t]
            spread = [max(v) - min(v) for v in t]
            cell = lambda k: "%8.2f (%5.2f)" % (med[k], spread[k])
            bw = (N * K + 4 * N) / (med[0] * 1e-6)
            ratio = med[0] / min(med[1], med[2])
            say("%-9s %6d %6d %3d | %16s %6.3f %5.1f%% | %16s %16s x%6.3f | %16s" % (name, N, K, M, cell(0), bw / 1e12, 100 * bw / NOMINAL, cell(1),
                                                                                     cell(2), ratio, cell(3)))
            if ratio > MARGIN:
                ok_at[M] = False
        del w16, q8, scratch
        torch.cuda.empty_cache()
    threshold = 64
    for M in MS:
        if not ok_at[M]:
            break
        threshold = M
    say("panel <= %.2f x min(dequant, rows slices) on all four shapes at M = %s" % (MARGIN, ", ".join(str(M) for M in MS if ok_at[M]) or "none"))
    say("dispatch threshold (the largest measured M with every smaller measured M inside the margin too): PANEL_MAX_ROWS = %d" % threshold)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
