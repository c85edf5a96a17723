"""otter_gemm_w8_rows (csrc/w8.hip) at the decode shapes of MPT-7B and 17 to 64 rows: microseconds per call on COLD weights, against the two
things a 17-to-64-row step could run instead.

For each of the four decoder shapes (N, K) and M in {17, 24, 32, 48, 64}, three contenders in the same process, in alternating rounds:
  rows     ops.gemm_w8_rows on the int8 weight (the Python wrapper the model calls, its checks and workspace look-up included);
  dequant  ops.dequant_w8 into one bf16 scratch, then F.linear on it: the step this kernel replaces (OTTER_W8_ROWS=0);
  bf16     F.linear on the bf16 weight: what the unquantised frozen layer runs under no_grad.
A decode step never sees a warm weight, so every call of a round reads a DIFFERENT weight buffer: enough distinct buffers that their
total exceeds the 256 MB last-level cache (the bf16 set and the int8 set are each sized that way).  Clock: one pair of hipEvents around
LAUNCHES back-to-back calls, after a warm-up pass over every buffer; the median of ROUNDS rounds.  Bytes per call = N K + 4 N (the int8
weight and its scales); the fraction is of the 8 TB/s nominal HBM bandwidth.  Condition: rows faster than dequant at every point.

  python tools/w8_rows_bench.py [--launches 64] [--rounds 5] [--out profiles/r12_w8_rows.txt]"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [("Wqkv", 12288, 4096), ("out_proj", 4096, 4096), ("up_proj", 16384, 4096), ("down_proj", 4096, 16384)]
MS = [17, 24, 32, 48, 64]
NOMINAL = 8.0e12
LLC = 256 << 20


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
    ap.add_argument("--launches", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w8_rows_bench: no GPU visible (this tool measures; it has no CPU mode)")
    from otter_amd import ops
    from otter_amd.quant import quantize_weight_int8

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.cuda.get_device_properties(0)
    say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
    say("cold weights: every call of a timed window reads another buffer, each set > 256 MB; %d launches per window, median of %d alternating rounds" % (
        a.launches, a.rounds))
    say("%-9s %6s %6s %3s | %9s %7s %6s | %10s %9s | %8s %9s" % ("layer", "N", "K", "M", "rows us", "TB/s", "of 8", "dequant us", "deq/rows", "bf16 us",
                                                               "bf16/rows"))
    g = torch.Generator(device="cuda").manual_seed(0)
    misses = []
    for name, N, K in SHAPES:
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
            ops.gemm_w8_rows(x, q8[0][0], q8[0][1], None, 0, out=y8)
            err = float((y8.float() - ref).abs().max() / ref.abs().max())
            assert err < 1e-2, err                     # (parity proper: tests/test_gpu_w8_rows.py)

            def f_rows(i):
                q, s = q8[i % nbuf8]
                ops.gemm_w8_rows(x, q, s, None, 0, out=y8)

            def f_deq(i):
                q, s = q8[i % nbuf8]
                F.linear(x, ops.dequant_w8(q, s, out=scratch))

            def f16(i):
                F.linear(x, w16[i % nbuf16])

            with torch.no_grad():
                timed(f_rows, nbuf8)                   # warm-up: code objects, library algorithm choice, allocator
                timed(f_deq, nbuf8)
                timed(f16, nbuf16)
                tr, td, tb = [], [], []
                for _ in range(a.rounds):
                    tr.append(timed(f_rows, a.launches))
                    td.append(timed(f_deq, a.launches))
                    tb.append(timed(f16, a.launches))
            ur, ud, ub = sorted(tr)[len(tr) // 2], sorted(td)[len(td) // 2], sorted(tb)[len(tb) // 2]
            bw = (N * K + 4 * N) / (ur * 1e-6)
            say("%-9s %6d %6d %3d | %9.2f %7.3f %5.1f%% | %10.2f x%8.2f | %8.2f x%8.2f" % (
                name, N, K, M, ur, bw / 1e12, 100 * bw / NOMINAL, ud, ud / ur, ub, ub / ur))
            if ur >= ud:
                misses.append((name, M, ur, ud))
        del w16, q8, scratch
        torch.cuda.empty_cache()
    if misses:
        say("MISSES (rows kernel not faster than dequantise + library GEMM): " + "; ".join("%s M=%d %.2f vs %.2f us" % m for m in misses))
    else:
        say("the rows kernel is faster than dequantise + library GEMM at all %d points" % (len(SHAPES) * len(MS)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
