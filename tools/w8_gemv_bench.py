"""otter_gemv_w8 (csrc/w8.hip) against the bf16 library product at the decode shapes of MPT-7B: microseconds per call on COLD weights.

For each of the four decoder shapes (N, K) and M in {1, 4, 16}: the int8 GEMV and F.linear on the bf16 weight (what an unquantised frozen
layer runs under no_grad) are timed in the same process, in alternating rounds.  A decode step never sees a warm weight, so every call of
a round reads a DIFFERENT weight buffer: enough distinct buffers that their total exceeds the 256 MB last-level cache (the bf16 set and
the int8 set are each sized that way).  Clock: one pair of hipEvents around LAUNCHES (>= 50) back-to-back calls, after a warm-up pass over
every buffer; the median of ROUNDS rounds is reported.  The int8 kernel is timed twice: through the C symbol with arguments prepared once
("int8 us": the kernel) and through ops.gemv_w8, the Python wrapper the model calls ("wrap us": its checks and workspace look-up included,
as F.linear's dispatch is included on the bf16 side).  Bytes per call = N K + 4 N (the int8 weight and its scales) for the GEMV and
2 N K for the bf16 product; the fraction is of the 8 TB/s nominal HBM bandwidth.

  python tools/w8_gemv_bench.py [--launches 64] [--rounds 5] [--out profiles/r08_w8_gemv.txt]"""
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
MS = [1, 4, 16]
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
        raise SystemExit("w8_gemv_bench: no GPU visible (this tool measures; it has no CPU mode)")
    from otter_amd import _capi as K_
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
    say("%-9s %6s %6s %3s | %9s %9s %7s | %9s %9s %7s | %s" % ("layer", "N", "K", "M", "int8 us", "TB/s", "of 8", "bf16 us", "TB/s", "of 8", "bf16/int8") + " | wrap us  bf16/wrap")
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
        for M in MS:
            x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
            y8 = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")

            # the C symbol itself, arguments prepared once per buffer: at 4-10 us per kernel the checks of the Python wrapper would be timed instead
            ws = torch.empty(ops.gemv_w8_workspace_bytes(M, N, K), dtype=torch.uint8, device="cuda")
            st = K_.stream()
            args8 = [(x.data_ptr(), K, q.data_ptr(), q.stride(0), s.data_ptr(), None, K_.F32, y8.data_ptr(), N, K_.BF16, M, N, K, 0, ws.data_ptr(),
                      ws.numel(), st) for q, s in q8]
            gemv = K_.lib().otter_gemv_w8
            ref = F.linear(x.float(), (q8[0][0].float() * q8[0][1][:, None]))
            ops.gemv_w8(x, q8[0][0], q8[0][1], None, 0, out=y8)
            err = float((y8.float() - ref).abs().max() / ref.abs().max())
            assert err < 1e-2, err                     # (parity proper: tests/test_gpu_w8.py)

            def f8(i):
                if gemv(*args8[i % nbuf8]) != 0:
                    raise RuntimeError(K_.lib().otter_last_error().decode())

            def f8w(i):
                q, s = q8[i % nbuf8]
                ops.gemv_w8(x, q, s, None, 0, out=y8)

            def f16(i):
                F.linear(x, w16[i % nbuf16])

            with torch.no_grad():
                timed(f8, nbuf8)                       # warm-up: code objects, library algorithm choice, allocator
                timed(f16, nbuf16)
                timed(f8w, nbuf8)
                t8, t16, t8w = [], [], []
                for _ in range(a.rounds):
                    t8.append(timed(f8, a.launches))
                    t16.append(timed(f16, a.launches))
                    t8w.append(timed(f8w, a.launches))
            u8, u16, u8w = sorted(t8)[len(t8) // 2], sorted(t16)[len(t16) // 2], sorted(t8w)[len(t8w) // 2]
            b8, b16 = (N * K + 4 * N) / (u8 * 1e-6), (2 * N * K) / (u16 * 1e-6)
            say("%-9s %6d %6d %3d | %9.2f %9.3f %6.1f%% | %9.2f %9.3f %6.1f%% | x%.2f      | %7.2f  x%.2f" % (
                name, N, K, M, u8, b8 / 1e12, 100 * b8 / NOMINAL, u16, b16 / 1e12, 100 * b16 / NOMINAL, u16 / u8, u8w, u16 / u8w))
            if max(u8, u8w) > u16:
                misses.append((name, M, max(u8, u8w), u16))
        del w16, q8
        torch.cuda.empty_cache()
    if misses:
        say("MISSES (int8 GEMV slower than the bf16 library product): " + "; ".join("%s M=%d %.2f vs %.2f us" % m for m in misses))
    else:
        say("the int8 GEMV is not slower than the bf16 library product at any of the %d points" % (len(SHAPES) * len(MS)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
