"""The token selection of one generation step alone: `ops.select_step` (csrc/select.hip) against the torch ops of the host block of
generation.generate_tokens on the same device tensors.

    greedy   host: argmax, where, full_like, two cats (ids and the mask), isin, ~, &, any       kernel: one launch
    sample   host: scores / T, _top_k_top_p (topk, sort over V, softmax, cumsum, scatter, masked_fill), softmax, multinomial and the same
             bookkeeping                                                                         kernel: q.exponential_() + one launch
             at top_k=50, top_p=0.9, temperature=0.7

Shapes N in {1, 4, 8} x V in {50432, 262144}, randn * 3 scores, a 512-token history, one eos id that no row selects.  The host block's
synchronising `bool(unfinished.any())` is left out of its clock (its `any()` launch is in): the device time of the ops is what is compared.
Clock: device events around ITERS back-to-back steps after a warm-up; ROUNDS rounds alternating the two paths in one process; reported per
shape and mode: the median microseconds per step of both paths, the spread (max - min) / median over rounds, and kernel / host.  A kernel
median above host x (1 + the larger spread) prints SLOWER.

  python tools/select_bench.py [--rounds 3] [--iters 100] [--out profiles/r18_select_ab.txt]"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

T, TOP_K, TOP_P = 0.7, 50, 0.9
L, EOS, PAD = 512, 3, 0


def make_paths(N, V, mode):
    from otter_amd import generation as G
    from otter_amd import ops

    dev = "cuda:0"
    scores = (torch.randn(N, V, generator=torch.Generator().manual_seed(V + N)) * 3).to(dev)
    scores[:, EOS] = -1e4                                            # never selected: every row stays unfinished
    ids0 = torch.randint(4, V, (N, L), generator=torch.Generator().manual_seed(1)).to(dev)
    mask0 = torch.ones(N, L, dtype=torch.long, device=dev)
    eos_t = torch.tensor([EOS], device=dev, dtype=torch.long)
    gen = torch.Generator(device=dev).manual_seed(5)
    inv_t = G.inv_temperature_f32(T)

    def host():
        unfinished = torch.ones(N, dtype=torch.bool, device=dev)
        if mode == "sample":
            s = G._top_k_top_p(scores / T, TOP_K, TOP_P)
            nxt = torch.multinomial(s.softmax(-1), 1, generator=gen).squeeze(1)
        else:
            nxt = scores.argmax(-1)
        nxt = torch.where(unfinished, nxt, torch.full_like(nxt, PAD))
        ids = torch.cat([ids0, nxt[:, None]], dim=1)
        mask = torch.cat([mask0, torch.ones_like(mask0[:, :1])], dim=1)
        unfinished = unfinished & ~torch.isin(nxt, eos_t)
        return ids, mask, unfinished.any()

    ids_buf = torch.zeros(N, L + 1, dtype=torch.long, device=dev)
    ids_buf[:, :L] = ids0
    unfinished = torch.ones(N, dtype=torch.bool, device=dev)
    n_unfinished = torch.full((1,), N, dtype=torch.int32, device=dev)
    eos32 = eos_t.to(torch.int32)
    q = torch.empty(N, V, device=dev)

    def kernel():
        if mode == "sample":
            q.exponential_(1, generator=gen)
            ops.select_step(scores, ids_buf, L, unfinished, n_unfinished, eos32, PAD, True, inv_t, TOP_K, TOP_P, q)
        else:
            ops.select_step(scores, ids_buf, L, unfinished, n_unfinished, eos32, PAD)
        return ids_buf

    return {"host": host, "kernel": kernel}


def clock(fn, iters):
    """Microseconds per call: device events around `iters` back-to-back calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("select_bench: no GPU visible (this tool measures; it has no CPU mode)")
    if a.rounds < 3:
        raise SystemExit("select_bench: at least three rounds (the spread over rounds is part of the result)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.cuda.get_device_properties(0)
    say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
    say("one selection step alone, device events around %d back-to-back steps, %d alternating rounds; sample: top_k=%d top_p=%g temperature=%g"
        % (a.iters, a.rounds, TOP_K, TOP_P, T))
    slower = 0
    for mode in ("greedy", "sample"):
        for V in (50432, 262144):
            for N in (1, 4, 8):
                paths = make_paths(N, V, mode)
                for fn in paths.values():
                    clock(fn, 10)                                    # warm-up: code objects, allocator
                t = {p: [] for p in paths}
                for _ in range(a.rounds):
                    for p, fn in paths.items():
                        t[p].append(clock(fn, a.iters))
                med = {p: sorted(v)[len(v) // 2] for p, v in t.items()}
                spread = {p: (max(v) - min(v)) / med[p] for p, v in t.items()}
                ratio = med["kernel"] / med["host"]
                miss = med["kernel"] > med["host"] * (1 + max(spread.values()))
                slower += miss
                say("%-6s N=%d V=%-6d host ops %8.1f us (spread %4.1f%%) | kernel %8.1f us (spread %4.1f%%) = x%.3f of the host ops%s"
                    % (mode, N, V, med["host"], 100 * spread["host"], med["kernel"], 100 * spread["kernel"], ratio, "  SLOWER" if miss else ""))
    say("shapes at which the kernel is slower than the host ops beyond the spread: %d of 12" % slower)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
