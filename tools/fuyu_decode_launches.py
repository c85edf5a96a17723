"""Launches per decode step and the decode kernel against its HBM floor, from a rocprofv3 kernel trace of
`tools/fuyu_decode_bench.py --profile` (rocprofv3 --kernel-trace --stats --output-format csv ... -- python tools/fuyu_decode_bench.py
--profile --batch B --steps N --prompt P --layers L).

  python tools/fuyu_decode_launches.py <dir with *kernel_trace.csv> B N P L [H]

The profile run decodes 4 warm-up steps, then N timed steps after a fresh prompt pass: the last L x N persimmon_decode_kernel dispatches
are the timed steps, L per step, so the dispatches between the first decode kernel of step 0 and that of step N - 1, over N - 1, are the
launches of one step (the period).  Floor of one otter_persimmon_decode_attn call at past length S (step i: S = P + i): past K + V read
(2 B H S 64 x 2 bytes) + new cache written (2 B H (S + 1) 64 x 2 bytes) over 8 TB/s; the call's time = the main kernel + the combine
kernel when it runs."""
import collections
import csv
import glob
import sys


def main():
    d, B, N, P, L = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    H = int(sys.argv[6]) if len(sys.argv) > 6 else 64
    f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
    ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))), key=lambda e: e[0])
    main_ix = [i for i, e in enumerate(ev) if "persimmon_decode_kernel" in e[2]]
    assert len(main_ix) >= L * N, (len(main_ix), L * N)
    main_ix = main_ix[-L * N:]
    first, last = main_ix[0], main_ix[(N - 1) * L]
    per_step = (last - first) / (N - 1)
    # one whole step window: from the first decode kernel of step 1 to that of step N - 1 (N - 2 periods)
    lo, hi = main_ix[L], main_ix[(N - 1) * L]
    win = ev[lo:hi]
    tot, cnt = collections.Counter(), collections.Counter()
    for s, e, n in win:
        tot[n] += e - s
        cnt[n] += 1
    steps = N - 2
    wall = (ev[hi][0] - ev[lo][0]) / 1e6 / steps
    ksum = sum(tot.values()) / 1e6 / steps
    print("# decode step at B=%d, prompt %d, %d layers: %.1f launches per step (%d dispatches over %d steps)" % (B, P, L, per_step, last - first, N - 1))
    print("# per step: GPU span %.3f ms, sum of kernel durations %.3f ms" % (wall, ksum))
    print("%-100s %8s %10s %9s %6s" % ("kernel", "calls", "ms/step", "avg_us", "pct"))
    for n, t in tot.most_common(30):
        print("%-100s %8.1f %10.4f %9.2f %6.2f" % (n[:100], cnt[n] / steps, t / 1e6 / steps, t / cnt[n] / 1e3, 100.0 * t / 1e6 / steps / ksum))
    # the new kernel against its floor, per call (main + combine of the same call)
    comb = [i for i, e in enumerate(ev) if "persimmon_decode_combine_kernel" in e[2] and i > main_ix[0]]
    comb_after = {}
    ci = 0
    for k, i in enumerate(main_ix):
        nxt = main_ix[k + 1] if k + 1 < len(main_ix) else len(ev)
        while ci < len(comb) and comb[ci] < i:
            ci += 1
        if ci < len(comb) and comb[ci] < nxt:
            comb_after[k] = comb[ci]
    t_call, t_floor = 0.0, 0.0
    for k, i in enumerate(main_ix):
        S = P + k // L
        t = ev[i][1] - ev[i][0]
        if k in comb_after:
            j = comb_after[k]
            t += ev[j][1] - ev[j][0]
        t_call += t
        t_floor += (2 * B * H * S * 64 * 2 + 2 * B * H * (S + 1) * 64 * 2) / 8e12 * 1e9
    n_calls = len(main_ix)
    print("# otter_persimmon_decode_attn: %d calls, mean %.2f us per call (main + combine: %d combine launches), HBM floor %.2f us per call "
          "at 8 TB/s -> %.1f %% of the floor rate" % (n_calls, t_call / n_calls / 1e3, len(comb_after), t_floor / n_calls / 1e3,
                                                      100.0 * t_floor / t_call))


if __name__ == "__main__":
    main()
