"""Graph-replayed decode step against the eager step, at OTTER-MPT7B shape: generate(cache_implementation="static",
cross_attention_cache=True, graph_decode=True) (otter_amd/graph_decode.py, otter_decode_attn_cached_dyn) against the same call without
graph_decode -- the eager static + media-cache step -- alternated in one process.

Full 32-layer OTTER-MPT7B with synthetic weights (bench.build_model: frozen weights bf16, trainable ones fp32, bf16 autocast), one 224 x 224
image per sentence, a 512-token prompt, greedy, no end token; B = 1 and B = 4; unquantised, then the same model after
quantize_decoder_int8().  Every timing is a whole `model.generate` call; the same call with ONE new token (the prompt pass alone) is timed
too.  ms per step = (t[NEW] - t[1] - capture) / (NEW - 1), where `capture` is the one-off cost of capturing the step (measured inside the
call: synchronize, capture, synchronize; 0 for the eager path); the figure without that subtraction is printed beside it.  Clock:
torch.cuda.synchronize() + perf_counter; one warm-up call per mode and case; the median of ROUNDS alternating rounds.
Condition: ms per step with the graph <= 1.03 x the eager step of the same process (3 %: the pool's box-to-box and run-to-run spread); a
case that misses prints MISS.

Launches per step: one `rocprofv3 --kernel-trace --stats` run per mode (a child process of this tool, B = 1; tracing only, no counters),
counted in the kernel trace between the first decode-attention kernel of one step and that of a later step.

  python tools/graph_decode_bench.py [--rounds 3] [--new 64] [--prompt 512] [--layers 32] [--no-trace] [--out profiles/r11_graph_decode_ab.txt]"""
from __future__ import annotations

import argparse
import csv
import gc
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

MODES = ("eager", "graph")
THRESHOLD = 1.03
BASE = dict(cache_implementation="static", cross_attention_cache=True)
TRACE_NEW = 24
TRACE_SECONDS = 300


def mode_kwargs(mode):
    return dict(BASE, graph_decode=True) if mode == "graph" else dict(BASE)


@torch.no_grad()
def timed_generate(model, vx, ids, new, kw):
    """(seconds, capture seconds, tokens) of one generate call."""
    from otter_amd.graph_decode import GraphDecodeStep

    captured, release = [0.0], GraphDecodeStep.release

    def spy(self):
        captured[0] += self.capture_seconds
        return release(self)

    GraphDecodeStep.release = spy
    try:
        gc.collect()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            toks = model.generate(vision_x=vx, lang_x=ids, max_new_tokens=new, eos_token_id=-1, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, captured[0], toks
    finally:
        GraphDecodeStep.release = release


def build(layers, int8):
    import bench

    model = bench.build_model("cuda:0", seed=0, debug_layers=0 if layers == 32 else layers).eval()
    if int8:
        model.quantize_decoder_int8()
    return model, bench


def trace_child(a):
    """Under rocprofv3: ONE generate call of TRACE_NEW new tokens at B = 1 (no warm-up call: only its last steps are counted)."""
    model, bench = build(a.layers, a.trace_child_int8)
    vx, ids, _, _, _ = bench.synth_batch(model, 1, a.prompt, "cuda:0", seed=17)
    timed_generate(model, vx.to(torch.bfloat16), ids, TRACE_NEW, mode_kwargs(a.trace_child))


def launches_per_step(trace_dir, layers):
    """Dispatches between the first decode-attention kernel of two steps of the LAST generate call of the trace, per step.  The last 8
    steps are used: in graph mode they are replays."""
    f = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    ev = sorted(((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))), key=lambda e: e[0])
    ix = [i for i, e in enumerate(ev) if "decode_cached_kernel" in e[1] or "decode_cached_dyn_kernel" in e[1]]
    steps = 8
    assert len(ix) >= layers * (steps + 1), (len(ix), layers)
    ix = ix[-layers * (steps + 1):]
    return (ix[steps * layers] - ix[0]) / steps


def trace(a, mode, int8):
    d = tempfile.mkdtemp(prefix="graph_decode_trace_")
    try:
        cmd = ["timeout", "-k", "10", str(TRACE_SECONDS), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
               "--trace-child", mode, "--layers", str(a.layers), "--prompt", str(a.prompt)] + (["--trace-child-int8"] if int8 else [])
        # its own process group: on a time limit the whole group goes (rocprofv3 AND the python child under it), here and by `timeout`
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True)
        try:
            out, _ = p.communicate(timeout=TRACE_SECONDS + 30)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)
            p.wait()
            raise SystemExit("graph_decode_bench: the rocprofv3 run of mode %s did not end in %d s; nothing more is started" % (mode, TRACE_SECONDS))
        if p.returncode != 0:
            raise SystemExit("graph_decode_bench: the rocprofv3 run of mode %s failed (%d):\n%s" % (mode, p.returncode, out.decode()[-2000:]))
        return launches_per_step(d, a.layers)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", choices=MODES, default=None)
    ap.add_argument("--trace-child-int8", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("graph_decode_bench: no GPU visible (this tool measures; it has no CPU mode)")
    if a.trace_child:
        return trace_child(a)

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
    say("model: OTTER-MPT7B shape, %d decoder layers, synthetic weights, bf16 autocast; 1 image per sentence; prompt %d; greedy, no end token; "
        "%d new tokens; static KV cache + media cache in both modes; times are whole generate() calls" % (a.layers, a.prompt, a.new))
    model, bench = build(a.layers, False)
    result, misses = {}, 0
    for quant in ("bf16", "int8"):
        if quant == "int8":
            model.quantize_decoder_int8()
        for B in a.batches:
            vx, ids, _, _, _ = bench.synth_batch(model, B, a.prompt, "cuda:0", seed=17)
            vx = vx.to(torch.bfloat16)
            tag = "prompt=%d B=%d %s" % (a.prompt, B, quant)
            for m in MODES:                              # warm-up: allocator, kernel loads, workspaces
                timed_generate(model, vx, ids, 4, mode_kwargs(m))
            t = {m: {"full": [], "one": [], "capture": []} for m in MODES}
            toks = {}
            for r in range(a.rounds):
                for m in MODES:
                    s1, _, _ = timed_generate(model, vx, ids, 1, mode_kwargs(m))
                    s, cap, out = timed_generate(model, vx, ids, a.new, mode_kwargs(m))
                    t[m]["full"].append(s)
                    t[m]["one"].append(s1)
                    t[m]["capture"].append(cap)
                    toks.setdefault(m, out.cpu())
                    say("%s round %d %-5s %.1f ms for %d new tokens (1 new token: %.1f ms; capture %.1f ms)" % (tag, r, m, s * 1e3, a.new, s1 * 1e3, cap * 1e3))
            med = lambda xs: sorted(xs)[len(xs) // 2]
            step = {m: med([(f - o - c) / (a.new - 1) * 1e3 for f, o, c in zip(t[m]["full"], t[m]["one"], t[m]["capture"])]) for m in MODES}
            gross = {m: med([(f - o) / (a.new - 1) * 1e3 for f, o in zip(t[m]["full"], t[m]["one"])]) for m in MODES}
            cap_ms = med(t["graph"]["capture"]) * 1e3
            equal = bool((toks["graph"] == toks["eager"]).all())
            ratio = step["graph"] / step["eager"]
            say("%s: median ms per step eager %.3f, graph replay %.3f (x%.3f of eager; condition <= %.2f); with the capture spread over the %d steps: "
                "graph %.3f; one-off capture %.1f ms; tokens equal: %s" % (tag, step["eager"], step["graph"], ratio, THRESHOLD, a.new - 1, gross["graph"],
                                                                          cap_ms, equal))
            if ratio > THRESHOLD:
                misses += 1
                say("MISS: %s: the graph-replayed step is more than %.0f %% slower than the eager step" % (tag, (THRESHOLD - 1) * 100))
            result[tag] = {"seconds": {m: t[m]["full"] for m in MODES}, "seconds_one_token": {m: t[m]["one"] for m in MODES},
                           "capture_seconds": t["graph"]["capture"], "ms_per_step": step, "ms_per_step_with_capture": gross,
                           "graph_over_eager": ratio, "tokens_equal": equal}
    say("cases with a MISS: %d of %d" % (misses, len(result)))
    del model
    gc.collect()
    torch.cuda.empty_cache()
    write_out()                                          # (the timings are kept whatever becomes of the traces)
    if not a.no_trace:
        for int8 in (False, True):
            for m in MODES:
                n = trace(a, m, int8)
                say("launches per step (rocprofv3 --kernel-trace --stats, B=1, %s, %s): %.1f" % ("int8" if int8 else "bf16", m, n))
                result["launches_per_step %s %s" % ("int8" if int8 else "bf16", m)] = n
    say(json.dumps(result))
    write_out()


if __name__ == "__main__":
    main()
