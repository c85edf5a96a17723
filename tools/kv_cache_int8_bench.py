"""The int8 static KV cache against the bf16 static KV cache, at OTTER-MPT7B shape: generate(cache_implementation="static",
kv_cache_dtype="int8") (otter_amd/kv_cache.py, csrc/decode_cache_i8.hip) against the same call without the keyword, alternated in one
process.

Parts (each a child process of this tool under its own `timeout`; the tool stops at the first non-zero status):
  kernel  us per call of ops.decode_attn_cached_i8 against ops.decode_attn_cached, H = 32, rows {1, 24, 64} x pos {512, 2048, 8192}, no beam
          table (every row's keys distinct), ALiBi on.  Each call takes the next of enough per-layer caches to exceed 1 GiB, as the layers of
          a step do, so no call finds its keys in a cache.  HIP events around CALLS calls, the median of REPS repetitions.  Achieved fraction
          of the nominal 8 TB/s: the distinct bytes a call must read (rows x 32 x pos x 2 x 256 bytes for bf16, x 2 x 132 for int8) over
          the time.
  a       full 32-layer OTTER-MPT7B, int8 decoder + cross-attention cache + graph replay (`generate(..., cross_attention_cache=True,
          graph_decode=True)` after quantize_decoder_int8())
  b       the same model unquantised, eager
For a and b: synthetic weights (bench.build_model: frozen weights bf16, trainable ones fp32, bf16 autocast), one 224 x 224 image per
sentence, no end token; rows 1, 4, 24 (8 sentences x num_beams=3) and 64; prompts of 512 and 1536 tokens.  Every timing is a whole
`model.generate` call; the same call with ONE new token (the prompt pass alone) is timed too; ms per step = (t[NEW] - t[1] - capture) /
(NEW - 1) with `capture` the one-off cost of capturing the step (0 when eager).  Clock: torch.cuda.synchronize() + perf_counter; one warm-up
call per cache form and point; the median of ROUNDS alternating rounds.  Also: the bytes of the cache (StaticKVCache.nbytes()),
torch.cuda.max_memory_allocated() of a call above what was allocated before it, the column at which the int8-cache tokens first part from
the bf16-cache tokens, and (part b, rows 1 and 4: eager steps are visible to a forward hook) the per-step relative logit error max_v |int8 -
bf16| / max_v |bf16| over the steps before that column.
Condition, per point: int8-cache ms per step <= 1.03 x the bf16-cache step of the same process (3 %: the pool's box-to-box and run-to-run
spread); a point that misses prints MISS.

  python tools/kv_cache_int8_bench.py [--parts kernel a b] [--rows 1 4 24 64] [--prompts 512 1536] [--rounds 3] [--new 64] [--layers 32]
                                      [--append] [--out profiles/r13_kv_int8_ab.txt]"""
from __future__ import annotations

import argparse
import gc
import json
import os
import signal
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

THRESHOLD = 1.03
FORMS = ("bf16", "int8")
ROW_CASES = {1: (1, {}), 4: (4, {}), 24: (8, dict(num_beams=3)), 64: (64, {})}     # rows -> (sentences, generate kwargs)
PART_SECONDS = {"kernel": 240, "a": 1080, "b": 1080}
PEAK_TBPS = 8.0
CALLS, REPS = 64, 5


# ---- part: kernel ---------------------------------------------------------------------------------------------------------------------

def kernel_part(a, say):
    from otter_amd import ops

    dev, H = "cuda:0", 32
    g = torch.Generator(device=dev).manual_seed(0)
    slopes = (2.0 ** -(8.0 * torch.arange(1, H + 1, device=dev, dtype=torch.float32) / H)).contiguous()
    result = {}
    for rows in (1, 24, 64):
        for pos in (512, 2048, 8192):
            S_max = pos + 8
            per_layer = rows * H * S_max * 128 * 2 * 2
            layers = min(32, max(2, -(-(1 << 30) // per_layer)))
            qkv = torch.randn(rows, 3, H, 128, device=dev, generator=g).bfloat16()
            q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
            kb = torch.randn(layers, rows, H, S_max, 128, device=dev, generator=g).bfloat16()
            vb = torch.randn(layers, rows, H, S_max, 128, device=dev, generator=g).bfloat16()
            kc = torch.randint(-127, 128, (layers, rows, H, S_max, 128), device=dev, generator=g, dtype=torch.int8)
            vc = torch.randint(-127, 128, (layers, rows, H, S_max, 128), device=dev, generator=g, dtype=torch.int8)
            ks = torch.rand(layers, rows, H, S_max, device=dev, generator=g) * (3.0 / 127)
            vs = torch.rand(layers, rows, H, S_max, device=dev, generator=g) * (3.0 / 127)

            def call(form, i):
                L = i % layers
                if form == "bf16":
                    return ops.decode_attn_cached(q, k, v, kb[L], vb[L], pos, 0.0884, slopes=slopes)
                return ops.decode_attn_cached_i8(q, k, v, kc[L], vc[L], ks[L], vs[L], pos, 0.0884, slopes=slopes)

            us = {f: [] for f in FORMS}
            for f in FORMS:
                for i in range(8):
                    call(f, i)
            for _ in range(REPS):
                for f in FORMS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for i in range(CALLS):
                        call(f, i)
                    e1.record()
                    torch.cuda.synchronize()
                    us[f].append(e0.elapsed_time(e1) * 1e3 / CALLS)
            med = {f: sorted(us[f])[REPS // 2] for f in FORMS}
            nbytes = {"bf16": rows * H * pos * 2 * 256, "int8": rows * H * pos * 2 * 132}
            frac = {f: nbytes[f] / (med[f] * 1e-6) / (PEAK_TBPS * 1e12) for f in FORMS}
            tag = "kernel rows=%d pos=%d" % (rows, pos)
            say("%s (%d caches in turn): bf16 %.1f us (%.1f MB, %.3f of %.0f TB/s) | int8 %.1f us (%.1f MB, %.3f) | int8 = x%.3f of bf16" % (
                tag, layers, med["bf16"], nbytes["bf16"] / 1e6, frac["bf16"], PEAK_TBPS, med["int8"], nbytes["int8"] / 1e6, frac["int8"],
                med["int8"] / med["bf16"]))
            result[tag] = {"us": med, "all_us": us, "bytes": nbytes, "fraction_of_peak": frac}
            del kb, vb, kc, vc, ks, vs
            gc.collect()
            torch.cuda.empty_cache()
    return result


# ---- parts: a, b ------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def timed_generate(model, vx, ids, new, kw, logits=None):
    """(seconds, capture seconds, peak bytes above the start, cache bytes, tokens) of one generate call; `logits`: a list that receives
    the last-position logits of every decoder call Python issues."""
    from otter_amd import kv_cache
    from otter_amd.graph_decode import GraphDecodeStep

    captured, release, made, cls = [0.0], GraphDecodeStep.release, [], kv_cache.StaticKVCache

    def spy(self):
        captured[0] += self.capture_seconds
        return release(self)

    class Recorded(cls):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self.nbytes())

    hook = None
    if logits is not None:
        hook = model.lang_encoder.register_forward_hook(lambda _m, _a, _k, out: logits.append(out.logits[:, -1].float()), with_kwargs=True)
    GraphDecodeStep.release, kv_cache.StaticKVCache = spy, Recorded
    try:
        gc.collect()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            toks = model.generate(vision_x=vx, lang_x=ids, max_new_tokens=new, eos_token_id=-1, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, captured[0], torch.cuda.max_memory_allocated() - base, made[0], toks
    finally:
        GraphDecodeStep.release, kv_cache.StaticKVCache = release, cls
        if hook is not None:
            hook.remove()


def model_part(a, part, say):
    import bench

    model = bench.build_model("cuda:0", seed=0, debug_layers=0 if a.layers == 32 else a.layers).eval()
    base = dict(cache_implementation="static")
    if part == "a":
        model.quantize_decoder_int8()
        base.update(cross_attention_cache=True, graph_decode=True)
    gc.collect()
    torch.cuda.empty_cache()
    say("part %s: %s; model resident: %.2f GB" % (part, "int8 decoder + media cache + graph replay" if part == "a" else "unquantised, eager",
                                                  torch.cuda.memory_allocated() / 1e9))
    form_kw = {"bf16": {}, "int8": dict(kv_cache_dtype="int8")}
    med = lambda xs: sorted(xs)[len(xs) // 2]
    result, misses = {}, 0
    for rows in a.rows:
        B, extra = ROW_CASES[rows]
        for prompt in a.prompts:
            vx, ids, _, _, _ = bench.synth_batch(model, B, prompt, "cuda:0", seed=17)
            vx = vx.to(torch.bfloat16)
            tag = "%s rows=%d prompt=%d" % (part, rows, prompt)
            kw = {f: dict(base, **extra, **form_kw[f]) for f in FORMS}
            for f in FORMS:                                  # warm-up: allocator, kernel loads, workspaces
                timed_generate(model, vx, ids, 4, kw[f])
            t = {f: [] for f in FORMS}
            peak, cache_bytes, toks = {}, {}, {}
            for r in range(a.rounds):
                for f in FORMS:
                    s1, c1, _, _, _ = timed_generate(model, vx, ids, 1, kw[f])
                    s, cap, pk, cb, out = timed_generate(model, vx, ids, a.new, kw[f])
                    t[f].append((s - cap - (s1 - c1)) / (a.new - 1) * 1e3)
                    peak[f], cache_bytes[f] = max(peak.get(f, 0), pk), cb
                    toks.setdefault(f, out.cpu())
                    say("%s round %d %-4s cache %.1f ms for %d new tokens (1 new token: %.1f ms; capture %.1f ms)" % (
                        tag, r, f, s * 1e3, a.new, s1 * 1e3, cap * 1e3))
            step = {f: med(t[f]) for f in FORMS}
            eq = (toks["int8"] == toks["bf16"]).all(dim=0).tolist()
            part_at = eq.index(False) - prompt if False in eq else None
            ratio = step["int8"] / step["bf16"]
            say("%s: median ms per step bf16 cache %.3f | int8 cache %.3f (x%.3f of bf16; condition <= %.2f); cache bytes bf16 %.3f GB, int8 %.3f GB "
                "(x%.4f); peak memory above the model bf16 %.3f GB, int8 %.3f GB; tokens part at new token %s of %d" % (
                    tag, step["bf16"], step["int8"], ratio, THRESHOLD, cache_bytes["bf16"] / 1e9, cache_bytes["int8"] / 1e9,
                    cache_bytes["int8"] / cache_bytes["bf16"], peak["bf16"] / 1e9, peak["int8"] / 1e9,
                    "none" if part_at is None else str(part_at), a.new))
            if ratio > THRESHOLD:
                misses += 1
                say("MISS: %s: the int8-cache step is more than %.0f %% slower than the bf16-cache step" % (tag, (THRESHOLD - 1) * 100))
            result[tag] = {"ms_per_step": step, "all": t, "int8_over_bf16": ratio, "cache_bytes": cache_bytes, "peak_bytes": peak,
                           "tokens_part_at": part_at}
            if part == "b" and rows in (1, 4):               # the drift: logits of the eager steps the two calls share
                lg = {f: [] for f in FORMS}
                for f in FORMS:
                    timed_generate(model, vx, ids, a.new, kw[f], logits=lg[f])
                shared = a.new if part_at is None else part_at + 1      # (the call that chooses new token i sees identical inputs for i <= part_at)
                drift = [float(((x - y).abs().amax(-1) / y.abs().amax(-1)).max()) for x, y in zip(lg["int8"][:shared], lg["bf16"][:shared])]
                say("%s: relative logit error of the int8 cache per decoder call (prompt pass first; %d calls with identical inputs): max %.3e, "
                    "median %.3e, last %.3e" % (tag, shared, max(drift), med(drift), drift[-1]))
                result[tag]["logit_drift"] = drift
            del vx, ids
            gc.collect()
            torch.cuda.empty_cache()
    say("part %s: conditions missed: %d of %d" % (part, misses, len(result)))
    return result


# ---- parent ---------------------------------------------------------------------------------------------------------------------------------

def run_child(a, part):
    cmd = ["timeout", "-k", "10", str(PART_SECONDS[part]), sys.executable, os.path.abspath(__file__), "--child", part, "--rounds", str(a.rounds),
           "--new", str(a.new), "--layers", str(a.layers), "--rows"] + [str(r) for r in a.rows] + ["--prompts"] + [str(p) for p in a.prompts]
    # its own process group: on a time limit the whole group goes, here and by `timeout`
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True, text=True)
    out = []
    try:
        for line in p.stdout:
            print(line, end="", flush=True)
            out.append(line.rstrip("\n"))
        p.wait(timeout=30)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.wait()
    return p.returncode, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", choices=list(PART_SECONDS), default=list(PART_SECONDS))
    ap.add_argument("--rows", type=int, nargs="+", choices=list(ROW_CASES), default=list(ROW_CASES))
    ap.add_argument("--prompts", type=int, nargs="+", default=[512, 1536])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--child", choices=list(PART_SECONDS), default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        if not torch.cuda.is_available():
            raise SystemExit("kv_cache_int8_bench: no GPU visible (this tool measures; it has no CPU mode)")
        say = lambda s: print(s, flush=True)
        dev = torch.cuda.get_device_properties(0)
        say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
        result = kernel_part(a, say) if a.child == "kernel" else model_part(a, a.child, say)
        say(json.dumps(result))
        return
    lines = ["kv_cache_int8_bench: parts %s; rows %s; prompts %s; %d rounds; %d new tokens; %d decoder layers" % (
        " ".join(a.parts), a.rows, a.prompts, a.rounds, a.new, a.layers)]
    status = 0
    for part in a.parts:
        rc, out = run_child(a, part)
        lines += out
        if rc != 0:
            lines.append("kv_cache_int8_bench: part %s ended with status %s; nothing more is started" % (part, rc))
            print(lines[-1], flush=True)
            status = 1
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
