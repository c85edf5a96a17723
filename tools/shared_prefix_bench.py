"""Beam search over a shared prompt against private prompt copies, at OTTER-MPT7B shape: generate(num_beams=3, cache_implementation="static",
share_prompt=True) (otter_amd/kv_cache.py: StaticKVCache.share_prompt, csrc/decode_cache_shared.hip) against the same call without the
keyword, alternated in one process.

Parts (each a child process of this tool under its own `timeout`; the tool stops at the first non-zero status):
  kernel    us per call at H = 32, rows 24 (8 sentences x 3 beams) and 3 (1 x 3), 512 / 2048 / 8192 shared keys + 64 own keys, ALiBi on, three
            contenders alternated in one process:
              grouped   ops.decode_attn_cached_shared: one workgroup per (range, head, sentence), a shared key loaded once
              table     ops.decode_attn_cached through the same table (columns [0, P) point at the leader): what OTTER_SHARED_PREFIX=0 runs
              private   ops.decode_attn_cached with every row's prefix in its own row: what the parent commit runs
            Each call takes the next of enough per-layer caches to exceed 1 GiB (at most 64), as the layers of a step do, so no call finds
            its keys in a cache.  HIP events around CALLS calls, the median of REPS repetitions.  Bytes/s over the DISTINCT bytes a call must
            read: (sentences x P + rows x 64) x 32 x 512 bytes for grouped and table, rows x (P + 64) x 32 x 512 for private.
  generate  whole `model.generate` calls of the full 32-layer OTTER-MPT7B: int8 decoder + static cache + cross-attention cache + graph replay,
            num_beams=3, no_repeat_ngram_size=3, no end token; B = 8 and 1, prompts of 512 and 1536 tokens, 128 new tokens; share_prompt on
            and off, one warm-up call each, then ROUNDS alternating rounds.  The same call with ONE new token is the prompt pass; ms per
            generated position = (t[NEW] - t[1] - capture) / (NEW - 1).  Clock: torch.cuda.synchronize() + perf_counter.
Beside every measured ratio the bytes ratio (P / nb + own) / (P + own) of the keys and values a step reads (own: the mean over the call).
Condition, per point: the share_prompt path <= 1.03 x the parent path (3 %: tools/regress.sh's margin); a point that misses prints MISS.

--kv-dtype int8 (the default, bf16, leaves every line above as it is): the int8 static cache and csrc/decode_cache_shared_i8.hip.
  kernel    the contenders are ops.decode_attn_cached_shared_i8 (grouped), ops.decode_attn_cached_i8 through the same table (table: what
            OTTER_SHARED_PREFIX_I8=0 and the parent commit run for a share_prompt call) and ops.decode_attn_cached_i8 on private copies
            (private: what the parent commit runs for an unshared call).  The points above plus rows 3 x {1024, 1536} and rows 24 x 128 shared
            keys, around the count from which `attend` takes the grouped kernel.  A cached vector is 132 bytes (128 codes + one fp32 scale):
            the distinct bytes are (sentences x P + rows x 64) x 32 x 264 for grouped and table, rows x (P + 64) x 32 x 264 for private.
            Condition: grouped <= 1.03 x table and <= 1.03 x private.
  generate  the same call plus kv_cache_dtype="int8", share_prompt=True on both sides: OTTER_SHARED_PREFIX_I8=0 (the parent commit's
            behaviour: the table path) against the variable unset, alternated in one process.

  python tools/shared_prefix_bench.py [--parts kernel generate] [--sentences 8 1] [--prompts 512 1536] [--rounds 3] [--new 128] [--layers 32]
                                      [--kv-dtype bf16|int8] [--append] [--out profiles/r19_shared_prefix_ab.txt]"""
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
NB, OWN = 3, 64
PART_SECONDS = {"kernel": 300, "generate": 1080}
CALLS, REPS = 64, 5
CONTENDERS = ("grouped", "table", "private")
# --kv-dtype int8: (rows, shared keys) of the kernel part -- the bf16 part's points, then those around the dispatch threshold
I8_POINTS = [(rows, P) for rows in (24, 3) for P in (512, 2048, 8192)] + [(3, 1024), (3, 1536), (24, 128)]
I8_LEVER = "OTTER_SHARED_PREFIX_I8"


# ---- part: kernel ---------------------------------------------------------------------------------------------------------------------

def kernel_part(a, say):
    from otter_amd import ops

    dev, H = "cuda:0", 32
    g = torch.Generator(device=dev).manual_seed(0)
    slopes = (2.0 ** -(8.0 * torch.arange(1, H + 1, device=dev, dtype=torch.float32) / H)).contiguous()
    result, misses = {}, 0
    for rows in (24, 3):
        for P in (512, 2048, 8192):
            pos, S_max = P + OWN, P + OWN + 8
            per_layer = rows * H * S_max * 128 * 2 * 2
            layers = min(64, max(2, -(-(1 << 30) // per_layer)))
            qkv = torch.randn(rows, 3, H, 128, device=dev, generator=g).bfloat16()
            q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
            kb = torch.randn(layers, rows, H, S_max, 128, device=dev, generator=g).bfloat16()
            vb = torch.randn(layers, rows, H, S_max, 128, device=dev, generator=g).bfloat16()
            n = torch.arange(rows, dtype=torch.int32, device=dev)
            own = (n // NB * NB + (n % NB + 1) % NB)[:, None].repeat(1, S_max - 1)        # the own part behind a sibling, as after a reorder
            shared = own.clone()
            shared[:, :P] = (n // NB * NB)[:, None]
            private = own.clone()
            private[:, :P] = n[:, None]

            def call(c, i):
                L = i % layers
                if c == "grouped":
                    return ops.decode_attn_cached_shared(q, k, v, kb[L], vb[L], pos, 0.0884, NB, P, src=shared, slopes=slopes)
                return ops.decode_attn_cached(q, k, v, kb[L], vb[L], pos, 0.0884, src=shared if c == "table" else private, slopes=slopes)

            us = {c: [] for c in CONTENDERS}
            for c in CONTENDERS:
                for i in range(8):
                    call(c, i)
            for _ in range(REPS):
                for c in CONTENDERS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for i in range(CALLS):
                        call(c, i)
                    e1.record()
                    torch.cuda.synchronize()
                    us[c].append(e0.elapsed_time(e1) * 1e3 / CALLS)
            med = {c: sorted(us[c])[REPS // 2] for c in CONTENDERS}
            spread = {c: (max(us[c]) - min(us[c])) / med[c] for c in CONTENDERS}
            distinct = (rows // NB * P + rows * OWN) * H * 512
            nbytes = {"grouped": distinct, "table": distinct, "private": rows * pos * H * 512}
            tbps = {c: nbytes[c] / (med[c] * 1e-6) / 1e12 for c in CONTENDERS}
            ratio, bytes_ratio = med["grouped"] / med["private"], (P / NB + OWN) / (P + OWN)
            tag = "kernel rows=%d shared=%d own=%d" % (rows, P, OWN)
            say("%s (%d caches in turn): grouped %.1f us (%.1f MB, %.2f TB/s) | table %.1f us (%.2f TB/s) | private %.1f us (%.1f MB, %.2f TB/s) | "
                "grouped = x%.3f of private, table = x%.3f of private (bytes ratio %.3f; spread %.1f / %.1f / %.1f %%)" % (
                    tag, layers, med["grouped"], distinct / 1e6, tbps["grouped"], med["table"], tbps["table"], med["private"],
                    nbytes["private"] / 1e6, tbps["private"], ratio, med["table"] / med["private"], bytes_ratio, spread["grouped"] * 100,
                    spread["table"] * 100, spread["private"] * 100))
            if ratio > THRESHOLD:
                misses += 1
                say("MISS: %s: the grouped kernel is more than %.0f %% slower than the existing kernel on private copies" % (tag, (THRESHOLD - 1) * 100))
            result[tag] = {"us": med, "all_us": us, "bytes": nbytes, "tbps": tbps, "grouped_over_private": ratio, "bytes_ratio": bytes_ratio}
            del kb, vb
            gc.collect()
            torch.cuda.empty_cache()
    say("part kernel: conditions missed: %d of %d" % (misses, len(result)))
    return result


def kernel_part_i8(a, say):
    """The kernel part over the int8 cache (module docstring)."""
    from otter_amd import ops

    dev, H = "cuda:0", 32
    g = torch.Generator(device=dev).manual_seed(0)
    slopes = (2.0 ** -(8.0 * torch.arange(1, H + 1, device=dev, dtype=torch.float32) / H)).contiguous()
    result, misses = {}, 0
    for rows, P in I8_POINTS:
        pos, S_max = P + OWN, P + OWN + 8
        per_layer = rows * H * S_max * 132 * 2
        layers = min(64, max(2, -(-(1 << 30) // per_layer)))
        qkv = torch.randn(rows, 3, H, 128, device=dev, generator=g).bfloat16()
        q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
        kb = torch.randint(-127, 128, (layers, rows, H, S_max, 128), device=dev, generator=g, dtype=torch.int8)
        vb = torch.randint(-127, 128, (layers, rows, H, S_max, 128), device=dev, generator=g, dtype=torch.int8)
        ksb = (0.5 + torch.rand(layers, rows, H, S_max, device=dev, generator=g)) * (3.0 / 127)
        vsb = (0.5 + torch.rand(layers, rows, H, S_max, device=dev, generator=g)) * (3.0 / 127)
        n = torch.arange(rows, dtype=torch.int32, device=dev)
        own = (n // NB * NB + (n % NB + 1) % NB)[:, None].repeat(1, S_max - 1)        # the own part behind a sibling, as after a reorder
        shared = own.clone()
        shared[:, :P] = (n // NB * NB)[:, None]
        private = own.clone()
        private[:, :P] = n[:, None]

        def call(c, i):
            L = i % layers
            if c == "grouped":
                return ops.decode_attn_cached_shared_i8(q, k, v, kb[L], vb[L], ksb[L], vsb[L], pos, 0.0884, NB, P, src=shared, slopes=slopes)
            return ops.decode_attn_cached_i8(q, k, v, kb[L], vb[L], ksb[L], vsb[L], pos, 0.0884, src=shared if c == "table" else private,
                                             slopes=slopes)

        us = {c: [] for c in CONTENDERS}
        for c in CONTENDERS:
            for i in range(8):
                call(c, i)
        for _ in range(REPS):
            for c in CONTENDERS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for i in range(CALLS):
                    call(c, i)
                e1.record()
                torch.cuda.synchronize()
                us[c].append(e0.elapsed_time(e1) * 1e3 / CALLS)
        med = {c: sorted(us[c])[REPS // 2] for c in CONTENDERS}
        spread = {c: (max(us[c]) - min(us[c])) / med[c] for c in CONTENDERS}
        distinct = (rows // NB * P + rows * OWN) * H * 264
        nbytes = {"grouped": distinct, "table": distinct, "private": rows * pos * H * 264}
        tbps = {c: nbytes[c] / (med[c] * 1e-6) / 1e12 for c in CONTENDERS}
        over_private, over_table, bytes_ratio = med["grouped"] / med["private"], med["grouped"] / med["table"], (P / NB + OWN) / (P + OWN)
        tag = "kernel int8 rows=%d shared=%d own=%d" % (rows, P, OWN)
        say("%s (sentences x shared = %d; %d caches in turn): grouped %.1f us (%.1f MB, %.2f TB/s) | table %.1f us (%.2f TB/s) | private %.1f us "
            "(%.1f MB, %.2f TB/s) | grouped = x%.3f of table, x%.3f of private; table = x%.3f of private (bytes ratio %.3f; spread %.1f / %.1f / "
            "%.1f %%)" % (tag, rows // NB * P, layers, med["grouped"], distinct / 1e6, tbps["grouped"], med["table"], tbps["table"], med["private"],
                          nbytes["private"] / 1e6, tbps["private"], over_table, over_private, med["table"] / med["private"], bytes_ratio,
                          spread["grouped"] * 100, spread["table"] * 100, spread["private"] * 100))
        if max(over_private, over_table) > THRESHOLD:
            misses += 1
            say("MISS: %s: the grouped kernel is more than %.0f %% slower than the existing int8 kernel %s" % (
                tag, (THRESHOLD - 1) * 100, "through the table" if over_table > THRESHOLD else "on private copies"))
        result[tag] = {"us": med, "all_us": us, "bytes": nbytes, "tbps": tbps, "grouped_over_private": over_private, "grouped_over_table": over_table,
                       "bytes_ratio": bytes_ratio, "sentences_x_shared": rows // NB * P}
        del kb, vb, ksb, vsb
        gc.collect()
        torch.cuda.empty_cache()
    say("part kernel (int8): conditions missed: %d of %d" % (misses, len(result)))
    return result


# ---- part: generate -------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def timed_generate(model, vx, ids, new, kw):
    """(seconds, capture seconds, tokens) of one generate call.  An "env" entry of `kw` is not a keyword: {variable: value or None (unset)}
    for the duration of the call."""
    from otter_amd.graph_decode import GraphDecodeStep

    kw = dict(kw)
    env = kw.pop("env", {})
    saved = {name: os.environ.get(name) for name in env}
    for name, value in env.items():
        os.environ.pop(name, None) if value is None else os.environ.__setitem__(name, value)

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
        for name, value in saved.items():
            os.environ.pop(name, None) if value is None else os.environ.__setitem__(name, value)


def generate_part(a, say):
    import bench

    model = bench.build_model("cuda:0", seed=0, debug_layers=0 if a.layers == 32 else a.layers).eval()
    model.quantize_decoder_int8()
    gc.collect()
    torch.cuda.empty_cache()
    say("part generate: int8 decoder + static cache + cross-attention cache + graph replay, %d beams; model resident: %.2f GB" % (
        NB, torch.cuda.memory_allocated() / 1e9))
    base = dict(cache_implementation="static", cross_attention_cache=True, graph_decode=True, num_beams=NB, no_repeat_ngram_size=3)
    kw = {"parent": base, "shared": dict(base, share_prompt=True)}
    if a.kv_dtype == "int8":        # share_prompt on both sides; the parent commit's behaviour is the table path
        base = dict(base, kv_cache_dtype="int8", share_prompt=True)
        kw = {"parent": dict(base, env={I8_LEVER: "0"}), "shared": dict(base, env={I8_LEVER: None})}
        say("int8 KV cache, share_prompt=True on both sides: parent = %s=0 (the table path), shared = %s unset" % (I8_LEVER, I8_LEVER))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    result, misses = {}, 0
    for B in a.sentences:
        for prompt in a.prompts:
            vx, ids, _, _, _ = bench.synth_batch(model, B, prompt, "cuda:0", seed=17)
            vx = vx.to(torch.bfloat16)
            tag = "generate B=%d prompt=%d" % (B, prompt)
            for f in kw:                                     # warm-up: allocator, kernel loads, workspaces
                timed_generate(model, vx, ids, 4, kw[f])
            first, step, toks = {f: [] for f in kw}, {f: [] for f in kw}, {}
            for r in range(a.rounds):
                for f in kw:
                    s1, c1, _ = timed_generate(model, vx, ids, 1, kw[f])
                    s, cap, out = timed_generate(model, vx, ids, a.new, kw[f])
                    first[f].append((s1 - c1) * 1e3)
                    step[f].append((s - cap - (s1 - c1)) / (a.new - 1) * 1e3)
                    toks.setdefault(f, out.cpu())
                    say("%s round %d %-6s %.1f ms for %d new tokens (1 new token: %.1f ms; capture %.1f ms)" % (tag, r, f, s * 1e3, a.new, s1 * 1e3,
                                                                                                              cap * 1e3))
            m1, ms = {f: med(first[f]) for f in kw}, {f: med(step[f]) for f in kw}
            spread = {f: (max(step[f]) - min(step[f])) / ms[f] for f in kw}
            eq = (toks["shared"] == toks["parent"]).all(dim=0).tolist()
            part_at = eq.index(False) - prompt if False in eq else None
            r1, rs = m1["shared"] / m1["parent"], ms["shared"] / ms["parent"]
            own = a.new / 2
            say("%s: prompt pass parent %.1f ms | shared %.1f ms (x%.3f; rows ratio %.3f) || ms per generated position parent %.3f | shared %.3f "
                "(x%.3f; KV bytes ratio %.3f; spread %.1f / %.1f %%; condition <= %.2f); tokens part at new token %s of %d" % (
                    tag, m1["parent"], m1["shared"], r1, 1 / NB, ms["parent"], ms["shared"], rs, (prompt / NB + own) / (prompt + own),
                    spread["parent"] * 100, spread["shared"] * 100, THRESHOLD, "none" if part_at is None else str(part_at), a.new))
            for what, ratio in (("prompt pass", r1), ("generated position", rs)):
                if ratio > THRESHOLD:
                    misses += 1
                    say("MISS: %s: the share_prompt %s is more than %.0f %% slower than the parent path's" % (tag, what, (THRESHOLD - 1) * 100))
            result[tag] = {"prompt_pass_ms": m1, "ms_per_position": ms, "all": step, "shared_over_parent": {"prompt_pass": r1, "position": rs},
                           "tokens_part_at": part_at}
            del vx, ids
            gc.collect()
            torch.cuda.empty_cache()
    say("part generate: conditions missed: %d of %d" % (misses, 2 * len(result)))
    return result


# ---- parent ---------------------------------------------------------------------------------------------------------------------------------

def run_child(a, part):
    cmd = ["timeout", "-k", "10", str(PART_SECONDS[part]), sys.executable, os.path.abspath(__file__), "--child", part, "--rounds", str(a.rounds),
           "--new", str(a.new), "--layers", str(a.layers), "--kv-dtype", a.kv_dtype, "--sentences"] + [str(r) for r in a.sentences] + ["--prompts"] + [str(p) for p in a.prompts]
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
    ap.add_argument("--sentences", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--prompts", type=int, nargs="+", default=[512, 1536])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--kv-dtype", choices=["bf16", "int8"], default="bf16")
    ap.add_argument("--child", choices=list(PART_SECONDS), default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        if not torch.cuda.is_available():
            raise SystemExit("shared_prefix_bench: no GPU visible (this tool measures; it has no CPU mode)")
        say = lambda s: print(s, flush=True)
        dev = torch.cuda.get_device_properties(0)
        say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
        kernel = kernel_part_i8 if a.kv_dtype == "int8" else kernel_part
        result = kernel(a, say) if a.child == "kernel" else generate_part(a, say)
        say(json.dumps(result))
        return
    lines = ["shared_prefix_bench: parts %s; sentences %s; prompts %s; %d rounds; %d new tokens; %d decoder layers" % (
        " ".join(a.parts), a.sentences, a.prompts, a.rounds, a.new, a.layers) + ("; int8 KV cache" if a.kv_dtype == "int8" else "")]
    status = 0
    for part in a.parts:
        rc, out = run_child(a, part)
        lines += out
        if rc != 0:
            lines.append("shared_prefix_bench: part %s ended with status %s; nothing more is started" % (part, rc))
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
