"""Rank classification over a cached prompt, at OTTER-MPT7B shape: `model.score_candidates` (StaticKVCache.attend_branches: csrc/flash.hip over
the cache in place + csrc/branch_attn.hip) against the two ways the code offered before, all three in one process.

Contenders, per point (B sentences, a prompt of --prompt tokens, C candidates of 1-8 tokens, the same list for every sentence):
  a  steps      the reference's cached procedure on the existing paths (evaluate.py:1049-1176 with cache_media): ONE prompt pass of B rows into a
                StaticKVCache + MediaCache, then per candidate the teacher-forced one-token steps of B rows (cache_implementation="static" +
                cross_attention_cache=True as the hosts run it), the cache rewound to the prompt after every candidate
  b  reforward  the reference's no_kv_caching branch: per candidate one uncached forward over prompt + candidate
  c  score      model.score_candidates
a and b are sequential per candidate, so their time per candidate does not depend on C: with --sample K they run the first K candidates and
the tool reports that time x C / K, marked "scaled".  One warm-up of every contender, then --rounds alternating rounds; the median.  Clock:
torch.cuda.synchronize() + perf_counter around the whole procedure, prompt pass and vision encoder included.
Also: the top-1 agreement of c with b (over the candidates b ran) and c's peak memory above the resident model.
Condition, per point: c <= 1.03 x a (3 %: tools/regress.sh's margin); a point that misses prints MISS.

Every point (B x decoder) is a child process of this tool under its own `timeout`; the tool stops at the first non-zero status.

  python tools/score_candidates_bench.py [--sentences 1 4] [--candidates 64 1000] [--decoders bf16 int8] [--prompt 512] [--rounds 3]
                                         [--sample 0] [--layers 32] [--max-rows 1024] [--out profiles/r22_score_candidates.txt]"""
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
T_MAX = 8
POINT_SECONDS = 1080
DEV = "cuda:0"


def candidates(C, vocab, media_id, seed=3):
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(5, min(vocab, 30000), (C, T_MAX), generator=g)
    cand[cand == media_id] = 4
    lens = torch.randint(1, T_MAX + 1, (C,), generator=g)
    lens[0] = T_MAX
    return cand.to(DEV), (torch.arange(T_MAX).expand(C, T_MAX) < lens[:, None]).to(DEV), lens.tolist()


@torch.no_grad()
def run_steps(model, vx, ids, cand, lens, K):
    """a: scores [B, K] of the first K candidates."""
    from otter_amd.kv_cache import StaticKVCache, cache_geometry
    from otter_amd.media_cache import MediaCache

    B, P = ids.shape
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    cache, mc = StaticKVCache(n_layers, B, n_kv, hd, P + T_MAX + 1, DEV), MediaCache(B, model.media_token_id)
    out = model(vision_x=vx, lang_x=ids, past_key_values=cache, use_cache=True, clear_conditioned_layers=False, media_cache=mc,
                _last_position_only=True)
    first = torch.log_softmax(out.logits[:, -1].float(), -1)
    seen = mc.seen.clone()
    scores = torch.zeros(B, K, device=DEV)
    for c in range(K):
        scores[:, c] = first[:, cand[c, 0]]
        for t in range(lens[c] - 1):
            out = model(vision_x=None, lang_x=cand[c, t].expand(B, 1), use_cached_vision_x=True, past_key_values=cache, use_cache=True,
                        clear_conditioned_layers=False, media_cache=mc, _last_position_only=True)
            scores[:, c] += torch.log_softmax(out.logits[:, -1].float(), -1)[:, cand[c, t + 1]]
        cache.length = P                                   # rewind to the prompt: the next candidate overwrites the slots behind it
        mc.seen.copy_(seen)
    model.lang_encoder.clear_conditioned_layers()
    return scores


@torch.no_grad()
def run_reforward(model, vx, ids, cand, lens, K):
    """b: scores [B, K] of the first K candidates."""
    B, P = ids.shape
    scores = torch.zeros(B, K, device=DEV)
    for c in range(K):
        L = lens[c]
        full = torch.cat([ids, cand[c, :L].expand(B, L)], dim=1)
        lp = torch.log_softmax(model(vision_x=vx, lang_x=full, use_cache=False).logits[:, P - 1:P + L - 1].float(), -1)
        scores[:, c] = lp.gather(2, cand[c, :L].expand(B, L).unsqueeze(-1)).sum(dim=(1, 2))
    return scores


@torch.no_grad()
def run_score(model, vx, ids, cand, cmask, max_rows):
    return model.score_candidates(vx, ids, None, candidates=cand, candidate_mask=cmask, max_rows=max_rows)


def point(a, say):
    import bench

    B, decoder = a.child
    model = bench.build_model(DEV, seed=0, debug_layers=0 if a.layers == 32 else a.layers).eval()
    if decoder == "int8":
        model.quantize_decoder_int8(gated_blocks=True, lm_head=True)
    gc.collect()
    torch.cuda.empty_cache()
    resident = torch.cuda.memory_allocated()
    say("point B=%d %s decoder, %d layers, prompt %d: model resident %.2f GB" % (B, decoder, a.layers, a.prompt, resident / 1e9))
    vx, ids, _, _, _ = bench.synth_batch(model, B, a.prompt, DEV, seed=17)
    vx = vx.to(torch.bfloat16)
    vocab = model.lang_encoder.get_input_embeddings().weight.shape[0]
    med = lambda xs: sorted(xs)[len(xs) // 2]
    result, misses = {}, 0
    for C in a.candidates:
        cand, cmask, lens = candidates(C, vocab, model.media_token_id)
        K = min(a.sample, C) if a.sample > 0 else C
        fns = {"steps": lambda: run_steps(model, vx, ids, cand, lens, K), "reforward": lambda: run_reforward(model, vx, ids, cand, lens, K),
               "score": lambda: run_score(model, vx, ids, cand, cmask, a.max_rows)}
        ms, out, peak = {f: [] for f in fns}, {}, 0
        with torch.autocast("cuda", dtype=torch.bfloat16):
            for r in range(-1, a.rounds):                  # round -1: the warm-up (allocator, kernel loads, workspaces)
                for f in fns:
                    gc.collect()
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    t0 = time.perf_counter()
                    out[f] = fns[f]()
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    if f == "score":
                        peak = max(peak, torch.cuda.max_memory_allocated() - resident)
                    if r >= 0:
                        ms[f].append(dt * (C / K if f != "score" else 1.0))
                        say("B=%d %s C=%d round %d %-9s %.1f ms%s" % (B, decoder, C, r, f, ms[f][-1], " (scaled from %d candidates)" % K
                                                                        if f != "score" and K < C else ""))
        m = {f: med(ms[f]) for f in fns}
        spread = {f: (max(ms[f]) - min(ms[f])) / m[f] for f in fns}
        top1 = float((out["score"][:, :K].argmax(1) == out["reforward"].argmax(1)).float().mean())
        top1_steps = float((out["steps"].argmax(1) == out["reforward"].argmax(1)).float().mean())
        ratio = m["score"] / m["steps"]
        tag = "B=%d %s C=%d" % (B, decoder, C)
        say("%s: steps %.1f ms | reforward %.1f ms | score_candidates %.1f ms = x%.4f of steps, x%.4f of reforward (spread %.1f / %.1f / %.1f %%; "
            "condition <= %.2f); top-1 of score_candidates = top-1 of reforward on %.0f %% of the sentences (steps: %.0f %%; among the first %d "
            "candidates); peak memory above the model %.2f GB" % (tag, m["steps"], m["reforward"], m["score"], ratio, m["score"] / m["reforward"],
                                                                   spread["steps"] * 100, spread["reforward"] * 100, spread["score"] * 100,
                                                                   THRESHOLD, top1 * 100, top1_steps * 100, K, peak / 1e9))
        if ratio > THRESHOLD:
            misses += 1
            say("MISS: %s: score_candidates is more than %.0f %% slower than the cached steps" % (tag, (THRESHOLD - 1) * 100))
        result[tag] = {"ms": m, "all_ms": ms, "score_over_steps": ratio, "score_over_reforward": m["score"] / m["reforward"], "top1_vs_reforward": top1,
                       "peak_bytes_above_model": peak, "sampled_candidates": K}
    say("point B=%d %s: conditions missed: %d of %d" % (B, decoder, misses, len(result)))
    return result


def run_child(a, B, decoder):
    cmd = ["timeout", "-k", "10", str(POINT_SECONDS), sys.executable, os.path.abspath(__file__), "--child", str(B), decoder, "--prompt", str(a.prompt),
           "--rounds", str(a.rounds), "--sample", str(a.sample), "--layers", str(a.layers), "--max-rows", str(a.max_rows), "--candidates"] + [
               str(c) for c in a.candidates]
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
    ap.add_argument("--sentences", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--candidates", type=int, nargs="+", default=[64, 1000])
    ap.add_argument("--decoders", nargs="+", choices=["bf16", "int8"], default=["bf16", "int8"])
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sample", type=int, default=0, help="contenders a and b run this many candidates, their time scaled by C / K (0: all)")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--max-rows", type=int, default=1024)
    ap.add_argument("--child", nargs=2, default=None, metavar=("B", "DECODER"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        if not torch.cuda.is_available():
            raise SystemExit("score_candidates_bench: no GPU visible (this tool measures; it has no CPU mode)")
        a.child = (int(a.child[0]), a.child[1])
        say = lambda s: print(s, flush=True)
        dev = torch.cuda.get_device_properties(0)
        say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
        say(json.dumps(point(a, say)))
        return
    lines = ["score_candidates_bench: sentences %s; candidates %s of 1-%d tokens; decoders %s; prompt %d; %d rounds; %d decoder layers; max_rows %d%s"
             % (a.sentences, a.candidates, T_MAX, a.decoders, a.prompt, a.rounds, a.layers, a.max_rows,
                "; contenders a and b on %d candidates, scaled" % a.sample if a.sample else "")]
    status = 0
    for decoder in a.decoders:
        for B in a.sentences:
            rc, out = run_child(a, B, decoder)
            lines += out
            if rc != 0:
                lines.append("score_candidates_bench: point B=%d %s ended with status %s; nothing more is started" % (B, decoder, rc))
                print(lines[-1], flush=True)
                status = 1
                break
        if status:
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
