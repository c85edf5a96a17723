"""Whole generate() calls with the logits processors in the clock: the HIP kernel (csrc/logits.hip, ops.logits_process) against the host loop
of otter_amd/generation.py (`ids.tolist()` + a Python loop over positions + one indexed store per row), alternated in one process through
OTTER_HIP_LOGITS -- the switch is read at every call of the processors.

Every model is random-init at full shape, as the decode tools build it (OTTER-MPT7B: bench.build_model, one 224 x 224 image per sentence, bf16
autocast; Fuyu-8B: the Persimmon decoder of tools/fuyu_static_decode_bench.py).  `eos_token_id=-1`: every call runs its full length.  The
arguments are those of the reference's call sites: `num_beams=3, no_repeat_ngram_size=3, bad_words_ids=` one 1-token and one 2-token word.

    point                    host          configuration
    mpt-graph-B8 / -B1       OTTER-MPT7B   int8 decoder + static KV cache + cross-attention cache + graph replay, 3 beams
    mpt-tuple-B8 / -B1       OTTER-MPT7B   bf16, the default tuple cache (use_cache=True), 3 beams
    mpt-greedy-B4            OTTER-MPT7B   int8 + static + cross-attention cache + graph replay, greedy, no_repeat_ngram_size=3 only
    fuyu-graph               Fuyu-8B       int8 decoder + StaticKVCache object + graph replay, 3 beams, one sentence, V = 262144

Clock: torch.cuda.synchronize() + perf_counter around one whole call; one warm-up call per path and point, then ROUNDS rounds alternating
the two paths.  Reported per point: ms per generated position (call time / new tokens) of both paths as the median over rounds, the spread
(max - min) / median, the ratio kernel / host, and whether both paths returned the same tokens -- they must: the tool exits non-zero if not.
Condition (DESIGN.md sections 4.10 / 4.11 / 4.14): kernel <= 1.03 x host at every point; a point that misses prints MISS.

`--switch beam` alternates OTTER_HIP_BEAM instead: the beam-search block between two steps -- candidate selection,
the scorer and the reorder -- in `ops.beam_step` (csrc/beam.hip) against the host block (`torch.topk`, three `.tolist()`, a Python double
loop, three copies back), with the logits processors on the kernel on both paths; the beam points only (the greedy point has no such block).
`--b8` / `--no-b8` keeps or drops the B = 8 points (the longest ones).

  python tools/generate_e2e_bench.py [--switch logits|beam] [--points mpt fuyu] [--rounds 3] [--new 128] [--out profiles/r16_logits_process_ab.txt]"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

PATHS = ("host", "kernel")
SWITCH = {"host": "0", "kernel": "1"}
SWITCH_VAR = {"logits": "OTTER_HIP_LOGITS", "beam": "OTTER_HIP_BEAM"}
WHAT = {"logits": "logits processors", "beam": "beam-search block"}
switch = "logits"                      # --switch
THRESHOLD = 1.03
BAD_WORDS = [[11], [12, 13]]
BEAM = dict(num_beams=3, no_repeat_ngram_size=3, bad_words_ids=BAD_WORDS)
GREEDY = dict(no_repeat_ngram_size=3)
FAST = dict(cache_implementation="static", cross_attention_cache=True, graph_decode=True)
FUYU_VOCAB = 262144


@torch.no_grad()
def timed(call, path):
    """(seconds, tokens on the host) of one whole generate call on `path`."""
    os.environ[SWITCH_VAR[switch]] = SWITCH[path]
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    toks = call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, toks.cpu()


def tie_diagnosis(call, kernel_tokens):
    """--switch beam, after the clock, when the two paths returned different tokens: torch.topk promises no order among equal sums and
    csrc/beam.hip states one (the larger sum first, then the smaller flat index), so the paths may part wherever the host path's top
    n_cand + 1 sums of a sentence hold a tie.  One more host-path call with torch.topk replaced by that rule (a stable descending sort):
    (the first step at which the top k + 1 sums of some sentence are not strictly decreasing, or None; whether that call's tokens equal
    the kernel path's)."""
    real, ties, steps = torch.topk, [], [0]

    def by_the_rule(x, k, dim=-1, largest=True, sorted=True):
        v, i = torch.sort(x, dim=dim, descending=True, stable=True)
        if x.dim() == 2 and x.shape[1] > k:
            ties.append((v[:, :k] <= v[:, 1:k + 1]).any())
        steps[0] += 1
        return v.narrow(dim, 0, k), i.narrow(dim, 0, k)

    torch.topk = by_the_rule
    try:
        _, toks = timed(call, "host")
    finally:
        torch.topk = real
    first = next((s for s, t in enumerate(ties) if bool(t)), None)
    return first, torch.equal(toks, kernel_tokens)


def measure(tag, call, new, rounds, say):
    """Warm-up, then `rounds` alternating rounds; returns the point's record."""
    first = first_tokens = {p: timed(call, p)[1] for p in PATHS}  # warm-up: allocator, kernel loads, workspaces; and the tokens
    t = {p: [] for p in PATHS}
    same = torch.equal(first["host"], first["kernel"])
    for r in range(rounds):
        for p in PATHS:
            s, toks = timed(call, p)
            t[p].append(s * 1e3 / new)
            same = same and torch.equal(toks, first["host"])
            say("%s round %d %-6s %.3f ms per generated position (%.1f ms for %d new tokens)" % (tag, r, p, s * 1e3 / new, s * 1e3, new))
    med = {p: sorted(v)[len(v) // 2] for p, v in t.items()}
    spread = {p: (max(v) - min(v)) / med[p] for p, v in t.items()}
    ratio = med["kernel"] / med["host"]
    say("%s: median ms per generated position host loop %.3f (spread %.1f%%) | kernel %.3f (spread %.1f%%) = x%.3f of the host loop (condition <= %.2f); "
        "tokens equal: %s" % (tag, med["host"], 100 * spread["host"], med["kernel"], 100 * spread["kernel"], ratio, THRESHOLD, same))
    if ratio > THRESHOLD:
        say("MISS: %s: the kernel path is more than %.0f %% slower than the host loop" % (tag, (THRESHOLD - 1) * 100))
    rec = {"ms_per_position": t, "median": med, "spread": spread, "kernel_over_host": ratio, "tokens_equal": same}
    if not same:
        say("TOKENS DIFFER: %s" % tag)
        if switch == "beam":
            first, by_rule = tie_diagnosis(call, first_tokens["kernel"])
            say("%s: the host path's first tie among the top n_cand + 1 sums of a sentence is at step %s (torch.topk promises no order there); "
                "host block with the stated tie rule (stable sort) against the kernel path: tokens equal: %s" % (tag, first, by_rule))
            rec["first_tie_step"], rec["tokens_equal_under_tie_rule"] = first, by_rule
    return rec


def mpt_points(a, say, result):
    import bench

    model = bench.build_model("cuda:0", seed=0, debug_layers=0 if a.layers == 32 else a.layers).eval()
    say("OTTER-MPT7B shape, %d decoder layers, synthetic weights, bf16 autocast; 1 image per sentence; prompt %d; %d new tokens"
        % (a.layers, a.prompt, a.new))

    def point(tag, B, kw):
        vx, ids, _, _, _ = bench.synth_batch(model, B, a.prompt, "cuda:0", seed=17)
        vx = vx.to(torch.bfloat16)

        def call():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return model.generate(vision_x=vx, lang_x=ids, max_new_tokens=a.new, eos_token_id=-1, pad_token_id=0, **kw)

        result[tag] = measure(tag, call, a.new, a.rounds, say)

    batches = (8, 1) if a.b8 else (1,)
    for B in batches:
        point("mpt-tuple-B%d (bf16, tuple cache, 3 beams)" % B, B, dict(BEAM, use_cache=True))
    model.quantize_decoder_int8()
    for B in batches:
        point("mpt-graph-B%d (int8, static + cross-attention cache, graph replay, 3 beams)" % B, B, dict(BEAM, **FAST))
    if switch == "logits":
        point("mpt-greedy-B4 (int8, static + cross-attention cache, graph replay, greedy)", 4, dict(GREEDY, **FAST))
    del model
    gc.collect()
    torch.cuda.empty_cache()


def fuyu_points(a, say, result):
    from fuyu_static_decode_bench import build_model

    from otter_amd.kv_cache import StaticKVCache

    model = build_model(a.fuyu_layers)
    model.quantize_decoder_int8()
    gc.collect()
    torch.cuda.empty_cache()
    say("Persimmon at Fuyu-8B shape, %d layers, vocabulary %d, int8 decoder, random init; prompt %d; %d new tokens"
        % (a.fuyu_layers, FUYU_VOCAB, a.fuyu_prompt, a.new))
    ids = torch.randint(0, FUYU_VOCAB, (1, a.fuyu_prompt), generator=torch.Generator().manual_seed(1)).cuda()
    cache = StaticKVCache.for_model(model, rows=3, max_len=a.fuyu_prompt + a.new + 1)

    def call():
        cache.reset()
        return model.generate(ids, max_new_tokens=a.new, eos_token_id=-1, pad_token_id=0, past_key_values=cache, graph_decode=True, **BEAM)

    tag = "fuyu-graph (int8, StaticKVCache, graph replay, 3 beams, prompt %d)" % a.fuyu_prompt
    result[tag] = measure(tag, call, a.new, a.rounds, say)
    del model, cache
    gc.collect()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", nargs="+", choices=("mpt", "fuyu"), default=["mpt", "fuyu"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--fuyu-prompt", type=int, default=1350)
    ap.add_argument("--fuyu-layers", type=int, default=36)
    ap.add_argument("--out", default=None)
    ap.add_argument("--switch", choices=tuple(SWITCH_VAR), default="logits")
    ap.add_argument("--b8", action=argparse.BooleanOptionalAction, default=True)
    a = ap.parse_args()
    global switch
    switch = a.switch
    if not torch.cuda.is_available():
        raise SystemExit("generate_e2e_bench: no GPU visible (this tool measures; it has no CPU mode)")
    if a.rounds < 3:
        raise SystemExit("generate_e2e_bench: at least three rounds (the spread over rounds is part of the result)")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
    say("whole generate() calls, %s in the clock; paths: host (%s=0, the Python loop) | kernel (%s); %d rounds, alternating"
        % (WHAT[switch], SWITCH_VAR[switch], {"logits": "otter_logits_process", "beam": "otter_beam_step"}[switch], a.rounds))
    result = {}
    if "mpt" in a.points:
        mpt_points(a, say, result)
        write_out()
    if "fuyu" in a.points:
        fuyu_points(a, say, result)
    misses = sum(1 for r in result.values() if r["kernel_over_host"] > THRESHOLD)
    differ = sum(1 for r in result.values() if not (r["tokens_equal"] or r.get("tokens_equal_under_tie_rule")))
    explained = sum(1 for r in result.values() if not r["tokens_equal"] and r.get("tokens_equal_under_tie_rule"))
    if explained:
        say("points whose tokens differ from torch.topk's at a tie and equal the host block's under the stated tie rule: %d" % explained)
    say("points with a MISS: %d of %d; points whose tokens differ: %d" % (misses, len(result), differ))
    say(json.dumps(result))
    write_out()
    if differ:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
