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

`--switch select` and `--switch sample` measure the token selection of `num_beams == 1` in `ops.select_step`
(csrc/select.hip) at greedy / sampled points of their own -- mpt-tuple-B1 and mpt-graph-B1 / -B4 / -B8 without beams, fuyu-graph with one
row -- with the logits processors on the kernel on both paths.  `select` alternates OTTER_HIP_SELECT on greedy calls (argmax, where, two cats,
isin and the synchronising any() against one launch).  `sample` alternates the host sampler against `device_sampling=True` at
`top_k=50, top_p=0.9, temperature=0.7` under one seed: the two follow different tie and rounding rules (include/otter_hip.h), so where their
tokens differ one more call runs the torch restatement of the kernel's rule (`device_sampling=True`, OTTER_HIP_SELECT=0) over the same draws
and the tool reports whether THAT equals the kernel path -- if so the kernel follows its stated rule -- and one more host-sampler call counts
the steps at which the host splits a group of equal values at the top-p boundary, beside the first position at which the tokens differ.
Several switches may be given: the models are built once.

  python tools/generate_e2e_bench.py [--switch logits|beam|select|sample ...] [--points mpt fuyu] [--rounds 3] [--new 128] [--out FILE]"""
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
SWITCH_VAR = {"logits": "OTTER_HIP_LOGITS", "beam": "OTTER_HIP_BEAM", "select": "OTTER_HIP_SELECT", "sample": "OTTER_HIP_SELECT"}
WHAT = {"logits": "logits processors", "beam": "beam-search block", "select": "greedy token selection", "sample": "token sampling"}
SYMBOL = {"logits": "otter_logits_process", "beam": "otter_beam_step", "select": "otter_select_step", "sample": "otter_select_step"}
SAMPLE = dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.7)
switch = "logits"                      # --switch
THRESHOLD = 1.03
BAD_WORDS = [[11], [12, 13]]
BEAM = dict(num_beams=3, no_repeat_ngram_size=3, bad_words_ids=BAD_WORDS)
GREEDY = dict(no_repeat_ngram_size=3)
FAST = dict(cache_implementation="static", cross_attention_cache=True, graph_decode=True)
FUYU_VOCAB = 262144


@torch.no_grad()
def timed(call, path):
    """(seconds, tokens on the host) of one whole generate call on `path` ("restated": --switch sample's diagnosis call)."""
    os.environ[SWITCH_VAR[switch]] = "1" if switch == "sample" and path != "restated" else SWITCH.get(path, "0")
    extra = {}
    if switch == "sample":
        extra = dict(SAMPLE, device_sampling=path != "host", generator=torch.Generator(device="cuda").manual_seed(1234))
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    toks = call(**extra)
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


def sample_diagnosis(call, host_tokens, kernel_tokens, new):
    """--switch sample, after the clock, when the host sampler and the kernel path returned different tokens.  The two follow different rules
    in two places (include/otter_hip.h): the host's unstable sort splits a group of equal values that straddles the top-p boundary where the
    kernel keeps or removes the group together, and the host normalises the softmax before the race.  Two more calls: the torch restatement of
    the kernel's rule over the same draws (does it return the kernel path's tokens?), and the host sampler with `_top_k_top_p` watched: a step
    SPLITS when, in some row, a value equal to the smallest kept one was removed.  Returns (restatement equals kernel, the first generated
    position at which host and kernel tokens differ, the host path's steps that split, as a list)."""
    from otter_amd import generation as G

    by_rule = torch.equal(timed(call, "restated")[1], kernel_tokens)
    real, split = G._top_k_top_p, []

    def watched(scores, top_k, top_p, min_keep=1):
        out = real(scores, top_k, top_p, min_keep)
        kept = out > float("-inf")
        smallest = torch.where(kept, scores, torch.full_like(scores, float("inf"))).amin(-1, keepdim=True)
        split.append(((scores == smallest) & ~kept).any())
        return out

    G._top_k_top_p = watched
    try:
        timed(call, "host")
    finally:
        G._top_k_top_p = real
    differ = (host_tokens[:, -new:] != kernel_tokens[:, -new:]).any(0).nonzero().flatten().tolist()
    return by_rule, (differ[0] if differ else None), [s for s, flag in enumerate(split) if bool(flag)]


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
        if switch == "sample":
            by_rule, first_diff, splits = sample_diagnosis(call, first_tokens["host"], first_tokens["kernel"], new)
            say("%s: the torch restatement of the kernel's rule (device_sampling=True, OTTER_HIP_SELECT=0) over the same draws against the kernel "
                "path: tokens equal: %s.  Host sampler against kernel path: the tokens first differ at generated position %s; on the host path a "
                "group of equal values is split at the top-p boundary in %d of %d steps, first at step %s (the kernel keeps or removes such a group "
                "together; where no split precedes the first difference, rounding and the host's normalisation before the race are what is left)"
                % (tag, by_rule, first_diff, len(splits), new, splits[0] if splits else None))
            rec["tokens_equal_restatement"], rec["first_difference"], rec["split_steps"] = by_rule, first_diff, splits
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

        def call(**extra):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return model.generate(vision_x=vx, lang_x=ids, max_new_tokens=a.new, eos_token_id=-1, pad_token_id=0, **kw, **extra)

        result[tag] = measure(tag, call, a.new, a.rounds, say)

    global switch
    batches = (8, 1) if a.b8 else (1,)
    for switch in a.switch:
        if switch in ("select", "sample"):
            point("%s: mpt-tuple-B1 (bf16, tuple cache, no beams)" % switch, 1, dict(GREEDY, use_cache=True))
            continue
        for B in batches:
            point("mpt-tuple-B%d (bf16, tuple cache, 3 beams)" % B, B, dict(BEAM, use_cache=True))
    model.quantize_decoder_int8()
    for switch in a.switch:
        if switch in ("select", "sample"):
            for B in ((1, 4, 8) if a.b8 else (1, 4)):
                point("%s: mpt-graph-B%d (int8, static + cross-attention cache, graph replay, no beams)" % (switch, B), B, dict(GREEDY, **FAST))
            continue
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
    global switch
    cache = None
    for switch in a.switch:
        kw = dict(GREEDY) if switch in ("select", "sample") else BEAM
        rows = kw.get("num_beams", 1)
        if cache is None or cache.rows != rows:
            cache = None
            gc.collect()
            torch.cuda.empty_cache()
            cache = StaticKVCache.for_model(model, rows=rows, max_len=a.fuyu_prompt + a.new + 1)

        def call(**extra):
            cache.reset()
            return model.generate(ids, max_new_tokens=a.new, eos_token_id=-1, pad_token_id=0, past_key_values=cache, graph_decode=True, **kw, **extra)

        tag = "fuyu-graph (int8, StaticKVCache, graph replay, 3 beams, prompt %d)" % a.fuyu_prompt
        if switch in ("select", "sample"):
            tag = "%s: fuyu-graph (int8, StaticKVCache, graph replay, no beams, one row, prompt %d)" % (switch, a.fuyu_prompt)
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
    ap.add_argument("--switch", nargs="+", choices=tuple(SWITCH_VAR), default=["logits"])
    ap.add_argument("--b8", action=argparse.BooleanOptionalAction, default=True)
    a = ap.parse_args()
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
    for sw in a.switch:
        say("whole generate() calls, %s in the clock; paths: host (%s) | kernel (%s); %d rounds, alternating"
            % (WHAT[sw], "the host sampler" if sw == "sample" else SWITCH_VAR[sw] + "=0, the host code", SYMBOL[sw], a.rounds))
    result = {}
    if "mpt" in a.points:
        mpt_points(a, say, result)
        write_out()
    if "fuyu" in a.points:
        fuyu_points(a, say, result)
    misses = sum(1 for r in result.values() if r["kernel_over_host"] > THRESHOLD)
    ok = lambda r: r["tokens_equal"] or r.get("tokens_equal_under_tie_rule") or r.get("tokens_equal_restatement")
    differ = sum(1 for r in result.values() if not ok(r))
    by_topk = sum(1 for r in result.values() if not r["tokens_equal"] and r.get("tokens_equal_under_tie_rule"))
    by_rule = sum(1 for r in result.values() if not r["tokens_equal"] and r.get("tokens_equal_restatement"))
    if by_topk:
        say("beam points whose tokens differ from torch.topk's at a tie and equal the host block's under the stated tie rule: %d" % by_topk)
    if by_rule:
        say("sample points whose tokens differ from the host sampler's and equal the torch restatement of the kernel's rule over the same draws: %d"
            % by_rule)
    say("points with a MISS: %d of %d; points whose tokens differ from the host path's: %d, of them not accounted for above: %d"
        % (misses, len(result), sum(1 for r in result.values() if not r["tokens_equal"]), differ))
    say(json.dumps(result))
    write_out()
    if differ:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
