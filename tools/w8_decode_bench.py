"""Cached generation at OTTER-MPT7B shape: ms per decode step of the int8 frozen decoder (otter_amd/quant.py, csrc/w8.hip) against the
unquantised bf16 decoder, alternated in one process.

Full 32-layer OTTER-MPT7B with synthetic weights (bench.build_model: frozen weights bf16, trainable ones fp32, bf16 autocast -- the
production mode), one 224 x 224 image, a PROMPT-token prompt (prefill, not timed), then STEPS greedy tokens (no end token) fed back one at
a time against the KV cache, the way generate(use_cache=True) does.  The quantised model is a deep copy of the unquantised one after
quantize_decoder_int8(); both stay resident.  Clock: torch.cuda.synchronize() + perf_counter around the decode steps only; one warm-up
run per model and batch before the timed rounds; the median of ROUNDS alternating rounds is reported, with torch.cuda.memory_allocated()
of either model.

  python tools/w8_decode_bench.py [--batch 1 4] [--rounds 3] [--steps 64] [--prompt 512] [--layers 32] [--out profiles/r08_w8_decode_ab.txt]"""
from __future__ import annotations

import argparse
import copy
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


@torch.no_grad()
def decode(model, vx, ids, steps):
    """prompt pass + `steps` greedy cached steps; returns (ms per step, generated ids [B, steps])."""
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(vision_x=vx, lang_x=ids, use_cache=True, clear_conditioned_layers=False)
        past = out.past_key_values
        nxt = out.logits[:, -1].argmax(-1, keepdim=True)
        toks = [nxt]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = model(vision_x=None, lang_x=nxt, use_cached_vision_x=True, past_key_values=past, use_cache=True, clear_conditioned_layers=False)
            past = out.past_key_values
            nxt = out.logits[:, -1].argmax(-1, keepdim=True)
            toks.append(nxt)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        model.lang_encoder.clear_conditioned_layers()
    return ms, torch.cat(toks, 1)[:, :steps]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("w8_decode_bench: no GPU visible (this tool measures; it has no CPU mode)")
    import bench

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.cuda.get_device_properties(0)
    say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
    say("model: OTTER-MPT7B shape, %d decoder layers, synthetic weights, bf16 autocast; 1 image, prompt %d tokens; %d greedy cached steps" % (
        a.layers, a.prompt, a.steps))
    gc.collect()
    m0 = torch.cuda.memory_allocated()
    plain = bench.build_model("cuda:0", seed=0, debug_layers=0 if a.layers == 32 else a.layers).eval()
    m1 = torch.cuda.memory_allocated()
    int8 = copy.deepcopy(plain)
    info = int8.quantize_decoder_int8()
    gc.collect()
    m2 = torch.cuda.memory_allocated()
    say("memory_allocated: unquantised model %.3f GB, quantised model %.3f GB (replaced %d linears: %.3f GB -> %.3f GB)" % (
        (m1 - m0) / 1e9, (m2 - m1) / 1e9, info["replaced"], info["bytes_before"] / 1e9, info["bytes_after"] / 1e9))
    models = {"int8": int8, "bf16": plain}
    result = {"memory_allocated": {"bf16": m1 - m0, "int8": m2 - m1}, "quantize": info}
    for B in a.batch:
        vx, ids, _, _, _ = bench.synth_batch(plain, B, a.prompt, "cuda:0", seed=17)
        vx = vx.to(torch.bfloat16)
        for k in models:                                 # warm-up: allocator, library handles, kernel loads, weight copies of the bf16 path
            decode(models[k], vx, ids, 8)
        t, tok = {"int8": [], "bf16": []}, {}
        for r in range(a.rounds):
            for k in ("int8", "bf16"):
                ms, out = decode(models[k], vx, ids, a.steps)
                t[k].append(ms)
                tok.setdefault(k, out[:, :16].cpu())
                say("B=%d round %d %-4s %.3f ms/step" % (B, r, k, ms))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        agree = float((tok["int8"] == tok["bf16"]).float().mean())
        result["B%d" % B] = {"ms_per_step": t, "median": med, "speedup": med["bf16"] / med["int8"], "first_16_tokens_equal_fraction": agree}
        say("B=%d median: int8 %.3f ms/step, bf16 %.3f ms/step (x%.3f); first 16 tokens equal: %.2f (different weights: quantisation error)" % (
            B, med["int8"], med["bf16"], med["bf16"] / med["int8"], agree))
        if med["int8"] > med["bf16"]:
            say("MISS: the quantised decode step is slower than the unquantised one at B=%d" % B)
    say("memory_allocated now (both models + caches of the bf16 path): %.3f GB" % (torch.cuda.memory_allocated() / 1e9))
    say(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
