"""Cached generation at Fuyu-8B shape: ms per decode step on the HIP decode path (csrc/persimmon_decode.hip) against the plain path
(OTTER_FUYU_HIP_DECODE=0), alternated in one process.

Random-init bf16 PersimmonForCausalLM at Fuyu-8B's shape (hidden 4096, 64 heads x 64, partial_rotary_factor 0.5, 36 layers, FFN 16384,
vocabulary 262144): a PROMPT-token prompt (HIP prefill, not timed), then STEPS greedy tokens (no end token) fed back one at a time
against the KV cache, the way generate() does.  Clock: torch.cuda.synchronize() + perf_counter around the decode steps only; one
warm-up run per path and batch before the timed rounds.  Token check: the first 32 generated tokens of the two paths, or the first
divergence with the plain path's top-2 logit margin there.

  python tools/fuyu_decode_bench.py [--batch 1 4] [--rounds 3] [--steps 128] [--prompt 1350] [--layers 36] [--out FILE]
  --profile: one prompt + STEPS HIP decode steps only (for rocprofv3 --kernel-trace --stats; see tools/fuyu_decode_launches.py)"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build_model(layers: int):
    from transformers import PersimmonConfig

    from otter_amd.fuyu import PersimmonForCausalLM

    cfg = PersimmonConfig(vocab_size=262144, hidden_size=4096, intermediate_size=16384, num_hidden_layers=layers, num_attention_heads=64,
                          max_position_embeddings=16384, qk_layernorm=True, partial_rotary_factor=0.5, hidden_act="relu2", layer_norm_eps=1e-5,
                          rope_theta=25000.0, tie_word_embeddings=False, use_cache=True)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = PersimmonForCausalLM(cfg)
    return model.to(torch.bfloat16).eval()


@torch.no_grad()
def decode(model, ids, steps, hip: bool, keep_top2: int = 0):
    """prompt pass + `steps` greedy cached steps; returns (ms per step, generated ids [B, steps], top-2 logits of the first steps)."""
    os.environ["OTTER_FUYU_HIP_DECODE"] = "1" if hip else "0"
    out = model(input_ids=ids, use_cache=True)
    past = out.past_key_values
    nxt = out.logits[:, -1].argmax(-1, keepdim=True)
    toks, top2 = [nxt], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = model(input_ids=nxt, past_key_values=past, use_cache=True)
        past = out.past_key_values
        lg = out.logits[:, -1]
        if i < keep_top2:
            top2.append(lg.float().topk(2, dim=-1).values)
        nxt = lg.argmax(-1, keepdim=True)
        toks.append(nxt)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return ms, torch.cat(toks, 1)[:, :steps], top2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--prompt", type=int, default=1350)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model = build_model(a.layers)
    g = torch.Generator().manual_seed(1)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.cuda.get_device_properties(0)
    say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
    say("model: Persimmon at Fuyu-8B shape, %d layers, bf16, random init; prompt %d tokens; %d greedy decode steps" % (a.layers, a.prompt, a.steps))
    if a.profile:
        ids = torch.randint(0, 262144, (a.batch[0], a.prompt), generator=g).cuda()
        decode(model, ids, 4, True)
        ms, _, _ = decode(model, ids, a.steps, True)
        say("profile run: B=%d, %.3f ms per step (HIP decode)" % (a.batch[0], ms))
        return
    result = {}
    for B in a.batch:
        ids = torch.randint(0, 262144, (B, a.prompt), generator=g).cuda()
        decode(model, ids, 8, True)            # warm-up of both paths (allocator, library handles, kernel loads)
        decode(model, ids, 8, False)
        t = {"hip": [], "plain": []}
        tok = {}
        for r in range(a.rounds):
            for mode in ("hip", "plain"):
                ms, ids_out, top2 = decode(model, ids, a.steps, mode == "hip", keep_top2=32 if r == 0 else 0)
                t[mode].append(ms)
                if r == 0:
                    tok[mode] = (ids_out[:, :32].cpu(), [x.cpu() for x in top2])
                say("B=%d round %d %-5s %.3f ms/step" % (B, r, mode, ms))
        h, p = tok["hip"][0], tok["plain"][0]
        same = bool(torch.equal(h, p))
        check = {"first_32_equal": same}
        if not same:
            for b in range(B):
                d = (h[b] != p[b]).nonzero()
                if len(d):
                    s = int(d[0])
                    # ids_out[:, 0] comes from the prompt pass; step s >= 1 was produced by decode step s - 1
                    vals = tok["plain"][1][s - 1][b] if s >= 1 else None
                    margin = float(vals[0] - vals[1]) if vals is not None else None
                    check.setdefault("divergence", []).append({"row": b, "token": s, "plain_top2_margin": margin})
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        result["B%d" % B] = {"ms_per_step": t, "median": med, "speedup": med["plain"] / med["hip"], "tokens": check}
        say("B=%d median: hip %.3f ms/step, plain %.3f ms/step (x%.3f); tokens %s" % (B, med["hip"], med["plain"], med["plain"] / med["hip"],
                                                                                   json.dumps(check)))
    say(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
