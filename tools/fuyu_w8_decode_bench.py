"""Cached generation at Fuyu-8B shape: ms per decode step of the int8 weight-only decoder (otter_amd/quant.py: quantize_persimmon_decoder,
csrc/w8.hip) against the unquantised bf16 model, alternated in one process.

Random-init PersimmonForCausalLM at Fuyu-8B's shape (hidden 4096, 64 heads x 64, partial_rotary_factor 0.5, 36 layers, FFN 16384, untied
vocabulary 262144), stored in bf16; the int8 model is a deep copy of it after quantize_decoder_int8() (4 linears per layer and lm_head);
both stay resident.  A PROMPT-token prompt (HIP prefill, not timed; BOTH models un-embed its last position only, as generate() does for
the quantised one -- B x PROMPT x 262144 logits are of no use here), then STEPS greedy tokens (no end token) fed back one at a time
against the KV cache on the fused decode step (csrc/persimmon_decode.hip), the way generate() does.  Clock: torch.cuda.synchronize() +
perf_counter around the decode steps only.  Per batch size: one untimed run of each model first (warm-up; it also records the tokens and
the bf16 model's top-2 logits), then ROUNDS rounds alternating the two models.  Reported per point: the median ms per cached step of
either model, the spread (max - min) / median over the rounds, torch.cuda.memory_allocated() of either model alone, and per row the step
at which the two greedy continuations first part, with the bf16 model's top-2 logit margin at that step.

  python tools/fuyu_w8_decode_bench.py [--batch 1 4] [--rounds 3] [--steps 128] [--prompt 1350] [--layers 36] [--out profiles/r14_fuyu_w8_decode_ab.txt]"""
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

VOCAB = 262144


def build_model(layers: int):
    from transformers import PersimmonConfig

    from otter_amd.fuyu import PersimmonForCausalLM

    cfg = PersimmonConfig(vocab_size=VOCAB, hidden_size=4096, intermediate_size=16384, num_hidden_layers=layers, num_attention_heads=64,
                          max_position_embeddings=16384, qk_layernorm=True, partial_rotary_factor=0.5, hidden_act="relu2", layer_norm_eps=1e-5,
                          rope_theta=25000.0, tie_word_embeddings=False, use_cache=True)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = PersimmonForCausalLM(cfg)
    return model.to(torch.bfloat16).eval()


@torch.no_grad()
def decode(model, ids, steps, keep_top2: bool = False):
    """prompt pass + `steps` greedy cached steps; returns (ms per step, generated ids [B, steps], top-2 logits [steps, B, 2] or None).
    Token s of the result comes from the prompt pass for s = 0 and from cached step s - 1 otherwise."""
    out = model(input_ids=ids, use_cache=True, _last_position_only=True)
    past = out.past_key_values
    lg = out.logits[:, -1]
    top2 = [lg.float().topk(2, dim=-1).values] if keep_top2 else None
    nxt = lg.argmax(-1, keepdim=True)
    toks = [nxt]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = model(input_ids=nxt, past_key_values=past, use_cache=True)
        past = out.past_key_values
        lg = out.logits[:, -1]
        if keep_top2:
            top2.append(lg.float().topk(2, dim=-1).values)
        nxt = lg.argmax(-1, keepdim=True)
        toks.append(nxt)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return ms, torch.cat(toks, 1)[:, :steps].cpu(), (torch.stack(top2[:steps]).cpu() if keep_top2 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--prompt", type=int, default=1350)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fuyu_w8_decode_bench: no GPU visible (this tool measures; it has no CPU mode)")
    if a.rounds < 3:
        raise SystemExit("fuyu_w8_decode_bench: at least three rounds (the spread over rounds is part of the result)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.cuda.get_device_properties(0)
    say("device: %s, %d CUs; torch %s" % (dev.name, dev.multi_processor_count, torch.__version__))
    say("model: Persimmon at Fuyu-8B shape, %d layers, vocabulary %d, bf16, random init; prompt %d tokens (last position un-embedded on "
        "both models); %d greedy cached steps" % (a.layers, VOCAB, a.prompt, a.steps))
    gc.collect()
    m0 = torch.cuda.memory_allocated()
    plain = build_model(a.layers)
    gc.collect()
    torch.cuda.empty_cache()
    m1 = torch.cuda.memory_allocated()
    int8 = copy.deepcopy(plain)
    info = int8.quantize_decoder_int8()
    gc.collect()
    torch.cuda.empty_cache()
    m2 = torch.cuda.memory_allocated()
    say("memory_allocated: bf16 model alone %.3f GB, int8 model alone %.3f GB (x%.3f; replaced %d linears: %.3f GB -> %.3f GB)" % (
        (m1 - m0) / 1e9, (m2 - m1) / 1e9, (m2 - m1) / (m1 - m0), info["replaced"], info["bytes_before"] / 1e9, info["bytes_after"] / 1e9))
    models = {"int8": int8, "bf16": plain}
    result = {"memory_allocated": {"bf16": m1 - m0, "int8": m2 - m1}, "quantize": info}
    g = torch.Generator().manual_seed(1)
    for B in a.batch:
        ids = torch.randint(0, VOCAB, (B, a.prompt), generator=g).cuda()
        tok, top2 = {}, None
        for k in ("int8", "bf16"):               # warm-up (allocator, library handles, kernel loads, the dequantisation scratch) + tokens
            _, tok[k], t2 = decode(models[k], ids, a.steps, keep_top2=True)
            top2 = t2 if k == "bf16" else top2
        t = {"int8": [], "bf16": []}
        for r in range(a.rounds):
            for k in ("int8", "bf16"):
                ms, out, _ = decode(models[k], ids, a.steps)
                t[k].append(ms)
                say("B=%d round %d %-4s %.3f ms/step" % (B, r, k, ms))
                if not torch.equal(out, tok[k]):
                    say("NOTE: B=%d round %d %s: tokens differ from the model's own first run" % (B, r, k))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
        div = []
        for b in range(B):
            d = (tok["int8"][b] != tok["bf16"][b]).nonzero()
            if len(d):
                s = int(d[0])
                div.append({"row": b, "token": s, "bf16_top2_margin": float(top2[s, b, 0] - top2[s, b, 1]), "bf16_top1": float(top2[s, b, 0])})
            else:
                div.append({"row": b, "token": None})
        ratio = med["bf16"] / med["int8"]
        result["B%d" % B] = {"ms_per_step": t, "median": med, "spread": spread, "bf16_over_int8": ratio, "first_divergence": div}
        say("B=%d median: int8 %.3f ms/step (spread %.2f%%), bf16 %.3f ms/step (spread %.2f%%): bf16 / int8 = x%.3f" % (
            B, med["int8"], 100 * spread["int8"], med["bf16"], 100 * spread["bf16"], ratio))
        say("B=%d greedy tokens first part at: %s" % (B, json.dumps(div)))
        if ratio - 1.0 <= max(spread.values()):
            say("B=%d: int8 is NOT faster than bf16 by more than the spread over rounds" % B)
    from otter_amd import quant

    say("dequantisation scratch: %d elements (largest decoder weight: %d)" % (sum(b.numel() for b in quant._scratch.values()), 16384 * 4096))
    say(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
