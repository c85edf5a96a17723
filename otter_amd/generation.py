"""Token generation for `OtterForConditionalGeneration.generate` (modeling_otter.py:999-1042).

The reference forwards its kwargs to the third-party `GenerationMixin.generate` of the pinned transformers==4.35.1 (not
importable with the transformers installed here).  What its own call sites use is restated here:
greedy search, beam search (`num_beams=3, no_repeat_ngram_size=3, bad_words_ids=...`: pipeline/demos/interactive/*.py,
pipeline/benchmarks/models/otter_{image,video}.py; `length_penalty`, `min_new_tokens`: the benchmark wrappers),
temperature / top-k / top-p sampling (pipeline/demos/demo_models.py:64-71,120-130; the serve UI's `do_sample` checkbox,
pipeline/serve/gradio_web_server.py:362-371) and -- no call site of the reference combines them, restated so that the two switches compose
as they do in GenerationMixin -- beam-sample (`num_beams > 1` with `do_sample`), diverse (group) beam search (`num_beam_groups > 1` with
`diversity_penalty`: generation/utils.py group_beam_search + HammingDiversityLogitsProcessor, round 6) and `prefix_allowed_tokens_fn`.  Not
restated: constrained beam search (`constraints` / `force_words_ids`), contrastive search, assisted decoding -- they raise.  The algorithm is transformers'
(generation/utils.py beam_search + generation/beam_search.py BeamSearchScorer + generation/logits_process.py), restated on
plain tensors around a `step` callback so that it serves both decoder hosts and both decode modes (KV cache or full
re-forward).  Pinned by tests/test_generation.py against `transformers`' own generate() on a shared tiny LLaMA.

On device tensors the tensor-valued logits processors are one HIP launch per step (`ops.logits_process`, csrc/logits.hip; OTTER_HIP_LOGITS=0
switches back); the host loop below is the only path for CPU tensors and the reference that kernel is tested against, bit for bit.  Plain beam
search on device tensors likewise runs candidate selection, the scorer and the reorder in `ops.beam_step` (csrc/beam.hip, `_DeviceBeam`;
OTTER_HIP_BEAM=0 switches back to the host block, which stays the path of CPU tensors, beam-sample and group beam search).  With
`num_beams == 1` the step's token is chosen on the device too (`ops.select_step`, csrc/select.hip, `_DeviceSelect`): greedy by default
(OTTER_HIP_SELECT=0 switches back to the host block), temperature / top-k / top-p sampling when the caller asks for it with
`device_sampling=True` -- its rule is stated in include/otter_hip.h and restated in torch by `_select_reference`, the path of CPU tensors.
"""
from __future__ import annotations

import math
import os
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import ops

NEG_INF = float("-inf")


# ---- logits processors (generation/logits_process.py), applied in transformers' order ----------------------------------


def _repetition_penalty(ids: torch.Tensor, scores: torch.Tensor, penalty: float) -> torch.Tensor:
    s = torch.gather(scores, 1, ids)
    s = torch.where(s < 0, s * penalty, s / penalty)
    return scores.scatter(1, ids, s)


def _no_repeat_ngram(ids: torch.Tensor, scores: torch.Tensor, n: int) -> torch.Tensor:
    """Ban every token that would complete an n-gram already present in the row (prompt included)."""
    L = ids.shape[1]
    if n <= 0 or L + 1 < n:
        return scores
    rows = ids.tolist()
    for r, seq in enumerate(rows):
        if n == 1:
            banned = set(seq)
        else:
            prefix = tuple(seq[L - n + 1:])
            banned = {seq[i + n - 1] for i in range(L - n + 1) if tuple(seq[i:i + n - 1]) == prefix}
        if banned:
            scores[r, list(banned)] = NEG_INF
    return scores


def _no_bad_words(ids: torch.Tensor, scores: torch.Tensor, bad_words: Sequence[Sequence[int]]) -> torch.Tensor:
    single = [w[0] for w in bad_words if len(w) == 1]
    if single:
        scores[:, single] = NEG_INF
    multi = [w for w in bad_words if len(w) > 1]
    if multi:
        rows = ids.tolist()
        for r, seq in enumerate(rows):
            for w in multi:
                k = len(w) - 1
                if k <= len(seq) and seq[len(seq) - k:] == list(w[:-1]):
                    scores[r, w[-1]] = NEG_INF
    return scores


def _top_k_top_p(scores: torch.Tensor, top_k: int, top_p: float, min_keep: int = 1) -> torch.Tensor:
    if top_k and top_k > 0:
        k = min(max(top_k, min_keep), scores.shape[-1])
        kth = torch.topk(scores, k)[0][..., -1, None]
        scores = scores.masked_fill(scores < kth, NEG_INF)
    if top_p is not None and top_p < 1.0:
        sorted_s, sorted_i = torch.sort(scores, descending=False)
        cum = sorted_s.softmax(-1).cumsum(-1)
        remove = cum <= (1 - top_p)
        remove[..., -min_keep:] = False
        scores = scores.masked_fill(remove.scatter(1, sorted_i, remove), NEG_INF)
    return scores


def pack_bad_words(bad_words: Sequence[Sequence[int]]) -> Tuple[List[int], List[int], List[int]]:
    """The lists ops.logits_process reads, from bad words as `_Processors` filtered them: (the one-token words, the tokens of the words of two
    or more tokens laid end to end, their offsets [words + 1]); word i is tokens[offsets[i] : offsets[i + 1]], in the order given."""
    single = [int(w[0]) for w in bad_words if len(w) == 1]
    tokens: List[int] = []
    offsets = [0]
    for w in bad_words:
        if len(w) > 1:
            tokens += [int(t) for t in w]
            offsets.append(len(tokens))
    return single, tokens, offsets


class _Processors:
    def __init__(self, prompt_len: int, eos: List[int], repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_new_tokens, min_length,
                 prefix_allowed_tokens_fn=None, beams_per_sentence: int = 1):
        self.prompt_len, self.eos = prompt_len, eos
        self.prefix_fn, self.per_sent = prefix_allowed_tokens_fn, max(1, int(beams_per_sentence))
        self.rp = float(repetition_penalty) if repetition_penalty not in (None, 1.0) else None
        self.ngram = int(no_repeat_ngram_size or 0)
        self.bad = [list(w) for w in (bad_words_ids or []) if list(w) != eos[:1] and not (len(w) == 1 and w[0] in eos)]
        self.min_new = int(min_new_tokens or 0)
        self.min_len = int(min_length or 0)
        self._lists = None             # the device lists of the HIP path, built on its first call: (device, V, ban, eos, tokens, offsets) or False

    def _device_lists(self, dev, V: int):
        """ban / eos / word tokens / word offsets as int32 tensors on `dev` (None for an empty list), built once.  False when the HIP kernel
        cannot state what the host loop does with them: it skips a listed token outside [0, V) where indexing wraps a negative one and raises
        on the rest, and a penalty it refuses (<= 0 or not finite as an fp32 number) is the host loop's to apply."""
        if self._lists is None or (self._lists is not False and self._lists[:2] != (dev, V)):
            single, tokens, offsets = pack_bad_words(self.bad)
            eos = list(self.eos) if (self.min_len > 0 or self.min_new > 0) else []      # (never suppressed otherwise)
            last = [tokens[o - 1] for o in offsets[1:]]
            if (any(not 0 <= t < V for t in single + eos + last) or any(not -2 ** 31 <= t < 2 ** 31 for t in tokens)
                    or (self.rp is not None and not (1e-30 < self.rp < 1e30))):
                self._lists = False
            else:
                i32 = lambda l: torch.tensor(l, dtype=torch.int32, device=dev) if l else None
                self._lists = (dev, V, i32(single), i32(eos), i32(tokens), i32(offsets) if tokens else None)
        return self._lists

    def _hip(self, ids: torch.Tensor, scores: torch.Tensor) -> bool:
        """The tensor-valued processors in one launch of ops.logits_process, in place on `scores`; False: not taken, the host loop runs."""
        if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1 and ids.device == scores.device
                and ids.dtype == torch.int64 and ids.stride(1) == 1 and 1 <= scores.shape[1] <= ops.LOGITS_PROCESS_MAX_VOCAB
                and ids.shape[1] >= 1 and scores.shape[0] >= 1 and os.environ.get("OTTER_HIP_LOGITS", "1") != "0"):
            return False
        lists = self._device_lists(scores.device, scores.shape[1])
        if lists is False:
            return False
        suppress = bool(self.eos) and (ids.shape[1] < self.min_len or ids.shape[1] - self.prompt_len < self.min_new)
        if self.rp is not None or self.ngram > 0 or self.bad or suppress:
            ops.logits_process(scores, ids, self.rp if self.rp is not None else 1.0, max(self.ngram, 0), lists[2], lists[3], suppress, lists[4],
                               lists[5])
        return True

    def __call__(self, ids: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
        if not self._hip(ids, scores):     # CPU tensors, OTTER_HIP_LOGITS=0, a vocabulary past the kernel's cap: the host loop, the reference
            if self.rp is not None:
                scores = _repetition_penalty(ids, scores, self.rp)
            if self.ngram > 0:
                scores = _no_repeat_ngram(ids, scores, self.ngram)
            if self.bad:
                scores = _no_bad_words(ids, scores, self.bad)
            if self.eos and (ids.shape[1] < self.min_len or ids.shape[1] - self.prompt_len < self.min_new):
                scores[:, self.eos] = NEG_INF
        if self.prefix_fn is not None:
            # PrefixConstrainedLogitsProcessor: fn(sentence index, tokens so far) -> the ids allowed next; rows are [sentence][beam]
            keep = torch.full_like(scores, NEG_INF)
            for r in range(ids.shape[0]):
                allowed = list(self.prefix_fn(r // self.per_sent, ids[r]))
                if not allowed:
                    raise ValueError("`prefix_allowed_tokens_fn` returned an empty list for sentence %d" % (r // self.per_sent))
                keep[r, allowed] = 0.0
            scores = scores + keep
        return scores


# ---- beam hypotheses (generation/beam_search.py) ---------------------------------------------------------------------


class _BeamHyps:
    def __init__(self, num_beams: int, length_penalty: float, early_stopping):
        self.num_beams, self.lp, self.early = num_beams, length_penalty, early_stopping
        self.beams: List[Tuple[float, torch.Tensor]] = []
        self.worst = 1e9

    def __len__(self):
        return len(self.beams)

    def add(self, hyp: torch.Tensor, sum_logprobs: float, generated_len: int):
        score = sum_logprobs / (generated_len ** self.lp)
        if len(self) < self.num_beams or score > self.worst:
            self.beams.append((score, hyp))
            if len(self) > self.num_beams:
                srt = sorted((s, i) for i, (s, _) in enumerate(self.beams))
                del self.beams[srt[0][1]]
                self.worst = srt[1][0]
            else:
                self.worst = min(score, self.worst)

    def is_done(self, best_sum_logprobs: float, cur_len: int, prompt_len: int, max_length: int) -> bool:
        if len(self) < self.num_beams:
            return False
        if self.early is True:
            return True
        if self.early is False:
            return self.worst >= best_sum_logprobs / (cur_len - prompt_len) ** self.lp
        # "never": the best score any continuation could still reach
        if self.lp > 0.0:
            return self.worst >= best_sum_logprobs / (max_length - prompt_len) ** self.lp
        return self.worst >= best_sum_logprobs / (cur_len - prompt_len) ** self.lp


def beam_len_pow(n: int, length_penalty: float) -> List[float]:
    """len_pow[g] = float(g) ** length_penalty for 0 <= g < n -- `generated_len ** self.lp` of _BeamHyps.add as Python evaluates it, so that the
    device divides by the host's own bits.  Entry 0 is never read (a hypothesis has at least one generated token); a negative penalty gives it inf."""
    lp = float(length_penalty)
    out = []
    for g in range(n):
        try:
            out.append(float(g) ** lp)
        except ZeroDivisionError:
            out.append(math.inf)
    return out


def rebuild_beam_hyps(nb: int, length_penalty: float, early_stopping, count: int, scores: Sequence[float], lens: Sequence[int],
                      slots: Sequence[int], worst: float, tokens: torch.Tensor) -> _BeamHyps:
    """The _BeamHyps of one sentence from the state ops.beam_step keeps: `beams` in list order -- entry i is (scores[i], tokens[slots[i],
    :lens[i]]), tokens [nb, max_len] on any device -- and `worst`."""
    h = _BeamHyps(nb, length_penalty, early_stopping)
    h.beams = [(float(scores[i]), tokens[int(slots[i]), :int(lens[i])]) for i in range(int(count))]
    h.worst = float(worst)
    return h


class _DeviceBeam:
    """The state of one beam search on the device, allocated once per generate_tokens call at fixed addresses: the scalars of the scorer in ONE
    byte blob (so that one copy brings them to the host after the loop), the hypotheses' token rows, the ping-pong token history
    [2, N, max_len], beam_idx, the length-penalty table and the kernel's workspace.  `step` is one ops.beam_step call and nothing else."""

    FIELDS = (("hyp_score", torch.float64, "N"), ("hyp_worst", torch.float64, "B"), ("beam_scores", torch.float32, "N"),
              ("hyp_len", torch.int32, "N"), ("hyp_slot", torch.int32, "N"), ("hyp_count", torch.int32, "B"), ("done", torch.int32, "B"),
              ("all_done", torch.int32, 2))

    @classmethod
    def carve(cls, blob: Optional[torch.Tensor], B: int, nb: int):
        """(views of `blob` by field name, the blob's size in bytes); every field starts on an 8-byte boundary."""
        views, off = {}, 0
        for name, dtype, n in cls.FIELDS:
            n = {"N": B * nb, "B": B}.get(n, n)
            size = n * torch.empty(0, dtype=dtype).element_size()
            if blob is not None:
                views[name] = blob[off:off + size].view(dtype)
            off += (size + 7) // 8 * 8
        return views, off

    @staticmethod
    def usable(logp: torch.Tensor, ids: torch.Tensor, nb: int, n_cand: int) -> bool:
        return (logp.is_cuda and logp.dtype == torch.float32 and logp.dim() == 2 and logp.stride(1) == 1 and ids.device == logp.device
                and ids.dtype == torch.int64 and ids.dim() == 2 and ids.stride(1) == 1 and ids.shape[1] >= 1 and ids.shape[0] == logp.shape[0]
                and n_cand <= ops.BEAM_STEP_MAX_CANDIDATES and n_cand <= nb * logp.shape[1] and nb * logp.shape[1] < 2 ** 31
                and logp.shape[0] <= 65535 and os.environ.get("OTTER_HIP_BEAM", "1") != "0")

    def __init__(self, B: int, nb: int, V: int, L0: int, max_len: int, eos: List[int], pad_token_id: int, length_penalty: float, early_stopping,
                 beam_scores: torch.Tensor):
        dev = beam_scores.device
        self.B, self.nb, self.L0, self.max_len, self.eos, self.pad = B, nb, L0, max_len, eos, int(pad_token_id)
        self.lp, self.early = float(length_penalty), early_stopping
        self.n_cand = max(2, 1 + len(eos)) * nb
        N = B * nb
        _, size = self.carve(None, B, nb)
        host = torch.zeros(size, dtype=torch.uint8)
        v, _ = self.carve(host, B, nb)
        v["hyp_worst"].fill_(1e9)
        self.blob = host.to(dev)
        self.v, _ = self.carve(self.blob, B, nb)
        self.v["beam_scores"].copy_(beam_scores)
        self.len_pow = torch.tensor(beam_len_pow(max_len - L0 + 1, self.lp), dtype=torch.float64).to(dev)
        self.eos_t = torch.tensor(eos, dtype=torch.int32).to(dev) if eos else None
        self.hyp_tokens = torch.zeros(B, nb, max_len, dtype=torch.int64, device=dev)
        self.ids_buf = torch.zeros(2, N, max_len, dtype=torch.int64, device=dev)
        self.beam_idx = torch.zeros(N, dtype=torch.int64, device=dev)
        self.workspace = torch.empty(ops.beam_step_workspace_bytes(B, nb, V, self.n_cand), dtype=torch.uint8, device=dev)
        self.steps = 0

    def step(self, logp: torch.Tensor, ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(the next ids [N, L + 1], a view of the other half of the ping-pong buffer; beam_idx [N])."""
        v = self.v
        nxt = self.ids_buf[self.steps % 2][:, :ids.shape[1] + 1]
        self.steps += 1
        if logp.stride(1) != 1:
            logp = logp.contiguous()
        ops.beam_step(logp, v["beam_scores"], ids, nxt, self.beam_idx, self.eos_t, self.pad, self.nb, self.n_cand, self.L0, self.max_len,
                      self.early, self.lp > 0.0, self.len_pow, v["done"], v["hyp_score"], self.hyp_tokens, v["hyp_len"], v["hyp_slot"],
                      v["hyp_count"], v["hyp_worst"], v["all_done"], self.workspace)
        return nxt, self.beam_idx

    def all_done(self) -> bool:
        """The 4-byte flag: the one synchronising read of a step (made only when an eos list exists -- nothing finishes early without one)."""
        return bool(self.v["all_done"][0].item())

    def finish(self) -> Tuple[List[_BeamHyps], List[bool], torch.Tensor]:
        """ONE copy of the scalar state to the host: (the _BeamHyps of every sentence, their token rows views of the device buffer; done; the beam
        scores as a CPU tensor)."""
        h, _ = self.carve(self.blob.cpu(), self.B, self.nb)
        nb = self.nb
        sc, ln, sl = h["hyp_score"].tolist(), h["hyp_len"].tolist(), h["hyp_slot"].tolist()
        cnt, worst = h["hyp_count"].tolist(), h["hyp_worst"].tolist()
        hyps = [rebuild_beam_hyps(nb, self.lp, self.early, cnt[b], sc[b * nb:(b + 1) * nb], ln[b * nb:(b + 1) * nb], sl[b * nb:(b + 1) * nb],
                                  worst[b], self.hyp_tokens[b]) for b in range(self.B)]
        return hyps, [bool(d) for d in h["done"].tolist()], h["beam_scores"]


# ---- token selection on the device (csrc/select.hip) --------------------------------------------------------------------------------------


def inv_temperature_f32(temperature) -> Optional[float]:
    """fp32(1) / fp32(temperature) as a Python float, what ops.select_step multiplies the scores by; None when the temperature or its
    reciprocal is not a finite positive fp32 number (the host block then keeps the call)."""
    try:
        t = torch.tensor(1.0 if temperature is None else float(temperature), dtype=torch.float32)
    except (TypeError, ValueError, OverflowError):
        return None
    inv = float(torch.ones((), dtype=torch.float32) / t)
    return inv if (math.isfinite(float(t)) and float(t) > 0.0 and math.isfinite(inv) and inv > 0.0) else None


def _select_reference(scores: torch.Tensor, q: torch.Tensor, inv_t: float, top_k: int, top_p: float) -> torch.Tensor:
    """The sample rule of otter_select_step (include/otter_hip.h) restated in torch, in the same fp32 arithmetic and with the same tie rules:
    the token [N] int64 of every row of scores fp32 [N, V] under the exponential draws q [N, V].  The path of `device_sampling=True` on CPU
    tensors and with OTTER_HIP_SELECT=0, and what the kernel is compared with."""
    s = scores.float() * float(inv_t) + 0.0                      # s' (the sum turns -0 into +0; values compare equal either way)
    q = q.float()
    N, V = s.shape
    out = torch.empty(N, dtype=torch.long, device=s.device)
    for r in range(N):
        row = s[r]
        m = row.max()
        if not bool(torch.isfinite(m)):                          # a NaN or no finite score: some token (the arg max; the host path raises here)
            out[r] = torch.argmax(row)
            continue
        keep = torch.ones(V, dtype=torch.bool, device=s.device)
        if top_k and top_k > 0:
            kth = torch.topk(row, min(max(int(top_k), 1), V))[0][-1]
            keep = row >= kth
        e = torch.exp(row - m)
        if top_p < 1.0:
            vals, order = torch.sort(row[keep])
            w = (e[keep][order].double() * float(2 ** 40)).to(torch.int64)     # floor: the numerators are >= 0
            cum = w.cumsum(0)                                    # exact: at most 2^18 terms of at most 2^40
            Z = int(cum[-1])
            R = min(int((1.0 - float(top_p)) * float(Z)), Z - 1)
            group_cum = cum[torch.searchsorted(vals, vals, right=True) - 1]      # equal values are kept or removed together
            keep = keep & (row >= vals[group_cum > R][0])
        ratio = e / q[r]
        ratio = torch.where(keep & ~torch.isnan(ratio), ratio, torch.full_like(ratio, -1.0))
        out[r] = (ratio == ratio.max()).nonzero()[0, 0]          # the smaller index among equal ratios
    return out


class _DeviceSelect:
    """The state of one greedy or sampled generation on the device, allocated once per generate_tokens call at fixed addresses: the token
    history [B, max_len] and the attention mask [B, max_len] (the step is handed [:, :L] views: nothing is concatenated), `unfinished`, the
    4-byte count of unfinished rows, the eos list and, in sample mode, the buffer of exponential draws.  `step` is one ops.select_step call
    (and, in sample mode, the refill of the draws)."""

    @staticmethod
    def usable(scores: torch.Tensor, ids: torch.Tensor, mask: Optional[torch.Tensor]) -> bool:
        return (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1 and ids.device == scores.device
                and ids.dtype == torch.int64 and ids.dim() == 2 and ids.shape[0] == scores.shape[0] and scores.shape[0] >= 1
                and 1 <= scores.shape[1] <= ops.SELECT_STEP_MAX_VOCAB and (mask is None or mask.device == scores.device)
                and os.environ.get("OTTER_HIP_SELECT", "1") != "0")

    def __init__(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], max_len: int, eos_t: Optional[torch.Tensor],
                 pad_token_id: int, sample: Optional[Tuple[float, int, float]], generator: Optional[torch.Generator]):
        B, L0 = input_ids.shape
        dev = input_ids.device
        self.L, self.max_len, self.pad, self.sample, self.generator = L0, max_len, int(pad_token_id), sample, generator
        self.ids_buf = torch.zeros(B, max_len, dtype=torch.int64, device=dev)
        self.ids_buf[:, :L0] = input_ids
        self.mask_buf = None
        if attention_mask is not None:
            self.mask_buf = torch.ones(B, max_len, dtype=attention_mask.dtype, device=dev)
            self.mask_buf[:, :L0] = attention_mask
        self.unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        self.n_unfinished = torch.full((1,), B, dtype=torch.int32, device=dev)
        self.eos_t = eos_t.to(torch.int32) if eos_t is not None else None          # (the loop's device list: no further copy from the host)
        self.q = None

    def views(self) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        return self.ids_buf[:, :self.L], (self.mask_buf[:, :self.L] if self.mask_buf is not None else None)

    def step(self, scores: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Writes the step's tokens into column L; (ids [B, L + 1], mask [B, L + 1] or None), views of the buffers."""
        if self.sample is None:
            ops.select_step(scores, self.ids_buf, self.L, self.unfinished, self.n_unfinished, self.eos_t, self.pad)
        else:
            if self.q is None:
                self.q = torch.empty(scores.shape, dtype=torch.float32, device=scores.device)
            self.q.exponential_(1, generator=self.generator)     # the draws torch.multinomial makes: a seeded generator advances as before
            inv_t, k, p = self.sample
            ops.select_step(scores, self.ids_buf, self.L, self.unfinished, self.n_unfinished, self.eos_t, self.pad, True, inv_t, k, p, self.q)
        self.L += 1
        return self.views()

    def all_finished(self) -> bool:
        """The 4-byte count: the one synchronising read of a step (made only when an eos list exists -- nothing finishes early without one)."""
        return int(self.n_unfinished.item()) <= 0

    def result(self) -> torch.Tensor:
        return self.ids_buf[:, :self.L].contiguous()


# ---- the loop ----------------------------------------------------------------------------------------------------------

# step(ids [N,L], mask [N,L] or None, past, beam_idx [N] or None) -> (last-position logits [N,V], past)
StepFn = Callable[[torch.Tensor, Optional[torch.Tensor], object, Optional[torch.Tensor]], Tuple[torch.Tensor, object]]


def resolve_max_length(prompt_len: int, max_new_tokens: Optional[int] = None, max_length: Optional[int] = None) -> int:
    """The total length (prompt included) generation stops at: `max_new_tokens` wins over `max_length`; neither: 20 new tokens."""
    if max_new_tokens is not None:
        return prompt_len + int(max_new_tokens)
    if max_length is not None:
        return int(max_length)
    return prompt_len + 20


@torch.no_grad()
def generate_tokens(step: StepFn, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, *, max_new_tokens: Optional[int] = None,
                    max_length: Optional[int] = None, eos_token_id=None, pad_token_id: Optional[int] = None, num_beams: int = 1,
                    num_return_sequences: int = 1, length_penalty: float = 1.0, early_stopping=False, no_repeat_ngram_size: int = 0,
                    bad_words_ids=None, min_new_tokens: int = 0, min_length: int = 0, repetition_penalty: float = 1.0,
                    do_sample: bool = False, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0,
                    generator: Optional[torch.Generator] = None, num_beam_groups: int = 1, diversity_penalty: float = 0.0,
                    prefix_allowed_tokens_fn=None, device_sampling: bool = False, _identical_groups_ok: bool = False, **unused) -> torch.Tensor:
    """Returns input_ids with the generated tokens appended ([B * num_return_sequences, L + new], right-padded with
    pad_token_id after eos), exactly the tensor `GenerationMixin.generate` returns for a decoder-only model."""
    if unused:
        bad = sorted(k for k, v in unused.items() if v is not None and k not in ("use_cache", "return_dict_in_generate", "output_scores"))
        if bad:
            raise NotImplementedError("otter_amd.generate: unsupported generation arguments %s" % bad)
    if num_return_sequences != 1 and not (num_beams > 1 and num_return_sequences <= num_beams):
        raise NotImplementedError("num_return_sequences > 1 needs num_beams >= num_return_sequences (beam search)")
    if device_sampling and (num_beams != 1 or not do_sample):
        raise ValueError("`device_sampling` chooses how `do_sample=True` with `num_beams == 1` draws its token: it needs both")
    num_beam_groups = int(num_beam_groups or 1)
    diversity_penalty = float(diversity_penalty or 0.0)
    if num_beam_groups > 1:    # GenerationConfig.validate's rules for the group mode
        if num_beams % num_beam_groups != 0:
            raise ValueError("`num_beams` (%d) should be divisible by `num_beam_groups` (%d)" % (num_beams, num_beam_groups))
        if do_sample:
            raise ValueError("`do_sample` must be False with `num_beam_groups` > 1 (diverse beam search does not sample)")
        if diversity_penalty <= 0.0 and not _identical_groups_ok:
            raise ValueError("`diversity_penalty` should be greater than 0.0 with `num_beam_groups` > 1, otherwise the groups will be identical")
    elif diversity_penalty != 0.0:
        raise ValueError("`diversity_penalty` is only used by group beam search: set `num_beam_groups` > 1")
    B, L0 = input_ids.shape
    dev = input_ids.device
    eos = [] if eos_token_id is None else ([int(eos_token_id)] if isinstance(eos_token_id, int) else [int(e) for e in eos_token_id])
    if pad_token_id is None:
        pad_token_id = eos[0] if eos else 0
    max_len = resolve_max_length(L0, max_new_tokens, max_length)
    proc = _Processors(L0, eos, repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_new_tokens, min_length, prefix_allowed_tokens_fn,
                       beams_per_sentence=(num_beams // num_beam_groups if num_beam_groups > 1 else num_beams))
    if max_len <= L0:
        return input_ids
    eos_t = torch.tensor(eos, device=dev, dtype=torch.long) if eos else None

    if num_beams == 1:
        ids, mask, past = input_ids, attention_mask, None
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        rule = None                    # device_sampling: (fp32 1 / T, top_k, top_p) of the stated rule; None: the host block below draws
        if device_sampling:
            inv_t, p = inv_temperature_f32(temperature), float(top_p if top_p is not None else 1.0)
            if inv_t is not None and 0.0 < p <= 1.0:
                rule = (inv_t, max(int(top_k or 0), 0), p)
        dsel, first = None, True       # the device path's state (_DeviceSelect), decided at the first step from the tensors it would read
        while ids.shape[1] < max_len:
            logits, past = step(ids, mask, past, None)
            scores = proc(ids, logits.float().clone())
            if first:
                first = False
                if ((not do_sample or rule is not None) and all(-2 ** 31 <= e < 2 ** 31 for e in eos)
                        and _DeviceSelect.usable(scores, ids, mask)):
                    dsel = _DeviceSelect(ids, mask, max_len, eos_t, pad_token_id, rule, generator)
            if dsel is not None:
                # the token, the pad of finished rows, the append and the eos bookkeeping in one ops.select_step call (csrc/select.hip); ids and
                # mask become [:, :L + 1] views of buffers allocated once.  Without an eos list nothing here synchronises.
                ids, mask = dsel.step(scores)
                if eos and dsel.all_finished():
                    break
                continue
            if rule is not None:       # CPU tensors or OTTER_HIP_SELECT=0: the kernel's rule restated in torch, over the same draws
                q = torch.empty(scores.shape, dtype=torch.float32, device=scores.device).exponential_(1, generator=generator)
                nxt = _select_reference(scores, q, *rule)
            elif do_sample:
                if temperature is not None and temperature != 1.0:
                    scores = scores / float(temperature)
                scores = _top_k_top_p(scores, int(top_k or 0), float(top_p if top_p is not None else 1.0))
                nxt = torch.multinomial(scores.softmax(-1), 1, generator=generator).squeeze(1)
            else:
                nxt = scores.argmax(-1)
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad_token_id))
            ids = torch.cat([ids, nxt[:, None]], dim=1)
            if mask is not None:
                mask = torch.cat([mask, torch.ones_like(mask[:, :1])], dim=1)
            if eos_t is not None:
                unfinished = unfinished & ~torch.isin(nxt, eos_t)
                if not bool(unfinished.any()):
                    break
        return ids if dsel is None else dsel.result()

    if num_beam_groups > 1:
        return _group_beam_search(step, input_ids, attention_mask, proc, eos, pad_token_id, max_len, int(num_beams), num_beam_groups,
                                  diversity_penalty, float(length_penalty), early_stopping, int(num_return_sequences))

    # ---- beam search ----
    nb = int(num_beams)
    ids = input_ids.repeat_interleave(nb, dim=0)
    mask = attention_mask.repeat_interleave(nb, dim=0) if attention_mask is not None else None
    beam_scores = torch.zeros(B, nb, dtype=torch.float32, device=dev)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1)
    hyps = [_BeamHyps(nb, float(length_penalty), early_stopping) for _ in range(B)]
    done = [False] * B
    past, beam_idx = None, None
    dbeam = None                       # the device path's state (_DeviceBeam), decided at the first step from the tensors it would read
    while True:
        logits, past = step(ids, mask, past, beam_idx)
        logp = torch.log_softmax(logits.float(), dim=-1)
        logp = proc(ids, logp)
        V = logp.shape[-1]
        n_cand = max(2, 1 + len(eos)) * nb
        if dbeam is None and beam_idx is None and not do_sample and _DeviceBeam.usable(logp, ids, nb, n_cand):
            dbeam = _DeviceBeam(B, nb, V, L0, max_len, eos, pad_token_id, float(length_penalty), early_stopping, beam_scores)
        if dbeam is not None:
            # selection, BeamSearchScorer.process and the reorder in one ops.beam_step call (csrc/beam.hip): no .tolist(), no host loop, no
            # copies back.  ids becomes a [:, :L + 1] view of the ping-pong buffer.
            ids, beam_idx = dbeam.step(logp, ids)
            if mask is not None:
                mask = torch.cat([mask[beam_idx], torch.ones_like(mask[:, :1])], dim=1)
            if ids.shape[1] >= max_len or (eos and dbeam.all_done()):
                break
            continue
        if do_sample:
            # beam-sample (generation/utils.py beam_sample): the warpers act on the processed log-probabilities of each beam (at least as many
            # tokens kept as candidates are drawn per beam pair), candidates are DRAWN from softmax(score + beam score) over all beams of a
            # sentence instead of taken by top-k, then ranked by that score
            if temperature is not None and temperature != 1.0:
                logp = logp / float(temperature)
            logp = _top_k_top_p(logp, int(top_k or 0), float(top_p if top_p is not None else 1.0), min_keep=max(2, 1 + len(eos)))
            scores = (logp + beam_scores[:, None]).view(B, nb * V)
            ni = torch.multinomial(scores.softmax(-1), n_cand, generator=generator)
            ns = scores.gather(1, ni)
            ns, order = torch.sort(ns, descending=True, dim=1)
            ni = ni.gather(1, order)
        else:
            scores = (logp + beam_scores[:, None]).view(B, nb * V)
            ns, ni = torch.topk(scores, n_cand, dim=1, largest=True, sorted=True)
        n_idx, n_tok = (ni // V).tolist(), (ni % V).tolist()
        ns_l = ns.tolist()
        cur_len = ids.shape[1] + 1
        new_scores = torch.zeros(B, nb, dtype=torch.float32)
        new_tokens = torch.full((B, nb), pad_token_id, dtype=torch.long)
        new_index = torch.zeros(B, nb, dtype=torch.long)
        for b in range(B):
            if done[b]:
                new_index[b] = b * nb          # padded beams of a finished sentence (transformers pads tokens, keeps index 0)
                continue
            k = 0
            for rank, (tok, sc, bi) in enumerate(zip(n_tok[b], ns_l[b], n_idx[b])):
                row = b * nb + bi
                if eos and tok in eos:
                    if rank >= nb:
                        continue
                    hyps[b].add(ids[row].clone(), sc, cur_len - L0)
                else:
                    new_scores[b, k], new_tokens[b, k], new_index[b, k] = sc, tok, row
                    k += 1
                if k == nb:
                    break
            done[b] = done[b] or hyps[b].is_done(max(ns_l[b]), cur_len, L0, max_len)
        beam_scores = new_scores.view(-1).to(dev)
        beam_idx = new_index.view(-1).to(dev)
        ids = torch.cat([ids[beam_idx], new_tokens.view(-1, 1).to(dev)], dim=1)
        if mask is not None:
            mask = torch.cat([mask[beam_idx], torch.ones_like(mask[:, :1])], dim=1)
        if all(done) or ids.shape[1] >= max_len:
            break
    if dbeam is not None:
        hyps, done, beam_scores = dbeam.finish()
    # finalize: open beams of unfinished sentences become hypotheses, best `num_return_sequences` per sentence
    bs = beam_scores.tolist()
    for b in range(B):
        if done[b]:
            continue
        for j in range(nb):
            hyps[b].add(ids[b * nb + j], bs[b * nb + j], ids.shape[1] - L0)
    return _pick_best([hyps[b].beams for b in range(B)], num_return_sequences, max_len, pad_token_id, eos, dev)


def _pick_best(beams_per_sentence, num_return_sequences: int, max_len: int, pad_token_id: int, eos: List[int], dev) -> torch.Tensor:
    """BeamSearchScorer.finalize's selection: the best `num_return_sequences` hypotheses of every sentence, best first, right-padded."""
    best = []
    for beams in beams_per_sentence:
        srt = sorted(beams, key=lambda x: x[0])
        for _ in range(num_return_sequences):
            best.append(srt.pop()[1])
    sent_max = min(max(int(h.shape[0]) for h in best) + 1, max_len)
    out = torch.full((len(best), sent_max), pad_token_id, dtype=torch.long, device=dev)
    for i, h in enumerate(best):
        out[i, :h.shape[0]] = h
        if h.shape[0] < sent_max and eos:
            out[i, h.shape[0]] = eos[0]
    return out


def _group_beam_search(step: StepFn, input_ids, attention_mask, proc: _Processors, eos: List[int], pad_token_id: int, max_len: int, nb: int,
                       ng: int, diversity_penalty: float, length_penalty: float, early_stopping, num_return_sequences: int) -> torch.Tensor:
    """Diverse beam search (transformers 4.35.1 generation/utils.py group_beam_search; Vijayakumar et al. 2016): the `nb` beams of a sentence
    are `ng` groups of `nb / ng`; one decoder step serves all of them, then the groups choose ONE AFTER THE OTHER, each an ordinary beam-search
    step over its own beams whose log-probabilities were first lowered by `diversity_penalty` x (how many beams of the EARLIER groups of the
    same sentence chose that token at this step) -- HammingDiversityLogitsProcessor, applied before the other processors as in
    `_get_logits_processor`.  Hypotheses are kept per (sentence, group) with `nb / ng` slots each (BeamSearchScorer with num_beam_groups);
    the returned sequences are the best of the union of a sentence's groups."""
    B, L0 = input_ids.shape
    dev = input_ids.device
    gs = nb // ng
    ids = input_ids.repeat_interleave(nb, dim=0)
    mask = attention_mask.repeat_interleave(nb, dim=0) if attention_mask is not None else None
    beam_scores = torch.full((B, nb), -1e9, dtype=torch.float32)
    beam_scores[:, ::gs] = 0.0           # one live beam per group at the first step
    beam_scores = beam_scores.view(-1)
    hyps = [[_BeamHyps(gs, length_penalty, early_stopping) for _ in range(ng)] for _ in range(B)]
    done = [[False] * ng for _ in range(B)]
    past, reorder = None, None
    n_cand = max(2, 1 + len(eos)) * gs
    while True:
        logits, past = step(ids, mask, past, reorder)
        logp_all = torch.log_softmax(logits.float(), dim=-1)
        V = logp_all.shape[-1]
        cur_len = ids.shape[1] + 1
        current = torch.zeros(B * nb, dtype=torch.long)          # this step's choice of every beam (earlier groups filled in first)
        reorder_l = torch.arange(B * nb, dtype=torch.long)
        new_scores = beam_scores.clone()
        ids_cpu = ids.cpu()
        for g in range(ng):
            rows = torch.tensor([b * nb + g * gs + j for b in range(B) for j in range(gs)], dtype=torch.long)
            rows_d = rows.to(dev)
            gids = ids.index_select(0, rows_d)
            logp = logp_all.index_select(0, rows_d).clone()
            if g > 0 and diversity_penalty != 0.0:
                for b in range(B):
                    freq = torch.bincount(current[b * nb: b * nb + g * gs], minlength=V).to(logp.dtype).to(dev)
                    logp[b * gs:(b + 1) * gs] -= diversity_penalty * freq
            logp = proc(gids, logp)
            scores = (logp + beam_scores.index_select(0, rows).to(dev)[:, None]).view(B, gs * V)
            ns, ni = torch.topk(scores, n_cand, dim=1, largest=True, sorted=True)
            n_idx, n_tok, ns_l = (ni // V).tolist(), (ni % V).tolist(), ns.tolist()
            for b in range(B):
                base = b * nb + g * gs
                if done[b][g]:
                    new_scores[base: base + gs] = 0.0
                    current[base: base + gs] = pad_token_id
                    continue
                k = 0
                for rank, (tok, sc, bi) in enumerate(zip(n_tok[b], ns_l[b], n_idx[b])):
                    if eos and tok in eos:
                        if rank >= gs:
                            continue
                        hyps[b][g].add(ids_cpu[base + bi].clone().to(dev), sc, cur_len - L0)
                    else:
                        new_scores[base + k], current[base + k], reorder_l[base + k] = sc, tok, base + bi
                        k += 1
                    if k == gs:
                        break
                done[b][g] = done[b][g] or hyps[b][g].is_done(max(ns_l[b]), cur_len, L0, max_len)
        beam_scores = new_scores
        reorder = reorder_l.to(dev)
        ids = torch.cat([ids.index_select(0, reorder), current.to(dev)[:, None]], dim=1)
        if mask is not None:
            mask = torch.cat([mask.index_select(0, reorder), torch.ones_like(mask[:, :1])], dim=1)
        if all(all(d) for d in done) or ids.shape[1] >= max_len:
            break
    bs = beam_scores.tolist()
    for b in range(B):
        for g in range(ng):
            if done[b][g]:
                continue
            for j in range(gs):
                r = b * nb + g * gs + j
                hyps[b][g].add(ids[r], bs[r], ids.shape[1] - L0)
    return _pick_best([[h for g in range(ng) for h in hyps[b][g].beams] for b in range(B)], num_return_sequences, max_len, pad_token_id, eos, dev)
