"""Static key / value cache for cached generation (`generate(..., cache_implementation="static")`).

The legacy cache of both decoder hosts is a tuple of tensors that grows by `torch.cat` every step and is physically re-gathered by
`index_select(0, beam_idx)` under beam search: every step reads and rewrites every key and value of every layer, twice with beams.
`StaticKVCache` is allocated once for the maximum length; a step appends in place, and beam search reorders a small int32 ancestry table
instead of the cache:

    k, v      [n_layers, rows, n_heads, max_len, head_dim]: key-major, dim contiguous -- the layout csrc/decode_cache.hip reads with one
              16-byte load per lane.  It belongs to this project (the object is opaque); `to_legacy()` gives the hosts' tuple layouts.
    length    host int: positions filled, the same for every row (left padding is a matter of the attention mask, as in the legacy path).
    src       int32 [rows, max_len] or None: src[n, t] = the cache row that holds sequence n's key / value at position t.  Created by the
              first `reorder`; greedy decoding and sampling never create it.  Columns >= length always hold the row's own index: a row
              writes the new position into its OWN row, whatever its ancestry, so no slot is ever written twice and a slot that other
              rows still point at is never overwritten.

Replay mode (`enable_replay`, once, after the prefill; `generate(..., graph_decode=True)`): everything a step reads that changes from step to
step lives at a fixed device address, so that one captured graph of the step can be replayed at every position:

    pos_dev   int32 [1] on the device, equal to `length`; `advance()` increments both (the device add is the last op of the captured step);
              a host ends every step with `end_step()`: `advance()` here, `length += 1` in the position-scalar mode.
    valid     uint8 [rows, max_len]: the prompt's attention mask in columns [0, S), ones after it (generation only ever appends ones).
    src       created eagerly when beams are in use, so that its address and the NULL / non-NULL choice are fixed before capture.

In that mode the step runs on `ops.decode_attn_cached_dyn`, which reads the position, the rotary table row and the mask columns itself.

The cached step runs on csrc/decode_cache.hip (`ops.decode_attn_cached`) on the GPU in bf16 with head_dim 128 and as many key / value heads
as query heads.  Everywhere else -- the CPU, fp32 compute, other head sizes -- `attend_reference` runs: a plain-torch restatement of exactly
what the kernel does.  Like `Int8FrozenLinear`'s, that branch is a deliberate exception to "no PyTorch path": it is what makes the bookkeeping
(the table, the append, the hosts' wiring) testable without a GPU, and it is the structure the kernel's oracle follows.

The int8 form (`StaticKVCache(..., kv_dtype="int8")`, `generate(..., cache_implementation="static", kv_cache_dtype="int8")`): opt-in and
lossy, like the int8 decoder.  Each cached vector is 128 int8 codes and one fp32 scale -- 132 bytes against 256:

    k, v              int8 [n_layers, rows, n_heads, max_len, head_dim]
    k_scale, v_scale  fp32 [n_layers, rows, n_heads, max_len]

THE FORMAT.  For a vector x[head_dim] exactly as the unquantised cache stores it (a key after rotary, rounded once to the compute dtype; a
value as projected), read as fp32:

    amax  = max_i |x[i]|
    scale = amax / 127                                        (fp32 IEEE division; 1 when amax == 0)
    code  = clamp(rint_half_even(x[i] / scale), -127, 127)    as int8 (-128 never occurs)
    value = float(code) * scale                               (what attention sees)

which is the rule of `quant.quantize_weight_int8`, applied per (layer, row, head, position): `quantize_kv_int8`.  These are a handful of
IEEE-exact operations, so torch on the CPU, torch on the GPU and csrc/decode_cache_i8.hip give the same codes and scales, bit for bit.  The
scale is per token because an append knows only its own vector: no scale of an earlier position is ever rewritten, so the in-place
invariant above carries over.  `fill` quantises the prompt with torch ops; a cached step quantises the new token as it appends it and
attends to it in its dequantised form, so a step returns what "append, then attend over the cache" returns.  `dtype` stays the compute
dtype (what `attend` and `to_legacy` return in).  The kernel conditions are those of the unquantised cache (`uses_kernel`); everywhere
else `attend_reference` runs its int8 branch.

The OtterHD / Fuyu-8B (Persimmon) host (otter_amd/fuyu.py: head_dim 64, q / k LayerNorm per head and a partial rotary embedding fused into the
step) takes the cache as an object: `StaticKVCache.for_model(model, rows, max_len)` passed to `generate` as `past_key_values`, `reset()`
between calls.  Its step is `attend_persimmon`: csrc/persimmon_decode_cache.hip (`ops.persimmon_decode_attn_cached`, `_dyn` in replay
mode) on the GPU in bf16 -- the arithmetic of csrc/persimmon_decode.hip line for line, so the static cache returns the default cache's
tokens there -- and `attend_persimmon_reference` everywhere else.  The layout, the table, replay mode and the in-place invariant are the
ones above; an int8 cache at head_dim 64 is not built (`NotImplementedError`).

A shared prompt (`share_prompt(group)` on the empty cache; `generate(..., num_beams=nb, cache_implementation="static", share_prompt=True)`):
under beam search the rows are sentences x `group` beams, the beams of a sentence contiguous, and every beam of a sentence carries the same
prompt.  The prompt pass then runs one row per sentence and `fill` writes its keys and values into the sentence's first row only (the
LEADER, row (n // group) * group):

    group       rows per sentence (1: no sharing); `rows % group == 0`.
    shared_len  the positions [0, shared_len) that every row reads from its leader: 0 until `fill`, then the prompt length.
    src         src[n, :shared_len] = (n // group) * group, the row's own index elsewhere; created by `fill`, so no later than the first
                cached step (and before `enable_replay`, which must find it: its address is fixed before capture).

`reorder` is unchanged: beam search never moves a row to another sentence (the precondition; checked where the index is a CPU tensor), so the
prefix columns stay on the leader whatever the ancestry.  `attend_reference`, `to_legacy` and the ungrouped kernels read through the table as
they are.  In bf16 at head_dim 128 `attend` takes csrc/decode_cache_shared.hip (`ops.decode_attn_cached_shared`, `_dyn` in replay mode) for the
group sizes it is built for, from SHARED_KERNEL_MIN_KEYS = 1 536 shared keys per head on (sentences x shared_len; below that the step is
latency-bound and the table path is as fast or faster): one workgroup carries the `group` queries of a sentence and loads each shared key
once.  OTTER_SHARED_PREFIX=0 keeps the table path (the A/B lever, like OTTER_HIP_BEAM) and =1 takes the kernel below the threshold too; other
group sizes stay on the table path.  The int8 cache has its own grouped kernel, csrc/decode_cache_shared_i8.hip
(`ops.decode_attn_cached_shared_i8`, `_dyn` in replay mode; `uses_shared_i8_kernel`): a shared key's codes and scales are loaded and
dequantised once for the group, from SHARED_I8_KERNEL_MIN_KEYS shared keys per head on.  Its lever is OTTER_SHARED_PREFIX_I8 ("0": the table
path through csrc/decode_cache_i8.hip; "1": the kernel below the threshold too); OTTER_SHARED_PREFIX=0 switches it off as well, and
OTTER_SHARED_PREFIX=1 does not force it.  The layout and the
allocation stay as they are: the non-leader rows' slots [0, shared_len) are allocated and never touched, so sharing saves prompt-pass work
and key / value traffic, not cache memory.

Candidate rows (`attend_branches`, `branches(C, T)`; `OtterForConditionalGeneration.score_candidates`): a filled cache of B prompts is READ by
N = B * C * T one-token rows, row n = (b C + c) T + t the t-th teacher-forced token of candidate c of sentence b, which attends over prompt b
and over tokens 0..t of its own candidate.  In bf16 at head_dim 128 that is the non-causal flash forward over `k[layer, :, :, :length]` in
place plus csrc/branch_attn.hip (`ops.branch_attn_merge`), everywhere else `attend_branches_reference`.  Nothing is appended and `length`
stays: the prompt serves any number of such passes.  A multi-token APPEND is still refused by `check_step`.
"""
from __future__ import annotations

import os
from typing import Optional

import torch


# a shared prompt: the grouped kernel from this many shared keys per head on (sentences x shared_len); measured, DESIGN.md 4.19
SHARED_KERNEL_MIN_KEYS = 1536
# the same for the int8 cache's grouped kernel (csrc/decode_cache_shared_i8.hip): the smallest measured count from which no measured point,
# kernel alone or whole generate() call, was more than 3 % slower than the table path (profiles/r20_shared_prefix_i8_ab.txt)
SHARED_I8_KERNEL_MIN_KEYS = 16384


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def cache_geometry(config):
    """(n_layers, key / value heads, head_dim, the host's position limit) of a decoder host's config (MPT, LLaMA or Persimmon; a FuyuConfig
    stands for its `text_config`)."""
    if getattr(config, "model_type", None) == "fuyu":
        config = config.text_config
    if hasattr(config, "d_model"):          # MPTConfig
        return int(config.n_layers), int(config.n_heads), int(config.d_model) // int(config.n_heads), int(config.max_seq_len)
    heads = int(config.num_attention_heads)
    head_dim = getattr(config, "head_dim", None) or int(config.hidden_size) // heads
    return (int(config.num_hidden_layers), int(getattr(config, "num_key_value_heads", None) or heads), int(head_dim),
            int(config.max_position_embeddings))


def quantize_kv_int8(x: torch.Tensor):
    """x [..., d] -> (codes int8 [..., d], scale fp32 [...]) by THE FORMAT of the module docstring: `quant.quantize_weight_int8` over the
    last dim."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    # tensor / tensor: a true division on every backend (a Python-scalar divisor may be turned into a multiplication by its reciprocal)
    scale = amax / torch.full_like(amax, 127.0)
    scale = torch.where(amax == 0, torch.ones_like(scale), scale)
    return torch.round(xf / scale.unsqueeze(-1)).clamp_(-127, 127).to(torch.int8), scale


def dequantize_kv_int8(codes: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """float(code) * scale in fp32 at least, rounded once to `dtype`."""
    ct = torch.float64 if dtype == torch.float64 else torch.float32
    return (codes.to(ct) * scale.to(ct).unsqueeze(-1)).to(dtype)


class StaticKVCache:
    def __init__(self, n_layers: int, rows: int, n_heads: int, head_dim: int, max_len: int, device, dtype: torch.dtype = torch.bfloat16,
                 kv_dtype: Optional[str] = None):
        if min(n_layers, rows, n_heads, head_dim) < 1 or max_len < 2:
            raise ValueError("StaticKVCache: n_layers, rows, n_heads, head_dim >= 1 and max_len >= 2")
        if kv_dtype not in (None, "int8"):
            raise ValueError("StaticKVCache: kv_dtype must be None or 'int8', got %r" % (kv_dtype,))
        self.n_layers, self.rows, self.n_heads, self.head_dim, self.max_len = int(n_layers), int(rows), int(n_heads), int(head_dim), int(max_len)
        shape = (self.n_layers, self.rows, self.n_heads, self.max_len, self.head_dim)
        self.kv_dtype, self._dtype = kv_dtype, dtype
        self.k = torch.zeros(shape, dtype=torch.int8 if self.int8 else dtype, device=device)
        self.v = torch.zeros(shape, dtype=torch.int8 if self.int8 else dtype, device=device)
        self.k_scale = torch.ones(shape[:-1], dtype=torch.float32, device=device) if self.int8 else None   # (a zero vector's scale is 1)
        self.v_scale = torch.ones(shape[:-1], dtype=torch.float32, device=device) if self.int8 else None
        self.length = 0
        self.src: Optional[torch.Tensor] = None
        self.pos_dev: Optional[torch.Tensor] = None     # replay mode (enable_replay)
        self.valid: Optional[torch.Tensor] = None
        self.kernel_steps = True        # replay mode: every `attend` so far ran on the dyn kernel (what a captured step needs)
        self.group, self.shared_len = 1, 0              # a shared prompt (share_prompt)

    # ---- bookkeeping ----------------------------------------------------------------------------------------------------------------

    @property
    def int8(self) -> bool:
        return self.kv_dtype == "int8"

    @property
    def device(self):
        return self.k.device

    @property
    def dtype(self):
        """The compute dtype: what the unquantised cache stores, and what `attend` and `to_legacy` return in."""
        return self._dtype

    def nbytes(self) -> int:
        """Bytes of the keys and values (codes and scales for the int8 form)."""
        return sum(t.numel() * t.element_size() for t in (self.k, self.v, self.k_scale, self.v_scale) if t is not None)

    def get_seq_length(self) -> int:
        return self.length

    def __len__(self):          # (a legacy cache answers len() with its layer count)
        return self.n_layers

    def data_ptrs(self):
        if self.int8:
            return (self.k.data_ptr(), self.v.data_ptr(), self.k_scale.data_ptr(), self.v_scale.data_ptr())
        return (self.k.data_ptr(), self.v.data_ptr())

    def check_step(self, rows: int, S: int) -> None:
        """The two things a forward may do with this cache: prefill it while empty, or append one position."""
        if torch.is_grad_enabled():
            raise RuntimeError("StaticKVCache is written in place and is for inference only: run the forward under torch.no_grad()")
        if rows != self.rows and not (self.group > 1 and self.length == 0 and rows == self.rows // self.group):
            if self.group > 1 and self.length == 0:
                raise ValueError("StaticKVCache shares the prompt among groups of %d rows: the prompt pass has %d rows (one per group), "
                                 "the forward has %d" % (self.group, self.rows // self.group, rows))
            raise ValueError("StaticKVCache was created for %d rows, the forward has %d" % (self.rows, rows))
        if self.length > 0 and S != 1:
            raise ValueError("StaticKVCache holds %d positions: only a one-token step can follow (got %d tokens)" % (self.length, S))
        if self.length + S > self.max_len:
            raise ValueError("StaticKVCache: %d + %d positions exceed max_len=%d" % (self.length, S, self.max_len))

    @classmethod
    def for_model(cls, model_or_config, rows: int, max_len: int, device=None, dtype=None, kv_dtype: Optional[str] = None) -> "StaticKVCache":
        """A cache of the geometry of a decoder host (`cache_geometry` of its config), for a caller who passes the cache to `generate` as
        `past_key_values` (the OtterHD / Fuyu host).  `model_or_config`: a model or its config; `device` / `dtype` default to the model's
        embedding's device and compute dtype (a config alone: the CPU and fp32)."""
        config = getattr(model_or_config, "config", model_or_config)
        n_layers, n_kv, head_dim, _ = cache_geometry(config)
        if device is None or dtype is None:
            emb = model_or_config.get_input_embeddings().weight if hasattr(model_or_config, "get_input_embeddings") else None
            if device is None:
                device = emb.device if emb is not None else torch.device("cpu")
            if dtype is None:
                dtype = emb.dtype if emb is not None and emb.dtype in (torch.bfloat16, torch.float64) else torch.float32
        return cls(n_layers, rows, n_kv, head_dim, max_len, device, dtype, kv_dtype=kv_dtype)

    def reset(self) -> None:
        """Make the cache empty again for the next `generate` call: no positions, no beam table, replay mode left.  The buffers stay as
        they are: nothing beyond `length` is ever read."""
        self.length = 0
        self.src = None
        self.pos_dev = None
        self.valid = None
        self.kernel_steps = True
        self.group, self.shared_len = 1, 0
        self.rotary_tables = None       # (the Persimmon host keeps the tables a replay-mode step reads here: otter_amd/fuyu.py)

    def share_prompt(self, group: int) -> None:
        """On the empty cache: the rows are sentences x `group` contiguous beams that share their prompt (module docstring).  The prompt pass
        then has rows // group rows, whose keys and values `fill` writes into the leaders' rows."""
        group = int(group)
        if self.length != 0 or self.replay:
            raise ValueError("StaticKVCache.share_prompt: the cache is not empty")
        if group < 1 or self.rows % group != 0:
            raise ValueError("StaticKVCache.share_prompt: %d rows are not whole groups of %d" % (self.rows, group))
        self.group, self.shared_len = group, 0

    def _shared_table(self, S: int) -> torch.Tensor:
        src = self._own_rows()
        src[:, :S] = (torch.arange(self.rows, dtype=torch.int32, device=self.device) // self.group * self.group).view(-1, 1)
        return src

    def fill(self, layer: int, k: torch.Tensor, v: torch.Tensor) -> None:
        """Prefill: k, v indexed [rows, n_heads, S, head_dim] (any strides: the views the flash and SDPA paths produce) -> positions [0, S).
        One strided copy per tensor.  int8: the prompt's vectors are rounded to the compute dtype first, so that the quantiser sees what
        the unquantised cache would hold.  A shared prompt (`share_prompt(group)`, group > 1): k, v [rows // group, n_heads, S, head_dim]
        go into the leaders' rows 0, group, 2 group, ... only, shared_len <- S, and the table that points every row's columns [0, S) at
        its leader is created."""
        if self.length != 0:
            raise ValueError("StaticKVCache.fill: the cache is not empty")
        S = k.shape[2]
        want = (self.rows // self.group, self.n_heads, S, self.head_dim)
        if tuple(k.shape) != want or tuple(v.shape) != want or S > self.max_len:
            raise ValueError("StaticKVCache.fill: expected k, v %s with S <= %d, got %s / %s" % (want, self.max_len, tuple(k.shape), tuple(v.shape)))
        g = self.group                                   # (rows 0, g, 2 g, ...: every row when nothing is shared)
        if g > 1 and self.shared_len != S:
            self.shared_len, self.src = S, self._shared_table(S)
        if self.int8:
            for codes, scales, t in ((self.k, self.k_scale, k), (self.v, self.v_scale, v)):
                c, s = quantize_kv_int8(t.to(self.dtype))
                codes[layer, ::g, :, :S].copy_(c)
                scales[layer, ::g, :, :S].copy_(s)
            return
        self.k[layer, ::g, :, :S].copy_(k)
        self.v[layer, ::g, :, :S].copy_(v)

    # ---- replay mode -----------------------------------------------------------------------------------------------------------------

    @property
    def replay(self) -> bool:
        return self.pos_dev is not None

    def enable_replay(self, attention_mask: Optional[torch.Tensor] = None, beams: bool = False) -> None:
        """Once, after the prefill: move what a step reads to fixed device addresses (module docstring).  `attention_mask` [rows, length]
        is the prompt's mask or None (all valid); `beams`: `reorder` will be called, so the table is created now."""
        if self.replay:
            raise ValueError("StaticKVCache.enable_replay: replay mode is enabled already")
        if self.length < 1:
            raise ValueError("StaticKVCache.enable_replay: the cache is empty (the prompt pass fills it)")
        if self.group > 1 and (self.src is None or self.shared_len != self.length):
            raise ValueError("StaticKVCache.enable_replay: the prompt is shared but `fill` has not laid the table over it")
        if attention_mask is not None and tuple(attention_mask.shape) != (self.rows, self.length):
            raise ValueError("StaticKVCache.enable_replay: attention_mask must be [%d, %d], got %s"
                             % (self.rows, self.length, tuple(attention_mask.shape)))
        self.valid = torch.ones((self.rows, self.max_len), dtype=torch.uint8, device=self.device)
        if attention_mask is not None:
            self.valid[:, :self.length] = attention_mask.to(self.device).ne(0).to(torch.uint8)
        if beams and self.src is None:
            self.src = self._own_rows()
        self.pos_dev = torch.full((1,), self.length, dtype=torch.int32, device=self.device)

    def advance(self) -> None:
        """The end of a replay-mode step: the device position and the host length move together (the device add is one tiny op, the last of
        a captured step; a graph replay runs it again, and `note_replay` moves the host side)."""
        if not self.replay:
            raise ValueError("StaticKVCache.advance: replay mode only (the position-scalar step sets `length` itself)")
        self.pos_dev.add_(1)
        self.length += 1

    def end_step(self) -> None:
        """The end of a cached step of a host, after the last layer: `advance()` in replay mode, otherwise the host length alone."""
        if self.replay:
            self.advance()
        else:
            self.length += 1

    def note_replay(self) -> None:
        """A captured step was replayed: the graph advanced `pos_dev`, the host length follows."""
        if self.length + 1 > self.max_len:
            raise ValueError("StaticKVCache: %d + 1 positions exceed max_len=%d" % (self.length, self.max_len))
        self.length += 1

    def _own_rows(self) -> torch.Tensor:
        return torch.arange(self.rows, dtype=torch.int32, device=self.device).view(-1, 1).repeat(1, self.max_len)

    def reorder(self, beam_idx: torch.Tensor) -> None:
        """Beam search: sequence n continues what was sequence beam_idx[n].  Only the table moves (rows x length x 4 bytes), in place.
        A shared prompt: the precondition is that beam_idx[n] is a row of n's own sentence (beam search never moves a row to another
        sentence) -- then columns [0, shared_len) stay on the leader and the arithmetic is the same.  It is checked where beam_idx is a
        CPU tensor (ValueError); an index on the GPU is not read back."""
        if self.group > 1 and not beam_idx.is_cuda:
            own = torch.arange(self.rows) // self.group
            if beam_idx.numel() != self.rows or not torch.equal(beam_idx.reshape(-1).long() // self.group, own):
                raise ValueError("StaticKVCache.reorder: with a shared prompt every row must continue a row of its own group of %d "
                                 "(beam_idx %s)" % (self.group, beam_idx.reshape(-1).tolist()))
        if self.src is None:
            if self.replay:
                raise ValueError("StaticKVCache.reorder: replay mode was enabled without beams (the table cannot appear after capture)")
            self.src = self._own_rows()
        L = self.length
        if L:
            self.src[:, :L] = self.src[:, :L].index_select(0, beam_idx.to(self.device))

    def _gathered(self, t: torch.Tensor, upto: int) -> torch.Tensor:
        """t [rows, H, max_len, d] -> [rows, H, upto, d]: position j of row n from row src[n, j].  (Scales: t [rows, H, max_len].)"""
        if self.src is None:
            return t[:, :, :upto]
        idx = self.src[:, :upto].long()                                        # [rows, upto]
        pos = torch.arange(upto, device=t.device).view(1, -1)
        if t.dim() == 3:
            return t[idx, :, pos].transpose(1, 2)                              # [rows, upto, H] -> [rows, H, upto]
        return t[idx, :, pos].permute(0, 2, 1, 3)                              # [rows, upto, H, d] -> [rows, H, upto, d]

    def to_legacy(self, host) -> tuple:
        """The tuple-of-tuples cache in the host's own layout, gathered through the table: "mpt" (or an MPT module) k [N,H,d,S], v [N,H,S,d];
        "llama" and "persimmon" (also a Persimmon / Fuyu module) k, v [N,H,S,d].  int8: dequantised, in the compute dtype."""
        name = host if isinstance(host, str) else type(host).__name__
        mpt = "mpt" in name.lower()
        if not mpt and not any(h in name.lower() for h in ("llama", "persimmon", "fuyu")):
            raise ValueError("StaticKVCache.to_legacy: host must be 'mpt' or 'llama' (or one of their modules), got %r" % (name,))
        out = []
        for i in range(self.n_layers):
            k, v = self._gathered(self.k[i], self.length), self._gathered(self.v[i], self.length)
            if self.int8:
                k = dequantize_kv_int8(k, self._gathered(self.k_scale[i], self.length), self.dtype)
                v = dequantize_kv_int8(v, self._gathered(self.v_scale[i], self.length), self.dtype)
            out.append((k.transpose(2, 3) if mpt else k, v))
        return tuple(out)

    # ---- the cached step ------------------------------------------------------------------------------------------------------------

    def uses_kernel(self, q: torch.Tensor, n_kv: int) -> bool:
        return q.is_cuda and q.dtype == torch.bfloat16 and self.dtype == torch.bfloat16 and self.head_dim == 128 and n_kv == q.shape[1]

    def uses_shared_kernel(self, q: torch.Tensor, n_kv: int) -> bool:
        """The step runs on csrc/decode_cache_shared.hip: a shared prompt in a group size the kernel is built for, a bf16 cache where
        `uses_kernel` holds, and OTTER_SHARED_PREFIX != "0" (the A/B lever: "0" keeps the existing kernel, through the table).  Unless the
        lever is "1" the kernel is taken only from SHARED_KERNEL_MIN_KEYS shared keys per head on (sentences x shared_len): below that the
        step is bound by latency and the grouped kernel, with a third of the workgroups, measured 3.5 % slower.  All of this
        is fixed for a whole generate call, so a captured step keeps its kernel."""
        return not self.int8 and self._uses_grouped_kernel(q, n_kv, os.environ.get("OTTER_SHARED_PREFIX", ""), SHARED_KERNEL_MIN_KEYS,
                                                           "DECODE_CACHED_SHARED_GROUPS")

    def uses_shared_i8_kernel(self, q: torch.Tensor, n_kv: int) -> bool:
        """The step runs on csrc/decode_cache_shared_i8.hip: an int8 cache with a shared prompt in a group size that kernel is built for,
        where `uses_kernel` holds, OTTER_SHARED_PREFIX != "0" (that lever switches every grouped kernel off) and OTTER_SHARED_PREFIX_I8 != "0"
        (this kernel's own A/B lever: "0" keeps csrc/decode_cache_i8.hip, through the table).  Unless OTTER_SHARED_PREFIX_I8 is "1" the kernel
        is taken only from SHARED_I8_KERNEL_MIN_KEYS shared keys per head on (sentences x shared_len).  OTTER_SHARED_PREFIX=1 does not force
        it.  All of this is fixed for a whole generate call, so a captured step keeps its kernel."""
        if os.environ.get("OTTER_SHARED_PREFIX", "") == "0":
            return False
        return self.int8 and self._uses_grouped_kernel(q, n_kv, os.environ.get("OTTER_SHARED_PREFIX_I8", ""), SHARED_I8_KERNEL_MIN_KEYS,
                                                       "DECODE_CACHED_SHARED_I8_GROUPS")

    def _uses_grouped_kernel(self, q: torch.Tensor, n_kv: int, lever: str, min_keys: int, groups: str) -> bool:
        """The rule the two grouped kernels share: a shared prompt, the kernel's lever not "0", `min_keys` shared keys per head (sentences x
        shared_len) unless the lever is "1", a group size in `ops.<groups>`, and `uses_kernel`."""
        if self.group < 2 or self.shared_len < 1 or lever == "0":
            return False
        if lever != "1" and (self.rows // self.group) * self.shared_len < min_keys:
            return False
        from . import ops

        return self.group in getattr(ops, groups) and self.uses_kernel(q, n_kv)

    def attend(self, layer: int, q, k_new, v_new, scale: float, cos=None, sin=None, key_valid=None, slopes=None) -> torch.Tensor:
        """One cached step of `layer` at position `length` (which the caller advances once per forward, after the last layer):
        q [N,H,d], k_new / v_new [N,H_kv,d] views of the projection output; cos / sin fp32 [d] rows of that position or None;
        key_valid uint8 / bool [N, length+1] or None; slopes fp32 [H] or None.  Returns o [N, H*d] in q's dtype.
        Replay mode: the position is `pos_dev`, cos / sin are the whole fp32 tables [>= max_len, d] (or None) and the mask is the cache's
        own `valid` (key_valid must be None)."""
        if self.replay and key_valid is not None:
            raise ValueError("StaticKVCache.attend: in replay mode the mask is the cache's own (`valid`); pass key_valid=None")
        n_kv = k_new.shape[1]
        if not self.uses_kernel(q, n_kv):
            if self.replay:
                self.kernel_steps = False   # (the restatement reads the position back to the host: such a step cannot be captured)
            return self.attend_reference(layer, q, k_new, v_new, scale, cos=cos, sin=sin, key_valid=key_valid, slopes=slopes)
        from . import ops

        # ONE choice of the op: over the int8 cache or not, grouped or through the table, with the position in device memory or not.  (Looked
        # up on `ops` at the call: the tests put stand-ins there.)
        grouped = self.uses_shared_i8_kernel(q, n_kv) if self.int8 else self.uses_shared_kernel(q, n_kv)
        op = getattr(ops, "decode_attn_cached" + ("_shared" if grouped else "") + ("_i8" if self.int8 else "") + ("_dyn" if self.replay else ""))
        caches = (self.k[layer], self.v[layer]) + ((self.k_scale[layer], self.v_scale[layer]) if self.int8 else ())
        grouping = (self.group, self.shared_len) if grouped else ()
        if self.replay:
            return op(q, k_new, v_new, *caches, self.pos_dev, scale, *grouping, cos_table=cos, sin_table=sin, src=self.src, key_valid=self.valid,
                      slopes=slopes)
        return op(q, k_new, v_new, *caches, self.length, scale, *grouping, cos=cos, sin=sin, src=self.src, key_valid=key_valid, slopes=slopes)

    def attend_reference(self, layer: int, q, k_new, v_new, scale: float, cos=None, sin=None, key_valid=None, slopes=None) -> torch.Tensor:
        """What csrc/decode_cache.hip does, in plain torch on any device and dtype: rotary (fp32 at least, k rounded to the cache dtype once),
        append at slot `length` of the row's own row, gather keys 0..length through the table, ALiBi slope * (j - length), padding mask,
        softmax in fp32 at least, a fully masked row -> 0.  Replay mode: the position is read from `pos_dev` (not from `length`), cos / sin
        are the whole tables, of which row `pos` is taken, and the mask is columns 0..pos of `valid`.  int8 (csrc/decode_cache_i8.hip): the
        rounded k and v are quantised, codes and scales stored, and the gathered codes dequantised -- key `pos` included."""
        pos, cos, sin, key_valid = self._step_inputs("attend_reference", "d", cos, sin, key_valid)
        ct = torch.float64 if q.dtype == torch.float64 else torch.float32
        qf, kf = q.to(ct), k_new.to(ct)
        if cos is not None:
            c, s = cos.to(ct), sin.to(ct)
            if c.dim() == 2:
                c, s = c[:, None], s[:, None]
            qf = qf * c + rotate_half(qf) * s
            kf = kf * c + rotate_half(kf) * s
        if self.int8:
            self.k[layer, :, :, pos], self.k_scale[layer, :, :, pos] = quantize_kv_int8(kf.to(self.dtype))
            self.v[layer, :, :, pos], self.v_scale[layer, :, :, pos] = quantize_kv_int8(v_new.to(self.dtype))
        else:
            self.k[layer, :, :, pos] = kf.to(self.dtype)
            self.v[layer, :, :, pos] = v_new.to(self.dtype)
        return self._attend_appended(layer, qf, pos, scale, key_valid, slopes, q.dtype)

    def _step_inputs(self, who: str, width: str, cos, sin, key_valid):
        """(pos, cos, sin, key_valid) as a restatement uses them: `length` and the caller's own, or in replay mode the position read back from
        `pos_dev`, row `pos` of the whole tables and the cache's own mask.  Either way 1 <= pos < max_len."""
        pos = self.length
        if self.replay:
            pos = int(self.pos_dev.item())
            if key_valid is not None:
                raise ValueError("StaticKVCache.%s: in replay mode the mask is the cache's own (`valid`); pass key_valid=None" % who)
            key_valid = self.valid
            if cos is not None:
                if cos.dim() != 2 or cos.shape[0] < self.max_len:
                    raise ValueError("StaticKVCache: replay mode takes the whole cos / sin tables [>= max_len, %s]" % width)
                if 0 <= pos < cos.shape[0]:
                    cos, sin = cos[pos], sin[pos]
        if pos < 1 or pos >= self.max_len:
            raise ValueError("StaticKVCache: a cached step needs 1 <= length < max_len (length=%d, max_len=%d)" % (pos, self.max_len))
        return pos, cos, sin, key_valid

    def _attend_appended(self, layer: int, qf, pos: int, scale: float, key_valid, slopes, out_dtype) -> torch.Tensor:
        """The tail of both restatements, slot `pos` written: qf [N,H,d] (rotated, in fp32 at least) over keys 0..pos gathered through the
        table (int8: dequantised), grouped heads repeated, ALiBi, padding mask, a fully masked row -> 0.  Returns o [N, H*d] in out_dtype."""
        (N, H, d), ct = qf.shape, qf.dtype
        k, v = self._gathered(self.k[layer], pos + 1), self._gathered(self.v[layer], pos + 1)     # column pos of the table is the row's own index
        if self.int8:
            k = dequantize_kv_int8(k, self._gathered(self.k_scale[layer], pos + 1), ct)
            v = dequantize_kv_int8(v, self._gathered(self.v_scale[layer], pos + 1), ct)
        else:
            k, v = k.to(ct), v.to(ct)
        if k.shape[1] != H:
            k, v = k.repeat_interleave(H // k.shape[1], dim=1), v.repeat_interleave(H // v.shape[1], dim=1)
        s_ = torch.einsum("nhd,nhjd->nhj", qf * scale, k)
        if slopes is not None:
            s_ = s_ + slopes.to(ct).view(1, H, 1) * torch.arange(-pos, 1, device=qf.device, dtype=ct).view(1, 1, -1)
        dead = None
        if key_valid is not None:
            ok = key_valid[:, :pos + 1].bool()
            s_ = s_.masked_fill(~ok[:, None, :], float("-inf"))
            dead = ~ok.any(dim=1)
            if bool(dead.any()):
                s_ = s_.masked_fill(dead[:, None, None], 0.0)
        o = torch.einsum("nhj,nhjd->nhd", torch.softmax(s_, dim=-1), v)
        if dead is not None:
            o = o.masked_fill(dead[:, None, None], 0.0)
        return o.reshape(N, H * d).to(out_dtype)

    # ---- candidate rows over the cached prompt (OtterForConditionalGeneration.score_candidates) -----------------------------------------------

    def _check_branches(self, q, k_new, v_new, C: int, T: int, key_valid):
        """The raises of `attend_branches` / `attend_branches_reference`; returns (B, P, N)."""
        if self.int8:
            raise NotImplementedError("StaticKVCache.attend_branches: an int8 key / value cache is not built for candidate rows")
        if self.replay:
            raise ValueError("StaticKVCache.attend_branches: the cache is in replay mode (its position belongs to a captured step)")
        if self.group > 1 or self.src is not None:
            raise ValueError("StaticKVCache.attend_branches: a shared-prompt cache or one with a beam table: candidate rows read row b of the "
                             "cache as the prompt of sentence b")
        if self.length == 0:
            raise ValueError("StaticKVCache.attend_branches: the cache is empty (the prompt pass fills it)")
        B, P, C, T = self.rows, self.length, int(C), int(T)
        if C < 1 or T < 1 or T > 64:
            raise ValueError("StaticKVCache.attend_branches: C >= 1 and 1 <= T <= 64 (got C=%d, T=%d)" % (C, T))
        N = B * C * T
        if q.dim() != 3 or q.shape[0] != N or q.shape[2] != self.head_dim or tuple(k_new.shape) != (N, self.n_heads, self.head_dim) \
                or tuple(v_new.shape) != tuple(k_new.shape) or q.shape[1] % self.n_heads:
            raise ValueError("StaticKVCache.attend_branches: q [%d, H, %d] and k_new / v_new [%d, %d, %d] for %d sentences x %d candidates x %d "
                             "positions, got %s / %s / %s" % (N, self.head_dim, N, self.n_heads, self.head_dim, B, C, T, tuple(q.shape),
                                                              tuple(k_new.shape), tuple(v_new.shape)))
        if key_valid is not None and tuple(key_valid.shape) != (B, P):
            raise ValueError("StaticKVCache.attend_branches: key_valid must be the prompt's mask [%d, %d], got %s" % (B, P, tuple(key_valid.shape)))
        return B, P, N

    def branches(self, C: int, T: int) -> "_BranchView":
        """The cache as a host's cached-step code sees it during a branch pass: `attend` is `attend_branches` for C candidates of T positions."""
        return _BranchView(self, C, T)

    def attend_branches(self, layer: int, q, k_new, v_new, scale: float, C: int, T: int, key_valid=None, slopes=None) -> torch.Tensor:
        """Candidate rows over the cached prompt: N = rows * C * T one-token rows, row n = (b C + c) T + t the t-th position of candidate c of
        sentence b.  Row (b, c, t) attends over the `length` prompt keys of cache row b and over the own keys (b, c, 0..t) of k_new -- nothing
        of another candidate.  q [N,H,d], k_new / v_new [N,H_kv,d] views of the projection output (LLaMA: q and k rotated already, at positions
        prompt position + t); key_valid uint8 / bool [rows, length], the PROMPT's mask, or None; slopes fp32 [H] or None (ALiBi: the newest
        key of row (b, c, t) is its own, `length + t`).  Returns o [N, H*d] in q's dtype.  Nothing is written into the cache and neither
        `length` nor `src` changes: the prompt stays reusable for any number of such passes.

        On the GPU in bf16 at head_dim 128 two launches: the non-causal flash forward of the sentence's C*T queries over the cache's own
        `k[layer, :, :, :length]` / `v[...]`, read in place through a [rows, length, H, 128] strided view (csrc/flash.hip returns o1 in fp32 and lse1),
        and csrc/branch_attn.hip (`ops.branch_attn_merge`), which scores the own keys and merges the two softmax pieces.  Everywhere else
        `attend_branches_reference`."""
        B, P, N = self._check_branches(q, k_new, v_new, C, T, key_valid)
        if not self.uses_kernel(q, k_new.shape[1]):
            return self.attend_branches_reference(layer, q, k_new, v_new, scale, C, T, key_valid=key_valid, slopes=slopes)
        from . import ops

        H, d, CT = q.shape[1], self.head_dim, int(C) * int(T)
        kp, vp = self.k[layer, :, :, :P].permute(0, 2, 1, 3), self.v[layer, :, :, :P].permute(0, 2, 1, 3)    # [rows, P, H, 128] views
        kv = key_valid.to(torch.uint8).contiguous() if key_valid is not None else None
        q4 = q.as_strided((B, CT, H, d), (CT * q.stride(0), q.stride(0), q.stride(1), 1))
        o1, lse1 = ops.flash_attn_fwd_f32(q4, kp, vp, slopes, kv, scale, causal=False)       # o1 unrounded: the answer is rounded once, by the merge
        o = ops.branch_attn_merge(q, k_new, v_new, o1.view(N, H, d), lse1, scale, int(T), CT, slopes=slopes)
        return o.view(N, H * d)

    def attend_branches_reference(self, layer: int, q, k_new, v_new, scale: float, C: int, T: int, key_valid=None, slopes=None) -> torch.Tensor:
        """The two stages of `attend_branches` in plain torch on any device and dtype, fp32 at least.  Stage 1, what the flash forward returns:
        every row's scores over the prompt keys of its sentence, ALiBi slope * (j - (length - 1)), padding mask -> lse1 and o1 (a fully
        masked prompt: lse1 = -inf, o1 = 0).  Stage 2, csrc/branch_attn.hip: L1 = lse1 - slope * (t + 1); own scores e_u = scale q . k_new[u]
        + slope * (u - t) for u <= t; M = max(L1, max e_u); o = (exp(L1 - M) o1 + sum exp(e_u - M) v_new[u]) / (exp(L1 - M) + sum exp(e_u - M))."""
        B, P, N = self._check_branches(q, k_new, v_new, C, T, key_valid)
        C, T = int(C), int(T)
        H, d = q.shape[1], self.head_dim
        ct = torch.float64 if q.dtype == torch.float64 else torch.float32
        rep = H // k_new.shape[1]
        grow = lambda t: t.repeat_interleave(rep, dim=1) if rep > 1 else t
        qf = q.to(ct).view(B, C * T, H, d) * scale
        sl = slopes.to(ct).view(1, H, 1, 1) if slopes is not None else None
        # stage 1: the prompt
        kp, vp = grow(self.k[layer, :, :, :P].to(ct)), grow(self.v[layer, :, :, :P].to(ct))                  # [B, H, P, d]
        s1 = torch.einsum("bnhd,bhjd->bhnj", qf, kp)
        if sl is not None:
            s1 = s1 + sl * torch.arange(1 - P, 1, device=q.device, dtype=ct).view(1, 1, 1, P)
        if key_valid is not None:
            s1 = s1.masked_fill(~key_valid.bool().view(B, 1, 1, P), float("-inf"))
        lse1 = torch.logsumexp(s1, dim=-1)                                                                   # [B, H, CT]; -inf: nothing visible
        p1 = torch.exp(s1 - torch.where(torch.isinf(lse1), torch.zeros_like(lse1), lse1).unsqueeze(-1))
        o1 = torch.einsum("bhnj,bhjd->bhnd", p1, vp)                                                         # (0 where nothing is visible)
        # stage 2: the own keys and the merge
        tpos = torch.arange(T, device=q.device)
        q5 = qf.view(B, C, T, H, d)
        k5, v5 = grow(k_new.to(ct)).view(B, C, T, H, d), grow(v_new.to(ct)).view(B, C, T, H, d)
        e = torch.einsum("bcthd,bcuhd->bchtu", q5, k5)
        rel = (tpos.view(1, T) - tpos.view(T, 1)).to(ct)                                                     # [t, u] = u - t
        if sl is not None:
            e = e + sl.view(1, 1, H, 1, 1) * rel
        e = e.masked_fill((rel > 0).view(1, 1, 1, T, T), float("-inf"))
        L1 = lse1.view(B, H, C, T).permute(0, 2, 1, 3)                                                       # [B, C, H, T]
        if sl is not None:
            L1 = L1 - sl.view(1, 1, H, 1) * (tpos + 1).to(ct).view(1, 1, 1, T)
        M = torch.maximum(L1, e.amax(dim=-1))
        w1, pu = torch.exp(L1 - M), torch.exp(e - M.unsqueeze(-1))
        o1 = o1.view(B, H, C, T, d).permute(0, 2, 1, 3, 4)                                                   # [B, C, H, T, d]
        o = (w1.unsqueeze(-1) * o1 + torch.einsum("bchtu,bcuhd->bchtd", pu, v5)) / (w1 + pu.sum(dim=-1)).unsqueeze(-1)
        return o.permute(0, 1, 3, 2, 4).reshape(N, H * d).to(q.dtype)

    # ---- the cached step of the Persimmon host (OtterHD / Fuyu-8B): q / k LayerNorm per head + partial rotary fused into the step ---------

    def uses_persimmon_kernel(self, qkv: torch.Tensor, rot: int) -> bool:
        return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and self.dtype == torch.bfloat16 and not self.int8 and self.head_dim == 64
                and rot % 16 == 0 and 0 < rot <= 64)

    def attend_persimmon(self, layer: int, qkv, gq, bq, gk, bk, cos, sin, rot: int, eps: float, scale: float, key_valid=None) -> torch.Tensor:
        """One cached step of `layer` of the Persimmon host at position `length` (which the caller advances once per forward, after the last
        layer): qkv [N,H,3,d] the projection of the new token (per head q | k | v); gq / bq / gk / bk fp32 [d] the q / k LayerNorm's gamma
        and beta; cos / sin fp32 [rot] rows of that position; key_valid uint8 / bool [N, length+1] or None.  Returns o [N, H*d] in qkv's
        dtype.  Replay mode: the position is `pos_dev`, cos / sin are the whole fp32 tables [>= max_len, rot] and the mask is the cache's
        own `valid` (key_valid must be None).  On csrc/persimmon_decode_cache.hip where `uses_persimmon_kernel` holds, everywhere else the
        plain-torch restatement."""
        if self.int8:
            raise NotImplementedError("StaticKVCache.attend_persimmon: an int8 key / value cache is not built for head_dim 64 (the Persimmon host)")
        if self.replay and key_valid is not None:
            raise ValueError("StaticKVCache.attend_persimmon: in replay mode the mask is the cache's own (`valid`); pass key_valid=None")
        if self.uses_persimmon_kernel(qkv, rot):
            from . import ops

            if self.replay:
                return ops.persimmon_decode_attn_cached_dyn(qkv, gq, bq, gk, bk, cos, sin, self.k[layer], self.v[layer], self.pos_dev, rot, eps,
                                                            scale, src=self.src, key_valid=self.valid)
            return ops.persimmon_decode_attn_cached(qkv, gq, bq, gk, bk, cos, sin, self.k[layer], self.v[layer], self.length, rot, eps, scale,
                                                    src=self.src, key_valid=key_valid)
        return self.attend_persimmon_reference(layer, qkv, gq, bq, gk, bk, cos, sin, rot, eps, scale, key_valid=key_valid)

    def attend_persimmon_reference(self, layer: int, qkv, gq, bq, gk, bk, cos, sin, rot: int, eps: float, scale: float,
                                   key_valid=None) -> torch.Tensor:
        """What csrc/persimmon_decode_cache.hip does, in plain torch on any device and dtype: LayerNorm of q and k over the head and the
        rotate-half rotary on their first `rot` dims in fp32 at least (fp64 for fp64 inputs), k rounded to the cache dtype once, k and the raw
        v appended at slot `length` of the row's own row, keys 0..length gathered through the table, padding mask, softmax in fp32 at
        least, a fully masked row -> 0.  Replay mode: the position is read from `pos_dev` (not from `length`), cos / sin are the whole
        tables, of which row `pos` is taken, the mask is columns 0..pos of `valid`, and `kernel_steps` is cleared (this step reads the
        position back to the host: it cannot be captured).  The same deliberate exception to "no PyTorch path" as `attend_reference`."""
        if self.int8:
            raise NotImplementedError("StaticKVCache.attend_persimmon: an int8 key / value cache is not built for head_dim 64 (the Persimmon host)")
        if self.replay:
            self.kernel_steps = False
        pos, cos, sin, key_valid = self._step_inputs("attend_persimmon_reference", "rot", cos, sin, key_valid)
        d, ct = qkv.shape[3], torch.float64 if qkv.dtype == torch.float64 else torch.float32
        qf, kf, v_new = qkv[:, :, 0].to(ct), qkv[:, :, 1].to(ct), qkv[:, :, 2]
        if gq is not None:
            qf = torch.nn.functional.layer_norm(qf, (d,), gq.to(ct), bq.to(ct), eps)
            kf = torch.nn.functional.layer_norm(kf, (d,), gk.to(ct), bk.to(ct), eps)
        c, s = cos.to(ct).view(1, 1, rot), sin.to(ct).view(1, 1, rot)
        qf = torch.cat((qf[..., :rot] * c + rotate_half(qf[..., :rot]) * s, qf[..., rot:]), dim=-1)
        kf = torch.cat((kf[..., :rot] * c + rotate_half(kf[..., :rot]) * s, kf[..., rot:]), dim=-1)
        qf = qf.to(qkv.dtype).to(ct)                                           # (the kernel rounds q' to the compute dtype, then scales)
        self.k[layer, :, :, pos] = kf.to(self.dtype)
        self.v[layer, :, :, pos] = v_new.to(self.dtype)
        return self._attend_appended(layer, qf, pos, scale, key_valid, None, qkv.dtype)


class _BranchView:
    """What a host's cached-step code gets in place of the cache during a branch pass (`StaticKVCache.branches(C, T)`): its `attend` is the
    cache's `attend_branches` for C candidates of T positions per sentence.  Rotary embeddings are the host's business here (the rows of one
    pass stand at T different positions): `attend` takes q and k rotated already and refuses cos / sin.  Never in replay mode."""
    replay = False

    def __init__(self, cache: StaticKVCache, C: int, T: int):
        self.cache, self.C, self.T = cache, int(C), int(T)

    @property
    def length(self) -> int:
        return self.cache.length

    def attend(self, layer: int, q, k_new, v_new, scale: float, cos=None, sin=None, key_valid=None, slopes=None) -> torch.Tensor:
        if cos is not None or sin is not None:
            raise ValueError("StaticKVCache.branches: q and k_new come rotated; cos / sin must be None")
        return self.cache.attend_branches(layer, q, k_new, v_new, scale, self.C, self.T, key_valid=key_valid, slopes=slopes)
