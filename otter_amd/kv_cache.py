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

The cached step runs on csrc/decode_cache.hip (`ops.decode_attn_cached`) on the GPU in bf16 with head_dim 128 and as many key / value heads
as query heads.  Everywhere else -- the CPU, fp32 compute, other head sizes -- `attend_reference` runs: a plain-torch restatement of exactly
what the kernel does.  Like `Int8FrozenLinear`'s, that branch is a deliberate exception to "no PyTorch path": it is what makes the bookkeeping
(the table, the append, the hosts' wiring) testable without a GPU, and it is the structure the kernel's oracle follows.
"""
from __future__ import annotations

from typing import Optional

import torch


def rotate_half(x: torch.Tensor) -> torch.Tensor:
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def cache_geometry(config):
    """(n_layers, key / value heads, head_dim, the host's position limit) of a decoder host's config (MPT or LLaMA)."""
    if hasattr(config, "d_model"):          # MPTConfig
        return int(config.n_layers), int(config.n_heads), int(config.d_model) // int(config.n_heads), int(config.max_seq_len)
    heads = int(config.num_attention_heads)
    head_dim = getattr(config, "head_dim", None) or int(config.hidden_size) // heads
    return (int(config.num_hidden_layers), int(getattr(config, "num_key_value_heads", None) or heads), int(head_dim),
            int(config.max_position_embeddings))


class StaticKVCache:
    def __init__(self, n_layers: int, rows: int, n_heads: int, head_dim: int, max_len: int, device, dtype: torch.dtype = torch.bfloat16):
        if min(n_layers, rows, n_heads, head_dim) < 1 or max_len < 2:
            raise ValueError("StaticKVCache: n_layers, rows, n_heads, head_dim >= 1 and max_len >= 2")
        self.n_layers, self.rows, self.n_heads, self.head_dim, self.max_len = int(n_layers), int(rows), int(n_heads), int(head_dim), int(max_len)
        shape = (self.n_layers, self.rows, self.n_heads, self.max_len, self.head_dim)
        self.k = torch.zeros(shape, dtype=dtype, device=device)
        self.v = torch.zeros(shape, dtype=dtype, device=device)
        self.length = 0
        self.src: Optional[torch.Tensor] = None

    # ---- bookkeeping ----------------------------------------------------------------------------------------------------------------

    @property
    def device(self):
        return self.k.device

    @property
    def dtype(self):
        return self.k.dtype

    def get_seq_length(self) -> int:
        return self.length

    def __len__(self):          # (a legacy cache answers len() with its layer count)
        return self.n_layers

    def data_ptrs(self):
        return (self.k.data_ptr(), self.v.data_ptr())

    def check_step(self, rows: int, S: int) -> None:
        """The two things a forward may do with this cache: prefill it while empty, or append one position."""
        if torch.is_grad_enabled():
            raise RuntimeError("StaticKVCache is written in place and is for inference only: run the forward under torch.no_grad()")
        if rows != self.rows:
            raise ValueError("StaticKVCache was created for %d rows, the forward has %d" % (self.rows, rows))
        if self.length > 0 and S != 1:
            raise ValueError("StaticKVCache holds %d positions: only a one-token step can follow (got %d tokens)" % (self.length, S))
        if self.length + S > self.max_len:
            raise ValueError("StaticKVCache: %d + %d positions exceed max_len=%d" % (self.length, S, self.max_len))

    def fill(self, layer: int, k: torch.Tensor, v: torch.Tensor) -> None:
        """Prefill: k, v indexed [rows, n_heads, S, head_dim] (any strides: the views the flash and SDPA paths produce) -> positions [0, S).
        One strided copy per tensor."""
        if self.length != 0:
            raise ValueError("StaticKVCache.fill: the cache is not empty")
        S = k.shape[2]
        want = (self.rows, self.n_heads, S, self.head_dim)
        if tuple(k.shape) != want or tuple(v.shape) != want or S > self.max_len:
            raise ValueError("StaticKVCache.fill: expected k, v %s with S <= %d, got %s / %s" % (want, self.max_len, tuple(k.shape), tuple(v.shape)))
        self.k[layer, :, :, :S].copy_(k)
        self.v[layer, :, :, :S].copy_(v)

    def reorder(self, beam_idx: torch.Tensor) -> None:
        """Beam search: sequence n continues what was sequence beam_idx[n].  Only the table moves (rows x length x 4 bytes)."""
        if self.src is None:
            self.src = torch.arange(self.rows, dtype=torch.int32, device=self.device).view(-1, 1).repeat(1, self.max_len)
        L = self.length
        if L:
            self.src[:, :L] = self.src[:, :L].index_select(0, beam_idx.to(self.device))

    def _gathered(self, t: torch.Tensor, upto: int) -> torch.Tensor:
        """t [rows, H, max_len, d] -> [rows, H, upto, d]: position j of row n from row src[n, j]."""
        if self.src is None:
            return t[:, :, :upto]
        idx = self.src[:, :upto].long()                                        # [rows, upto]
        pos = torch.arange(upto, device=t.device).view(1, -1)
        return t[idx, :, pos].permute(0, 2, 1, 3)                              # [rows, upto, H, d] -> [rows, H, upto, d]

    def to_legacy(self, host) -> tuple:
        """The tuple-of-tuples cache in the host's own layout, gathered through the table: "mpt" (or an MPT module) k [N,H,d,S], v [N,H,S,d];
        "llama" k, v [N,H,S,d]."""
        name = host if isinstance(host, str) else type(host).__name__
        mpt = "mpt" in name.lower()
        if not mpt and "llama" not in name.lower():
            raise ValueError("StaticKVCache.to_legacy: host must be 'mpt' or 'llama' (or one of their modules), got %r" % (name,))
        out = []
        for i in range(self.n_layers):
            k, v = self._gathered(self.k[i], self.length), self._gathered(self.v[i], self.length)
            out.append((k.transpose(2, 3) if mpt else k, v))
        return tuple(out)

    # ---- the cached step ------------------------------------------------------------------------------------------------------------

    def uses_kernel(self, q: torch.Tensor, n_kv: int) -> bool:
        return q.is_cuda and q.dtype == torch.bfloat16 and self.dtype == torch.bfloat16 and self.head_dim == 128 and n_kv == q.shape[1]

    def attend(self, layer: int, q, k_new, v_new, scale: float, cos=None, sin=None, key_valid=None, slopes=None) -> torch.Tensor:
        """One cached step of `layer` at position `length` (which the caller advances once per forward, after the last layer):
        q [N,H,d], k_new / v_new [N,H_kv,d] views of the projection output; cos / sin fp32 [d] rows of that position or None;
        key_valid uint8 / bool [N, length+1] or None; slopes fp32 [H] or None.  Returns o [N, H*d] in q's dtype."""
        if self.uses_kernel(q, k_new.shape[1]):
            from . import ops

            return ops.decode_attn_cached(q, k_new, v_new, self.k[layer], self.v[layer], self.length, scale, cos=cos, sin=sin, src=self.src,
                                          key_valid=key_valid, slopes=slopes)
        return self.attend_reference(layer, q, k_new, v_new, scale, cos=cos, sin=sin, key_valid=key_valid, slopes=slopes)

    def attend_reference(self, layer: int, q, k_new, v_new, scale: float, cos=None, sin=None, key_valid=None, slopes=None) -> torch.Tensor:
        """What csrc/decode_cache.hip does, in plain torch on any device and dtype: rotary (fp32 at least, k rounded to the cache dtype once),
        append at slot `length` of the row's own row, gather keys 0..length through the table, ALiBi slope * (j - length), padding mask,
        softmax in fp32 at least, a fully masked row -> 0."""
        pos, N, H, d = self.length, q.shape[0], q.shape[1], q.shape[2]
        if pos < 1 or pos >= self.max_len:
            raise ValueError("StaticKVCache: a cached step needs 1 <= length < max_len (length=%d, max_len=%d)" % (pos, self.max_len))
        ct = torch.float64 if q.dtype == torch.float64 else torch.float32
        qf, kf = q.to(ct), k_new.to(ct)
        if cos is not None:
            c, s = cos.to(ct), sin.to(ct)
            if c.dim() == 2:
                c, s = c[:, None], s[:, None]
            qf = qf * c + rotate_half(qf) * s
            kf = kf * c + rotate_half(kf) * s
        self.k[layer, :, :, pos] = kf.to(self.dtype)
        self.v[layer, :, :, pos] = v_new.to(self.dtype)
        k = self._gathered(self.k[layer], pos + 1).to(ct)                      # column pos of the table is the row's own index
        v = self._gathered(self.v[layer], pos + 1).to(ct)
        if k.shape[1] != H:
            k, v = k.repeat_interleave(H // k.shape[1], dim=1), v.repeat_interleave(H // v.shape[1], dim=1)
        s_ = torch.einsum("nhd,nhjd->nhj", qf * scale, k)
        if slopes is not None:
            s_ = s_ + slopes.to(ct).view(1, H, 1) * torch.arange(-pos, 1, device=q.device, dtype=ct).view(1, 1, -1)
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
        return o.reshape(N, H * d).to(q.dtype)
