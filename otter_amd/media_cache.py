"""Cross-attention cache for cached generation (`generate(..., cross_attention_cache=True)`).

A cached step of the legacy path recomputes `media_locations` from its one-token `input_ids`: text_time is 0, the masked cross-attention
contributes exactly 0 (a quirk of the reference, reproduced on purpose) -- and every gated block still casts and
re-projects the media through `to_kv` and runs the 64-row-tile attention kernel on one query per row to get that zero.  `MediaCache`
carries what a step needs to return what the last position of the full re-forward returns:

    seen      int32 [rows]: the number of <image> tokens each row has consumed so far.  Set by the prompt pass (`media_locations.sum(1)`),
              advanced on the device each step (`seen += (new_id == media_token_id)`), never read by the host.  The advanced value IS the
              step's text_time (attend_previous=True), the same for every gated layer.  `reorder(beam_idx)` is an index_select.
    kv[i]     [sentences, T_img * n, 2 * inner] in the compute dtype, for every decoder layer i that has a gated block (None elsewhere): the
              media projected through that block's `to_kv`, computed once after the prompt pass.  One copy per SENTENCE, not per beam
              (sentences = rows / rows_per_media): the beams of a sentence are contiguous and beam search never moves a row to another
              sentence, so kv is never reordered and its pointers never change.
    geometry  T_img, n (latents per media), heads, mask mode; state empty / filled.

The step's attention core runs on csrc/xattn_decode.hip (`ops.xattn_decode`) on the GPU in bf16.  Everywhere else -- the CPU, fp32 compute --
`attend_reference` runs: a plain-torch restatement of exactly what the kernel does.  Like `StaticKVCache.attend_reference`, that branch is
a deliberate exception to "no PyTorch path": it is what makes the bookkeeping and the hosts' wiring testable without a GPU, and it is the
structure the kernel's oracle follows.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn.functional as F

from ._capi import MASK_EQ, MASK_GE

HEAD_DIM = 64


class MediaCache:
    def __init__(self, rows: int, media_token_id: int, rows_per_media: int = 1):
        rows, rows_per_media = int(rows), int(rows_per_media)
        if rows < 1 or rows_per_media < 1 or rows % rows_per_media != 0:
            raise ValueError("MediaCache: rows >= 1 and a multiple of rows_per_media >= 1 (got %d, %d)" % (rows, rows_per_media))
        self.rows, self.rows_per_media, self.media_token_id = rows, rows_per_media, int(media_token_id)
        self.sentences = rows // rows_per_media
        self.seen: Optional[torch.Tensor] = None
        self.kv: List[Optional[torch.Tensor]] = []
        self.T_img = self.n = self.heads = 0
        self.mask_mode = MASK_EQ
        self.filled = False
        self.fixed_address = False      # generate(..., graph_decode=True): `seen` is read by a captured graph and must never be replaced

    # ---- bookkeeping ----------------------------------------------------------------------------------------------------------------

    def data_ptrs(self):
        return tuple(t.data_ptr() for t in self.kv if t is not None)

    def check_step(self, rows: int, S: int, placement_augmentation: bool = False) -> None:
        """The two things a forward may do with this cache: fill it while empty (the prompt pass), or advance it by one token."""
        if torch.is_grad_enabled():
            raise RuntimeError("MediaCache is advanced in place and is for inference only: run the forward under torch.no_grad()")
        if placement_augmentation:
            raise ValueError("MediaCache: use_media_placement_augmentation draws attend_previous per forward; a cached step cannot follow it")
        if rows != self.rows:
            raise ValueError("MediaCache was created for %d rows, the forward has %d" % (self.rows, rows))
        if self.filled and S != 1:
            raise ValueError("MediaCache is filled: only a one-token step can follow (got %d tokens)" % S)

    def fill(self, media_locations: torch.Tensor, layers) -> None:
        """After the prompt pass: `layers` are the conditioned OtterLayers of the decoder (vis_x [rows, T_img, n, Dv], the beams of a
        sentence holding equal media).  seen <- the rows' <image> counts; kv[i] <- to_kv of layer i's gated block on the sentences' media."""
        if self.filled:
            raise ValueError("MediaCache.fill: the cache is not empty")
        self.seen = media_locations.sum(dim=1).to(torch.int32)
        self.kv = []
        for layer in layers:
            g = getattr(layer, "gated_cross_attn_layer", None)
            if g is None:
                self.kv.append(None)
                continue
            vis = layer.vis_x
            if vis is None or vis.shape[0] != self.rows:
                raise ValueError("MediaCache.fill: every gated layer must be conditioned on vis_x of %d rows" % self.rows)
            a = g.attn
            geo = (int(vis.shape[1]), int(vis.shape[2]), int(a.heads), MASK_EQ if a.only_attend_immediate_media else MASK_GE)
            if self.T_img and geo != (self.T_img, self.n, self.heads, self.mask_mode):
                raise ValueError("MediaCache.fill: the gated layers differ in geometry")
            self.T_img, self.n, self.heads, self.mask_mode = geo
            self.kv.append(self._project(vis[::self.rows_per_media], a.to_kv.weight))
        if not self.T_img:
            raise ValueError("MediaCache.fill: the decoder has no gated cross-attention layer")
        self.filled = True

    def _project(self, vis: torch.Tensor, Wkv: torch.Tensor) -> torch.Tensor:
        from . import functional as OF

        S, T_img, n, Dv = vis.shape
        cd = torch.float64 if vis.dtype == torch.float64 else OF.compute_dtype_for(vis)
        med = vis.reshape(S * T_img * n, Dv).contiguous()
        if vis.is_cuda and cd == torch.bfloat16:
            from . import ops

            kv = ops.gemm_nt(ops.cast(med, cd), OF.shadows.w(Wkv, cd))
        else:
            kv = F.linear(med.to(cd), Wkv.detach().to(cd))
        return kv.view(S, T_img * n, Wkv.shape[0])

    def expand(self, beams: int) -> None:
        """After a prompt pass that ran one row per sentence (`generate(..., share_prompt=True)`): every row becomes `beams` contiguous rows
        of the same sentence.  The counts are repeated; kv, one copy per sentence already, is untouched.  Before `fixed_address` is set
        (`seen` is replaced here) and before any cached step."""
        beams = int(beams)
        if not self.filled:
            raise ValueError("MediaCache.expand: the cache is empty (the prompt pass fills it)")
        if self.rows_per_media != 1 or self.fixed_address:
            raise ValueError("MediaCache.expand: only a cache of one row per sentence that no captured graph reads can be expanded")
        if beams < 1:
            raise ValueError("MediaCache.expand: beams >= 1 (got %d)" % beams)
        self.seen = self.seen.repeat_interleave(beams)
        self.rows, self.rows_per_media = self.sentences * beams, beams

    def rows_view(self, n: int) -> "MediaCache":
        """A filled cache read for rows * n rows, row r reading the media and the <image> count of this cache's row r // n: what the candidate
        rows of `score_candidates` attend through (n = C * T rows per sentence, none of which holds the media token, so the count IS their
        text_time).  A new object with its own copy of the counts over the SAME projected media: this cache is not changed, may be read
        through any number of views, and goes on as it was.  (`expand` is the mutating, one-call form beam search uses.)"""
        n = int(n)
        if not self.filled:
            raise ValueError("MediaCache.rows_view: the cache is empty (the prompt pass fills it)")
        if n < 1:
            raise ValueError("MediaCache.rows_view: n >= 1 (got %d)" % n)
        view = MediaCache(self.rows * n, self.media_token_id, rows_per_media=self.rows_per_media * n)
        view.seen, view.kv = self.seen.repeat_interleave(n), self.kv
        view.T_img, view.n, view.heads, view.mask_mode, view.filled = self.T_img, self.n, self.heads, self.mask_mode, True
        return view

    def advance(self, new_ids: torch.Tensor) -> torch.Tensor:
        """One step: new_ids [rows] or [rows, 1].  Returns the step's text_time, int32 [rows] (the cache's own tensor)."""
        if not self.filled:
            raise ValueError("MediaCache.advance: the cache is empty (the prompt pass fills it)")
        self.seen += (new_ids.reshape(-1) == self.media_token_id).to(torch.int32)
        return self.seen

    def reorder(self, beam_idx: torch.Tensor) -> None:
        """Beam search: row n continues what was row beam_idx[n] (a row of the same sentence).  Only the counts move."""
        if self.filled and self.fixed_address:
            self.seen.copy_(self.seen.index_select(0, beam_idx.to(self.seen.device)))
        elif self.filled:
            self.seen = self.seen.index_select(0, beam_idx.to(self.seen.device))

    # ---- the cached step ------------------------------------------------------------------------------------------------------------

    def uses_kernel(self, q: torch.Tensor, layer: int) -> bool:
        return q.is_cuda and q.dtype == torch.bfloat16 and self.kv[layer].dtype == torch.bfloat16

    def attend(self, layer: int, q: torch.Tensor) -> torch.Tensor:
        """The attention core of gated layer `layer` for this step: q [rows, heads * 64] (any row stride) -> o [rows, heads * 64]."""
        if self.uses_kernel(q, layer):
            from . import ops

            kv, inner = self.kv[layer], self.heads * HEAD_DIM
            return ops.xattn_decode(q, kv[..., :inner], kv[..., inner:], self.heads, self.seen, self.n, self.rows_per_media, self.mask_mode,
                                    HEAD_DIM ** -0.5)
        return self.attend_reference(layer, q)

    def attend_reference(self, layer: int, q: torch.Tensor, text_time: Optional[torch.Tensor] = None) -> torch.Tensor:
        """What csrc/xattn_decode.hip does, in plain torch on any device and dtype: row r reads the media of sentence r / rows_per_media;
        key j belongs to media j / n + 1; EQ admits media == text_time, GE media <= text_time; a row with no admitted key is uniform over
        ALL keys (the reference's masked_fill(-finfo.max)); a row with text_time == 0 is zeroed in EQ mode only.  fp32 at least."""
        kv, H, n = self.kv[layer], self.heads, self.n
        inner = H * HEAD_DIM
        N, M = q.shape[0], kv.shape[1]
        ct = torch.float64 if q.dtype == torch.float64 else torch.float32
        tt = (self.seen if text_time is None else text_time).to(q.device).long().view(N, 1)
        sent = torch.arange(N, device=q.device) // self.rows_per_media
        k = kv[sent, :, :inner].to(ct).view(N, M, H, HEAD_DIM)
        v = kv[sent, :, inner:].to(ct).view(N, M, H, HEAD_DIM)
        s = torch.einsum("nhd,nmhd->nhm", q.to(ct).view(N, H, HEAD_DIM) * (HEAD_DIM ** -0.5), k)
        media_time = (torch.arange(M, device=q.device) // n + 1).view(1, M)
        allowed = (tt == media_time) if self.mask_mode == MASK_EQ else (tt >= media_time)          # [N, M]
        none = ~allowed.any(dim=1, keepdim=True)
        s = torch.where((allowed | none)[:, None, :], s, torch.full_like(s, float("-inf")))
        s = torch.where(none[:, None, :], torch.zeros_like(s), s)
        o = torch.einsum("nhm,nmhd->nhd", torch.softmax(s, dim=-1), v)
        if self.mask_mode == MASK_EQ:
            o = o.masked_fill((tt == 0).view(N, 1, 1), 0.0)
        return o.reshape(N, inner).to(q.dtype)
