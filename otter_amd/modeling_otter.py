"""Drop-in mirror of the reference's `src/otter_ai/models/otter/modeling_otter.py` for the fusion hot path.

Same class names, constructor arguments, parameter names (state-dict keys) and forward()/generate() signatures as
the reference, so `pipeline/train/instruction_following.py` can import this module in place of
the original.  The arithmetic of every class below runs in libotter_hip.so through the autograd
functions of `otter_amd.functional`; the nn.LayerNorm / nn.Linear children are parameter containers only (their own
forward() is never called), kept so that checkpoints load/save with the reference's key names.

Reference lines: OtterPerceiverBlock :129-184, OtterPerceiverResampler :187-235, OtterMaskedCrossAttention :238-340,
OtterGatedCrossAttentionBlock :343-395, OtterLayer :398-442, OtterLMMixin :445-520, OtterForConditionalGeneration :739-1042.
"""
from __future__ import annotations

import os
import random
import sys
import warnings
from typing import List, Optional

import torch
import torch.nn as nn
from transformers import PreTrainedModel
from transformers.modeling_outputs import CausalLMOutputWithPast

from . import functional as OF
from . import ops
from ._capi import MASK_EQ, MASK_GE, MASK_NONE, RowMap
from .clip import CLIPVisionModel
from .configuration_otter import OtterConfig
from .mpt import MPTForCausalLM

__KNOWN_DECODER_LAYERS_ATTR_NAMES = {"llama": "model.layers", "MPTForCausalLM": "transformer.blocks"}


def master_print(*args, **kwargs):
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        if dist.get_rank() == 0:
            print(*args, **kwargs)
    else:
        print(*args, **kwargs)


def _infer_decoder_layers_attr_name(model: nn.Module):
    for k, v in __KNOWN_DECODER_LAYERS_ATTR_NAMES.items():
        if k.lower() in model.__class__.__name__.lower():
            return v
    raise ValueError("We require the attribute name for the nn.ModuleList in the decoder storing the transformer block layers.")


def extend_instance(obj, mixin):
    """Apply mixins to a class instance after creation (modeling_otter.py:94-98)."""
    base_cls = obj.__class__
    obj.__class__ = type(base_cls.__name__, (mixin, base_cls), {})


def getattr_recursive(obj, att):
    if att == "":
        return obj
    i = att.find(".")
    return getattr(obj, att) if i < 0 else getattr_recursive(getattr(obj, att[:i]), att[i + 1:])


def setattr_recursive(obj, att, val):
    if "." in att:
        obj = getattr_recursive(obj, ".".join(att.split(".")[:-1]))
    setattr(obj, att.split(".")[-1], val)


def exists(val):
    return val is not None


# ======================================================================================================================
# perceiver resampler
# ======================================================================================================================


class OtterPerceiverBlock(nn.Module):
    def __init__(self, *, dim: int, dim_head: int = 64, heads: int = 8, mult: int = 4):
        super().__init__()
        if dim_head != OF.HEAD_DIM:
            raise NotImplementedError("otter_amd attention kernels are built for dim_head=64 (the reference's only value)")
        self.scale = dim_head ** -0.5
        self.heads = heads
        inner_dim = dim_head * heads
        ff_dim = dim * mult
        self.norm_media = nn.LayerNorm(dim)
        self.norm_latents = nn.LayerNorm(dim)
        self.to_q = nn.Linear(dim, inner_dim, bias=False)
        self.to_kv = nn.Linear(dim, inner_dim * 2, bias=False)
        self.to_out = nn.Linear(inner_dim, dim, bias=False)
        self.feed_forward = nn.ModuleList([nn.LayerNorm(dim), nn.Linear(dim, ff_dim, bias=False), nn.GELU(),
                                           nn.Linear(ff_dim, dim, bias=False)])

    def forward(self, x: torch.Tensor, latents: torch.Tensor) -> torch.Tensor:
        """x (b, T, n1, D) image features; latents (b, T, n2, D)."""
        b, T, n1, D = x.shape
        n2 = latents.shape[2]
        ff = self.feed_forward
        y = OF.PerceiverBlockFn.apply(x.reshape(b * T, n1, D), latents.reshape(b * T, n2, D), self.heads, self.norm_media.eps,
                                      self.norm_media.weight, self.norm_media.bias, self.norm_latents.weight,
                                      self.norm_latents.bias, self.to_q.weight, self.to_kv.weight, self.to_out.weight,
                                      ff[0].weight, ff[0].bias, ff[1].weight, ff[3].weight)
        return y.view(b, T, n2, D)


class _BroadcastEmbAddFn(torch.autograd.Function):
    """x [outer, F, inner, D] + emb[:F] (broadcast over outer and inner): frame_embs / media_time_embs
    (modeling_otter.py:224-229).  Forward = one in-place row add on a copy; backward = column sums per embedding row."""

    @staticmethod
    def forward(ctx, x4, emb):
        outer, F, inner, D = x4.shape
        y = x4.contiguous().clone()
        e = emb.detach()[:F].contiguous().float()
        ops.K.check(ops.K.lib().otter_add_frame_embs(y.data_ptr(), ops.K.dt(y), e.data_ptr(), outer, F, inner, D, ops.K.stream()),
                    "add_frame_embs")
        ctx.shape = (outer, F, inner, D)
        ctx.emb_shape = emb.shape
        ctx.emb_dtype = emb.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        outer, F, inner, D = ctx.shape
        demb = None
        if ctx.needs_input_grad[1]:
            dy2 = dy.contiguous().view(outer * F * inner, D)
            demb = torch.zeros(ctx.emb_shape, dtype=torch.float32, device=dy.device)
            flat = demb.view(-1, D)
            for f in range(F):
                ops.colsum(dy2, RowMap(inner, F * inner, f * inner), outer * inner, out=flat[f])
            demb = demb.to(ctx.emb_dtype)
        return (dy if ctx.needs_input_grad[0] else None), demb


class OtterPerceiverResampler(nn.Module):
    def __init__(self, *, dim: int, depth: int = 6, dim_head: int = 64, heads: int = 8, num_latents: int = 64,
                 max_num_media: Optional[int] = None, max_num_frames: Optional[int] = None, ff_mult: int = 4):
        super().__init__()
        self.latents = nn.Parameter(torch.randn(num_latents, dim))
        self.frame_embs = nn.Parameter(torch.randn(max_num_frames, dim)) if exists(max_num_frames) else None
        self.media_time_embs = nn.Parameter(torch.randn(max_num_media, 1, dim)) if exists(max_num_media) else None
        self.layers = nn.ModuleList([OtterPerceiverBlock(dim=dim, dim_head=dim_head, heads=heads, mult=ff_mult)
                                     for _ in range(depth)])
        self.norm = nn.LayerNorm(dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (b, T, F, v, D) -> (b, T, n, D)."""
        b, T, F, v, D = x.shape
        if exists(self.frame_embs):
            x = _BroadcastEmbAddFn.apply(x.reshape(b * T, F, v, D), self.frame_embs).view(b, T, F, v, D)
        x = x.reshape(b, T, F * v, D)
        if exists(self.media_time_embs):
            x = _BroadcastEmbAddFn.apply(x.reshape(b, T, F * v, D), self.media_time_embs).view(b, T, F * v, D)
        latents = OF.ExpandLatentsFn.apply(self.latents, b * T).view(b, T, *self.latents.shape)
        for block in self.layers:
            latents = block(x, latents)
        return OF.layer_norm(latents, self.norm.weight, self.norm.bias, self.norm.eps, latents.dtype)


# ======================================================================================================================
# masked / gated cross attention
# ======================================================================================================================


def _mask_mode(media_locations, only_attend_immediate_media):
    if media_locations is None:
        return MASK_NONE
    return MASK_EQ if only_attend_immediate_media else MASK_GE


class OtterMaskedCrossAttention(nn.Module):
    def __init__(self, *, dim: int, dim_visual: int, dim_head: int = 64, heads: int = 8, only_attend_immediate_media: bool = True):
        super().__init__()
        if dim_head != OF.HEAD_DIM:
            raise NotImplementedError("otter_amd attention kernels are built for dim_head=64 (the reference's only value)")
        self.scale = dim_head ** -0.5
        self.heads = heads
        inner_dim = dim_head * heads
        self.norm = nn.LayerNorm(dim)
        self.to_q = nn.Linear(dim, inner_dim, bias=False)
        self.to_kv = nn.Linear(dim_visual, inner_dim * 2, bias=False)
        self.to_out = nn.Linear(inner_dim, dim, bias=False)
        self.only_attend_immediate_media = only_attend_immediate_media

    def forward(self, x, media, media_locations=None, attend_previous: bool = True, text_time=None):
        """x (B, T_txt, D); media (B, T_img, n, D_img); media_locations bool (B, T_txt).  Stand-alone use of the attention
        sub-module (inside the gated block the fused function is used instead)."""
        mode = _mask_mode(media_locations, self.only_attend_immediate_media)
        tt = text_time
        if mode != MASK_NONE and tt is None:
            tt = ops.text_time(media_locations, attend_previous)
        return OF.masked_cross_attention(x, media, tt, mode, self.heads, self.norm.eps, self.norm.weight, self.norm.bias,
                                         self.to_q.weight, self.to_kv.weight, self.to_out.weight)


class OtterGatedCrossAttentionBlock(nn.Module):
    accepts_deferred = True      # forward(..., deferred=): see OtterLayer.forward / otter_amd.mpt._gated_takes_deferred

    def __init__(self, *, dim: int, dim_visual: int, dim_head: int = 64, heads: int = 8, ff_mult: int = 4,
                 only_attend_immediate_media: bool = True):
        super().__init__()
        self.attn = OtterMaskedCrossAttention(dim=dim, dim_visual=dim_visual, dim_head=dim_head, heads=heads,
                                              only_attend_immediate_media=only_attend_immediate_media)
        self.attn_gate = nn.Parameter(torch.tensor([0.0]))
        self.feed_forward = nn.ModuleList([nn.LayerNorm(dim), nn.Linear(dim, dim * ff_mult, bias=False), nn.GELU(),
                                           nn.Linear(dim * ff_mult, dim, bias=False)])
        self.ff_gate = nn.Parameter(torch.tensor([0.0]))

    def forward(self, x, media, media_locations=None, attend_previous: bool = True, text_time=None, deferred=None):
        """`deferred` (otter_amd extension): an addend of the residual stream that has not been added yet (the MPT host hands each
        block's FFN output to the NEXT LayerNorm pass); the block computes on x + deferred, the add fused into its first LayerNorm."""
        a, ff = self.attn, self.feed_forward
        mode = _mask_mode(media_locations, a.only_attend_immediate_media)
        tt = text_time
        if mode != MASK_NONE and tt is None:
            tt = ops.text_time(media_locations, attend_previous)
        if self.ffn_is_int8():
            return self._forward_int8_ffn(x, media, tt, mode, deferred)
        return OF.GatedCrossAttentionFn.apply(x, media, tt, mode, a.heads, a.norm.eps, a.norm.weight, a.norm.bias, a.to_q.weight,
                                              a.to_kv.weight, a.to_out.weight, self.attn_gate, ff[0].weight, ff[0].bias,
                                              ff[1].weight, ff[3].weight, self.ff_gate, deferred)

    def ffn_is_int8(self) -> bool:
        """Whether `quantize_decoder_int8(gated_blocks=True)` has replaced feed_forward[1] and [3] (otter_amd/quant.py: always both)."""
        return not isinstance(self.feed_forward[1], nn.Linear)

    def _forward_int8_ffn(self, x, media, tt, mode, deferred):
        """forward() with an int8 FFN: the fused GatedCrossAttentionFn takes weights, so the attention half runs
        through OF.masked_cross_attention, then its gate residual, then LayerNorm and the two Int8FrozenLinear by their own routes (GELU in
        the first product's epilogue, the tanh-gate residual in the second's tail).  Inference only: under autograd the quantised FFN
        raises."""
        a, ff = self.attn, self.feed_forward
        if deferred is not None:
            x = x + deferred.to(x.dtype)
        attn = OF.masked_cross_attention(x, media, tt, mode, a.heads, a.norm.eps, a.norm.weight, a.norm.bias, a.to_q.weight, a.to_kv.weight,
                                         a.to_out.weight)
        x1 = (attn.float() * torch.tanh(self.attn_gate.float()) + x.float()).to(x.dtype)
        f = OF.layer_norm(x1, ff[0].weight, ff[0].bias, ff[0].eps, OF.compute_dtype_for(x))
        return ff[3].forward_gated(ff[1](f, act="gelu"), self.ff_gate, x1)

    @torch.no_grad()
    def decode_step(self, x, cache, layer_index: int, deferred=None):
        """One cached step over a MediaCache (otter_amd/media_cache.py): x [rows, 1, D], the step's text_time and this layer's projected media
        come from `cache`.  The launch sequence of GatedCrossAttentionFn.forward with the same ops and epilogues, minus the media cast, the
        `to_kv` product and the side stream they ran on, and with csrc/xattn_decode.hip in place of the 64-row-tile attention kernel:
        (add+)LayerNorm -> to_q -> xattn_decode -> to_out (scale + residual tail) -> LayerNorm -> FF up (GELU tail) -> FF down (scale +
        residual tail).  With an int8 FFN (`ffn_is_int8`) the two FF products are the Int8FrozenLinear's: `ff[1](f, act="gelu")` and
        `ff[3].forward_gated(h, ff_gate, x1)`, the same two tails in the epilogues of csrc/w8.hip, still one chain of launches on one stream.
        On the CPU / in fp32 compute: the same sequence in plain torch around `MediaCache.attend_reference`."""
        a, ff = self.attn, self.feed_forward
        N, S, D = x.shape
        if S != 1:
            raise ValueError("decode_step: one token per row (got %d)" % S)
        cd, rd = OF.compute_dtype_for(x), x.dtype
        x2 = x.reshape(N, D).contiguous()
        d2 = deferred.reshape(N, D).contiguous() if deferred is not None else None
        if x.is_cuda and cd == torch.bfloat16:
            w = OF.shadows.w
            ga, gf = OF._flat_gate(self.attn_gate), OF._flat_gate(self.ff_gate)
            nw, nb = a.norm.weight.detach(), a.norm.bias.detach()
            if d2 is not None:
                x2, xn, _, _ = ops.add_layernorm_fwd(x2, d2, nw, nb, cd, a.norm.eps, need_stats=False)
            else:
                xn = ops.layernorm_fwd(x2, nw, nb, cd, a.norm.eps, need_stats=False)[0]
            q = ops.gemm_nt(xn, w(a.to_q.weight, cd))
            o = cache.attend(layer_index, q)
            x1 = ops.gemm_nt(o, w(a.to_out.weight, cd), out_dtype=rd, kind=OF.EPI_SCALE_RES, gate=ga, R=x2)       # attn*tanh(g)+x
            f = ops.layernorm_fwd(x1, ff[0].weight.detach(), ff[0].bias.detach(), cd, ff[0].eps, need_stats=False)[0]
            if self.ffn_is_int8():                          # [N, 1, .] views: a one-token step, so 17 to 64 rows take the rows kernel
                h = ff[1](f.view(N, 1, D), act="gelu")
                return ff[3].forward_gated(h, gf, x1.view(N, 1, D))
            h = ops.gemm_nt(f, w(ff[1].weight, cd), kind=OF.EPI_GELU)
            y = ops.gemm_nt(h, w(ff[3].weight, cd), out_dtype=rd, kind=OF.EPI_SCALE_RES, gate=gf, R=x1)           # ff*tanh(g)+x1
            return y.view(N, 1, D)
        F = torch.nn.functional
        if d2 is not None:
            x2 = x2 + d2.to(rd)
        lin = lambda t, W: F.linear(t, W.detach().to(cd))
        xn = F.layer_norm(x2.float(), (D,), a.norm.weight.float(), a.norm.bias.float(), a.norm.eps).to(cd)
        o = cache.attend(layer_index, lin(xn, a.to_q.weight))
        x1 = (lin(o, a.to_out.weight).float() * torch.tanh(self.attn_gate.float()) + x2.float()).to(rd)
        f = F.layer_norm(x1.float(), (D,), ff[0].weight.float(), ff[0].bias.float(), ff[0].eps).to(cd)
        if self.ffn_is_int8():
            return ff[3].forward_gated(ff[1](f.view(N, 1, D), act="gelu"), self.ff_gate, x1.view(N, 1, D))
        y = (lin(F.gelu(lin(f, ff[1].weight)), ff[3].weight).float() * torch.tanh(self.ff_gate.float()) + x1.float()).to(rd)
        return y.view(N, 1, D)


class OtterLayer(nn.Module):
    def __init__(self, gated_cross_attn_layer: nn.Module, decoder_layer: nn.Module):
        super().__init__()
        self.gated_cross_attn_layer = gated_cross_attn_layer
        self.decoder_layer = decoder_layer
        self.vis_x = None
        self.media_locations = None
        self.attend_previous = None
        self.text_time = None
        self.media_step = None

    def is_conditioned(self) -> bool:
        return self.vis_x is not None

    def condition_vis_x(self, vis_x) -> None:
        self.vis_x = vis_x

    def condition_media_locations(self, media_locations) -> None:
        self.media_locations = media_locations
        self.text_time = None

    def condition_attend_previous(self, attend_previous) -> None:
        self.attend_previous = attend_previous

    def condition_text_time(self, text_time) -> None:
        """otter_amd extension: the media-time scan is shared by all layers instead of being recomputed per layer."""
        self.text_time = text_time

    def condition_media_step(self, media_step) -> None:
        """otter_amd extension: (MediaCache, this layer's index) for ONE cached step over a media cache, or None (every other forward)."""
        self.media_step = media_step

    def forward(self, lang_x: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, **decoder_layer_kwargs):
        if self.gated_cross_attn_layer is None:
            return self.decoder_layer(lang_x, attention_mask=attention_mask, **decoder_layer_kwargs)
        if self.vis_x is None:
            raise ValueError("vis_x must be conditioned before forward pass")
        if self.media_locations is None:
            raise ValueError("media_locations must be conditioned before forward pass")
        # otter_amd's MPT host may hand over the previous layer's FFN output un-added (`deferred`, mpt.py): the gated block fuses the add
        # into its first LayerNorm; the decoder layer then starts from the block's (materialised) output, which it both normalises and
        # carries on (`fork_input`: one LayerNorm-backward pass instead of an extra gradient add)
        deferred = decoder_layer_kwargs.pop("deferred", None)
        gkw = {"deferred": deferred} if deferred is not None else {}
        if self.media_step is not None:
            lang_x = self.gated_cross_attn_layer.decode_step(lang_x, *self.media_step, **gkw)
        else:
            lang_x = self.gated_cross_attn_layer(lang_x, self.vis_x, media_locations=self.media_locations,
                                                 attend_previous=self.attend_previous, text_time=self.text_time, **gkw)
        if "defer_out" in decoder_layer_kwargs:       # (only otter_amd's MPTBlock takes the extension keywords)
            decoder_layer_kwargs["fork_input"] = True
        return self.decoder_layer(lang_x, attention_mask=attention_mask, **decoder_layer_kwargs)


class OtterLMMixin(nn.Module):
    """Mixin to add cross-attention layers to a language model (modeling_otter.py:445-520)."""

    def set_decoder_layers_attr_name(self, decoder_layers_attr_name):
        self.decoder_layers_attr_name = decoder_layers_attr_name

    def _get_decoder_layers(self):
        return getattr_recursive(self, self.decoder_layers_attr_name)

    def _set_decoder_layers(self, value):
        setattr_recursive(self, self.decoder_layers_attr_name, value)

    def init_otter(self, media_token_id: int, vis_hidden_size: int, cross_attn_every_n_layers: int,
                   use_media_placement_augmentation: bool):
        gated = nn.ModuleList([
            OtterGatedCrossAttentionBlock(dim=self.config.hidden_size, dim_visual=vis_hidden_size)
            if (layer_idx + 1) % cross_attn_every_n_layers == 0 else None
            for layer_idx, _ in enumerate(self._get_decoder_layers())
        ])
        self._set_decoder_layers(nn.ModuleList([OtterLayer(g, d) for g, d in zip(gated, self._get_decoder_layers())]))
        self.media_token_id = media_token_id
        self.use_media_placement_augmentation = use_media_placement_augmentation
        self.initialized_otter = True

    def forward(self, *input, **kwargs):
        """Condition the Otter layers on the media locations before forward()."""
        if not getattr(self, "initialized_otter", False):
            raise ValueError("Otter layers are not initialized. Please call `init_otter` first.")
        media_cache = kwargs.pop("media_cache", None)
        input_ids = kwargs["input_ids"] if "input_ids" in kwargs else input[0]
        media_locations = input_ids == self.media_token_id
        layers = self._get_decoder_layers()
        if media_cache is not None:
            media_cache.check_step(input_ids.shape[0], input_ids.shape[1], self.use_media_placement_augmentation)
            if media_cache.filled:
                return self._forward_media_step(media_cache, media_locations, input, kwargs)
        attend_previous = (random.random() < 0.5) if self.use_media_placement_augmentation else True
        tt = ops.text_time(media_locations, attend_previous)
        for layer in layers:
            layer.condition_media_locations(media_locations)
            layer.condition_attend_previous(attend_previous)
            layer.condition_text_time(tt)
        out = super().forward(*input, **kwargs)
        if media_cache is not None:          # the prompt pass was the ordinary forward; the cache takes the counts and the projected media
            media_cache.fill(media_locations, layers)
        return out

    def _forward_media_step(self, media_cache, media_locations, input, kwargs):
        """One cached step over a filled MediaCache (otter_amd/media_cache.py): the running <image> count is advanced on the device and is the
        text_time of every gated layer, whose blocks run `decode_step` on the cached media projections."""
        layers = self._get_decoder_layers()
        tt = media_cache.advance(kwargs["input_ids"] if "input_ids" in kwargs else input[0])
        try:
            for i, layer in enumerate(layers):
                layer.condition_media_locations(media_locations)
                layer.condition_attend_previous(True)
                layer.condition_text_time(tt.view(-1, 1))
                layer.condition_media_step((media_cache, i))
            return super().forward(*input, **kwargs)
        finally:
            for layer in layers:
                layer.condition_media_step(None)

    @torch.no_grad()
    def forward_branches(self, branch_ids, cache, media_cache, attention_mask=None):
        """Candidate rows over a cached prompt (OtterForConditionalGeneration.score_candidates): branch_ids int64 [B, C, T], the first T input
        tokens of C continuations of each prompt; `cache` the StaticKVCache and `media_cache` the MediaCache the prompt pass filled;
        attention_mask the prompt's [B, P] or None.  The decoder host runs all B*C*T tokens as one-token rows (`_forward_branches` of
        otter_amd/mpt.py and llama.py); every gated block runs its `decode_step` over a view of the media cache in which row r reads
        sentence r // (C*T) (`MediaCache.rows_view`: neither cache is changed).  Returns the final-norm hidden rows [B, C, T, D]."""
        decoder = self.get_decoder() if hasattr(self, "get_decoder") else None
        if not hasattr(decoder, "_forward_branches"):
            raise NotImplementedError("forward_branches: the decoder host %s has no branch pass (MPT and LLaMA have)" % type(self).__name__)
        B, C, T = branch_ids.shape
        layers = self._get_decoder_layers()
        view = media_cache.rows_view(C * T)
        locations = torch.zeros((B * C * T, 1), dtype=torch.bool, device=branch_ids.device)    # (no candidate row holds the media token)
        before = [(l.media_locations, l.attend_previous, l.text_time) for l in layers]
        try:
            for i, layer in enumerate(layers):
                layer.condition_media_locations(locations)
                layer.condition_attend_previous(True)
                layer.condition_text_time(view.seen.view(-1, 1))
                layer.condition_media_step((view, i))
            return decoder._forward_branches(branch_ids, cache, attention_mask)
        finally:
            for layer, (ml, ap, tt) in zip(layers, before):
                layer.condition_media_step(None)
                layer.condition_media_locations(ml)
                layer.condition_attend_previous(ap)
                layer.condition_text_time(tt)

    def is_conditioned(self) -> bool:
        return all(l.is_conditioned() for l in self._get_decoder_layers())

    def clear_conditioned_layers(self) -> None:
        for layer in self._get_decoder_layers():
            layer.condition_vis_x(None)
            layer.condition_media_locations(None)
            layer.condition_attend_previous(None)
            layer.condition_media_step(None)


# ======================================================================================================================
# model
# ======================================================================================================================


class OtterStubTokenizer:
    """Used only when the MPT tokenizer files are not available locally (no network): carries the four special-token ids
    the model needs.  For the 50432-row MPT-7B vocabulary they are the ids the real tokenizer assigns after
    `add_special_tokens` (50277..50280); for toy vocabularies they are the last four rows."""

    eos_token = "<|endoftext|>"
    pad_token = "<PAD>"

    def __init__(self, vocab_size: int):
        base = 50277 if vocab_size >= 50281 else vocab_size - 4
        self.vocab_size = vocab_size
        self.special = {"<|endofchunk|>": base, "<image>": base + 1, "<answer>": base + 2, "<PAD>": base + 3,
                        "<|endoftext|>": 0}

    def add_special_tokens(self, d):
        return 0

    def encode(self, s):
        return [self.special[s]]

    def __call__(self, s, add_special_tokens=False, **kw):
        return {"input_ids": self.encode(s)}

    def __len__(self):
        return self.vocab_size


def _load_tokenizer(name: str, vocab_size: int):
    """modeling_otter.py:750-757.  The stub is used ONLY when the tokenizer files are not on this machine (OSError from
    `local_files_only=True`: benches and tests run without network) or on explicit request (OTTER_STUB_TOKENIZER=1) -- and
    says so; any other failure (a broken tokenizers install, a corrupt file) propagates, because the stub's hard-coded
    special-token ids would silently change <image> / <|endofchunk|> (and alias real ids of a LLaMA vocabulary)."""
    import os
    import warnings

    if os.environ.get("OTTER_STUB_TOKENIZER") != "1":
        from transformers import AutoTokenizer

        try:
            tok = AutoTokenizer.from_pretrained(name, local_files_only=True)
        except OSError as e:
            warnings.warn("otter_amd: tokenizer files for %r not found locally (%s); using OtterStubTokenizer "
                          "(special-token ids only)" % (name, type(e).__name__), stacklevel=2)
        else:
            tok.add_special_tokens({"additional_special_tokens": ["<|endofchunk|>", "<image>", "<answer>"]})
            if tok.pad_token is None:
                tok.add_special_tokens({"pad_token": "<PAD>"})
            return tok
    return OtterStubTokenizer(vocab_size)


def _use_hip_rmsnorm(lang_encoder: nn.Module) -> None:
    """Config C4 (LLaMA host, third-party transformers class as in the reference): route every LlamaRMSNorm through the
    HIP RMSNorm kernel (same parameters, same state-dict keys; only `forward` is rebound)."""
    import types

    def _fwd(self, hidden_states):
        eps = getattr(self, "variance_epsilon", getattr(self, "eps", 1e-6))
        return OF.rms_norm(hidden_states, self.weight, eps)

    for mod in lang_encoder.modules():
        if mod.__class__.__name__ == "LlamaRMSNorm":
            mod.forward = types.MethodType(_fwd, mod)


class OtterPreTrainedModel(PreTrainedModel):
    config_class = OtterConfig
    base_model_prefix = "otter"
    supports_gradient_checkpointing = False
    _no_split_modules = ["OtterPerceiverBlock", "OtterLayer", "CLIPVisionModel"]

    def _init_weights(self, module):
        """Otter requires no specific initialization."""
        return


class OtterForConditionalGeneration(OtterPreTrainedModel):
    config_class = OtterConfig

    def __init__(self, config: OtterConfig):
        super().__init__(config)
        tc = config.text_config
        arch = (getattr(tc, "architectures", None) or ["MPTForCausalLM"])[0]
        if arch == "MPTForCausalLM":
            text_tokenizer = _load_tokenizer("mosaicml/mpt-7b-instruct", tc.vocab_size)
            lang_encoder = MPTForCausalLM(tc)
        elif arch == "LlamaForCausalLM":
            if os.environ.get("OTTER_HF_LLAMA") == "1":   # A/B switch: the third-party class the reference uses, HIP RMSNorm only
                from transformers import LlamaForCausalLM

                lang_encoder = LlamaForCausalLM(tc)
                _use_hip_rmsnorm(lang_encoder)
            else:
                from .llama import LlamaForCausalLM       # MI355X-native host with the same class surface and state-dict keys

                lang_encoder = LlamaForCausalLM(tc)
            text_tokenizer = _load_tokenizer(getattr(tc, "_name_or_path", "") or "llama", tc.vocab_size)
        else:
            raise NotImplementedError(arch)
        vision_encoder = CLIPVisionModel(config.vision_config)
        self.text_tokenizer = text_tokenizer
        self.eoc_token_id = text_tokenizer.encode("<|endofchunk|>")[-1]
        self.media_token_id = text_tokenizer.encode("<image>")[-1]

        extend_instance(lang_encoder, OtterLMMixin)
        lang_encoder.set_decoder_layers_attr_name(_infer_decoder_layers_attr_name(lang_encoder))
        self.lang_encoder = lang_encoder
        self.cross_attn_every_n_layers = config.cross_attn_every_n_layers
        self.use_media_placement_augmentation = False  # strictly false for Otter (modeling_otter.py:786)
        self.max_num_frames = config.max_num_frames if hasattr(config, "max_num_frames") else None
        vision_encoder.output_tokens = True
        self.vision_encoder = vision_encoder
        self.vis_dim = 1024
        self.perceiver = OtterPerceiverResampler(dim=self.vis_dim, max_num_frames=self.max_num_frames)
        self.lang_encoder.init_otter(media_token_id=self.media_token_id, vis_hidden_size=self.vis_dim,
                                     cross_attn_every_n_layers=self.cross_attn_every_n_layers,
                                     use_media_placement_augmentation=self.use_media_placement_augmentation)
        if "lora_config" in config.__dict__:
            # modeling_otter.py:808-829: low-rank adapters on the frozen decoder's Wqkv (MPT) / q_proj + v_proj (LLaMA); the wrapper
            # nesting, parameter names and class rename of peft are restated in otter_amd/lora.py (peft itself is not installed here)
            from .lora import get_lora_model

            master_print(f"Using LoRA with config:{config.lora_config}")
            self.lang_encoder = get_lora_model(self.lang_encoder, config.lora_config, arch)
            self.lang_encoder.master_print_trainable_parameters()
        self.post_init()

    @classmethod
    def from_pretrained(cls, *args, **kwargs):
        model = super().from_pretrained(*args, **kwargs)
        # transformers >= 5 builds the model on the meta device and materialises NEW Parameter objects while loading, which
        # drops the requires_grad flags set by init_weights() in __init__ (the pinned 4.35.1 loaded in place): re-apply.
        model.init_weights()
        return model

    def quantize_decoder_int8(self, gated_blocks: bool = False, lm_head: bool = False, wide_steps: bool = False) -> dict:
        """Opt-in, for generation: hold the frozen decoder's linears as int8 weights with one fp32 scale per output row
        (otter_amd/quant.py: `quantize_frozen_decoder`), put the model in eval mode and return {"replaced", "bytes_before", "bytes_after"}:
        what THIS call replaced.  `gated_blocks=True` also replaces the two FFN linears of every gated cross-attention block
        (`quantize_gated_blocks`: trainable layers, so the keyword is the statement that training is over), `lm_head=True` the un-embedding
        (`quantize_unembedding`: an int8 copy of MPT's tied table, LLaMA's `lm_head`), of which generate() then computes only the last
        position of the prompt pass.  A later call with more keywords quantises only what is still unquantised.
        `wide_steps=True` lets cached steps of 65 to `quant.PANEL_MAX_ROWS` rows (batch x beams) run the panel kernel instead of
        dequantising: it sets `panel_rows` on every Int8FrozenLinear of the model, whichever call quantised it, and
        changes nothing in the returned dict.

        This is an IN-MEMORY transformation done after loading: checkpoints stay in the reference's format.  `state_dict()` of a quantised
        model (qweight / scale buffers instead of weights) is not a reference-format checkpoint, so `save_pretrained` on it raises; the
        quantised decoder is inference-only (no autograd through it).  Calling it again replaces nothing."""
        from .quant import quantize_frozen_decoder, quantize_gated_blocks, quantize_unembedding, set_wide_steps

        parts = [quantize_frozen_decoder(self.lang_encoder)]
        if gated_blocks:
            parts.append(quantize_gated_blocks(self.lang_encoder))
        if lm_head:
            parts.append(quantize_unembedding(self.lang_encoder))
        if wide_steps:
            set_wide_steps(self)
        self.eval()
        return {k: sum(p[k] for p in parts) for k in ("replaced", "bytes_before", "bytes_after")}

    def save_pretrained(self, *args, **kwargs):
        quant = sys.modules.get(__package__ + ".quant")          # (not loaded: nothing was ever quantised)
        if quant is not None and any(isinstance(m, quant.Int8FrozenLinear) for m in self.modules()):
            raise RuntimeError("save_pretrained: the decoder of this model was quantised in memory (quantize_decoder_int8); its state_dict is "
                               "not a reference-format checkpoint.  Save the model before quantising it.")
        return super().save_pretrained(*args, **kwargs)

    # ---- accessors used by pipeline/train/instruction_following.py ----
    def get_input_embeddings(self) -> nn.Module:
        return self.lang_encoder.get_input_embeddings()

    def set_input_embeddings(self, new_embeddings):
        self.lang_encoder.set_input_embeddings(new_embeddings)

    def get_output_embeddings(self) -> nn.Module:
        return self.lang_encoder.get_output_embeddings()

    def set_output_embeddings(self, new_embeddings):
        self.lang_encoder.set_output_embeddings(new_embeddings)

    def get_image_encoder(self) -> nn.Module:
        return self.vision_encoder

    def get_lang_encoder(self) -> nn.Module:
        return self.lang_encoder

    def init_weights(self):
        """Freeze everything except gated cross-attention layers, the perceiver and the input embeddings
        (modeling_otter.py:851-915)."""
        cfg = self.config.__dict__
        if not cfg.get("train_full_model", False):
            for p in self.parameters():
                p.requires_grad = False
        if cfg.get("train_vision_encoder", False):
            for p in self.vision_encoder.parameters():
                p.requires_grad = True
        if cfg.get("train_lang_encoder", False):
            for p in self.lang_encoder.parameters():
                p.requires_grad = True
        if "lora_config" in cfg:                      # modeling_otter.py:889-894
            for name, p in self.lang_encoder.named_parameters():
                if "lora" in name:
                    p.requires_grad = True
        for name, p in self.lang_encoder.named_parameters():
            if "gated_cross_attn_layer" in name:
                p.requires_grad = True
        for name, p in self.named_parameters():
            if "perceiver" in name:
                p.requires_grad = True
        self.lang_encoder.get_input_embeddings().requires_grad_(True)
        if "LlamaForCausalLM" in self.lang_encoder.__class__.__name__:
            self.lang_encoder.lm_head.requires_grad_(True)

    def forward(self, vision_x: torch.Tensor, lang_x: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                labels: Optional[torch.Tensor] = None, use_cached_vision_x: bool = False, clear_conditioned_layers: bool = True,
                past_key_values: Optional[List[torch.FloatTensor]] = None, use_cache: bool = False,
                **kwargs) -> CausalLMOutputWithPast:
        assert (vision_x is not None) or use_cached_vision_x, "Must provide either vision_x or use_cached_vision_x to True."
        if use_cached_vision_x:
            assert vision_x is None, "Expect vision_x to be None when use_cached_vision_x is True."
            assert self.lang_encoder.is_conditioned()
        else:
            self._encode_vision_x(vision_x=vision_x)
        output = self.lang_encoder(input_ids=lang_x, attention_mask=attention_mask, labels=labels,
                                   past_key_values=past_key_values, use_cache=use_cache, **kwargs)
        if clear_conditioned_layers:
            self.lang_encoder.clear_conditioned_layers()
        return output

    def _encode_vision_x(self, vision_x: torch.Tensor):
        """(b, T_img, F, C, H, W) -> CLIP tokens (CLS dropped) -> perceiver -> condition every decoder layer."""
        assert vision_x.ndim == 6, "vision_x should be of shape (b, T_img, F, C, H, W)"
        b, T, F = vision_x.shape[:3]
        flat = vision_x.reshape((b * T * F,) + tuple(vision_x.shape[3:]))
        with torch.no_grad() if not any(p.requires_grad for p in self.vision_encoder.parameters()) else _nullctx():
            feats = self.vision_encoder(flat)[0][:, 1:, :]
        feats = feats.reshape(b, T, F, feats.shape[1], feats.shape[2])
        vis = self.perceiver(feats)
        for layer in self.lang_encoder._get_decoder_layers():
            layer.condition_vis_x(vis)

    @torch.no_grad()
    def generate(self, vision_x: torch.Tensor, lang_x: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                 **generate_kwargs):
        """The reference's call contract (modeling_otter.py:999-1042): encode the vision input once (every beam of a sample is
        conditioned on that sample's media, the reference's `vision_x.repeat_interleave(num_beams)`), decode with
        eos_token_id = <|endofchunk|> unless the caller overrides it, clear the conditioning, return lang_x with the new tokens
        appended.  The decoding itself -- greedy, beam search with `no_repeat_ngram_size` / `bad_words_ids` /
        `length_penalty` / `min_new_tokens`, temperature / top-k / top-p sampling: what the reference's demos, benchmark
        wrappers and serving code pass -- is otter_amd/generation.py (the pinned transformers' algorithm, restated).
        `use_cache` selects between the two decode modes of SURVEY.md section 3.2 (default: the LM config's use_cache, False
        for OTTER-MPT7B).  `cache_implementation="static"` (implies use_cache) keeps the keys and values in one preallocated
        StaticKVCache (otter_amd/kv_cache.py): a step appends in place and beam search reorders an int32 table instead of the cache;
        None or "dynamic" is the growing tuple cache.  `kv_cache_dtype="int8"` (needs cache_implementation="static") stores that cache as
        int8 codes with one fp32 scale per cached vector, 0.516 of the bytes (kv_cache.py: an opt-in, lossy format, like the int8 decoder;
        csrc/decode_cache_i8.hip quantises as it appends and dequantises as it attends).  `cross_attention_cache=True` (needs a cached mode) makes every cached step return
        what the last position of the full re-forward returns: a MediaCache (otter_amd/media_cache.py) carries each row's <image> count and
        the projected media, so the step attends to the image instead of reproducing the reference's zero; without it every path is
        unchanged.  `graph_decode=True` (needs cache_implementation="static" AND cross_attention_cache=True) captures one cached step
        into a graph after a short warm-up and replays it for every further step (otter_amd/graph_decode.py); the tokens are those of
        the same call without it.  Both are needed because a captured step must be one chain of launches at fixed addresses: only the
        static cache keeps keys and values in place, and the legacy cached gated block forks a side stream and re-projects the media
        every step -- a graph of it would have parallel branches -- while the MediaCache step is a single chain."""
        from .generation import generate_tokens, resolve_max_length
        from .graph_decode import GraphDecodeStep
        from .kv_cache import StaticKVCache, cache_geometry
        from .media_cache import MediaCache

        num_beams = int(generate_kwargs.get("num_beams", 1) or 1)
        use_cache = bool(generate_kwargs.pop("use_cache", getattr(self.lang_encoder.config, "use_cache", False)))
        cache_impl = generate_kwargs.pop("cache_implementation", None)
        if cache_impl not in (None, "dynamic", "static"):
            raise ValueError("generate: cache_implementation must be None, 'dynamic' or 'static', got %r" % (cache_impl,))
        static = cache_impl == "static"
        use_cache = use_cache or static
        kv_cache_dtype = generate_kwargs.pop("kv_cache_dtype", None)
        if kv_cache_dtype not in (None, "int8"):
            raise ValueError("generate: kv_cache_dtype must be None or 'int8', got %r" % (kv_cache_dtype,))
        if kv_cache_dtype is not None and not static:
            raise ValueError("generate: kv_cache_dtype='int8' needs cache_implementation='static'")
        media = [None]                                       # the MediaCache of this call, created beside the KV cache
        want_media = bool(generate_kwargs.pop("cross_attention_cache", False))
        graph_decode = bool(generate_kwargs.pop("graph_decode", False))
        if graph_decode and not (static and want_media):
            raise ValueError("generate: graph_decode=True needs cache_implementation='static' and cross_attention_cache=True")
        if want_media:
            if not use_cache:
                raise ValueError("generate: cross_attention_cache=True needs use_cache=True or cache_implementation='static'")
            media[0] = False                                 # (wanted, not created yet)
        share = bool(generate_kwargs.pop("share_prompt", False))
        if share and not (static and num_beams > 1):
            raise ValueError("generate: share_prompt=True needs cache_implementation='static' and num_beams > 1")
        graph_step = [None]                                  # the GraphDecodeStep of this call, created after the prompt pass
        generate_kwargs.setdefault("eos_token_id", self.eoc_token_id)
        self._encode_vision_x(vision_x=vision_x)
        lm = self.lang_encoder
        # an int8 un-embedding (quantize_decoder_int8(lm_head=True)): only the last position of a pass is un-embedded -- every caller below
        # reads logits[:, -1] -- through the private keyword of otter_amd's own hosts
        quant = sys.modules.get(__package__ + ".quant")
        lkw = ({"_last_position_only": True} if quant is not None and getattr(lm, "accepts_last_position_only", False)
               and any(isinstance(m, quant.Int8Unembedding) for m in lm.modules()) else {})

        def repeat_vis_x():
            for layer in lm._get_decoder_layers():
                if layer.vis_x is not None:
                    layer.condition_vis_x(layer.vis_x.repeat_interleave(num_beams, dim=0))

        if num_beams > 1 and not share:   # perceiver output repeated per beam: same conditioning as encoding the repeated frames, 1/num_beams the work
            repeat_vis_x()

        def new_static_cache(ids):
            n_layers, n_kv, head_dim, host_max = cache_geometry(lm.config)
            max_len = min(resolve_max_length(lang_x.shape[1], generate_kwargs.get("max_new_tokens"), generate_kwargs.get("max_length")), host_max)
            emb = lm.get_input_embeddings().weight
            return StaticKVCache(n_layers, ids.shape[0], n_kv, head_dim, max(max_len, ids.shape[1] + 1), emb.device, OF.compute_dtype_for(emb),
                                 kv_dtype=kv_cache_dtype)

        def media_kw(ids, past, beam_idx):
            if media[0] is None:
                return {}
            if past is None and share:                   # the prompt pass has one row per sentence; `expand` follows it
                media[0] = MediaCache(ids.shape[0] // num_beams, self.media_token_id, rows_per_media=1)
            elif past is None:
                media[0] = MediaCache(ids.shape[0], self.media_token_id, rows_per_media=num_beams)
            elif beam_idx is not None:
                media[0].reorder(beam_idx)
            return {"media_cache": media[0]}

        def shared_prompt_pass(ids, mask, mkw):
            """share_prompt=True: generate_tokens has repeated the prompt per beam; the pass runs the sentences' first rows only, the gated
            layers conditioned on the un-repeated perceiver output, and fills the leaders' rows of a cache of sentences x beams rows
            (StaticKVCache.share_prompt).  Every beam then starts from its sentence's logits."""
            past = new_static_cache(ids)
            past.share_prompt(num_beams)
            out = lm(input_ids=ids[::num_beams].contiguous(), attention_mask=mask[::num_beams].contiguous() if mask is not None else None,
                     past_key_values=past, use_cache=True, **mkw, **lkw)
            if media[0] is not None:
                media[0].expand(num_beams)                   # (before enable_replay and the GraphDecodeStep: `seen` is replaced)
            repeat_vis_x()                                   # the legacy cached gated block still reads vis_x per row
            return out.logits[:, -1, :].repeat_interleave(num_beams, dim=0), past

        def step(ids, mask, past, beam_idx):
            mkw = media_kw(ids, past, beam_idx)
            if static:
                if past is None and share:
                    return shared_prompt_pass(ids, mask, mkw)
                if past is None:                             # rows = sentences x beams: generate_tokens has repeated the prompt already
                    return_ids, past = ids, new_static_cache(ids)
                else:
                    if beam_idx is not None:
                        past.reorder(beam_idx)               # the table moves, the cache does not
                    return_ids = ids[:, -1:]
                if graph_decode and past.length > 0:         # every cached step: replay mode, one graph replay after the warm-up
                    if graph_step[0] is None:
                        past.enable_replay(mask[:, :past.length] if mask is not None else None, beams=num_beams > 1)
                        graph_step[0] = GraphDecodeStep(lm, past, media[0])
                    return graph_step[0](return_ids), past
                out = lm(input_ids=return_ids, attention_mask=mask, past_key_values=past, use_cache=True, **mkw, **lkw)
                return out.logits[:, -1, :], past
            if use_cache and past is not None:
                if beam_idx is not None:
                    past = [tuple(t.index_select(0, beam_idx) for t in layer) for layer in past]   # a list: the MPT host fills it in place
                out = lm(input_ids=ids[:, -1:], attention_mask=mask, past_key_values=past, use_cache=True, **mkw, **lkw)
            else:
                out = lm(input_ids=ids, attention_mask=mask, use_cache=use_cache, **mkw, **lkw)
            return out.logits[:, -1, :], (out.past_key_values if use_cache else None)

        try:
            return generate_tokens(step, lang_x, attention_mask, **generate_kwargs)
        finally:
            if graph_step[0] is not None:
                graph_step[0].release()
            self.lang_encoder.clear_conditioned_layers()


    @torch.no_grad()
    def score_candidates(self, vision_x: torch.Tensor, lang_x: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, *, candidates,
                         candidate_mask=None, max_rows: int = 1024, return_token_logprobs: bool = False):
        """Rank classification over a cached prompt (the reference's pipeline/benchmarks/public_datasets_suite/evaluate.py:1049-1176: encode
        image and prompt once, teacher-force every class name over the cached prompt, rank by the product of the token probabilities).
        `candidates`: int64 [C, T] (the same list for every sentence) or [B, C, T], right-padded, T <= 64; `candidate_mask`: bool of the same
        shape, True on real tokens (default: all real).  Returns fp32 [B, C]: the sum over a candidate's real tokens of
        log P(token | image, prompt, earlier tokens) -- the log of the reference's `class_prob`; with `return_token_logprobs=True` also the
        terms, [B, C, T] (0 on padding).

        One prompt pass of B rows fills a fresh StaticKVCache and MediaCache (the path of `generate(cache_implementation="static",
        cross_attention_cache=True)`); its last-position logits give every candidate's first token.  Tokens 1..T-1 come from branch passes
        (`forward_branches`): all positions of all candidates of a chunk go through the decoder at once as one-token rows that read the
        shared prompt in place -- `StaticKVCache.attend_branches`, csrc/flash.hip + csrc/branch_attn.hip on the GPU in bf16.  The rows are
        un-embedded by the host's own head (its int8 form included) and the token log-probabilities picked by csrc/loss.hip's forward.
        Candidates are chunked so that a pass has at most `max_rows` rows (never less than one candidate per sentence); a chunk is as long
        as its longest candidate.  `max_rows` bounds the memory of a pass (rows x vocabulary logits above all); 1024 is not a tuned figure.
        T == 1 runs no branch pass.  The conditioning is cleared on the way out, also after an exception.

        ValueError: a candidate that holds the media token (it would change the image count of the rows after it), T > 64, a candidate
        without a real token, a mask that is not right-padded, shapes that do not fit."""
        from .kv_cache import StaticKVCache, cache_geometry
        from .media_cache import MediaCache

        lm = self.lang_encoder
        if not hasattr(lm, "_unembed") or not hasattr(lm, "forward_branches"):
            raise NotImplementedError("score_candidates: the MPT and LLaMA decoder hosts only")
        if lang_x.dim() != 2:
            raise ValueError("score_candidates: lang_x must be [B, P], got %s" % (tuple(lang_x.shape),))
        B, P = lang_x.shape
        cand = torch.as_tensor(candidates)
        if cand.dtype != torch.int64 or cand.dim() not in (2, 3):
            raise ValueError("score_candidates: candidates must be int64 [C, T] or [B, C, T], got %s %s" % (cand.dtype, tuple(cand.shape)))
        cmask = torch.ones_like(cand, dtype=torch.bool) if candidate_mask is None else torch.as_tensor(candidate_mask)
        if cmask.dtype != torch.bool or tuple(cmask.shape) != tuple(cand.shape):
            raise ValueError("score_candidates: candidate_mask must be bool of the candidates' shape %s, got %s %s"
                             % (tuple(cand.shape), cmask.dtype, tuple(cmask.shape)))
        if cand.dim() == 2:
            cand, cmask = cand.unsqueeze(0).expand(B, -1, -1), cmask.unsqueeze(0).expand(B, -1, -1)
        if cand.shape[0] != B or cand.shape[1] < 1 or cand.shape[2] < 1:
            raise ValueError("score_candidates: candidates %s for %d sentences: [C, T] or [%d, C, T] with C, T >= 1" % (tuple(cand.shape), B, B))
        C, T = cand.shape[1:]
        if T > 64:
            raise ValueError("score_candidates: T=%d: a candidate has at most 64 tokens" % T)
        if attention_mask is not None and tuple(attention_mask.shape) != (B, P):
            raise ValueError("score_candidates: attention_mask must be [%d, %d], got %s" % (B, P, tuple(attention_mask.shape)))
        max_rows = int(max_rows)
        if max_rows < 1:
            raise ValueError("score_candidates: max_rows >= 1 (got %d)" % max_rows)
        cand, cmask = cand.to(lang_x.device), cmask.to(lang_x.device)
        lengths = cmask.sum(dim=-1)                                               # [B, C]
        if bool((lengths == 0).any()):
            raise ValueError("score_candidates: a candidate without a real token")
        if bool((cmask[..., 1:] & ~cmask[..., :-1]).any()):
            raise ValueError("score_candidates: candidate_mask must be right-padded (real tokens first)")
        vocab = self.lang_encoder.get_input_embeddings().weight.shape[0]
        if bool((cmask & ((cand < 0) | (cand >= vocab))).any()):
            raise ValueError("score_candidates: a candidate token outside the vocabulary [0, %d)" % vocab)
        if bool((cmask & (cand == self.media_token_id)).any()):
            raise ValueError("score_candidates: a candidate holds the media token %d: it would change the image count of the rows after it"
                             % self.media_token_id)
        n_layers, n_kv, head_dim, host_max = cache_geometry(lm.config)
        if P + T > host_max:
            raise ValueError("score_candidates: prompt %d + candidate %d tokens exceed the host's %d positions" % (P, T, host_max))
        ids = torch.where(cmask, cand, torch.zeros_like(cand))                    # (a padded slot feeds token 0; nothing real reads it)
        labels = torch.where(cmask, cand, torch.full_like(cand, -100))
        lengths = lengths.cpu()
        self._encode_vision_x(vision_x=vision_x)
        try:
            emb = lm.get_input_embeddings().weight
            cache = StaticKVCache(n_layers, B, n_kv, head_dim, max(P + 1, 2), emb.device, OF.compute_dtype_for(emb))
            media = MediaCache(B, self.media_token_id, rows_per_media=1)
            lkw = {"_last_position_only": True} if getattr(lm, "accepts_last_position_only", False) else {}
            out = lm(input_ids=lang_x, attention_mask=attention_mask, past_key_values=cache, use_cache=True, media_cache=media, **lkw)
            tok = torch.zeros((B, C, T), dtype=torch.float32, device=lang_x.device)
            tok[:, :, 0] = OF.token_logprobs(out.logits[:, -1, :], labels[:, :, 0])
            step = max(1, max_rows // (B * max(T - 1, 1)))
            for c0 in range(0, C, step):
                c1 = min(c0 + step, C)
                Tc = int(lengths[:, c0:c1].max())
                if Tc < 2:
                    continue
                h = lm.forward_branches(ids[:, c0:c1, :Tc - 1].contiguous(), cache, media, attention_mask)      # [B, Cc, Tc-1, D]
                N = B * (c1 - c0) * (Tc - 1)
                logits = lm._unembed(h.reshape(N, 1, h.shape[-1])).view(N, -1)
                tok[:, c0:c1, 1:Tc] = OF.token_logprobs(logits, labels[:, c0:c1, 1:Tc].reshape(N, 1)).view(B, c1 - c0, Tc - 1)
        finally:
            lm.clear_conditioned_layers()
        scores = tok.sum(dim=-1)
        return (scores, tok) if return_token_logprobs else scores


class _nullctx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


# the reference exposes the same architecture under these names as well (flamingo/modeling_flamingo.py:696; otter/:539)
OtterModel = OtterForConditionalGeneration
FlamingoForConditionalGeneration = OtterForConditionalGeneration
