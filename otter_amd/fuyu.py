"""OtterHD / Fuyu-8B path (BASELINE config C5), MI355X-native.

Reference: src/otter_ai/models/fuyu/modeling_fuyu.py (FuyuForCausalLM: word embeddings + `vision_embed_tokens` linear patch
projection scattered into the sequence, `gather_continuous_embeddings` :44-77, forward :79-143) over
fuyu/modeling_persimmon.py (the decoder with flash-attn's fused ops: fused_layer_norm :286-287,360,374, fused rotary
:303-304, flash_attn_func :310, fused sq-relu MLP :180-194).  No vision tower, no gated cross-attention: a decoder whose
first ~1300 positions are linear projections of 30x30x3 image patches, fully fine-tuned.

Same class surface and state-dict keys as the reference / transformers (`language_model.model.layers.{i}.self_attn.
{query_key_value,dense,q_layernorm,k_layernorm}`, `.mlp.{dense_h_to_4h,dense_4h_to_h}`, `.input_layernorm`,
`.post_attention_layernorm`, `language_model.model.{embed_tokens,final_layernorm}`, `language_model.lm_head`,
`vision_embed_tokens`), taking transformers' `FuyuConfig` / `PersimmonConfig`.

bf16 GPU path (every parameter is trainable here, so the GEMMs are torch / hipBLASLt with their wgrad):
  LayerNorm (+ fused residual add)       csrc/norm.hip
  q / k LayerNorm over head_dim + partial RoPE   csrc/fuyu.hip: otter_qk_norm_rope_fwd / _bwd, reading the per-head interleaved
                                         [H,3,d] projection buffer in place, writing compact [B,S,H,64] q / k
  causal attention                       csrc/flash.hip, head_dim 64 (round 3): two heads per workgroup on the 128-wide tile layouts,
                                         v read in place from the projection buffer, ctx written as [B,S,H*64], dv written into the
                                         v slots of dqkv.  (Round 2 zero-padded the heads to 128 columns: twice the attention FLOPs
                                         and padded q / k / v / dO / o copies; still used for an odd head count, OTTER_FUYU_PAD128=1.)
  squared-ReLU                           csrc/fuyu.hip: otter_sqrelu_fwd / _bwd
  patch embeddings into the sequence     csrc/fuyu.hip: otter_scatter_rows (+ gather for the backward)
  cached decode step (S = 1, no grad)    csrc/persimmon_decode.hip: otter_persimmon_decode_attn -- q/k LayerNorm + rotary of the new token,
                                         the cache append (one read of the past, one write of the new cache) and the single-query
                                         attention in one pass; OTTER_FUYU_HIP_DECODE=0 keeps the plain path (A/B switch)
  the same step over a StaticKVCache     csrc/persimmon_decode_cache.hip: otter_persimmon_decode_attn_cached (/ _dyn in replay mode) -- the
  (`generate(past_key_values=cache)`)    same arithmetic, the new key / value written in place at the row's own slot, the past never
                                         moved, beams through the cache's int32 table; with `graph_decode=True` one captured step is
                                         replayed (otter_amd/graph_decode.py).  OTTER_FUYU_HIP_DECODE=0: the plain-torch restatement
fp32 / CPU: the plain PyTorch expression of the same arithmetic (parity mode; pinned by tests/golden/fuyu_tiny.npz, generated
by the reference's own FuyuForCausalLM)."""
from __future__ import annotations

import math
import os
import sys
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from transformers import FuyuConfig, PersimmonConfig, PreTrainedModel
from transformers.modeling_outputs import BaseModelOutputWithPast, CausalLMOutputWithPast

from . import functional as OF
from . import ops
from .kv_cache import StaticKVCache, cache_geometry


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def _cfg_get(cfg, name, default=None):
    v = getattr(cfg, name, None)
    if v is None:
        rp = getattr(cfg, "rope_parameters", None) or {}
        v = rp.get(name, None)
    return default if v is None else v


def _is_int8(m) -> bool:
    """isinstance(m, quant.Int8FrozenLinear) without importing otter_amd.quant: a model that was never quantised never loads that module."""
    q = sys.modules.get(__package__ + ".quant")
    return q is not None and isinstance(m, q.Int8FrozenLinear)


def _linear(mod, x):
    """A decoder linear: the quantised module itself (otter_amd/quant.py: no `weight` to read), else OF.trainable_linear as ever."""
    return mod(x) if _is_int8(mod) else OF.trainable_linear(mod, x)


def _refuse_save_if_int8(model):
    quant = sys.modules.get(__package__ + ".quant")          # (not loaded: nothing was ever quantised)
    if quant is not None and any(isinstance(m, quant.Int8FrozenLinear) for m in model.modules()):
        raise RuntimeError("save_pretrained: the decoder of this model was quantised in memory (quantize_decoder_int8); its state_dict is "
                           "not a reference-format checkpoint.  Save the model before quantising it.")


def _check_static_cache_kind(cache, who: str) -> None:
    if cache.int8:
        raise NotImplementedError("%s: an int8 StaticKVCache (kv_dtype='int8') is not built for the Persimmon host (head_dim 64)" % who)


def _same_device(a, b) -> bool:
    a, b = torch.device(a), torch.device(b)
    if a.type != b.type:
        return False
    return a.type != "cuda" or (torch.cuda.current_device() if a.index is None else a.index) == (torch.cuda.current_device() if b.index is None
                                                                                                  else b.index)


def _pop_static_cache(who: str, generate_kwargs: dict, config, emb, rows: int, prompt_len: int):
    """`generate(..., past_key_values=cache)`: pop and check a caller's StaticKVCache (None when none was given; anything else stays in
    the arguments and is refused as ever).  `config`: the Persimmon config; `rows` = batch x beams."""
    from .generation import resolve_max_length

    cache = generate_kwargs.get("past_key_values")
    if not isinstance(cache, StaticKVCache):
        return None
    del generate_kwargs["past_key_values"]
    _check_static_cache_kind(cache, who)
    if cache.length != 0:
        raise ValueError("%s: the StaticKVCache holds %d positions; pass an empty one (cache.reset())" % (who, cache.length))
    cd = OF.compute_dtype_for(emb)
    if not _same_device(cache.device, emb.device) or cache.dtype != cd:
        raise ValueError("%s: the StaticKVCache is on %s in %s, the model computes on %s in %s" % (who, cache.device, cache.dtype, emb.device, cd))
    n_layers, n_kv, head_dim, host_max = cache_geometry(config)
    if (cache.n_layers, cache.n_heads, cache.head_dim) != (n_layers, n_kv, head_dim):
        raise ValueError("%s: the StaticKVCache has %d layers of %d heads x %d, the model %d of %d x %d (StaticKVCache.for_model)"
                         % (who, cache.n_layers, cache.n_heads, cache.head_dim, n_layers, n_kv, head_dim))
    if cache.rows != rows:
        raise ValueError("%s: the StaticKVCache has %d rows, this call needs batch x num_beams = %d" % (who, cache.rows, rows))
    need = min(resolve_max_length(prompt_len, generate_kwargs.get("max_new_tokens"), generate_kwargs.get("max_length")), host_max)
    if cache.max_len < need:
        raise ValueError("%s: the StaticKVCache holds at most %d positions, this call can reach %d" % (who, cache.max_len, need))
    return cache


def _static_cache_step(model, lm, cache, num_beams: int, graph_decode: bool, graph_step: list, prompt_kw: dict, kw: dict):
    """The step closure of `generate(past_key_values=cache)` (OtterForConditionalGeneration.generate's static branch): the prompt pass goes
    through `model` with `prompt_kw` (the image patches) and fills the cache; on a beam step the cache's table is reordered, not the
    cache; later steps feed the last token.  `graph_decode`: after the prompt pass the cache enters replay mode and the steps go through
    one GraphDecodeStep (kept in `graph_step[0]` for the caller's `finally`)."""
    from .graph_decode import GraphDecodeStep

    def cached(ids):
        return model(input_ids=ids, past_key_values=cache, use_cache=True, **kw).logits[:, -1, :]

    def step(ids, mask, past, beam_idx):
        if past is None:                                # rows = sentences x beams: generate_tokens has repeated the prompt already
            out = model(input_ids=ids, attention_mask=mask, past_key_values=cache, use_cache=True, **prompt_kw, **kw)
            return out.logits[:, -1, :], cache
        if beam_idx is not None:
            cache.reorder(beam_idx)                     # the table moves, the cache does not
        if graph_decode:
            if graph_step[0] is None:
                cache.enable_replay(mask[:, :cache.length] if mask is not None else None, beams=num_beams > 1)
                graph_step[0] = GraphDecodeStep(lm, cache, None, step_fn=cached, kernel_head_dim=64)
            return graph_step[0](ids[:, -1:]), cache
        out = model(input_ids=ids[:, -1:], attention_mask=mask, past_key_values=cache, use_cache=True, **kw)
        return out.logits[:, -1, :], cache

    return step


class PersimmonMLP(nn.Module):
    def __init__(self, config: PersimmonConfig):
        super().__init__()
        if getattr(config, "hidden_act", "relu2") != "relu2":
            raise NotImplementedError("Persimmon host: hidden_act must be relu2 (squared ReLU)")
        self.dense_h_to_4h = nn.Linear(config.hidden_size, config.intermediate_size)
        self.dense_4h_to_h = nn.Linear(config.intermediate_size, config.hidden_size)

    def forward(self, x):
        up, dn = self.dense_h_to_4h, self.dense_4h_to_h
        if _is_int8(up) or _is_int8(dn):        # int8 decoder (otter_amd/quant.py): relu(h)^2 in the first product's epilogue
            h = up(x, act="relu2") if _is_int8(up) else torch.square(F.relu(OF.trainable_linear(up, x)))
            return _linear(dn, h)
        # relu(h)^2 and the second Linear in one autograd node: the activation's backward rides in the input-gradient GEMM's tail
        return OF.sqrelu_linear(self.dense_4h_to_h, OF.trainable_linear(self.dense_h_to_4h, x))


class PersimmonAttention(nn.Module):
    def __init__(self, config: PersimmonConfig):
        super().__init__()
        self.hidden = config.hidden_size
        self.n_heads = config.num_attention_heads
        self.head_dim = self.hidden // self.n_heads
        if self.head_dim * self.n_heads != self.hidden:
            raise ValueError("hidden_size must be divisible by num_heads")
        if getattr(config, "attention_dropout", 0.0):
            raise NotImplementedError("Persimmon host: attention_dropout != 0 is not implemented")
        rs = getattr(config, "rope_scaling", None)
        if rs and rs.get("rope_type", rs.get("type", "default")) not in ("default", None):
            raise NotImplementedError("Persimmon host: rope scaling is not implemented (Fuyu-8B uses none)")
        self.rot = int(float(_cfg_get(config, "partial_rotary_factor", 0.5)) * self.head_dim)
        self.theta = float(_cfg_get(config, "rope_theta", 25000.0))
        self.query_key_value = nn.Linear(self.hidden, 3 * self.hidden, bias=True)
        self.dense = nn.Linear(self.hidden, self.hidden, bias=True)
        self.qk_layernorm = bool(getattr(config, "qk_layernorm", True))
        if self.qk_layernorm:
            self.q_layernorm = nn.LayerNorm(self.head_dim, eps=config.layer_norm_eps, elementwise_affine=True)
            self.k_layernorm = nn.LayerNorm(self.head_dim, eps=config.layer_norm_eps, elementwise_affine=True)
        self.scale = 1.0 / math.sqrt(self.head_dim)

    def hip_ok(self, x, s_past, default_pos) -> bool:
        return (x.is_cuda and OF.compute_dtype_for(x) == torch.bfloat16 and self.head_dim == 64 and self.qk_layernorm and self.rot % 16 == 0
                and 0 < self.rot <= 64 and s_past == 0 and default_pos and os.environ.get("OTTER_NO_FLASH") != "1")

    def _ln_f32(self):
        """fp32 contiguous (gamma_q, beta_q, gamma_k, beta_k) for the decode kernel, refreshed when a parameter changes."""
        ps = (self.q_layernorm.weight, self.q_layernorm.bias, self.k_layernorm.weight, self.k_layernorm.bias)
        key = tuple((p.data_ptr(), p._version, p.dtype) for p in ps)
        c = getattr(self, "_ln32", None)
        if c is None or c[0] != key:
            c = (key, tuple(p.detach().float().contiguous() for p in ps))
            self._ln32 = c
        return c[1]

    def decode_step(self, x, cos_row, sin_row, past_key_value, key_valid, use_cache):
        """Cached decode step on HIP (x [B,1,D] bf16, no autograd): the projection, then q/k LayerNorm + rotary at position S_past, the
        cache append and the single-query attention in one kernel (csrc/persimmon_decode.hip), then `dense`.  The past is read, never
        written: the new cache is a fresh [B,H,S_past+1,64] pair, as the plain path's torch.cat makes it."""
        B = x.shape[0]
        qkv = _linear(self.query_key_value, x)                      # [B,1,H*3*64]
        gq, bq, gk, bk = self._ln_f32()
        o, k, v = ops.persimmon_decode_attn(qkv.view(B, self.n_heads, 3, 64), gq, bq, gk, bk, cos_row, sin_row, past_key_value[0],
                                            past_key_value[1], key_valid, self.rot, self.q_layernorm.eps, self.scale)
        return _linear(self.dense, o.view(B, 1, self.hidden)), ((k, v) if use_cache else None)

    def static_step(self, x, cos, sin, cache, layer: int, key_valid, reference: bool = False):
        """Cached decode step over a StaticKVCache (x [B,1,D], no autograd): the projection, then `cache.attend_persimmon` -- q/k LayerNorm +
        rotary at the cache's position, the in-place append and the single-query attention, on csrc/persimmon_decode_cache.hip where the
        cache's kernel conditions hold, the plain-torch restatement elsewhere (and with `reference`) -- then `dense`.  cos / sin: the rows of
        the position, or in replay mode the whole tables."""
        B = x.shape[0]
        qkv = _linear(self.query_key_value, x).view(B, self.n_heads, 3, self.head_dim)
        if not self.qk_layernorm:
            ln, reference = (None, None, None, None), True          # (the kernel fuses the LayerNorm: without one, the restatement)
        elif qkv.is_cuda and qkv.dtype == torch.bfloat16:
            ln = self._ln_f32()
        else:
            ln = (self.q_layernorm.weight, self.q_layernorm.bias, self.k_layernorm.weight, self.k_layernorm.bias)
        fn = cache.attend_persimmon_reference if reference else cache.attend_persimmon
        eps = self.q_layernorm.eps if self.qk_layernorm else 0.0
        o = fn(layer, qkv, ln[0], ln[1], ln[2], ln[3], cos, sin, self.rot, eps, self.scale, key_valid=key_valid)
        return _linear(self.dense, o.view(B, 1, self.hidden))

    def forward(self, x, cos, sin, attn_mask=None, past_key_value=None, use_cache=False, hip=False, key_valid=None):
        B, S, _ = x.shape
        H, d = self.n_heads, self.head_dim
        qkv = _linear(self.query_key_value, x)                      # [B,S,H*3*d], per head (q | k | v)
        if hip:
            kw = {} if key_valid is None else {"key_valid": key_valid}
            if use_cache:
                ctx, k, v = OF.persimmon_attention(qkv, self.q_layernorm, self.k_layernorm, cos, sin, H, self.rot, self.scale, want_kv=True, **kw)
                return _linear(self.dense, ctx), (k, v)
            ctx = OF.persimmon_attention(qkv, self.q_layernorm, self.k_layernorm, cos, sin, H, self.rot, self.scale, **kw)
            return _linear(self.dense, ctx), None
        q5 = qkv.view(B, S, H, 3, d)
        q, k, v = q5[..., 0, :], q5[..., 1, :], q5[..., 2, :]
        if self.qk_layernorm:
            q = self.q_layernorm(q)
            k = self.k_layernorm(k)
        q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)       # [B,H,S,d]
        c, s_ = (cos[:, None], sin[:, None]) if cos.dim() == 3 else (cos[None, None], sin[None, None])
        c, s_ = c.to(q.dtype), s_.to(q.dtype)
        r = self.rot
        q = torch.cat((q[..., :r] * c + _rotate_half(q[..., :r]) * s_, q[..., r:]), dim=-1)
        k = torch.cat((k[..., :r] * c + _rotate_half(k[..., :r]) * s_, k[..., r:]), dim=-1)
        if past_key_value is not None and len(past_key_value) == 2:
            k = torch.cat([past_key_value[0], k], dim=2)
            v = torch.cat([past_key_value[1], v], dim=2)
        new_past = (k, v) if use_cache else None
        ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask, dropout_p=0.0, is_causal=False, scale=self.scale)
        return self.dense(ctx.transpose(1, 2).reshape(B, S, H * d)), new_past


class PersimmonDecoderLayer(nn.Module):
    """modeling_persimmon.py:322-392 (pre-LN block, dropout 0)."""

    def __init__(self, config: PersimmonConfig):
        super().__init__()
        if getattr(config, "hidden_dropout", 0.0):
            raise NotImplementedError("Persimmon host: hidden_dropout != 0 is not implemented")
        self.self_attn = PersimmonAttention(config)
        self.mlp = PersimmonMLP(config)
        self.input_layernorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.post_attention_layernorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)

    def forward(self, x, cos, sin, attn_mask=None, past_key_value=None, use_cache=False, hip=False, pending=None, defer=False, key_valid=None,
                decode=None, static=None):
        """hip path: `pending` is the previous layer's MLP output, not yet added to the residual stream -- the add rides in this layer's
        first LayerNorm pass; with `defer` the layer hands its own MLP output back the same way ((x, past, mlp_out) instead of (x, past)).
        `key_valid`: uint8 [B,S] key-padding mask of a left-padded prompt (inference only); `decode` = (cos_row, sin_row): the cached
        one-token step on csrc/persimmon_decode.hip against `past_key_value` (key_valid then [B,S_past+1]).  `static` = (cache, layer index,
        reference): the one-token step over a StaticKVCache (`PersimmonAttention.static_step`), on either path; cos / sin as it takes them."""
        if hip:
            n1, n2 = self.input_layernorm, self.post_attention_layernorm
            if pending is not None:
                x, a = OF.add_layer_norm(x, pending, n1.weight, n1.bias, n1.eps, torch.bfloat16)   # x = x + pending ; a = LN(x)  (one pass)
            else:
                a = OF.layer_norm(x, n1.weight, n1.bias, n1.eps, torch.bfloat16)
            if static is not None:
                b, new_past = self.self_attn.static_step(a, cos, sin, static[0], static[1], key_valid, static[2]), None
            elif decode is not None:
                b, new_past = self.self_attn.decode_step(a, decode[0], decode[1], past_key_value, key_valid, use_cache)
            else:
                b, new_past = self.self_attn(a, cos, sin, use_cache=use_cache, hip=True, key_valid=key_valid)
            x, m = OF.add_layer_norm(x, b, n2.weight, n2.bias, n2.eps, torch.bfloat16)   # x = x + b ; m = LN(x)  (one pass)
            if defer:
                return x, new_past, self.mlp(m)
            return x + self.mlp(m), new_past
        if static is not None:
            b, new_past = self.self_attn.static_step(self.input_layernorm(x), cos, sin, static[0], static[1], key_valid, static[2]), None
        else:
            b, new_past = self.self_attn(self.input_layernorm(x), cos, sin, attn_mask=attn_mask, past_key_value=past_key_value, use_cache=use_cache)
        x = x + b
        return x + self.mlp(self.post_attention_layernorm(x)), new_past


class PersimmonPreTrainedModel(PreTrainedModel):
    config_class = PersimmonConfig
    base_model_prefix = "model"
    _no_split_modules = ["PersimmonDecoderLayer"]
    _supports_sdpa = True
    _supports_flash_attn = False
    _supports_flex_attn = False

    def _init_weights(self, module):
        std = getattr(self.config, "initializer_range", 0.02)
        if isinstance(module, nn.Linear):
            nn.init.normal_(module.weight, 0.0, std)
            if module.bias is not None:
                nn.init.zeros_(module.bias)
        elif isinstance(module, nn.Embedding):
            nn.init.normal_(module.weight, 0.0, std)
        elif isinstance(module, nn.LayerNorm):
            nn.init.ones_(module.weight)
            nn.init.zeros_(module.bias)


class PersimmonModel(PersimmonPreTrainedModel):
    def __init__(self, config: PersimmonConfig):
        super().__init__(config)
        self.embed_tokens = nn.Embedding(config.vocab_size, config.hidden_size, getattr(config, "pad_token_id", None))
        self.layers = nn.ModuleList([PersimmonDecoderLayer(config) for _ in range(config.num_hidden_layers)])
        self.final_layernorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self._tab = None
        self.post_init()

    def get_input_embeddings(self):
        return self.embed_tokens

    def set_input_embeddings(self, value):
        self.embed_tokens = value

    def _tables(self, n, device):
        att = self.layers[0].self_attn
        if self._tab is None or self._tab[0].device != device or self._tab[0].shape[0] < n:
            na = max(n, 512)
            inv = 1.0 / (att.theta ** (torch.arange(0, att.rot, 2, dtype=torch.float32, device=device) / att.rot))
            fr = torch.arange(na, dtype=torch.float32, device=device)[:, None] * inv[None, :]
            emb = torch.cat((fr, fr), dim=-1)
            self._tab = (emb.cos().contiguous(), emb.sin().contiguous())
        return self._tab

    def _hip_decode_ok(self, x, past_key_values, s_past, default_pos) -> bool:
        """The cached one-token step on csrc/persimmon_decode.hip: CUDA, bf16 compute, S == 1 after a prompt, default positions, q/k
        LayerNorm, rot % 16 == 0, no autograd, and every layer's past a bf16 [B,H,S_past,64] pair the kernel reads in place."""
        B, S = x.shape[:2]
        att = self.layers[0].self_attn
        if not (x.is_cuda and S == 1 and s_past > 0 and default_pos and OF.compute_dtype_for(x) == torch.bfloat16 and att.head_dim == 64
                and att.qk_layernorm and att.rot % 16 == 0 and 0 < att.rot <= 64 and s_past + 1 <= ops.PERSIMMON_DECODE_MAX_KEYS
                and os.environ.get("OTTER_FUYU_HIP_DECODE", "1") != "0" and os.environ.get("OTTER_NO_FLASH") != "1"):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        if len(past_key_values) < len(self.layers):
            return False
        for i in range(len(self.layers)):
            pkv = past_key_values[i]
            if pkv is None or len(pkv) != 2 or not all(t.is_cuda and ops._decode_past_ok(t, B, att.n_heads, s_past) for t in pkv):
                return False
        return True

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None, use_cache=None,
                return_dict=True, **unused):
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("You have to specify either input_ids or inputs_embeds")
        # HF / reference default: the config's use_cache, in train mode too; the cache entries are views, not copies
        use_cache = bool(use_cache) if use_cache is not None else bool(getattr(self.config, "use_cache", True))
        x = self.embed_tokens(input_ids) if inputs_embeds is None else inputs_embeds
        B, S = x.shape[:2]
        s_past = 0
        # a StaticKVCache (otter_amd/kv_cache.py) as `past_key_values`: empty, the ordinary prompt pass below fills it; after that a
        # one-token step appends in place (`_static_step`).  The object itself is returned as the new cache.
        cache = past_key_values if isinstance(past_key_values, StaticKVCache) else None
        if cache is not None:
            _check_static_cache_kind(cache, "PersimmonModel.forward")
            cache.check_step(B, S)
            if cache.length > 0:
                return self._static_step(x, cache, attention_mask, position_ids)
            past_key_values, use_cache = None, True
        if past_key_values is not None and len(past_key_values) and past_key_values[0] is not None and len(past_key_values[0]) == 2:
            s_past = past_key_values[0][0].shape[2]
        s_k = S + s_past
        cos_t, sin_t = self._tables(s_k, x.device)
        default_pos = position_ids is None
        if not default_pos and position_ids.shape[0] == 1 and bool((position_ids[0] == torch.arange(s_past, s_k, device=position_ids.device)).all()):
            default_pos = True            # the reference's forward always passes arange(past, past + S) (modeling_fuyu.py:116-119)
        if default_pos:
            cos, sin = cos_t[s_past:s_k], sin_t[s_past:s_k]
        else:
            cos, sin = cos_t[position_ids], sin_t[position_ids]
        am = None
        if attention_mask is not None:
            am = attention_mask.bool()
            if bool(am.all()):
                am = None
        # HIP path: causal only, like the reference's flash_attn_func(causal=True) which never sees the padding mask
        # (modeling_persimmon.py:310): with right padding the real positions are identical.  A left-padded prompt without autograd
        # (generate()) runs it too, with the key-padding mask evaluated in the flash kernel (pad-query rows, whose keys are all masked,
        # come out as 0: finite); under autograd left padding takes the plain path
        key_valid = None
        hip = self.layers[0].self_attn.hip_ok(x, s_past, default_pos)
        if hip and am is not None and not bool(am[:, 0].all()):
            if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
                hip = False
            else:
                key_valid = am[:, -s_k:].to(torch.uint8).contiguous()
        # cached one-token step on csrc/persimmon_decode.hip (the plain path's mask semantics on key_valid)
        dec = None
        if not hip and self._hip_decode_ok(x, past_key_values, s_past, default_pos):
            dec = (cos_t[s_past], sin_t[s_past])
            key_valid = am[:, -s_k:].to(torch.uint8).contiguous() if am is not None else None
        mask = None
        if not hip and dec is None:
            neg = torch.finfo(torch.float32).min
            mask = torch.zeros(1, 1, S, s_k, dtype=torch.float32, device=x.device)
            if S > 1:
                causal = torch.ones(S, s_k, dtype=torch.bool, device=x.device).tril(diagonal=s_k - S)
                mask = mask.masked_fill(~causal, neg)
            if am is not None:
                mask = mask.expand(B, -1, -1, -1).masked_fill(~am[:, None, None, -s_k:], neg)
            mask = mask.to(OF.compute_dtype_for(x))
        new_pasts = [] if use_cache else None
        pending = None      # hip path: a layer's MLP output joins the residual stream inside the NEXT LayerNorm pass (one kernel less per layer)
        for i, layer in enumerate(self.layers):
            pkv = past_key_values[i] if (past_key_values is not None and len(past_key_values) > i) else None
            if hip or dec is not None:
                x, npkv, pending = layer(x, cos, sin, past_key_value=pkv, use_cache=use_cache, hip=True, pending=pending, defer=True,
                                         key_valid=key_valid, decode=dec)
            else:
                x, npkv = layer(x, cos, sin, attn_mask=mask, past_key_value=pkv, use_cache=use_cache)
            if cache is not None:
                cache.fill(i, npkv[0], npkv[1])      # one strided copy each, from the views the pass returns
            elif use_cache:
                new_pasts.append(npkv)
        if cache is not None:
            cache.length = S
        n = self.final_layernorm
        if pending is not None:
            x = OF.add_layer_norm(x, pending, n.weight, n.bias, n.eps, OF.compute_dtype_for(x))[1]
        else:
            x = OF.layer_norm(x, n.weight, n.bias, n.eps, OF.compute_dtype_for(x)) if x.is_cuda else n(x)
        if cache is not None:
            return BaseModelOutputWithPast(last_hidden_state=x, past_key_values=cache)
        return BaseModelOutputWithPast(last_hidden_state=x, past_key_values=tuple(new_pasts) if use_cache else None)

    def _static_step(self, x, cache, attention_mask, position_ids):
        """The one-token step over a non-empty StaticKVCache: per layer the projection, `cache.attend_persimmon` and `dense`; the position
        moves once, after the last layer.  On the GPU in bf16 the layer runs its fused LayerNorm passes as the default cache's HIP step
        does, so that the two give the same logits; OTTER_FUYU_HIP_DECODE=0 sends the attention to the plain-torch restatement.
        Replay mode (`cache.enable_replay`): nothing here may depend on the position on the host side -- `attention_mask` and
        `position_ids` must be None (the mask is the cache's own), and the rotary tables are built to the cache's capacity before the first
        such step and must not move afterwards."""
        s_past = cache.length
        key_valid = None
        if cache.replay:
            if attention_mask is not None or position_ids is not None:
                raise ValueError("PersimmonModel.forward: a StaticKVCache in replay mode takes attention_mask=None and position_ids=None "
                                 "(the mask is the cache's own `valid`, the position its `pos_dev`)")
            tabs = getattr(cache, "rotary_tables", None)
            if tabs is None:                        # the first replay-mode step: built to the capacity, the address is fixed from here on
                tabs = cache.rotary_tables = self._tables(cache.max_len, x.device)
            elif self._tab is None or self._tab[0] is not tabs[0]:
                raise RuntimeError("PersimmonModel.forward: the rotary tables were rebuilt while a StaticKVCache is in replay mode (a longer "
                                   "forward ran in between): a captured step reads them at a fixed address")
            cos, sin = tabs
        else:
            if position_ids is not None and not (position_ids.shape[0] == 1 and position_ids.shape[1] == 1 and int(position_ids[0, 0]) == s_past):
                raise ValueError("PersimmonModel.forward: a step over a StaticKVCache takes the default positions (position_ids=None)")
            cos_t, sin_t = self._tables(s_past + 1, x.device)
            cos, sin = cos_t[s_past], sin_t[s_past]
            if attention_mask is not None:
                am = attention_mask.bool()
                if not bool(am.all()):
                    key_valid = am[:, -(s_past + 1):].to(torch.uint8).contiguous()
        hip = x.is_cuda and OF.compute_dtype_for(x) == torch.bfloat16 and os.environ.get("OTTER_NO_FLASH") != "1"
        reference = os.environ.get("OTTER_FUYU_HIP_DECODE", "1") == "0"
        pending = None
        for i, layer in enumerate(self.layers):
            if hip:
                x, _, pending = layer(x, cos, sin, hip=True, pending=pending, defer=True, key_valid=key_valid, static=(cache, i, reference))
            else:
                x, _ = layer(x, cos, sin, key_valid=key_valid, static=(cache, i, reference))
        cache.end_step()
        n = self.final_layernorm
        if pending is not None:
            x = OF.add_layer_norm(x, pending, n.weight, n.bias, n.eps, OF.compute_dtype_for(x))[1]
        else:
            x = OF.layer_norm(x, n.weight, n.bias, n.eps, OF.compute_dtype_for(x)) if x.is_cuda else n(x)
        return BaseModelOutputWithPast(last_hidden_state=x, past_key_values=cache)


class PersimmonForCausalLM(PersimmonPreTrainedModel):
    def __init__(self, config: PersimmonConfig):
        super().__init__(config)
        self.model = PersimmonModel(config)
        self.vocab_size = config.vocab_size
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.post_init()

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def set_input_embeddings(self, value):
        self.model.embed_tokens = value

    def get_output_embeddings(self):
        return self.lm_head

    def get_decoder(self):
        return self.model

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None, labels=None,
                use_cache=None, return_dict=True, _last_position_only=False, **unused):
        """`_last_position_only` (private; generate() passes it when `lm_head` is quantised): un-embed only the last position, logits
        [B, 1, V] -- a quantised un-embedding then runs as a GEMV / rows product on the prompt pass too instead of dequantising itself."""
        out = self.model(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, past_key_values=past_key_values,
                         inputs_embeds=inputs_embeds, use_cache=use_cache)
        h = out.last_hidden_state
        logits = _linear(self.lm_head, h[:, -1:, :] if _last_position_only else h)
        loss = None
        if labels is not None:
            lab = torch.full_like(labels, -100)
            lab[:, :-1] = labels[:, 1:]
            flat, lab = logits.view(-1, logits.size(-1)), lab.to(logits.device).view(-1)
            if flat.is_cuda and flat.dtype == torch.bfloat16 and flat.size(-1) % 4 == 0 and os.environ.get("OTTER_TORCH_CE") != "1":
                loss = OF.cross_entropy_bf16(flat, lab)
            else:
                loss = F.cross_entropy(flat.float(), lab, ignore_index=-100)
        return CausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=out.past_key_values)

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, **generate_kwargs):
        """Text-only decoding (transformers 5.x no longer gives PreTrainedModel a generate()): otter_amd/generation.py over this model."""
        from .generation import generate_tokens

        use_cache = bool(generate_kwargs.pop("use_cache", getattr(self.config, "use_cache", True)))
        if generate_kwargs.pop("kv_cache_dtype", None) is not None:
            raise NotImplementedError("PersimmonForCausalLM.generate: kv_cache_dtype quantises the static cache, which is not built for the "
                                      "Persimmon host (head_dim 64)")

        kw = {"_last_position_only": True} if _is_int8(self.lm_head) else {}
        nb = int(generate_kwargs.get("num_beams", 1) or 1)
        cache = _pop_static_cache("PersimmonForCausalLM.generate", generate_kwargs, self.config, self.model.embed_tokens.weight,
                                  input_ids.shape[0] * nb, input_ids.shape[1])
        if cache is not None:           # a caller's StaticKVCache (implies use_cache); `graph_decode=True` only together with one
            graph_step = [None]
            step = _static_cache_step(self, self, cache, nb, bool(generate_kwargs.pop("graph_decode", False)), graph_step, {}, kw)
            try:
                return generate_tokens(step, input_ids, attention_mask, **generate_kwargs)
            finally:
                if graph_step[0] is not None:
                    graph_step[0].release()

        def step(ids, mask, past, beam_idx):
            if use_cache and past is not None:
                if beam_idx is not None:
                    past = tuple(tuple(t.index_select(0, beam_idx) for t in layer) for layer in past)
                out = self(input_ids=ids[:, -1:], attention_mask=mask, past_key_values=past, use_cache=True, **kw)
            else:
                out = self(input_ids=ids, attention_mask=mask, use_cache=use_cache, **kw)
            return out.logits[:, -1, :], (out.past_key_values if use_cache else None)

        return generate_tokens(step, input_ids, attention_mask, **generate_kwargs)

    def quantize_decoder_int8(self, lm_head: bool = True, wide_steps: bool = False) -> dict:
        """Opt-in, for generation: hold the decoder's linears (`query_key_value`, `dense`, `dense_h_to_4h`, `dense_4h_to_h` of every layer)
        and, with `lm_head`, the untied un-embedding as int8 weights with one fp32 scale per output row (otter_amd/quant.py:
        `quantize_persimmon_decoder`), put the model in eval mode and return {"replaced", "bytes_before", "bytes_after"}.  The layers are
        quantised whatever their requires_grad is: the call states that training is over.

        This is an IN-MEMORY transformation done after loading: checkpoints stay in the reference's format.  `state_dict()` of a quantised
        model (qweight / scale buffers instead of weights) is not a reference-format checkpoint, so `save_pretrained` on it raises; the
        quantised decoder is inference-only (no autograd through it).  Calling it again replaces nothing.  `wide_steps=True` sets
        `panel_rows = quant.PANEL_MAX_ROWS` on every Int8FrozenLinear of the model, whichever call quantised it: one-token steps of 65 to
        that many rows then run the panel kernel instead of dequantising; the returned dict does not change."""
        from .quant import quantize_persimmon_decoder, set_wide_steps

        info = quantize_persimmon_decoder(self, lm_head=lm_head)
        if wide_steps:
            set_wide_steps(self)
        self.eval()
        return info

    def save_pretrained(self, *args, **kwargs):
        _refuse_save_if_int8(self)
        return super().save_pretrained(*args, **kwargs)


class FuyuPreTrainedModel(PreTrainedModel):
    config_class = FuyuConfig
    base_model_prefix = "fuyu"
    _no_split_modules = ["PersimmonDecoderLayer"]
    _supports_sdpa = True
    _supports_flash_attn = False
    _supports_flex_attn = False

    def _init_weights(self, module):
        std = getattr(self.config, "initializer_range", 0.02)
        if isinstance(module, nn.Linear):
            nn.init.normal_(module.weight, 0.0, std)
            if module.bias is not None:
                nn.init.zeros_(module.bias)
        elif isinstance(module, nn.Embedding):
            nn.init.normal_(module.weight, 0.0, std)


class FuyuForCausalLM(FuyuPreTrainedModel):
    """modeling_fuyu.py:19-143.  `image_patches`: [B, n_patches, patch*patch*channels] (or a list of [1, n_i, ...] tensors as the
    reference's processor emits); `image_patches_indices` [B, S]: -1 for text positions, else the index of the patch whose
    embedding replaces the word embedding at that position."""

    def __init__(self, config: FuyuConfig):
        super().__init__(config)
        self.padding_idx = getattr(config, "pad_token_id", None)
        self.vocab_size = config.text_config.vocab_size
        self.language_model = PersimmonForCausalLM(config.text_config)
        self.vision_embed_tokens = nn.Linear(config.patch_size * config.patch_size * config.num_channels, config.text_config.hidden_size)
        self.post_init()

    def get_input_embeddings(self):
        return self.language_model.get_input_embeddings()

    def set_input_embeddings(self, value):
        self.language_model.set_input_embeddings(value)

    def gather_continuous_embeddings(self, word_embeddings: torch.Tensor, continuous_embeddings: List[torch.Tensor],
                                     image_patch_input_indices: torch.Tensor) -> torch.Tensor:
        """modeling_fuyu.py:44-77: out[b, dst] = continuous[b][idx[b, dst]] wherever idx >= 0 (one HIP scatter on the GPU)."""
        if word_embeddings.shape[0] != len(continuous_embeddings):
            raise ValueError(f"Batch sizes must match! Got {len(continuous_embeddings)=} and {word_embeddings.shape[0]=}")
        B = word_embeddings.shape[0]
        idx = image_patch_input_indices
        n_rows = torch.tensor([c.shape[0] for c in continuous_embeddings], device=idx.device)
        n_idx = (idx >= 0).sum(dim=1)
        # one host synchronisation for both checks (the reference's per-sample loop has one per sample)
        bad_count, bad_range = (torch.stack([(n_idx > n_rows).any(), (idx.max(dim=1).values >= n_rows).any()]).tolist() if B else (False, False))
        if bad_count:
            b = int(torch.nonzero(n_idx > n_rows)[0])
            raise ValueError(f"Number of continuous embeddings {continuous_embeddings[b].shape=} does not match number of continuous "
                             f"token ids {int(n_idx[b])} in batch element {b}.")
        if bad_range:   # the reference's `continuous_embeddings[b][src]` raises IndexError for these
            b = int(torch.nonzero(idx.max(dim=1).values >= n_rows)[0])
            raise IndexError(f"image_patch_input_indices of batch element {b} reach {int(idx[b].max())}, but it has only "
                             f"{continuous_embeddings[b].shape[0]} continuous embeddings")
        if word_embeddings.is_cuda and all(c.shape[0] == continuous_embeddings[0].shape[0] for c in continuous_embeddings):
            return OF.scatter_patch_rows(word_embeddings, torch.stack(list(continuous_embeddings), 0), image_patch_input_indices)
        out = word_embeddings.clone()
        for b in range(B):
            dst = torch.nonzero(image_patch_input_indices[b] >= 0, as_tuple=True)[0]
            src = image_patch_input_indices[b][dst]
            out[b, dst] = continuous_embeddings[b][src].to(out.dtype)
        return out

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, attention_mask=None, image_patches=None,
                                      image_patches_indices=None, **kwargs):
        """modeling_fuyu.py:145-175 (the pinned transformers' hook): with a cache only the last token is fed and the patches are dropped."""
        if past_key_values is not None:
            input_ids = input_ids[:, -1:]
        return {"input_ids": input_ids, "past_key_values": past_key_values, "use_cache": kwargs.get("use_cache"), "attention_mask": attention_mask,
                "image_patches": image_patches if past_key_values is None else None,
                "image_patches_indices": image_patches_indices if past_key_values is None else None}

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, image_patches=None, image_patches_indices: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, **generate_kwargs):
        """`model.generate(**processor_outputs, max_new_tokens=...)` as the reference's OtterHD inference calls it
        (pipeline/demos/demo_models.py:171; the pinned transformers mixes GenerationMixin into PreTrainedModel, 5.x no longer does).
        Decoding = otter_amd/generation.py (greedy / beam / sampling, the same restatement OtterForConditionalGeneration.generate uses).
        The image patches enter on the prompt pass only; with `use_cache` (default: the config's) later steps feed one token against
        the KV cache, without it the whole sequence is re-run with the patch positions of the prompt and -1 for the new tokens."""
        from .generation import generate_tokens

        use_cache = bool(generate_kwargs.pop("use_cache", getattr(self.config.text_config, "use_cache", True)))
        if generate_kwargs.pop("kv_cache_dtype", None) is not None:
            raise NotImplementedError("FuyuForCausalLM.generate: kv_cache_dtype quantises the static cache, which is not built for the "
                                      "Persimmon host (head_dim 64)")
        cache_impl = generate_kwargs.pop("cache_implementation", None)
        if cache_impl == "static":
            raise NotImplementedError("FuyuForCausalLM.generate: cache_implementation='static' is not built for the Persimmon host (head_dim 64, "
                                      "fused q/k LayerNorm + partial rotary): use the default cache, whose step runs on csrc/persimmon_decode.hip, or pass a "
                                      "cache object: past_key_values=StaticKVCache.for_model(model, rows, max_len)")
        if cache_impl not in (None, "dynamic"):
            raise ValueError("generate: cache_implementation must be None, 'dynamic' or 'static', got %r" % (cache_impl,))
        L0 = input_ids.shape[1]
        nb = int(generate_kwargs.get("num_beams", 1) or 1)
        cache = _pop_static_cache("FuyuForCausalLM.generate", generate_kwargs, self.config.text_config,
                                  self.language_model.model.embed_tokens.weight, input_ids.shape[0] * nb, L0)
        graph_decode = bool(generate_kwargs.pop("graph_decode", False))
        if graph_decode and cache is None:
            raise NotImplementedError("FuyuForCausalLM.generate: graph_decode=True replays a step over the static cache, which is not built "
                                      "for the Persimmon host (what is built takes a cache object: past_key_values=StaticKVCache.for_model("
                                      "model, rows, max_len), with graph_decode=True beside it)")
        patches, idx0 = image_patches, image_patches_indices
        if nb > 1 and patches is not None:          # every beam of a sample sees that sample's image
            patches = (patches.repeat_interleave(nb, dim=0) if torch.is_tensor(patches) else [p for p in patches for _ in range(nb)])
            idx0 = idx0.repeat_interleave(nb, dim=0)

        kw = {"_last_position_only": True} if _is_int8(self.language_model.lm_head) else {}
        if cache is not None:           # a caller's StaticKVCache (implies use_cache): the prompt pass, with the patches, fills it
            graph_step = [None]
            step = _static_cache_step(self, self.language_model, cache, nb, graph_decode, graph_step,
                                      {"image_patches": patches, "image_patches_indices": idx0}, kw)
            try:
                return generate_tokens(step, input_ids, attention_mask, **generate_kwargs)
            finally:
                if graph_step[0] is not None:
                    graph_step[0].release()

        def step(ids, mask, past, beam_idx):
            if use_cache and past is not None:
                if beam_idx is not None:
                    past = tuple(tuple(t.index_select(0, beam_idx) for t in layer) for layer in past)
                out = self(input_ids=ids[:, -1:], attention_mask=mask, past_key_values=past, use_cache=True, **kw)
            else:
                idx = idx0
                if idx is not None and ids.shape[1] > L0:
                    idx = torch.cat([idx, idx.new_full((idx.shape[0], ids.shape[1] - L0), -1)], dim=1)
                out = self(input_ids=ids, image_patches=patches, image_patches_indices=idx, attention_mask=mask, use_cache=use_cache, **kw)
            return out.logits[:, -1, :], (out.past_key_values if use_cache else None)

        return generate_tokens(step, input_ids, attention_mask, **generate_kwargs)

    def quantize_decoder_int8(self, lm_head: bool = True, wide_steps: bool = False) -> dict:
        """`PersimmonForCausalLM.quantize_decoder_int8` on `language_model` (same contract: in-memory, eval mode, inference-only,
        `save_pretrained` raises afterwards, a second call replaces nothing); `vision_embed_tokens` and the embedding stay as they are.
        Returns {"replaced", "bytes_before", "bytes_after"}."""
        info = self.language_model.quantize_decoder_int8(lm_head=lm_head, wide_steps=wide_steps)
        self.eval()
        return info

    def save_pretrained(self, *args, **kwargs):
        _refuse_save_if_int8(self)
        return super().save_pretrained(*args, **kwargs)

    def forward(self, input_ids=None, labels=None, image_patches=None, image_patches_indices=None, attention_mask=None, position_ids=None,
                past_key_values=None, inputs_embeds=None, use_cache=None, return_dict=True, _last_position_only=False, **unused):
        if input_ids is not None and inputs_embeds is not None:
            raise ValueError("You cannot specify both decoder_input_ids and decoder_inputs_embeds at the same time")
        if input_ids is None and inputs_embeds is None:
            raise ValueError("You have to specify either decoder_input_ids or decoder_inputs_embeds")
        if inputs_embeds is None:
            inputs_embeds = self.language_model.get_input_embeddings()(input_ids)
            if image_patches is not None and (past_key_values is None or (isinstance(past_key_values, StaticKVCache)
                                                                          and past_key_values.length == 0)):
                w = self.vision_embed_tokens
                if torch.is_tensor(image_patches):
                    pe = list(w(image_patches.to(w.weight.dtype)))                  # one GEMM for the whole batch
                elif (len(image_patches) and all(p.dim() == 3 and p.shape[0] == 1 and p.shape == image_patches[0].shape for p in image_patches)):
                    # the processor's list of same-size [1, n, patch_dim] images: the same single GEMM as the tensor form, so both forms give
                    # the same bits (per-image GEMMs of another row count may round differently, depending on the BLAS kernel chosen)
                    pe = list(w(torch.cat([p.to(w.weight.dtype) for p in image_patches], 0)))
                else:
                    pe = [w(p.to(w.weight.dtype)).squeeze(0) for p in image_patches]
                inputs_embeds = self.gather_continuous_embeddings(inputs_embeds, pe, image_patches_indices)
        kw = {"_last_position_only": True} if _last_position_only else {}
        return self.language_model(inputs_embeds=inputs_embeds, labels=labels, attention_mask=attention_mask, position_ids=position_ids,
                                   past_key_values=past_key_values, use_cache=use_cache, **kw)
