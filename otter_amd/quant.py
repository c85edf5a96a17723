"""Int8 weight-only form of the frozen decoder for generation.

`generate(use_cache=True)` feeds the frozen decoder one token per sequence: every decoder linear sees B x num_beams rows (1 to 64) and
the step is a single pass over the weights.  Storing those weights as int8 with one fp32 scale per output row halves the bytes a step
moves and the decoder's footprint; the activations stay bf16 and the accumulation fp32 (csrc/w8.hip).  This is an opt-in, in-memory
transformation applied after loading (`OtterForConditionalGeneration.quantize_decoder_int8()`); nothing on the training path changes.
The OtterHD / Fuyu host has the same method (`FuyuForCausalLM.quantize_decoder_int8()`): `quantize_persimmon_decoder`.
`quantize_decoder_int8(gated_blocks=True, lm_head=True)` on the MPT and LLaMA hosts adds the last weights a cached step still streams in
bf16: the two FFN linears of every gated cross-attention block (`quantize_gated_blocks`; the second product
carries the block's tanh-gate residual in its tail, `Int8FrozenLinear.forward_gated`) and the un-embedding (`quantize_unembedding`,
`Int8Unembedding`).

Format.  For a weight W [N, K] read as fp32:
    amax[n]  = max_k |W[n, k]|
    scale[n] = amax[n] / 127          (fp32 IEEE division; 1 when amax[n] == 0)
    q[n, k]  = clamp(round_half_even(W[n, k] / scale[n]), -127, 127)  as int8 (-128 is never produced)
stored as `qweight` int8 [N, K] (row-major) and `scale` fp32 [N].  The quantiser is a handful of IEEE-exact torch ops, so it gives the
same bits on the GPU and on the CPU.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as OF
from . import ops

GEMV_MAX_ROWS = ops.GEMV_W8_MAX_ROWS
ROWS_MAX_ROWS = ops.GEMM_W8_ROWS_MAX_ROWS
# what `quantize_decoder_int8(wide_steps=True)` sets `Int8FrozenLinear.panel_rows` to: the largest measured row count (of 72, 96, 128, 192,
# 256) up to which the panel kernel is at most 1.03 x the faster of the two routes it replaces on all four MPT-7B linears; at 256 rows the
# dequantising route is ahead on two of them (profiles/r23_w8_panel.txt).  The kernel itself takes up to 256 rows.
PANEL_MAX_ROWS = 192


def route(rows: int, one_token: bool, panel_rows: int = 0) -> str:
    """Which product an Int8FrozenLinear runs for a GPU input of `rows` rows (leading dimensions flattened):
      "gemv"     rows <= 16: ops.gemv_w8;
      "rows"     17 <= rows <= 64 in a one-token step (the input has at least three dimensions and x.shape[-2] == 1, as every cached
                 step of the MPT and LLaMA hosts passes it): ops.gemm_w8_rows.  OTTER_W8_ROWS=0 sends this case to "dequant" (A/B);
      "panel"    64 < rows <= panel_rows in a one-token step: ops.gemm_w8_panel.  `panel_rows` is the layer's `panel_rows` attribute, 0
                 (never) unless `quantize_decoder_int8(wide_steps=True)` set it.  OTTER_W8_PANEL=0 sends this case to "dequant" (A/B);
      "dequant"  everything else -- prompt passes of any size above 16 rows, steps of more than max(64, panel_rows) rows: ops.dequant_w8 +
                 library GEMM.
    """
    if rows <= GEMV_MAX_ROWS:
        return "gemv"
    if one_token and rows <= ROWS_MAX_ROWS and os.environ.get("OTTER_W8_ROWS", "1") != "0":
        return "rows"
    if one_token and ROWS_MAX_ROWS < rows <= panel_rows and os.environ.get("OTTER_W8_PANEL", "1") != "0":
        return "panel"
    return "dequant"


def quantize_weight_int8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """W [N, K] (bf16 / fp16 / fp32) -> (qweight int8 [N, K], scale fp32 [N]) on W's device, by the definition in the module docstring."""
    if w.dim() != 2 or not w.is_floating_point():
        raise ValueError("quantize_weight_int8: a 2-d floating-point weight is expected, got %s %s" % (tuple(w.shape), w.dtype))
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    # tensor / tensor: a true division on every backend (a Python-scalar divisor may be turned into a multiplication by its reciprocal)
    scale = amax / torch.full_like(amax, 127.0)
    scale = torch.where(amax == 0, torch.ones_like(scale), scale)
    q = torch.round(wf / scale[:, None]).clamp_(-127, 127).to(torch.int8)
    return q.contiguous(), scale.contiguous()


def dequantize_weight_int8(q: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(qweight, scale) -> float(q) * scale[:, None] in fp32, rounded once to `dtype`."""
    return (q.float() * scale.float()[:, None]).to(dtype)


# one bf16 scratch per device for the dequantised weight of the more-than-16-row path: sized to the largest weight seen, shared by every
# layer (work on one device is ordered by the stream the kernels are launched on, as for ops._ws)
_scratch: Dict[Tuple[str, Optional[int]], torch.Tensor] = {}


def _dequant_scratch(numel: int, device: torch.device) -> torch.Tensor:
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    b = _scratch.get(key)
    if b is None or b.numel() < numel:
        _scratch.pop(key, None)                    # (the smaller buffer is released before the larger one is allocated)
        del b
        b = torch.empty(numel, dtype=torch.bfloat16, device=device)
        _scratch[key] = b
    return b


def release_scratch() -> None:
    """Drop the shared dequantisation scratch buffers (reallocated by the next prefill)."""
    _scratch.clear()


_ACT_CODES = {None: 0, "gelu": 1, "relu2": 3}          # the `act` argument of otter_gemv_w8 / otter_gemm_w8_rows (include/otter_hip.h)


class Int8FrozenLinear(nn.Module):
    """A frozen nn.Linear held as int8 weights + one fp32 scale per output row (buffers `qweight`, `scale`, `bias`).  Inference only.

    forward(x, act=None) -- `act="gelu"` applies the exact-erf GELU to the output, `act="relu2"` the squared ReLU of the Persimmon MLP:
      * GPU input of at most 16 rows (leading dimensions flattened): `ops.gemv_w8`, one pass over the int8 weight, scale / bias / activation
        in its epilogue.  x is cast to bf16 if it is not; the output has the compute dtype the unquantised layer would have produced.
      * GPU input of 17 to 64 rows in a one-token step ([rows, 1, K]: batch x beams of a cached step): `ops.gemm_w8_rows`, the same
        single pass over the int8 weight (see `route`).
      * Any other GPU input (prompt prefill, more than 64 rows): `ops.dequant_w8` into the process-wide bf16 scratch, then the library GEMM
        (then the GELU / squared-ReLU kernel).
      * CPU input: F.linear(x, dequantize_weight_int8(...), bias).  The ONE deliberate exception to this package's "no CPU fallback"
        rule: the host contract (module swap, parity with the fake-quantised model, error paths) has to be testable without a GPU.  No
        product path runs the decoder on the CPU.
    forward_gated(x, gate, residual) -- the same product with the tanh-gate residual tail of a gated cross-attention block, by the same routes.

    `panel_rows` (a plain attribute, 0 by default; `quantize_decoder_int8(wide_steps=True)` sets it to PANEL_MAX_ROWS): one-token steps of
    65 to `panel_rows` rows run `ops.gemm_w8_panel` / `ops.gemm_w8_panel_gated` instead of dequantising.
    """

    panel_rows = 0

    def __init__(self, qweight: torch.Tensor, scale: torch.Tensor, bias: Optional[torch.Tensor] = None):
        super().__init__()
        if qweight.dtype != torch.int8 or qweight.dim() != 2 or scale.dtype != torch.float32 or tuple(scale.shape) != (qweight.shape[0],):
            raise ValueError("Int8FrozenLinear: qweight int8 [N, K] and scale fp32 [N] are expected")
        self.out_features, self.in_features = qweight.shape
        self.register_buffer("qweight", qweight.contiguous())
        self.register_buffer("scale", scale.contiguous())
        self.register_buffer("bias", None if bias is None else bias.detach().clone())

    def _apply(self, fn, *a, **k):
        # .half() / .to(torch.bfloat16) cast floating-point buffers: the scale is part of the format and stays fp32 (qweight is int8 and
        # is never cast); moves between devices go through as usual
        exact = self.scale
        super()._apply(fn, *a, **k)
        if self.scale.dtype != torch.float32:
            self.scale = exact.to(self.scale.device)
        return self

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "Int8FrozenLinear":
        if lin.weight.requires_grad:
            raise ValueError("Int8FrozenLinear.from_linear: the layer is trainable (weight.requires_grad); only frozen layers are quantised")
        q, s = quantize_weight_int8(lin.weight)
        return cls(q, s, lin.bias)

    def extra_repr(self) -> str:
        return "in_features=%d, out_features=%d, bias=%s, int8" % (self.in_features, self.out_features, self.bias is not None)

    def nbytes(self) -> int:
        return self.qweight.numel() + 4 * self.scale.numel() + (self.bias.numel() * self.bias.element_size() if self.bias is not None else 0)

    def forward(self, x: torch.Tensor, act: Optional[str] = None) -> torch.Tensor:
        if act not in _ACT_CODES:
            raise ValueError("Int8FrozenLinear: act must be None, 'gelu' or 'relu2'")
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("the int8 decoder is inference-only: its input requires grad (run it under torch.no_grad(); training or LoRA "
                               "on quantised weights is not supported)")
        if not x.is_cuda:
            y = F.linear(x, dequantize_weight_int8(self.qweight, self.scale, x.dtype), None if self.bias is None else self.bias.to(x.dtype))
            return F.gelu(y) if act == "gelu" else torch.square(F.relu(y)) if act == "relu2" else y
        cd = OF.compute_dtype_for(x)
        lead = x.shape[:-1]
        x2 = x.reshape(-1, self.in_features)
        xb = x2 if x2.dtype == torch.bfloat16 else x2.to(torch.bfloat16)
        how = route(xb.shape[0], x.dim() >= 3 and x.shape[-2] == 1, self.panel_rows)
        if how != "dequant":
            if xb.stride(1) != 1 or (xb.shape[0] > 1 and xb.stride(0) % 8) or xb.data_ptr() % 16:
                xb = xb.contiguous()
            product = {"gemv": ops.gemv_w8, "rows": ops.gemm_w8_rows, "panel": ops.gemm_w8_panel}[how]
            y = product(xb, self.qweight, self.scale, self.bias, _ACT_CODES[act], out_dtype=cd)
            return y.view(lead + (self.out_features,))
        n, k = self.qweight.shape
        w = ops.dequant_w8(self.qweight, self.scale, out=_dequant_scratch(n * k, x.device)[: n * k].view(n, k))
        with torch.autocast("cuda", enabled=False):
            y = F.linear(xb, w, None if self.bias is None else self.bias.to(torch.bfloat16))
        if act == "gelu":
            y = OF.gelu(y)
        elif act == "relu2":
            y = ops.sqrelu_fwd(y)
        return (y if cd == torch.bfloat16 else y.to(cd)).view(lead + (self.out_features,))


    def forward_gated(self, x: torch.Tensor, gate: Optional[torch.Tensor], residual: torch.Tensor) -> torch.Tensor:
        """self(x) * tanh(gate) + residual, the tail in fp32 on the fp32 product and rounded once to residual's dtype: the second FFN
        product of a gated cross-attention block.  `gate`: one fp32 value (None: 1), `residual`: x's leading
        dimensions x out_features.  The routes are `forward`'s: "gemv" / "rows" / "panel" run `ops.gemv_w8_gated` / `ops.gemm_w8_rows_gated` /
        `ops.gemm_w8_panel_gated`,
        "dequant" the library GEMM of the unquantised block with its EPI_SCALE_RES tail on the dequantised weight, the CPU plain torch."""
        if torch.is_grad_enabled() and (x.requires_grad or residual.requires_grad):
            raise RuntimeError("the int8 decoder is inference-only: its input requires grad (run it under torch.no_grad(); training or LoRA "
                               "on quantised weights is not supported)")
        lead, rd = x.shape[:-1], residual.dtype
        if tuple(residual.shape) != tuple(lead) + (self.out_features,):
            raise ValueError("Int8FrozenLinear.forward_gated: residual %s against an output of %s" % (tuple(residual.shape), tuple(lead) + (self.out_features,)))
        if gate is not None:
            gate = gate.detach().reshape(1)
        if not x.is_cuda:
            v = F.linear(x, dequantize_weight_int8(self.qweight, self.scale, x.dtype), None if self.bias is None else self.bias.to(x.dtype))
            return (v.float() * (torch.tanh(gate.float()) if gate is not None else 1.0) + residual.float()).to(rd)
        x2, r2 = x.reshape(-1, self.in_features), residual.reshape(-1, self.out_features)
        xb = x2 if x2.dtype == torch.bfloat16 else x2.to(torch.bfloat16)
        how = route(xb.shape[0], x.dim() >= 3 and x.shape[-2] == 1, self.panel_rows)
        if r2.stride(1) != 1 or r2.dtype not in (torch.bfloat16, torch.float32):
            r2 = r2.contiguous() if r2.dtype in (torch.bfloat16, torch.float32) else r2.float()
        if how != "dequant":
            if xb.stride(1) != 1 or (xb.shape[0] > 1 and xb.stride(0) % 8) or xb.data_ptr() % 16:
                xb = xb.contiguous()
            product = {"gemv": ops.gemv_w8_gated, "rows": ops.gemm_w8_rows_gated, "panel": ops.gemm_w8_panel_gated}[how]
            return product(xb, self.qweight, self.scale, gate, r2, self.bias, out_dtype=rd).view(residual.shape)
        if self.bias is not None:
            raise NotImplementedError("Int8FrozenLinear.forward_gated: a bias on the dequantising route (the gated blocks have none)")
        n, k = self.qweight.shape
        w = ops.dequant_w8(self.qweight, self.scale, out=_dequant_scratch(n * k, x.device)[: n * k].view(n, k))
        return ops.gemm_nt(xb, w, out_dtype=rd, kind=OF.EPI_SCALE_RES, gate=gate, R=r2).view(residual.shape)


def _decoder_layers(lang_encoder: nn.Module):
    if hasattr(lang_encoder, "_get_decoder_layers"):
        return list(lang_encoder._get_decoder_layers())
    for path in ("transformer.blocks", "model.layers"):
        obj = lang_encoder
        try:
            for part in path.split("."):
                obj = getattr(obj, part)
        except AttributeError:
            continue
        return list(obj)
    raise ValueError("quantize_frozen_decoder: no decoder layers found in %s" % lang_encoder.__class__.__name__)


def quantize_frozen_decoder(lang_encoder: nn.Module) -> dict:
    """Replace every frozen FrozenAwareLinear inside the decoder layers (MPT: Wqkv, out_proj, up_proj, down_proj; LLaMA: q/k/v/o_proj,
    gate/up/down_proj) by an Int8FrozenLinear.  Left alone: LoRA-wrapped layers, anything trainable, the embedding / tied un-embedding and
    lm_head, the gated cross-attention blocks (those two are `quantize_unembedding` and `quantize_gated_blocks`, behind keywords of their
    own) and the perceiver and CLIP, which are not part of the language model.  The compute-dtype and
    transposed copies of what is replaced are released.  Returns {"replaced", "bytes_before", "bytes_after"}; a second call replaces nothing."""
    from .lora import LoraLinear
    from .mpt import FrozenAwareLinear

    replaced, before, after = 0, 0, 0
    for layer in _decoder_layers(lang_encoder):
        core = getattr(layer, "decoder_layer", layer)          # OtterLayer wraps (gated_cross_attn_layer, decoder_layer)
        swapped = {}
        for parent in list(core.modules()):
            for name, child in list(parent.named_children()):
                if (not isinstance(child, FrozenAwareLinear) or isinstance(child, LoraLinear) or child.weight.requires_grad
                        or (child.bias is not None and child.bias.requires_grad) or child.in_features % 16):
                    continue
                new = Int8FrozenLinear.from_linear(child)
                before += child.weight.numel() * child.weight.element_size()
                before += child.bias.numel() * child.bias.element_size() if child.bias is not None else 0
                after += new.nbytes()
                child.release_copies()
                setattr(parent, name, new)
                swapped[id(child)] = new
                replaced += 1
        if swapped:
            for parent in core.modules():                       # the LLaMA host's fused q|k|v / gate|up helpers hold their modules by reference
                for attr in ("_qkv", "_gu"):
                    f = getattr(parent, attr, None)
                    if f is not None and hasattr(f, "mods"):
                        f.release()
                        f.mods = [swapped.get(id(m), m) for m in f.mods]     # (or the replaced weights stay alive; `usable()` is False for these)
    return {"replaced": replaced, "bytes_before": before, "bytes_after": after}


class _Tally:
    """What one quantising call replaced: the {"replaced", "bytes_before", "bytes_after"} every such call returns."""

    def __init__(self):
        self.replaced, self.before, self.after = 0, 0, 0

    def add(self, weight: torch.Tensor, bias: Optional[torch.Tensor], new: "Int8FrozenLinear") -> None:
        self.replaced += 1
        self.before += weight.numel() * weight.element_size() + (bias.numel() * bias.element_size() if bias is not None else 0)
        self.after += new.nbytes()

    def info(self) -> dict:
        return {"replaced": self.replaced, "bytes_before": self.before, "bytes_after": self.after}


def _release_shadows(weight: torch.Tensor) -> None:
    for store in (OF.shadows._w, OF.shadows._wt):               # the compute-dtype copies a training run left of the replaced weight
        for key in [k for k in store if k[0] == id(weight)]:
            del store[key]


def _swap_linear(parent: nn.Module, name: str, tally: _Tally, cls=None) -> None:
    """Replace the plain nn.Linear `parent.name` (in_features % 16 == 0) by an Int8FrozenLinear (or the subclass `cls`), whatever its
    requires_grad is: through `quantize_weight_int8` and the constructor, since `from_linear` refuses trainable layers."""
    child = getattr(parent, name)
    if type(child) is not nn.Linear or child.in_features % 16:
        return
    q, s = quantize_weight_int8(child.weight)
    new = (cls or Int8FrozenLinear)(q, s, None if child.bias is None else child.bias.detach())
    tally.add(child.weight, child.bias, new)
    _release_shadows(child.weight)
    setattr(parent, name, new)


def quantize_gated_blocks(lang_encoder: nn.Module) -> dict:
    """Replace `feed_forward[1]` and `feed_forward[3]` of every OtterGatedCrossAttentionBlock of the decoder by an Int8FrozenLinear
    (DESIGN.md section 4.21).  These are trainable nn.Linear: as on the OtterHD host the call is the user's statement that training is over.
    Left alone: `attn.to_q` / `to_kv` / `to_out`, both LayerNorms, both gates.  Returns the usual dict; a second call replaces nothing."""
    tally = _Tally()
    for layer in _decoder_layers(lang_encoder):
        block = getattr(layer, "gated_cross_attn_layer", None)
        ff = getattr(block, "feed_forward", None)
        if ff is not None and all(type(ff[i]) is nn.Linear and ff[i].in_features % 16 == 0 for i in (1, 3)):     # both or neither
            _swap_linear(block.feed_forward, "1", tally)
            _swap_linear(block.feed_forward, "3", tally)
    return tally.info()


class Int8Unembedding(Int8FrozenLinear):
    """The un-embedding (MPT: an int8 copy of the tied table, LLaMA: `lm_head`) as an Int8FrozenLinear that never dequantises: on the GPU
    at most 16 rows run `ops.gemv_w8`, more run `ops.gemm_w8_rows` in slices of at most 64 rows (the rows of that kernel do not depend on
    each other), so a pass of any size leaves the shared dequantisation scratch at the largest decoder weight.  generate() sends only the
    last position of the prompt pass here.  With `panel_rows` set (and OTTER_W8_PANEL not 0) a pass of more than 64 rows is cut into slices
    of `panel_rows` rows through `ops.gemm_w8_panel`, whose rows do not depend on each other either."""

    def forward(self, x: torch.Tensor, act: Optional[str] = None) -> torch.Tensor:
        if not x.is_cuda or act is not None or x.numel() // self.in_features <= GEMV_MAX_ROWS:
            return super().forward(x, act)
        if torch.is_grad_enabled() and x.requires_grad:
            return super().forward(x, act)                      # (raises: inference-only)
        x2 = x.reshape(-1, self.in_features)
        xb = x2 if x2.dtype == torch.bfloat16 else x2.to(torch.bfloat16)
        if xb.stride(1) != 1 or xb.stride(0) % 8 or xb.data_ptr() % 16:
            xb = xb.contiguous()
        y = torch.empty((xb.shape[0], self.out_features), dtype=OF.compute_dtype_for(x), device=x.device)
        wide = xb.shape[0] > ROWS_MAX_ROWS < self.panel_rows and os.environ.get("OTTER_W8_PANEL", "1") != "0"
        step, product = (min(self.panel_rows, ops.GEMM_W8_PANEL_MAX_ROWS), ops.gemm_w8_panel) if wide else (ROWS_MAX_ROWS, ops.gemm_w8_rows)
        for r in range(0, xb.shape[0], step):
            product(xb[r:r + step], self.qweight, self.scale, self.bias, 0, out=y[r:r + step])
        return y.view(x.shape[:-1] + (self.out_features,))


def quantize_unembedding(lang_encoder: nn.Module) -> dict:
    """MPT: give the tied table `transformer.wte` an int8 copy, `wte.unembed_int8`, which `SharedEmbedding.forward(unembed=True)` then uses;
    the table itself stays for the lookup (so the model grows by the copy while a step reads half the bytes: "bytes_before" is what the
    un-embedding read before).  LLaMA: replace `lm_head`; a table it is tied to stays with `embed_tokens` in the same way.  Returns the
    usual dict; a second call replaces nothing."""
    from .mpt import SharedEmbedding

    tally = _Tally()
    wte = next((m for m in lang_encoder.modules() if isinstance(m, SharedEmbedding)), None)
    if wte is not None:
        if getattr(wte, "unembed_int8", None) is None and wte.weight.shape[1] % 16 == 0:
            wte.unembed_int8 = Int8Unembedding(*quantize_weight_int8(wte.weight))
            tally.add(wte.weight, None, wte.unembed_int8)
        return tally.info()
    owner = next((m for m in lang_encoder.modules() if isinstance(getattr(m, "lm_head", None), nn.Module)), None)
    if owner is None:
        raise ValueError("quantize_unembedding: neither a tied table nor an lm_head in %s" % lang_encoder.__class__.__name__)
    _swap_linear(owner, "lm_head", tally, Int8Unembedding)
    return tally.info()


def quantize_persimmon_decoder(lm: nn.Module, lm_head: bool = True) -> dict:
    """Replace `query_key_value`, `dense`, `dense_h_to_4h` and `dense_4h_to_h` of every PersimmonDecoderLayer of `lm` (a
    fuyu.PersimmonForCausalLM) by an Int8FrozenLinear, and with `lm_head` the untied un-embedding too.  Left alone: `embed_tokens`, every
    LayerNorm (q_layernorm / k_layernorm included) and whatever lives outside `lm` (Fuyu's vision_embed_tokens).  The OtterHD recipe
    fine-tunes the whole model, so these are ordinary trainable nn.Linear: the call is the user's statement that training is over and
    they are quantised whatever their requires_grad is (`Int8FrozenLinear.from_linear` keeps refusing trainable layers; this goes through
    `quantize_weight_int8` and the constructor).  Returns {"replaced", "bytes_before", "bytes_after"}; a second call replaces nothing."""
    from .fuyu import PersimmonDecoderLayer

    tally = _Tally()
    swap = lambda parent, name: _swap_linear(parent, name, tally)

    for layer in list(lm.modules()):
        if isinstance(layer, PersimmonDecoderLayer):
            swap(layer.self_attn, "query_key_value")
            swap(layer.self_attn, "dense")
            swap(layer.mlp, "dense_h_to_4h")
            swap(layer.mlp, "dense_4h_to_h")
    if lm_head:
        swap(lm, "lm_head")
    return tally.info()


def set_wide_steps(model: nn.Module, rows: int = PANEL_MAX_ROWS) -> int:
    """Set `panel_rows = rows` on every Int8FrozenLinear of `model` (the decoder's, the gated blocks', the un-embedding, whichever call
    quantised them): what the hosts' `quantize_decoder_int8(wide_steps=True)` does.  Returns how many there are."""
    n = 0
    for m in model.modules():
        if isinstance(m, Int8FrozenLinear):
            m.panel_rows = rows
            n += 1
    return n
