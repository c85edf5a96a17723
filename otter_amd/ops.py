"""Tensor-level wrappers over the C ABI (one Python function per entry point of include/otter_hip.h).

PyTorch is used here for device memory (torch.empty), the current HIP stream and nothing else: all arithmetic
happens in libotter_hip.so.  Every wrapper validates devices/dtypes/contiguity and raises on error."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _capi as K
from ._capi import BF16, EPI_GATE_BWD, EPI_GELU, EPI_SCALE_RES, EPI_STORE, F32, MASK_EQ, MASK_GE, MASK_NONE, RowMap

_IDENT = RowMap(0, 0, 0)


class _Workspace:
    """Grow-only scratch buffer per (device, stream): reuse is ordered by the stream the kernels are launched on (torch's current stream).
    Keyed by the stream since round 5: the fusion modules launch on side streams too (functional._SideStream), and two kernels on two
    streams must never share one scratch buffer."""

    def __init__(self):
        self.bufs = {}

    def get(self, nbytes: int, device) -> torch.Tensor:
        key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
        b = self.bufs.get(key)
        if b is None or b.numel() < nbytes:
            b = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
            self.bufs[key] = b
        return b

    def drop_stream(self, device, stream) -> None:
        """Forget the buffer of one stream.  otter_amd/graph_decode.py calls it at the end of every generate(graph_decode=True) call for
        its capture stream (one per device, kept for the life of the process): the buffer is allocated again, in ordinary memory, by the
        next call's warm-up steps, so nothing of this project's that is keyed by that stream outlives a call."""
        self.bufs.pop((device.type, device.index, stream.cuda_stream), None)


_ws = _Workspace()


# OTTER_GEMM_LOG=1: count the GEMM shapes of a run and print them at exit (tuning aid)
_GEMM_LOG = None
if os.environ.get("OTTER_GEMM_LOG") == "1":
    import atexit
    import collections

    _GEMM_LOG = collections.Counter()
    atexit.register(lambda: print("\n".join("gemm M=%d N=%d K=%d epi=%d %s->%s  x%d" % (k + (v,)) for k, v in sorted(_GEMM_LOG.items()))))


def _c2d(t: torch.Tensor) -> torch.Tensor:
    if t.dim() != 2 or t.stride(1) != 1:
        raise K.OtterHipError(f"expected a row-major 2-D tensor, got shape {tuple(t.shape)} strides {t.stride()}")
    return t


# ----------------------------------------------------------------------------------------------------------------------
# norms
# ----------------------------------------------------------------------------------------------------------------------


def layernorm_fwd(x2d, gamma, beta, out_dtype, eps=1e-5, y=None, ymap: Optional[RowMap] = None, y2=None, need_stats=True):
    """x2d [rows, D] contiguous.  Returns (y, mean, rstd)."""
    K.require_cuda(x2d, gamma, beta)
    x2d = _c2d(x2d)
    assert x2d.is_contiguous()
    rows, D = x2d.shape
    if y is None:
        y = torch.empty((rows, D), dtype=out_dtype, device=x2d.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x2d.device) if need_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device) if need_stats else None
    wdt = K.dt(gamma) if gamma is not None else F32
    if gamma is not None and beta is not None and gamma.dtype != beta.dtype:
        raise K.OtterHipError("layernorm: gamma/beta dtype mismatch")
    K.check(K.lib().otter_layernorm_fwd(x2d.data_ptr(), K.dt(x2d), K.ptr(gamma), K.ptr(beta), wdt, y.data_ptr(), K.dt(y),
                                        ymap or _IDENT, K.ptr(y2), K.ptr(mean), K.ptr(rstd), rows, D, float(eps), K.stream()),
            "layernorm_fwd")
    return y, mean, rstd


def add_layernorm_fwd(x2d, delta2d, gamma, beta, out_dtype, eps=1e-5, need_stats=True):
    """(xsum, y, mean, rstd) with xsum = x + delta (x's dtype) and y = LN(xsum)."""
    K.require_cuda(x2d, delta2d, gamma, beta)
    assert x2d.is_contiguous() and delta2d.is_contiguous() and x2d.shape == delta2d.shape
    rows, D = x2d.shape
    xsum = torch.empty_like(x2d)
    y = torch.empty((rows, D), dtype=out_dtype, device=x2d.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x2d.device) if need_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device) if need_stats else None
    wdt = K.dt(gamma) if gamma is not None else F32
    K.check(K.lib().otter_add_layernorm_fwd(x2d.data_ptr(), K.dt(x2d), delta2d.data_ptr(), K.dt(delta2d), xsum.data_ptr(),
                                            K.ptr(gamma), K.ptr(beta), wdt, y.data_ptr(), K.dt(y), K.ptr(mean), K.ptr(rstd), rows, D,
                                            float(eps), K.stream()), "add_layernorm_fwd")
    return xsum, y, mean, rstd


def layernorm_bwd(dy, x2d, gamma, mean, rstd, dx_dtype, dres=None, dymap: Optional[RowMap] = None, need_dw=True,
                  need_dbeta=True, need_dx=True, dx_bf16=None):
    """Returns (dx, dgamma, dbeta) -- dgamma/dbeta fp32.  dx_bf16: optional preallocated bf16 [rows, D] tensor that
    receives a bf16 copy of dx in the same pass."""
    K.require_cuda(dy, x2d)
    rows, D = x2d.shape
    dev = x2d.device
    dx = torch.empty((rows, D), dtype=dx_dtype, device=dev) if need_dx else None
    if dres is not None and dres.dtype != dx_dtype:
        raise K.OtterHipError("layernorm_bwd: dres must have the dx dtype")
    if dx_bf16 is not None and (dx_bf16.dtype != torch.bfloat16 or not dx_bf16.is_contiguous() or tuple(dx_bf16.shape) != (rows, D)):
        raise K.OtterHipError("layernorm_bwd: dx_bf16 must be a contiguous bf16 [rows, D] tensor")
    dg = torch.empty(D, dtype=torch.float32, device=dev) if need_dw else None
    db = torch.empty(D, dtype=torch.float32, device=dev) if (need_dw and need_dbeta) else None
    ws = None
    if need_dw:
        ws = _ws.get(K.lib().otter_layernorm_bwd_workspace_bytes(rows, D), dev)
    wdt = K.dt(gamma) if gamma is not None else F32
    K.check(K.lib().otter_layernorm_bwd(dy.data_ptr(), K.dt(dy), dymap or _IDENT, x2d.data_ptr(), K.dt(x2d), K.ptr(gamma), wdt,
                                        mean.data_ptr(), rstd.data_ptr(), K.ptr(dres), K.ptr(dx), K.dt_of(dx_dtype), K.ptr(dx_bf16),
                                        K.ptr(dg), K.ptr(db), 0, K.ptr(ws), rows, D, K.stream()), "layernorm_bwd")
    return dx, dg, db


def colsum(src2d, src_map: Optional[RowMap], rows: int, out=None, accumulate=False):
    """out[c] (+)= sum over r < rows of src2d[map(r)][c]; fp32 [D]."""
    D = src2d.shape[1]
    if out is None:
        out = torch.empty(D, dtype=torch.float32, device=src2d.device)
    ws = _ws.get(K.lib().otter_layernorm_bwd_workspace_bytes(rows, D), src2d.device)
    K.check(K.lib().otter_colsum(src2d.data_ptr(), K.dt(src2d), src_map or _IDENT, out.data_ptr(), 1 if accumulate else 0,
                                 ws.data_ptr(), rows, D, K.stream()), "colsum")
    return out


def rmsnorm_fwd(x2d, w, eps=1e-6):
    K.require_cuda(x2d, w)
    rows, D = x2d.shape
    y = torch.empty_like(x2d)
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    K.check(K.lib().otter_rmsnorm_fwd(x2d.data_ptr(), K.dt(x2d), w.data_ptr(), K.dt(w), y.data_ptr(), rstd.data_ptr(), rows, D,
                                      float(eps), K.stream()), "rmsnorm_fwd")
    return y, rstd


def rmsnorm_bwd(dy, x2d, w, rstd):
    """(dx, dw) in x's dtype / fp32.  The C function takes ONE dtype for dy, x and dx."""
    if dy.dtype != x2d.dtype:
        raise K.OtterHipError(f"rmsnorm_bwd: dy must have the dtype of x ({x2d.dtype}), got {dy.dtype}; rmsnorm_bwd_ex takes mixed dtypes")
    rows, D = x2d.shape
    dx = torch.empty_like(x2d)
    dw = torch.empty(D, dtype=torch.float32, device=x2d.device)
    ws = _ws.get(K.lib().otter_layernorm_bwd_workspace_bytes(rows, D), x2d.device)
    K.check(K.lib().otter_rmsnorm_bwd(dy.data_ptr(), x2d.data_ptr(), K.dt(x2d), w.data_ptr(), K.dt(w), rstd.data_ptr(),
                                      dx.data_ptr(), dw.data_ptr(), 0, ws.data_ptr(), rows, D, K.stream()), "rmsnorm_bwd")
    return dx, dw


def add_rmsnorm_fwd(x2d, delta2d, w, out_dtype, eps=1e-6):
    """LLaMA host: (xsum, y, rstd) with xsum = x + delta (x's dtype; None when delta is None) and y = RMSNorm(xsum) in
    `out_dtype` (bf16 of the fp32 result when the stream is fp32)."""
    K.require_cuda(x2d, delta2d, w)
    assert x2d.is_contiguous() and (delta2d is None or (delta2d.is_contiguous() and delta2d.shape == x2d.shape))
    rows, D = x2d.shape
    xsum = torch.empty_like(x2d) if delta2d is not None else None
    y = torch.empty((rows, D), dtype=out_dtype, device=x2d.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    K.check(K.lib().otter_add_rmsnorm_fwd(x2d.data_ptr(), K.dt(x2d), K.ptr(delta2d), K.dt(delta2d) if delta2d is not None else F32, K.ptr(xsum),
                                          w.data_ptr(), K.dt(w), y.data_ptr(), K.dt(y), rstd.data_ptr(), rows, D, float(eps), K.stream()),
            "add_rmsnorm_fwd")
    return xsum, y, rstd


def rmsnorm_bwd_ex(dy, x2d, w, rstd, dx_dtype, dres=None, need_dw=False, dx_bf16=None):
    """(dx, dw): dx = RMSNorm'(dy) (+ dres), optional bf16 copy of dx into dx_bf16, dw fp32 [D] only when need_dw."""
    K.require_cuda(dy, x2d, w, rstd, dres, dx_bf16)
    rows, D = x2d.shape
    dev = x2d.device
    assert dy.is_contiguous() and tuple(dy.shape) == (rows, D)
    if dres is not None and (dres.dtype != dx_dtype or not dres.is_contiguous()):
        raise K.OtterHipError("rmsnorm_bwd_ex: dres must be contiguous and have the dx dtype")
    dx = torch.empty((rows, D), dtype=dx_dtype, device=dev)
    dw = torch.empty(D, dtype=torch.float32, device=dev) if need_dw else None
    ws = _ws.get(K.lib().otter_layernorm_bwd_workspace_bytes(rows, D), dev) if need_dw else None
    K.check(K.lib().otter_rmsnorm_bwd_ex(dy.data_ptr(), K.dt(dy), x2d.data_ptr(), K.dt(x2d), w.data_ptr(), K.dt(w), rstd.data_ptr(), K.ptr(dres),
                                         dx.data_ptr(), K.dt(dx), K.ptr(dx_bf16), K.ptr(dw), 0, K.ptr(ws), rows, D, K.stream()), "rmsnorm_bwd_ex")
    return dx, dw


# ----------------------------------------------------------------------------------------------------------------------
# GEMM
# ----------------------------------------------------------------------------------------------------------------------


def gemm_nt(A, B, out_dtype=None, out=None, kind=EPI_STORE, gate=None, R=None, C2=None, aux=None, aux_gelu=False,
            partial=None, accumulate=False, k=None, a_kmajor=False, b_kmajor=False):
    """C[M,N] = epilogue(A[M,K] . B[N,K]^T).  A, B row-major 2-D (row stride free), same dtype.
    `k` restricts the reduction to the first k columns (used with zero-padded transposed operands).
    a_kmajor / b_kmajor (see `gemm`): the operand is given as [K, M] / [K, N] instead."""
    K.require_cuda(A, B)
    A, B = _c2d(A), _c2d(B)
    if A.dtype != B.dtype:
        raise K.OtterHipError(f"gemm: operand dtypes differ ({A.dtype} vs {B.dtype})")
    M, Ka = (A.shape[1], A.shape[0]) if a_kmajor else A.shape
    N, Kb = (B.shape[1], B.shape[0]) if b_kmajor else B.shape
    Kd = k if k is not None else Ka
    if Kd > Ka or Kd > Kb or (k is None and Ka != Kb):
        raise K.OtterHipError(f"gemm: K mismatch A{tuple(A.shape)} B{tuple(B.shape)} k={k}")
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype or A.dtype, device=A.device)
    out = _c2d(out)
    e = K.EpilogueArgs()
    e.kind = kind
    e.accumulate = 1 if accumulate else 0
    e.gate = K.ptr(gate)
    if R is not None:
        R = _c2d(R)
        e.R, e.ldr, e.r_dtype = R.data_ptr(), R.stride(0), K.dt(R)
    if C2 is not None:
        C2 = _c2d(C2)
        if C2.dtype != out.dtype:
            raise K.OtterHipError("gemm: C2 must have the dtype of C")
        e.C2, e.ldc2 = C2.data_ptr(), C2.stride(0)
    if aux is not None:
        aux = _c2d(aux)
        e.aux, e.ldaux, e.aux_dtype = aux.data_ptr(), aux.stride(0), K.dt(aux)
    # activation whose derivative the GATE_BWD tail applies to aux; "stash": the derivative itself travels (GELU launch: C2 = GELU'(acc),
    # GATE_BWD launch: aux holds it)
    e.aux_is_gelu_input = 3 if aux_gelu == "stash" else (2 if aux_gelu == "sqrelu" else (1 if aux_gelu else 0))
    e.partial = K.ptr(partial)
    e.grid_mode = _grid_mode
    if _GEMM_LOG is not None:
        _GEMM_LOG[(M, N, Kd, kind, str(A.dtype).split(".")[-1], str(out.dtype).split(".")[-1])] += 1
    if a_kmajor or b_kmajor:
        K.check(K.lib().otter_gemm(A.data_ptr(), A.stride(0), 1 if a_kmajor else 0, B.data_ptr(), B.stride(0), 1 if b_kmajor else 0, out.data_ptr(),
                                   out.stride(0), M, N, Kd, K.dt(A), K.dt(out), C.byref(e), K.stream()), "gemm")
        return out
    K.check(K.lib().otter_gemm_nt(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), out.stride(0), M, N, Kd,
                                  K.dt(A), K.dt(out), C.byref(e), K.stream()), "gemm_nt")
    return out


def gemm_kmajor_supported(M, N, Kd, lda, ldb, a_kmajor, b_kmajor, dtype) -> bool:
    """True when otter_gemm takes these operands in place (K-major = [K rows][M or N columns]); else transpose + gemm_nt."""
    if dtype != torch.bfloat16:
        return False
    return bool(K.lib().otter_gemm_kmajor_supported(int(M), int(N), int(Kd), int(lda), int(ldb), 1 if a_kmajor else 0, 1 if b_kmajor else 0, BF16))


def gemm(A, B, a_kmajor=False, b_kmajor=False, **kw):
    """C = epilogue(op(A) . op(B)^T) with K-MAJOR operands read in place: a_kmajor -> A is [K, M] (the reduction index is the row
    index), b_kmajor -> B is [K, N].  dW = dy^T x is gemm(dy, x, True, True); dx = dy W (W stored [out, in]) is gemm(dy, W, False, True)."""
    return gemm_nt(A, B, a_kmajor=a_kmajor, b_kmajor=b_kmajor, **kw)


def gemm_num_partials(M, N, dtype) -> int:
    return int(K.lib().otter_gemm_num_partials(M, N, K.dt_of(dtype)))


def reduce_partials(partial, gate=None, out=None, accumulate=False):
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=partial.device)
    K.check(K.lib().otter_reduce_partials(partial.data_ptr(), partial.numel(), K.ptr(gate), out.data_ptr(), 1 if accumulate else 0,
                                          K.stream()), "reduce_partials")
    return out


def transpose(src, out_dtype, want_same=False, pad_to=8):
    """src [rows, cols] -> (src^T as [cols, rows_padded] with zero tail columns, optional same-layout cast copy).
    rows_padded = roundup(rows, pad_to) so the result can feed gemm_nt as a K-contiguous operand."""
    K.require_cuda(src)
    src = _c2d(src)
    rows, cols = src.shape
    rp = (rows + pad_to - 1) // pad_to * pad_to
    if rp != rows:
        dst_t = torch.zeros((cols, rp), dtype=out_dtype, device=src.device)
    else:
        dst_t = torch.empty((cols, rp), dtype=out_dtype, device=src.device)
    same = torch.empty((rows, cols), dtype=out_dtype, device=src.device) if want_same else None
    K.check(K.lib().otter_transpose(src.data_ptr(), src.stride(0), K.dt(src), dst_t.data_ptr(), dst_t.stride(0), K.ptr(same),
                                    cols if want_same else 0, K.dt_of(out_dtype), rows, cols, K.stream()), "transpose")
    return (dst_t, same) if want_same else dst_t


def cast(src, out_dtype):
    K.require_cuda(src)
    if src.dtype == out_dtype:
        return src
    src = src.contiguous()
    out = torch.empty(src.shape, dtype=out_dtype, device=src.device)
    K.check(K.lib().otter_cast(src.data_ptr(), K.dt(src), out.data_ptr(), K.dt(out), src.numel(), K.stream()), "cast")
    return out


# ----------------------------------------------------------------------------------------------------------------------
# attention + mask
# ----------------------------------------------------------------------------------------------------------------------


def text_time(media_locations: torch.Tensor, attend_previous: bool = True) -> torch.Tensor:
    """bool/uint8 [B,T] -> int32 [B,T] (modeling_otter.py:298-311)."""
    K.require_cuda(media_locations)
    ml = media_locations.to(torch.uint8).contiguous()
    B, T = ml.shape
    tt = torch.empty((B, T), dtype=torch.int32, device=ml.device)
    K.check(K.lib().otter_text_time(ml.data_ptr(), tt.data_ptr(), B, T, 1 if attend_previous else 0, K.stream()), "text_time")
    return tt


def attn_fwd(q, k, v, H, tt, n_per_media, mask_mode, scale, need_lse=True):
    """q [B,Tq,H*64]; k, v [B,M,H*64] (may be strided views of one [B,M,2*H*64] buffer).  Returns (o, lse)."""
    K.require_cuda(q, k, v)
    B, Tq, HD = q.shape
    M = k.shape[1]
    if HD != H * 64:
        raise K.OtterHipError(f"attention core supports head_dim 64 only (got inner={HD}, heads={H})")
    if q.stride(2) != 1 or k.stride(2) != 1 or v.stride(2) != 1 or k.stride(1) != v.stride(1):
        raise K.OtterHipError("attn: bad strides")
    if q.stride(0) != Tq * q.stride(1) or k.stride(0) != M * k.stride(1) or v.stride(0) != M * v.stride(1):
        raise K.OtterHipError("attn: batch stride must equal rows*row_stride")
    o = torch.empty((B, Tq, HD), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, Tq), dtype=torch.float32, device=q.device) if need_lse else None
    K.check(K.lib().otter_attn_fwd(q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(), k.stride(1), o.data_ptr(), o.stride(1),
                                   K.ptr(lse), K.ptr(tt), B, H, Tq, M, n_per_media, mask_mode, float(scale), K.dt(q), K.stream()),
            "attn_fwd")
    return o, lse


def attn_bwd(q, k, v, o, do, lse, H, tt, n_per_media, mask_mode, scale, dkv_out=None):
    """Returns (dq [B,Tq,H*64], dkv [B,M,2*H*64]) -- dk in the first half of the last axis, dv in the second."""
    B, Tq, HD = q.shape
    M = k.shape[1]
    dq = torch.empty((B, Tq, HD), dtype=q.dtype, device=q.device)
    dkv = dkv_out if dkv_out is not None else torch.empty((B, M, 2 * HD), dtype=q.dtype, device=q.device)
    dk, dv = dkv[..., :HD], dkv[..., HD:]
    ws = _ws.get(K.lib().otter_attn_bwd_workspace_bytes(B, H, Tq, M), q.device)
    do = do.contiguous()
    K.check(K.lib().otter_attn_bwd(q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(), k.stride(1), o.data_ptr(), do.data_ptr(),
                                   o.stride(1), lse.data_ptr(), K.ptr(tt), dq.data_ptr(), dq.stride(1), dk.data_ptr(),
                                   dv.data_ptr(), dkv.stride(1), ws.data_ptr(), B, H, Tq, M, n_per_media, mask_mode, float(scale),
                                   K.dt(q), K.stream()), "attn_bwd")
    return dq, dkv


# ----------------------------------------------------------------------------------------------------------------------
# misc
# ----------------------------------------------------------------------------------------------------------------------


def _flash_view(t: torch.Tensor, hd: int = 128) -> K.FlashView:
    """t: a [B, S, H, head_dim] bf16 view with unit stride along the head dim."""
    if t.dim() != 4 or t.shape[3] != hd or t.stride(3) != 1 or t.dtype != torch.bfloat16:
        raise K.OtterHipError(f"flash attention wants [B,S,H,{hd}] bf16 views (got {tuple(t.shape)}, {t.dtype}, strides {t.stride()})")
    return K.FlashView(t.stride(0), t.stride(1), t.stride(2))


def _flash_desc(q, k, v, o, lse, slopes, key_valid, scale, causal) -> K.FlashDesc:
    K.require_cuda(q, k, v, o, lse, slopes, key_valid)
    B, Sq, H, hd = q.shape
    Sk = k.shape[1]
    if hd not in (64, 128) or (hd == 64 and H % 2):
        raise K.OtterHipError(f"flash attention: head_dim 128, or 64 with an even number of heads (got head_dim {hd}, {H} heads)")
    if key_valid is not None and (key_valid.dtype != torch.uint8 or not key_valid.is_contiguous() or key_valid.shape != (B, Sk)):
        raise K.OtterHipError("flash attention: key_valid must be a contiguous uint8 [B, Sk] tensor")
    if slopes is not None and (slopes.dtype != torch.float32 or not slopes.is_contiguous() or slopes.numel() != H):
        raise K.OtterHipError("flash attention: alibi slopes must be a contiguous fp32 [H] tensor")
    d = K.FlashDesc()
    d.q, d.k, d.v, d.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    d.qv, d.kv, d.vv, d.ov = _flash_view(q, hd), _flash_view(k, hd), _flash_view(v, hd), _flash_view(o, hd)
    d.lse = lse.data_ptr()
    d.alibi_slopes = K.ptr(slopes)
    d.key_valid = K.ptr(key_valid)
    d.B, d.H, d.Sq, d.Sk, d.head_dim, d.causal = B, H, Sq, Sk, hd, int(bool(causal))
    d.scale = float(scale)
    return d


def flash_attn_fwd(q, k, v, slopes, key_valid, scale, causal=True):
    """Decoder-host attention (mpt/attention.py:22-84 + ALiBi :447-464) on [B,S,H,128] bf16 views, or Persimmon's
    (fuyu/modeling_persimmon.py:310) on [B,S,H,64] views with H even.  Returns (o [B,Sq,H,head_dim] contiguous, lse [B,H,Sq] fp32)."""
    B, Sq, H, hd = q.shape
    o = torch.empty((B, Sq, H, hd), dtype=torch.bfloat16, device=q.device)
    lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    d = _flash_desc(q, k, v, o, lse, slopes, key_valid, scale, causal)
    K.check(K.lib().otter_flash_attn_fwd(C.byref(d), K.stream()), "flash_attn_fwd")
    return o, lse


def flash_attn_fwd_f32(q, k, v, slopes, key_valid, scale, causal=True):
    """`flash_attn_fwd` at head_dim 128 with the output unrounded (otter_flash_attn_fwd_f32): returns (o fp32 [B,Sq,H,128] contiguous, lse
    [B,H,Sq] fp32).  Its probabilities enter the second product as a bf16 hi + lo pair, so o is fp32-accurate.  For a consumer that goes on
    computing with o and rounds at its own output (`branch_attn_merge`)."""
    B, Sq, H, hd = q.shape
    if hd != 128:
        raise K.OtterHipError(f"flash attention with fp32 output: head_dim 128 only (got {hd})")
    o = torch.empty((B, Sq, H, hd), dtype=torch.float32, device=q.device)
    lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device)
    d = _flash_desc(q, k, v, q, lse, slopes, key_valid, scale, causal)       # (d.o is not written: any valid bf16 view stands in)
    K.check(K.lib().otter_flash_attn_fwd_f32(C.byref(d), o.data_ptr(), K.stream()), "flash_attn_fwd_f32")
    return o, lse


def flash_attn_bwd(q, k, v, o, lse, dout, dq, dk, dv, slopes, key_valid, scale, causal=True):
    """Writes dq / dk / dv (caller-provided [B,S,H,head_dim] views, e.g. the three slices of one dqkv buffer)."""
    K.require_cuda(dout, dq, dk, dv)
    hd = q.shape[3]
    d = _flash_desc(q, k, v, o, lse, slopes, key_valid, scale, causal)
    delta = torch.empty((2,) + tuple(lse.shape), dtype=torch.float32, device=lse.device)  # row dots + log2-domain lse
    d.dout, d.dov = dout.data_ptr(), _flash_view(dout, hd)
    d.delta = delta.data_ptr()
    d.dq, d.dk, d.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    d.dqv, d.dkv, d.dvv = _flash_view(dq, hd), _flash_view(dk, hd), _flash_view(dv, hd)
    K.check(K.lib().otter_flash_attn_bwd(C.byref(d), K.stream()), "flash_attn_bwd")


def rope(x, cos, sin, rot_dim=None, inverse=False, out=None):
    """x [B,S,H,d] contiguous, cos/sin fp32 [S,rot]."""
    K.require_cuda(x, cos, sin)
    x = x.contiguous()
    B, S, H, d = x.shape
    rot = rot_dim or d
    y = out if out is not None else torch.empty_like(x)
    K.check(K.lib().otter_rope(x.data_ptr(), y.data_ptr(), cos.data_ptr(), sin.data_ptr(), B, S, H, d, rot, 1 if inverse else 0,
                               K.dt(x), K.stream()), "rope")
    return y


def rope_strided(x, y, cos, sin, tokens, S, H, d, x_token_stride, y_token_stride, inverse=False):
    """bf16 full-rotary RoPE on `tokens` = B*S tokens of H contiguous heads each, tokens x_/y_token_stride elements apart
    (x / y are any tensors whose data_ptr is the first rotated element; in place when y is x).  cos/sin fp32 [S, d]."""
    K.require_cuda(x, y, cos, sin)
    if x.dtype != torch.bfloat16 or y.dtype != torch.bfloat16 or cos.dtype != torch.float32 or sin.dtype != torch.float32:
        raise K.OtterHipError("rope_strided: bf16 data, fp32 tables")
    if not cos.is_contiguous() or not sin.is_contiguous() or tuple(cos.shape) != (S, d) or tuple(sin.shape) != (S, d):
        raise K.OtterHipError("rope_strided: cos/sin must be contiguous [S, d]")
    K.check(K.lib().otter_rope_strided(x.data_ptr(), y.data_ptr(), cos.data_ptr(), sin.data_ptr(), tokens, S, H, d, 1 if inverse else 0,
                                       x_token_stride, y_token_stride, K.stream()), "rope_strided")
    return y


def quick_gelu_(x):
    """In place x * sigmoid(1.702 x) on a contiguous bf16 / f32 tensor (CLIP MLP activation)."""
    K.require_cuda(x)
    if not x.is_contiguous() or x.numel() % 8:
        raise K.OtterHipError("quick_gelu: contiguous tensor with numel % 8 == 0")
    K.check(K.lib().otter_quick_gelu(x.data_ptr(), x.data_ptr(), x.numel(), K.dt(x), K.stream()), "quick_gelu")
    return x


def gelu_fwd(x):
    """Exact-erf GELU (nn.GELU() default) of a contiguous bf16 / f32 tensor, numel % 8 == 0 (MPT MLP activation)."""
    K.require_cuda(x)
    if not x.is_contiguous() or x.numel() % 8:
        raise K.OtterHipError("gelu_fwd: contiguous tensor with numel % 8 == 0")
    y = torch.empty_like(x)
    K.check(K.lib().otter_gelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), K.dt(x), K.stream()), "gelu_fwd")
    return y


def gelu_bwd(x, dy):
    """dx = dy * gelu'(x) (exact-erf form), same layout rules as gelu_fwd."""
    K.require_cuda(x, dy)
    if not x.is_contiguous() or not dy.is_contiguous() or x.numel() % 8 or dy.shape != x.shape or dy.dtype != x.dtype:
        raise K.OtterHipError("gelu_bwd: x and dy must be contiguous, same shape / dtype, numel % 8 == 0")
    dx = torch.empty_like(x)
    K.check(K.lib().otter_gelu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), K.dt(x), K.stream()), "gelu_bwd")
    return dx


def swiglu_fwd(gu2d):
    """gu2d [rows, 2*I] bf16 contiguous (gate | up) -> h [rows, I] = silu(gate) * up."""
    K.require_cuda(gu2d)
    rows, I2 = gu2d.shape
    if gu2d.dtype != torch.bfloat16 or not gu2d.is_contiguous() or I2 % 16:
        raise K.OtterHipError("swiglu: contiguous bf16 [rows, 2*I] with I % 8 == 0")
    h = torch.empty((rows, I2 // 2), dtype=torch.bfloat16, device=gu2d.device)
    K.check(K.lib().otter_swiglu_fwd(gu2d.data_ptr(), h.data_ptr(), rows, I2 // 2, K.stream()), "swiglu_fwd")
    return h


def swiglu_bwd(gu2d, dh2d):
    K.require_cuda(gu2d, dh2d)
    rows, I2 = gu2d.shape
    if dh2d.dtype != torch.bfloat16 or not dh2d.is_contiguous() or tuple(dh2d.shape) != (rows, I2 // 2):
        raise K.OtterHipError("swiglu_bwd: dh must be contiguous bf16 [rows, I]")
    dgu = torch.empty_like(gu2d)
    K.check(K.lib().otter_swiglu_bwd(gu2d.data_ptr(), dh2d.data_ptr(), dgu.data_ptr(), rows, I2 // 2, K.stream()), "swiglu_bwd")
    return dgu


def decode_attn(q, k, v, slopes, key_valid, scale):
    """Single-query attention over a KV cache.  q [B,H,128] bf16; k, v: 4-d bf16 tensors indexed [b, h, key, dim] through their own
    strides (pass `k_cache.transpose(2, 3)` for the MPT layout [B,H,d,S]); slopes fp32 [H] or None; key_valid uint8 [B,Sk] or None.
    Returns o [B,H,128]."""
    K.require_cuda(q, k, v, slopes, key_valid)
    B, H, d = q.shape
    Sk = k.shape[2]
    if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16 or d != 128 or q.stride(2) != 1:
        raise K.OtterHipError("decode_attn: bf16, head_dim 128, unit-stride q")
    if tuple(k.shape) != (B, H, Sk, d) or tuple(v.shape) != (B, H, Sk, d):
        raise K.OtterHipError("decode_attn: k, v must be indexable as [B,H,Sk,128]")
    if key_valid is not None and (key_valid.dtype != torch.uint8 or not key_valid.is_contiguous() or tuple(key_valid.shape) != (B, Sk)):
        raise K.OtterHipError("decode_attn: key_valid must be contiguous uint8 [B,Sk]")
    o = torch.empty((B, H, d), dtype=torch.bfloat16, device=q.device)
    K.check(K.lib().otter_decode_attn(q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), k.stride(2), k.stride(3),
                                      v.data_ptr(), v.stride(0), v.stride(1), v.stride(2), v.stride(3), o.data_ptr(), o.stride(0), o.stride(1),
                                      K.ptr(slopes), K.ptr(key_valid), B, H, Sk, d, float(scale), K.stream()), "decode_attn")
    return o


PERSIMMON_DECODE_MAX_KEYS = 65536      # include/otter_hip.h: S_past + 1 <= 65536
DECODE_CACHED_MAX_KEYS = 65536        # include/otter_hip.h: S_max <= 65536


def persimmon_decode_workspace_bytes(B: int, H: int, Sk: int) -> int:
    """OTTER_PERSIMMON_DECODE_WORKSPACE_BYTES of include/otter_hip.h; its _CACHED (Sk = pos + 1) and _CACHED_DYN (Sk = S_max) forms are the same."""
    return B * H * ((Sk + 127) // 128) * 66 * 4


persimmon_decode_cached_workspace_bytes = persimmon_decode_cached_dyn_workspace_bytes = persimmon_decode_workspace_bytes


def decode_attn_cached_workspace_bytes(N: int, H: int, Sk: int) -> int:
    """OTTER_DECODE_CACHED_WORKSPACE_BYTES of include/otter_hip.h (Sk = pos + 1); its _DYN (Sk = S_max), _I8 and _I8_DYN forms are the same."""
    return N * H * ((Sk + 127) // 128) * 130 * 4


decode_attn_cached_dyn_workspace_bytes = decode_attn_cached_i8_workspace_bytes = decode_attn_cached_i8_dyn_workspace_bytes = \
    decode_attn_cached_workspace_bytes


# ---- the argument checks of the cached-decode entry points -------------------------------------------------------------------------------
# One checker per kind of argument; each takes the entry point's name (the prefix of its messages) and whatever varies between entry points.
# They look at dtype, shape, strides and alignment only, so they run on CPU tensors: tests/test_decode_bindings_cpu.py holds every message,
# the order of the checks and every argument tuple to a recording.  DESIGN.md 4.9 lists what differs between entry points on purpose.

def _decode_past_ok(t, B, H, S_past) -> bool:
    return (t.dtype == torch.bfloat16 and t.dim() == 4 and tuple(t.shape) == (B, H, S_past, 64) and t.stride(3) == 1
            and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0 and t.stride(2) % 8 == 0 and t.data_ptr() % 16 == 0)


def _check_new_128(name, q, k_new, v_new):
    """The new token at head_dim 128, three views; returns (N, H)."""
    if q.dim() != 3:
        raise K.OtterHipError(f"{name}: q must be [N,H,128]")
    N, H = q.shape[:2]
    for t in (q, k_new, v_new):
        if (t.dtype != torch.bfloat16 or t.dim() != 3 or tuple(t.shape) != (N, H, 128) or (st := t.stride())[2] != 1 or st[0] % 8 or st[1] % 8
                or t.data_ptr() % 16):
            raise K.OtterHipError(f"{name}: q / k_new / v_new must be bf16 [N,H,128], unit dim stride, strides % 8 == 0, 16-B aligned")
    return N, H


def _check_qkv_64(name, qkv):
    """The new token at head_dim 64, one fused tensor; returns (N, H)."""
    if qkv.dtype != torch.bfloat16 or qkv.dim() != 4 or qkv.shape[2:] != (3, 64) or not qkv.is_contiguous() or qkv.data_ptr() % 16:
        raise K.OtterHipError(f"{name}: qkv must be contiguous bf16 [N,H,3,64], 16-B aligned")
    return qkv.shape[:2]


def _check_caches(name, k_cache, v_cache, N, H, dtype, hd, mod):
    """The static cache pair: `dtype` [N,H,S_max,hd], row and head strides % mod (8 elements of bf16, 16 of int8: 16 bytes); returns S_max."""
    S_max = k_cache.shape[2] if k_cache.dim() == 4 else -1
    for t in (k_cache, v_cache):
        if (t.dtype != dtype or t.dim() != 4 or tuple(t.shape) != (N, H, S_max, hd) or (st := t.stride())[3] != 1 or st[2] != hd
                or st[0] % mod or st[1] % mod or st[1] < S_max * hd or t.data_ptr() % 16):
            raise K.OtterHipError(f"{name}: k_cache / v_cache must be {'int8' if dtype == torch.int8 else 'bf16'} [N,H,S_max,{hd}] "
                                  f"with key stride {hd}, unit dim stride, 16-B aligned")
    return S_max


def _check_scales(name, k_scale, v_scale, N, H, S_max):
    for t in (k_scale, v_scale):
        if t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape) != (N, H, S_max) or t.stride(2) != 1 or t.stride(1) < S_max:
            raise K.OtterHipError(f"{name}: k_scale / v_scale must be fp32 [N,H,S_max] with a unit key stride")


def _check_s_max(name, S_max, limit):
    if S_max < 2 or S_max > limit:
        raise K.OtterHipError(f"{name}: S_max={S_max} outside [2, {limit}]")


def _check_pos(name, pos, S_max, limit=None):
    """The position scalar; returns it as an int.  `limit`: the upper limit of S_max is part of this check and of its message (the head_dim-128
    entry points, which have no S_max check of their own)."""
    pos = int(pos)
    if (limit is not None and S_max > limit) or pos < 1 or pos >= S_max:
        raise K.OtterHipError(f"{name}: pos={pos} outside [1, S_max) with S_max={S_max}" + (f" (limit {limit})" if limit is not None else ""))
    return pos


def _check_pos_dev(name, pos_dev):
    if pos_dev.dtype != torch.int32 or pos_dev.numel() != 1:
        raise K.OtterHipError(f"{name}: pos_dev must be an int32 tensor of one element")


def _check_norm_rot(name, gq, bq, gk, bk, rot):
    for t in (gq, bq, gk, bk):
        if t.dtype != torch.float32 or t.numel() != 64 or not t.is_contiguous():
            raise K.OtterHipError(f"{name}: gamma / beta must be contiguous fp32 [64]")
    if rot <= 0 or rot > 64 or rot % 16:
        raise K.OtterHipError(f"{name}: rot={rot} must be a multiple of 16 in (0, 64]")


def _check_rotary_rows_64(name, cos_row, sin_row, rot):
    for t in (cos_row, sin_row):
        if t.dtype != torch.float32 or t.numel() != rot or not t.is_contiguous():
            raise K.OtterHipError(f"{name}: cos_row / sin_row must be contiguous fp32 [rot]")


def _check_rotary_rows_128(name, cos, sin, N):
    """Both or neither; [128] (one row for all) or [N,128].  Returns the row stride handed to the library (0: one row, or no rotary)."""
    if (cos is None) != (sin is None):
        raise K.OtterHipError(f"{name}: cos and sin must both be given or both be None")
    if cos is None:
        return 0
    for t in (cos, sin):
        if (t.dtype != torch.float32 or t.shape[-1] != 128 or t.stride(-1) != 1 or tuple(t.shape) not in ((128,), (N, 128))
                or tuple(t.shape) != tuple(cos.shape) or t.stride() != cos.stride()):
            raise K.OtterHipError(f"{name}: cos / sin must be fp32 [128] or [N,128] with a unit dim stride and equal strides")
    return cos.stride(0) if cos.dim() == 2 else 0


def _check_rotary_tables(name, cos_table, sin_table, S_max, width, width_text, optional):
    """fp32 [>= S_max, width] with equal strides; `optional`: both may be None (head_dim 128).  Returns the row stride (0: no rotary)."""
    if optional:
        if (cos_table is None) != (sin_table is None):
            raise K.OtterHipError(f"{name}: cos_table and sin_table must both be given or both be None")
        if cos_table is None:
            return 0
    for t in (cos_table, sin_table):
        if (t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < S_max or t.shape[1] != width or t.stride(1) != 1 or t.stride(0) < width
                or t.stride() != cos_table.stride()):
            raise K.OtterHipError(f"{name}: cos_table / sin_table must be fp32 [>= S_max, {width_text}] with a unit dim stride and equal strides")
    return cos_table.stride(0)


def _check_rows(name, t, what, dtype, N, need, need_text, strict):
    """src (int32) or key_valid (uint8): [N, >= need] or None.  Returns the row stride handed to the library (0 for None).  `strict`: a row
    stride below `need` is refused here when N > 1 and raised to `need` when N == 1; otherwise it is passed as it is and the library decides."""
    if t is None:
        return 0
    if (t.dtype != dtype or t.dim() != 2 or t.shape[0] != N or t.shape[1] < need or t.stride(1) != 1
            or (strict and N > 1 and t.stride(0) < need)):
        raise K.OtterHipError(f"{name}: {what} must be {str(dtype)[6:]} [N, >= {need_text}] with a unit column stride")
    return max(t.stride(0), need) if strict else t.stride(0)


def _check_slopes(name, slopes, H):
    if slopes is not None and (slopes.dtype != torch.float32 or not slopes.is_contiguous() or slopes.numel() != H):
        raise K.OtterHipError(f"{name}: slopes must be contiguous fp32 [H]")


def _out_or_new(name, out, N, H, hd, device):
    if out is None:
        return torch.empty((N, H * hd), dtype=torch.bfloat16, device=device)
    if out.dtype != torch.bfloat16 or tuple(out.shape) != (N, H * hd) or not out.is_contiguous():
        raise K.OtterHipError(f"{name}: out must be a contiguous bf16 [N, H*{hd}] tensor")
    return out


def persimmon_decode_attn(qkv, gq, bq, gk, bk, cos_row, sin_row, k_past, v_past, key_valid, rot, eps, scale):
    """One cached Persimmon decode step (otter_persimmon_decode_attn).  qkv [B,H,3,64] bf16 contiguous (the new token's projection, per
    head q|k|v); gq / bq / gk / bk fp32 [64]; cos_row / sin_row fp32 [rot] (position S_past); k_past / v_past bf16 [B,H,S_past,64] with a
    unit dim stride and strides that are multiples of 8 (read only); key_valid uint8 [B,S_past+1] or None.
    Returns (o [B,H*64], k_new [B,H,S_past+1,64], v_new [B,H,S_past+1,64]), all bf16 and freshly allocated."""
    K.require_cuda(qkv, gq, bq, gk, bk, cos_row, sin_row, k_past, v_past, key_valid)
    args, ret = _persimmon_decode_args(qkv, gq, bq, gk, bk, cos_row, sin_row, k_past, v_past, key_valid, rot, eps, scale)
    K.check(K.lib().otter_persimmon_decode_attn(*args, K.stream()), "persimmon_decode_attn")
    return ret


def _persimmon_decode_args(qkv, gq, bq, gk, bk, cos_row, sin_row, k_past, v_past, key_valid, rot, eps, scale):
    name = "persimmon_decode_attn"
    if qkv.dtype != torch.bfloat16 or qkv.dim() != 4 or qkv.shape[2:] != (3, 64) or not qkv.is_contiguous():
        raise K.OtterHipError("persimmon_decode_attn: qkv must be contiguous bf16 [B,H,3,64]")
    B, H = qkv.shape[:2]
    S_past = k_past.shape[2] if k_past.dim() == 4 else -1
    if S_past < 1 or S_past + 1 > PERSIMMON_DECODE_MAX_KEYS:
        raise K.OtterHipError(f"persimmon_decode_attn: past length {S_past} outside [1, {PERSIMMON_DECODE_MAX_KEYS - 1}]")
    if not _decode_past_ok(k_past, B, H, S_past) or not _decode_past_ok(v_past, B, H, S_past):
        raise K.OtterHipError("persimmon_decode_attn: k_past / v_past must be bf16 [B,H,S_past,64], unit dim stride, strides % 8 == 0, 16-B aligned")
    _check_norm_rot(name, gq, bq, gk, bk, rot)
    _check_rotary_rows_64(name, cos_row, sin_row, rot)
    Sk = S_past + 1
    if key_valid is not None and (key_valid.dtype != torch.uint8 or not key_valid.is_contiguous() or tuple(key_valid.shape) != (B, Sk)):
        raise K.OtterHipError("persimmon_decode_attn: key_valid must be contiguous uint8 [B,S_past+1]")
    k_new = torch.empty((B, H, Sk, 64), dtype=torch.bfloat16, device=qkv.device)
    v_new = torch.empty_like(k_new)
    o = torch.empty((B, H * 64), dtype=torch.bfloat16, device=qkv.device)
    ws = _ws.get(persimmon_decode_workspace_bytes(B, H, Sk), qkv.device)
    return (qkv.data_ptr(), gq.data_ptr(), bq.data_ptr(), gk.data_ptr(), bk.data_ptr(), cos_row.data_ptr(), sin_row.data_ptr(),
            k_past.data_ptr(), k_past.stride(0), k_past.stride(1), k_past.stride(2), k_past.stride(3), v_past.data_ptr(), v_past.stride(0),
            v_past.stride(1), v_past.stride(2), v_past.stride(3), K.ptr(key_valid), k_new.data_ptr(), v_new.data_ptr(), o.data_ptr(),
            ws.data_ptr(), ws.numel(), B, H, S_past, 64, int(rot), float(eps), float(scale)), (o, k_new, v_new)


def _persimmon_cached_args(name, dyn, qkv, gq, bq, gk, bk, cos, sin, k_cache, v_cache, pos, rot, eps, scale, src, key_valid, out):
    """The two static-cache entry points at head_dim 64, from tensors to (the library's arguments up to the stream, o) or an OtterHipError.
    `dyn`: `pos` is pos_dev, cos / sin are the tables, and src / key_valid must cover every position."""
    N, H = _check_qkv_64(name, qkv)
    S_max = _check_caches(name, k_cache, v_cache, N, H, torch.bfloat16, 64, 8)
    _check_s_max(name, S_max, PERSIMMON_DECODE_MAX_KEYS)
    _check_norm_rot(name, gq, bq, gk, bk, rot)
    if dyn:
        _check_pos_dev(name, pos)
        rotary = (cos.data_ptr(), sin.data_ptr(), _check_rotary_tables(name, cos, sin, S_max, rot, "rot", False))
        keys, pos = S_max, pos.data_ptr()
    else:
        keys = pos = _check_pos(name, pos, S_max)
        keys += 1
        _check_rotary_rows_64(name, cos, sin, rot)
        rotary = (cos.data_ptr(), sin.data_ptr())
    src_rs = _check_rows(name, src, "src", torch.int32, N, keys - 1, "S_max - 1" if dyn else "pos", True)
    kv_rs = _check_rows(name, key_valid, "key_valid", torch.uint8, N, keys, "S_max" if dyn else "pos+1", True)
    o = _out_or_new(name, out, N, H, 64, qkv.device)
    ws = _ws.get(persimmon_decode_cached_workspace_bytes(N, H, keys), qkv.device)
    return (qkv.data_ptr(), gq.data_ptr(), bq.data_ptr(), gk.data_ptr(), bk.data_ptr(), *rotary, k_cache.data_ptr(), k_cache.stride(0),
            k_cache.stride(1), v_cache.data_ptr(), v_cache.stride(0), v_cache.stride(1), K.ptr(src), src_rs, K.ptr(key_valid), kv_rs,
            o.data_ptr(), ws.data_ptr(), ws.numel(), N, H, pos, S_max, 64, int(rot), float(eps), float(scale)), o


def persimmon_decode_attn_cached(qkv, gq, bq, gk, bk, cos_row, sin_row, k_cache, v_cache, pos, rot, eps, scale, src=None, key_valid=None):
    """One cached Persimmon decode step over a static cache (otter_persimmon_decode_attn_cached).  qkv [N,H,3,64] bf16 contiguous; gq / bq /
    gk / bk fp32 [64]; cos_row / sin_row fp32 [rot] (position `pos`); k_cache / v_cache bf16 [N,H,S_max,64] with key stride 64, written in
    place at slot `pos` (1 <= pos < S_max) of every row; src int32 [N, >= pos] (row stride free) or None; key_valid uint8 [N, >= pos+1] or
    None.  Returns o [N,H*64] bf16."""
    K.require_cuda(qkv, gq, bq, gk, bk, cos_row, sin_row, k_cache, v_cache, src, key_valid)
    args, o = _persimmon_cached_args("persimmon_decode_attn_cached", False, qkv, gq, bq, gk, bk, cos_row, sin_row, k_cache, v_cache, pos, rot,
                                     eps, scale, src, key_valid, None)
    K.check(K.lib().otter_persimmon_decode_attn_cached(*args, K.stream()), "persimmon_decode_attn_cached")
    return o


def persimmon_decode_attn_cached_dyn(qkv, gq, bq, gk, bk, cos_table, sin_table, k_cache, v_cache, pos_dev, rot, eps, scale, src=None,
                                     key_valid=None, out=None):
    """persimmon_decode_attn_cached with the position in device memory (otter_persimmon_decode_attn_cached_dyn): pos_dev int32 [1] on the
    device, read by the kernel (a value outside [1, S_max) makes the call a no-op); cos_table / sin_table fp32 [>= S_max, rot] (the kernel
    takes row pos); src int32 [N, >= S_max - 1]; key_valid uint8 [N, >= S_max].  No argument of the launch depends on the position: the same
    call, captured in a graph, serves every step.  Returns o [N,H*64] bf16 (`out`: a contiguous bf16 [N,H*64] tensor to write instead)."""
    K.require_cuda(qkv, gq, bq, gk, bk, cos_table, sin_table, k_cache, v_cache, pos_dev, src, key_valid, out)
    args, o = _persimmon_cached_args("persimmon_decode_attn_cached_dyn", True, qkv, gq, bq, gk, bk, cos_table, sin_table, k_cache, v_cache,
                                     pos_dev, rot, eps, scale, src, key_valid, out)
    K.check(K.lib().otter_persimmon_decode_attn_cached_dyn(*args, K.stream()), "persimmon_decode_attn_cached_dyn")
    return o


def _decode_cached_args(name, dyn, q, k_new, v_new, k_cache, v_cache, scales, pos, scale, cos, sin, src, key_valid, slopes, out):
    """The four static-cache entry points at head_dim 128, from tensors to (the library's arguments up to the stream, o) or an OtterHipError.
    `scales`: (k_scale, v_scale) of an int8 cache, None for a bf16 one; `dyn`: `pos` is pos_dev, cos / sin are the tables, src / key_valid
    must cover every position and their row stride is checked here (the position-scalar forms leave it to the library)."""
    i8 = scales is not None
    N, H = _check_new_128(name, q, k_new, v_new)
    S_max = _check_caches(name, k_cache, v_cache, N, H, torch.int8 if i8 else torch.bfloat16, 128, 16 if i8 else 8)
    if i8:
        _check_scales(name, scales[0], scales[1], N, H, S_max)
        _check_slopes(name, slopes, H)                  # (the bf16 entry points check slopes after key_valid)
    if dyn:
        _check_s_max(name, S_max, DECODE_CACHED_MAX_KEYS)
        _check_pos_dev(name, pos)
        rot_stride = _check_rotary_tables(name, cos, sin, S_max, 128, "128", True)
        keys, pos = S_max, pos.data_ptr()
    else:
        keys = pos = _check_pos(name, pos, S_max, DECODE_CACHED_MAX_KEYS)
        keys += 1
        rot_stride = _check_rotary_rows_128(name, cos, sin, N)
    src_rs = _check_rows(name, src, "src", torch.int32, N, keys - 1, "S_max - 1" if dyn else "pos", dyn)
    kv_rs = _check_rows(name, key_valid, "key_valid", torch.uint8, N, keys, "S_max" if dyn else "pos+1", dyn)
    if not i8:
        _check_slopes(name, slopes, H)
    o = _out_or_new(name, out, N, H, 128, q.device)
    ws = _ws.get(decode_attn_cached_workspace_bytes(N, H, keys), q.device)
    caches = (k_cache.data_ptr(), k_cache.stride(0), k_cache.stride(1), v_cache.data_ptr(), v_cache.stride(0), v_cache.stride(1))
    if i8:
        ks, vs = scales
        caches += (ks.data_ptr(), ks.stride(0), ks.stride(1), vs.data_ptr(), vs.stride(0), vs.stride(1))
    return (q.data_ptr(), q.stride(0), q.stride(1), k_new.data_ptr(), k_new.stride(0), k_new.stride(1), v_new.data_ptr(), v_new.stride(0),
            v_new.stride(1), K.ptr(cos), K.ptr(sin), rot_stride, *caches, K.ptr(src), src_rs, K.ptr(key_valid), kv_rs, K.ptr(slopes),
            o.data_ptr(), ws.data_ptr(), ws.numel(), N, H, pos, S_max, 128, float(scale)), o


def decode_attn_cached(q, k_new, v_new, k_cache, v_cache, pos, scale, cos=None, sin=None, src=None, key_valid=None, slopes=None):
    """One cached decode step over a static cache (otter_decode_attn_cached).  q / k_new / v_new bf16 [N,H,128] views (unit dim stride,
    strides % 8 == 0, 16-B aligned: slices of a fused projection row or separate projection outputs, read in place); k_cache / v_cache bf16
    [N,H,S_max,128] with key stride 128, written in place at slot `pos` (1 <= pos < S_max) of every row; cos / sin fp32 [128] or [N,128]
    rows of position `pos` (both or neither: rotate_half rotary on q and k_new); src int32 [N, >= pos] (row stride free) or None;
    key_valid uint8 [N, >= pos+1] or None; slopes fp32 [H] or None.  Returns o [N,H*128] bf16."""
    K.require_cuda(q, k_new, v_new, k_cache, v_cache, cos, sin, src, key_valid, slopes)
    args, o = _decode_cached_args("decode_attn_cached", False, q, k_new, v_new, k_cache, v_cache, None, pos, scale, cos, sin, src, key_valid,
                                  slopes, None)
    K.check(K.lib().otter_decode_attn_cached(*args, K.stream()), "decode_attn_cached")
    return o


def decode_attn_cached_dyn(q, k_new, v_new, k_cache, v_cache, pos_dev, scale, cos_table=None, sin_table=None, src=None, key_valid=None, slopes=None,
                           out=None):
    """decode_attn_cached with the position in device memory (otter_decode_attn_cached_dyn): pos_dev int32 [1] on the device, read by the
    kernel (a value outside [1, S_max) makes the call a no-op); cos_table / sin_table fp32 [>= S_max, 128] (the kernel takes row pos) or
    None; src int32 [N, >= S_max - 1]; key_valid uint8 [N, >= S_max].  No argument of the launch depends on the position: the same call,
    captured in a graph, serves every step.  Everything else as decode_attn_cached.  Returns o [N,H*128] bf16 (`out`: a contiguous bf16
    [N,H*128] tensor to write instead)."""
    K.require_cuda(q, k_new, v_new, k_cache, v_cache, pos_dev, cos_table, sin_table, src, key_valid, slopes, out)
    args, o = _decode_cached_args("decode_attn_cached_dyn", True, q, k_new, v_new, k_cache, v_cache, None, pos_dev, scale, cos_table, sin_table,
                                  src, key_valid, slopes, out)
    K.check(K.lib().otter_decode_attn_cached_dyn(*args, K.stream()), "decode_attn_cached_dyn")
    return o


def decode_attn_cached_i8(q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, pos, scale, cos=None, sin=None, src=None, key_valid=None,
                          slopes=None):
    """decode_attn_cached over an int8 cache (otter_decode_attn_cached_i8): k_cache / v_cache int8 codes [N,H,S_max,128] (key stride 128,
    strides % 16 == 0, 16-B aligned) and k_scale / v_scale fp32 [N,H,S_max] (unit key stride), all four written in place at slot `pos`
    with the quantised new token, which is attended in its dequantised form.  Everything else as decode_attn_cached.
    Returns o [N,H*128] bf16."""
    K.require_cuda(q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, cos, sin, src, key_valid, slopes)
    args, o = _decode_cached_args("decode_attn_cached_i8", False, q, k_new, v_new, k_cache, v_cache, (k_scale, v_scale), pos, scale, cos, sin,
                                  src, key_valid, slopes, None)
    K.check(K.lib().otter_decode_attn_cached_i8(*args, K.stream()), "decode_attn_cached_i8")
    return o


def decode_attn_cached_i8_dyn(q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, pos_dev, scale, cos_table=None, sin_table=None, src=None,
                              key_valid=None, slopes=None, out=None):
    """decode_attn_cached_dyn over an int8 cache (otter_decode_attn_cached_i8_dyn): the caches and scales of decode_attn_cached_i8, every
    other argument as decode_attn_cached_dyn.  Returns o [N,H*128] bf16 (`out`: a contiguous bf16 [N,H*128] tensor to write instead)."""
    K.require_cuda(q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, pos_dev, cos_table, sin_table, src, key_valid, slopes, out)
    args, o = _decode_cached_args("decode_attn_cached_i8_dyn", True, q, k_new, v_new, k_cache, v_cache, (k_scale, v_scale), pos_dev, scale,
                                  cos_table, sin_table, src, key_valid, slopes, out)
    K.check(K.lib().otter_decode_attn_cached_i8_dyn(*args, K.stream()), "decode_attn_cached_i8_dyn")
    return o


DECODE_CACHED_SHARED_GROUPS = (2, 3, 4, 5, 6)     # include/otter_hip.h: 2 .. OTTER_DECODE_CACHED_SHARED_MAX_GROUP, one kernel instance each

decode_attn_cached_shared_workspace_bytes = decode_attn_cached_shared_dyn_workspace_bytes = decode_attn_cached_workspace_bytes


def _check_shared(name, dyn, N, group, shared_len, pos, S_max):
    """The grouping of the shared-prompt entry points: `group` rows per sentence, `shared_len` leading keys read from the sentence's first
    row.  `pos`: the position scalar (ignored with `dyn`).  Returns (group, shared_len) as ints."""
    group, shared_len = int(group), int(shared_len)
    if group not in DECODE_CACHED_SHARED_GROUPS:
        raise K.OtterHipError(f"{name}: group={group}: the kernel is built for groups of {DECODE_CACHED_SHARED_GROUPS[0]} to "
                              f"{DECODE_CACHED_SHARED_GROUPS[-1]} rows")
    if N % group:
        raise K.OtterHipError(f"{name}: N={N} rows are not whole groups of {group}")
    if dyn:
        if shared_len < 1 or shared_len >= S_max:
            raise K.OtterHipError(f"{name}: shared_len={shared_len} outside [1, S_max) with S_max={S_max}")
    elif shared_len < 1 or shared_len > pos:
        raise K.OtterHipError(f"{name}: shared_len={shared_len} outside [1, pos] with pos={pos}")
    return group, shared_len


def decode_attn_cached_shared(q, k_new, v_new, k_cache, v_cache, pos, scale, group, shared_len, cos=None, sin=None, src=None, key_valid=None,
                              slopes=None):
    """decode_attn_cached for beam search over a shared prompt (otter_decode_attn_cached_shared): the N rows are sentences x `group` beams
    (contiguous), and keys [0, shared_len) of every beam are read from the sentence's first row, once for the whole group -- what
    decode_attn_cached returns for a table whose columns [0, shared_len) hold (n // group) * group; columns < shared_len of `src` are not
    read.  group in DECODE_CACHED_SHARED_GROUPS, N % group == 0, 1 <= shared_len <= pos.  Everything else as decode_attn_cached.
    Returns o [N,H*128] bf16."""
    K.require_cuda(q, k_new, v_new, k_cache, v_cache, cos, sin, src, key_valid, slopes)
    name = "decode_attn_cached_shared"
    args, o = _decode_cached_args(name, False, q, k_new, v_new, k_cache, v_cache, None, pos, scale, cos, sin, src, key_valid, slopes, None)
    grouping = _check_shared(name, False, q.shape[0], group, shared_len, int(pos), k_cache.shape[2])
    K.check(K.lib().otter_decode_attn_cached_shared(*args, *grouping, K.stream()), name)
    return o


def decode_attn_cached_shared_dyn(q, k_new, v_new, k_cache, v_cache, pos_dev, scale, group, shared_len, cos_table=None, sin_table=None, src=None,
                                  key_valid=None, slopes=None, out=None):
    """decode_attn_cached_shared with the position in device memory (otter_decode_attn_cached_shared_dyn): every argument but `group` and
    `shared_len` as decode_attn_cached_dyn; 1 <= shared_len < S_max, a host scalar that stays the same over a generate() call (a position
    below it, like one outside [1, S_max), makes the call a no-op).  Returns o [N,H*128] bf16 (`out`: a contiguous bf16 [N,H*128] tensor
    to write instead)."""
    K.require_cuda(q, k_new, v_new, k_cache, v_cache, pos_dev, cos_table, sin_table, src, key_valid, slopes, out)
    name = "decode_attn_cached_shared_dyn"
    args, o = _decode_cached_args(name, True, q, k_new, v_new, k_cache, v_cache, None, pos_dev, scale, cos_table, sin_table, src, key_valid,
                                  slopes, out)
    grouping = _check_shared(name, True, q.shape[0], group, shared_len, None, k_cache.shape[2])
    K.check(K.lib().otter_decode_attn_cached_shared_dyn(*args, *grouping, K.stream()), name)
    return o


# csrc/decode_cache_shared_i8.hip: every group size of DECODE_CACHED_SHARED_GROUPS has an instance (none was left on the table path)
DECODE_CACHED_SHARED_I8_GROUPS = DECODE_CACHED_SHARED_GROUPS

decode_attn_cached_shared_i8_workspace_bytes = decode_attn_cached_shared_i8_dyn_workspace_bytes = decode_attn_cached_workspace_bytes


def decode_attn_cached_shared_i8(q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, pos, scale, group, shared_len, cos=None, sin=None, src=None,
                                 key_valid=None, slopes=None):
    """decode_attn_cached_i8 for beam search over a shared prompt (otter_decode_attn_cached_shared_i8): the grouping of
    decode_attn_cached_shared over the int8 cache.  Keys [0, shared_len) of every beam are read from the sentence's first row -- codes and
    scales, once for the whole group, dequantised once -- what decode_attn_cached_i8 returns for a table whose columns [0, shared_len) hold
    (n // group) * group; columns < shared_len of `src` and the other rows' codes and scales [0, shared_len) are not read.
    group in DECODE_CACHED_SHARED_I8_GROUPS, N % group == 0, 1 <= shared_len <= pos.  Everything else as decode_attn_cached_i8.
    Returns o [N,H*128] bf16."""
    K.require_cuda(q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, cos, sin, src, key_valid, slopes)
    name = "decode_attn_cached_shared_i8"
    args, o = _decode_cached_args(name, False, q, k_new, v_new, k_cache, v_cache, (k_scale, v_scale), pos, scale, cos, sin, src, key_valid, slopes,
                                  None)
    grouping = _check_shared(name, False, q.shape[0], group, shared_len, int(pos), k_cache.shape[2])
    K.check(K.lib().otter_decode_attn_cached_shared_i8(*args, *grouping, K.stream()), name)
    return o


def decode_attn_cached_shared_i8_dyn(q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, pos_dev, scale, group, shared_len, cos_table=None,
                                     sin_table=None, src=None, key_valid=None, slopes=None, out=None):
    """decode_attn_cached_shared_i8 with the position in device memory (otter_decode_attn_cached_shared_i8_dyn): every argument but `group`
    and `shared_len` as decode_attn_cached_i8_dyn; 1 <= shared_len < S_max, a host scalar that stays the same over a generate() call (a
    position below it, like one outside [1, S_max), makes the call a no-op).  Returns o [N,H*128] bf16 (`out`: a contiguous bf16 [N,H*128]
    tensor to write instead)."""
    K.require_cuda(q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, pos_dev, cos_table, sin_table, src, key_valid, slopes, out)
    name = "decode_attn_cached_shared_i8_dyn"
    args, o = _decode_cached_args(name, True, q, k_new, v_new, k_cache, v_cache, (k_scale, v_scale), pos_dev, scale, cos_table, sin_table, src,
                                  key_valid, slopes, out)
    grouping = _check_shared(name, True, q.shape[0], group, shared_len, None, k_cache.shape[2])
    K.check(K.lib().otter_decode_attn_cached_shared_i8_dyn(*args, *grouping, K.stream()), name)
    return o


BRANCH_ATTN_MAX_T = 64                # include/otter_hip.h: OTTER_BRANCH_ATTN_MAX_T, one lane of a wave per own key


def _branch_attn_args(q, k_new, v_new, o1, lse1, scale, T, rows_per_sentence, slopes, out):
    """otter_branch_attn_merge, from tensors to (the library's arguments up to the stream, o) or an OtterHipError.  Like the cached-decode
    checkers it looks at dtype, shape, strides and alignment only, so it runs on CPU tensors (tests/test_branch_attn_abi.py)."""
    name = "branch_attn_merge"
    N, H = _check_new_128(name, q, k_new, v_new)
    T, rps = int(T), int(rows_per_sentence)
    if T < 1 or T > BRANCH_ATTN_MAX_T:
        raise K.OtterHipError(f"{name}: T={T} outside [1, {BRANCH_ATTN_MAX_T}]")
    if N < 1 or N % T:
        raise K.OtterHipError(f"{name}: N={N} rows are not whole candidates of T={T}")
    if rps < T or rps % T or N % rps:
        raise K.OtterHipError(f"{name}: rows_per_sentence={rps} must be a multiple of T={T} that divides N={N}")
    if o1.dtype != torch.float32 or tuple(o1.shape) != (N, H, 128) or not o1.is_contiguous() or o1.data_ptr() % 16:
        raise K.OtterHipError(f"{name}: o1 must be a contiguous fp32 [N,H,128] tensor, 16-B aligned")
    if lse1.dtype != torch.float32 or tuple(lse1.shape) != (N // rps, H, rps) or not lse1.is_contiguous():
        raise K.OtterHipError(f"{name}: lse1 must be a contiguous fp32 [N / rows_per_sentence, H, rows_per_sentence] tensor")
    _check_slopes(name, slopes, H)
    if out is None:
        out = torch.empty((N, H, 128), dtype=torch.bfloat16, device=q.device)
    elif out.dtype != torch.bfloat16 or tuple(out.shape) != (N, H, 128) or not out.is_contiguous() or out.data_ptr() % 16:
        raise K.OtterHipError(f"{name}: out must be a contiguous bf16 [N,H,128] tensor, 16-B aligned")
    return (q.data_ptr(), q.stride(0), q.stride(1), k_new.data_ptr(), k_new.stride(0), k_new.stride(1), v_new.data_ptr(), v_new.stride(0),
            v_new.stride(1), o1.data_ptr(), lse1.data_ptr(), K.ptr(slopes), out.data_ptr(), N, H, T, rps, 128, float(scale)), out


def branch_attn_merge(q, k_new, v_new, o1, lse1, scale, T, rows_per_sentence, slopes=None, out=None):
    """The own-candidate half of branch attention and its merge with the prompt half (otter_branch_attn_merge, csrc/branch_attn.hip).
    Rows n = (b C + c) T + t.  q / k_new / v_new bf16 [N,H,128] views (unit dim stride, strides % 8 == 0, 16-B aligned: slices of the
    projection output, read in place); o1 fp32 [N,H,128] contiguous and lse1 fp32 [B,H,C*T]: what `flash_attn_fwd_f32(q.view(B, C*T, H, 128),
    prompt keys, prompt values, slopes, key_valid, scale, causal=False)` returns; rows_per_sentence = C * T; slopes fp32 [H] or None.
    Returns o [N,H,128] bf16 (`out`: a contiguous bf16 [N,H,128] tensor to write instead)."""
    K.require_cuda(q, k_new, v_new, o1, lse1, slopes, out)
    args, o = _branch_attn_args(q, k_new, v_new, o1, lse1, scale, T, rows_per_sentence, slopes, out)
    K.check(K.lib().otter_branch_attn_merge(*args, K.stream()), "branch_attn_merge")
    return o


XATTN_DECODE_MAX_KEYS = 65536        # include/otter_hip.h: M = T_img * n_per_media <= 65536


def xattn_decode(q, k, v, H, text_time, n_per_media, rows_per_media, mask_mode, scale, out=None):
    """The masked cross-attention core of one cached step over a media cache (otter_xattn_decode).  q bf16 [N, H*64] (row stride free, % 8);
    k, v bf16 [sentences, M, H*64] views of one buffer (shared row stride % 8, sentence stride M * row stride; usually the two halves of a
    to_kv output); row r reads sentence r // rows_per_media; text_time int32 [N]; mask_mode EQ or GE.  Returns o [N, H*64] bf16 (`out`:
    a contiguous bf16 [N, H*64] tensor to write instead)."""
    K.require_cuda(q, k, v, text_time, out)
    if q.dim() != 2 or k.dim() != 3 or v.dim() != 3 or k.shape != v.shape:
        raise K.OtterHipError("xattn_decode: q must be [N, H*64], k and v [sentences, M, H*64] of equal shape")
    N, HD = q.shape
    S, M = k.shape[:2]
    n_per_media, rows_per_media = int(n_per_media), int(rows_per_media)
    if HD != H * 64 or k.shape[2] != HD:
        raise K.OtterHipError(f"xattn_decode: head_dim 64 only (q inner={HD}, k inner={k.shape[2]}, heads={H})")
    if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
        raise K.OtterHipError("xattn_decode: q, k, v must be bf16")
    if n_per_media < 1 or M < 1 or M % n_per_media != 0 or M > XATTN_DECODE_MAX_KEYS:
        raise K.OtterHipError(f"xattn_decode: M={M} must be a positive multiple of n_per_media={n_per_media}, at most {XATTN_DECODE_MAX_KEYS}")
    if rows_per_media < 1 or N != S * rows_per_media:
        raise K.OtterHipError(f"xattn_decode: N={N} rows need {S} sentences x rows_per_media={rows_per_media}")
    if q.stride(1) != 1 or k.stride(2) != 1 or v.stride(2) != 1 or k.stride(1) != v.stride(1) or q.stride(0) % 8 or k.stride(1) % 8:
        raise K.OtterHipError("xattn_decode: unit dim strides, a shared k / v row stride, row strides % 8 == 0")
    if q.stride(0) < HD or k.stride(1) < HD or (S > 1 and (k.stride(0) != M * k.stride(1) or v.stride(0) != M * v.stride(1))):
        raise K.OtterHipError("xattn_decode: row strides >= H*64 and a sentence stride of M * row stride")
    if q.data_ptr() % 16 or k.data_ptr() % 16 or v.data_ptr() % 16:
        raise K.OtterHipError("xattn_decode: q, k, v must be 16-byte aligned")
    if text_time.dtype != torch.int32 or tuple(text_time.shape) != (N,) or not text_time.is_contiguous():
        raise K.OtterHipError("xattn_decode: text_time must be contiguous int32 [N]")
    if mask_mode not in (MASK_EQ, MASK_GE):
        raise K.OtterHipError(f"xattn_decode: mask_mode {mask_mode} (EQ or GE only)")
    if out is None:
        out = torch.empty((N, HD), dtype=torch.bfloat16, device=q.device)
    elif out.dtype != torch.bfloat16 or tuple(out.shape) != (N, HD) or not out.is_contiguous():
        raise K.OtterHipError("xattn_decode: out must be a contiguous bf16 [N, H*64] tensor")
    K.check(K.lib().otter_xattn_decode(q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(1), text_time.data_ptr(), out.data_ptr(),
                                       N, H, M // n_per_media, n_per_media, rows_per_media, int(mask_mode), float(scale), K.stream()),
            "xattn_decode")
    return out


GEMV_W8_MAX_ROWS = 16                 # include/otter_hip.h: 1 <= M <= 16


def gemv_w8_workspace_bytes(M: int, N: int, K: int) -> int:
    """OTTER_GEMV_W8_WORKSPACE_BYTES of include/otter_hip.h."""
    return 8 * M * N * 4


def _w8_weight_ok(qweight, scale) -> bool:
    return (qweight.dtype == torch.int8 and qweight.dim() == 2 and qweight.stride(1) == 1 and qweight.stride(0) % 16 == 0
            and qweight.shape[1] % 16 == 0 and qweight.data_ptr() % 16 == 0 and scale.dtype == torch.float32 and scale.is_contiguous()
            and scale.numel() == qweight.shape[0])


def gemv_w8(x, qweight, scale, bias=None, act: int = 0, out_dtype=torch.bfloat16, out=None):
    """y [M, N] = (x [M, K] . qweight [N, K]^T) * scale [N] (+ bias), then `act` (0 none, 1 exact-erf GELU, 3 squared ReLU relu(v)^2 in
    fp32; no other code), 1 <= M <= 16 (otter_gemv_w8, csrc/w8.hip).  x bf16 with unit column stride, qweight int8 (row stride % 16 == 0), scale fp32 [N], bias bf16 / fp32 [N]
    or None; y bf16 or fp32 (`out`: a caller-owned [M, N] view with unit column stride, written in place)."""
    K.require_cuda(x, qweight, scale, bias, out)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
        raise K.OtterHipError("gemv_w8: x must be bf16 [M, K] with a unit column stride")
    if not _w8_weight_ok(qweight, scale):
        raise K.OtterHipError("gemv_w8: qweight int8 [N, K] (K % 16 == 0, row stride % 16 == 0, 16-B aligned), scale contiguous fp32 [N]")
    M, Kd = x.shape
    N = qweight.shape[0]
    if Kd != qweight.shape[1] or not 1 <= M <= GEMV_W8_MAX_ROWS:
        raise K.OtterHipError(f"gemv_w8: x {tuple(x.shape)} against qweight {tuple(qweight.shape)} (1 <= M <= {GEMV_W8_MAX_ROWS})")
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        raise K.OtterHipError("gemv_w8: bias must be contiguous [N]")
    y = torch.empty((M, N), dtype=out_dtype, device=x.device) if out is None else out
    if tuple(y.shape) != (M, N) or y.stride(1) != 1 or y.device != x.device:
        raise K.OtterHipError("gemv_w8: out must be [M, N] with a unit column stride on x's device")
    ldx, ldy = (x.stride(0), y.stride(0)) if M > 1 else (Kd, N)      # (the row stride of a one-row view is arbitrary)
    ws = _ws.get(gemv_w8_workspace_bytes(M, N, Kd), x.device)
    K.check(K.lib().otter_gemv_w8(x.data_ptr(), ldx, qweight.data_ptr(), qweight.stride(0), scale.data_ptr(), K.ptr(bias),
                                  K.dt(bias) if bias is not None else K.F32, y.data_ptr(), ldy, K.dt(y), M, N, Kd, int(act), ws.data_ptr(),
                                  ws.numel(), K.stream()), "gemv_w8")
    return y


GEMM_W8_ROWS_MAX_ROWS = 64            # include/otter_hip.h: 1 <= M <= 64


def gemm_w8_rows_workspace_bytes(M: int, N: int, K: int) -> int:
    """OTTER_GEMM_W8_ROWS_WORKSPACE_BYTES of include/otter_hip.h."""
    return 8 * M * N * 4


def gemm_w8_rows(x, qweight, scale, bias=None, act: int = 0, out_dtype=torch.bfloat16, out=None):
    """gemv_w8's product, arguments, `act` codes (0, 1, 3) and rules for 1 <= M <= 64 (otter_gemm_w8_rows, csrc/w8.hip): the one-token steps of 17 to 64 rows.
    Row m of the result has the same bits whatever M is and whatever the other rows of x hold."""
    K.require_cuda(x, qweight, scale, bias, out)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
        raise K.OtterHipError("gemm_w8_rows: x must be bf16 [M, K] with a unit column stride")
    if not _w8_weight_ok(qweight, scale):
        raise K.OtterHipError("gemm_w8_rows: qweight int8 [N, K] (K % 16 == 0, row stride % 16 == 0, 16-B aligned), scale contiguous fp32 [N]")
    M, Kd = x.shape
    N = qweight.shape[0]
    if Kd != qweight.shape[1] or not 1 <= M <= GEMM_W8_ROWS_MAX_ROWS:
        raise K.OtterHipError(f"gemm_w8_rows: x {tuple(x.shape)} against qweight {tuple(qweight.shape)} (1 <= M <= {GEMM_W8_ROWS_MAX_ROWS})")
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        raise K.OtterHipError("gemm_w8_rows: bias must be contiguous [N]")
    y = torch.empty((M, N), dtype=out_dtype, device=x.device) if out is None else out
    if tuple(y.shape) != (M, N) or y.stride(1) != 1 or y.device != x.device:
        raise K.OtterHipError("gemm_w8_rows: out must be [M, N] with a unit column stride on x's device")
    ldx, ldy = (x.stride(0), y.stride(0)) if M > 1 else (Kd, N)      # (the row stride of a one-row view is arbitrary)
    ws = _ws.get(gemm_w8_rows_workspace_bytes(M, N, Kd), x.device)
    K.check(K.lib().otter_gemm_w8_rows(x.data_ptr(), ldx, qweight.data_ptr(), qweight.stride(0), scale.data_ptr(), K.ptr(bias),
                                       K.dt(bias) if bias is not None else K.F32, y.data_ptr(), ldy, K.dt(y), M, N, Kd, int(act),
                                       ws.data_ptr(), ws.numel(), K.stream()), "gemm_w8_rows")
    return y


def _w8_gated(name, max_rows, x, qweight, scale, gate, R, bias, out_dtype, out):
    K.require_cuda(x, qweight, scale, gate, R, bias, out)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
        raise K.OtterHipError(f"{name}: x must be bf16 [M, K] with a unit column stride")
    if not _w8_weight_ok(qweight, scale):
        raise K.OtterHipError(f"{name}: qweight int8 [N, K] (K % 16 == 0, row stride % 16 == 0, 16-B aligned), scale contiguous fp32 [N]")
    M, Kd = x.shape
    N = qweight.shape[0]
    if Kd != qweight.shape[1] or not 1 <= M <= max_rows:
        raise K.OtterHipError(f"{name}: x {tuple(x.shape)} against qweight {tuple(qweight.shape)} (1 <= M <= {max_rows})")
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        raise K.OtterHipError(f"{name}: bias must be contiguous [N]")
    if gate is not None and (gate.dtype != torch.float32 or gate.numel() != 1):
        raise K.OtterHipError(f"{name}: gate must be one fp32 value on the device (or None)")
    if R is None or R.dtype not in (torch.bfloat16, torch.float32) or tuple(R.shape) != (M, N) or R.stride(1) != 1 or R.device != x.device:
        raise K.OtterHipError(f"{name}: R must be bf16 / fp32 [M, N] with a unit column stride on x's device")
    y = torch.empty((M, N), dtype=out_dtype, device=x.device) if out is None else out
    if tuple(y.shape) != (M, N) or y.stride(1) != 1 or y.device != x.device:
        raise K.OtterHipError(f"{name}: out must be [M, N] with a unit column stride on x's device")
    ldx, ldy, ldr = (x.stride(0), y.stride(0), R.stride(0)) if M > 1 else (Kd, N, N)      # (the row stride of a one-row view is arbitrary)
    ws = _ws.get(gemm_w8_panel_workspace_bytes(M, N, Kd) if max_rows == GEMM_W8_PANEL_MAX_ROWS else 8 * M * N * 4, x.device)
    K.check(getattr(K.lib(), "otter_" + name)(x.data_ptr(), ldx, qweight.data_ptr(), qweight.stride(0), scale.data_ptr(), K.ptr(bias),
                                              K.dt(bias) if bias is not None else K.F32, y.data_ptr(), ldy, K.dt(y), M, N, Kd, K.ptr(gate),
                                              R.data_ptr(), ldr, K.dt(R), ws.data_ptr(), ws.numel(), K.stream()), name)
    return y


def gemv_w8_gated(x, qweight, scale, gate, R, bias=None, out_dtype=torch.bfloat16, out=None):
    """y [M, N] = v * tanh(gate) + R, v = (x [M, K] . qweight [N, K]^T) * scale [N] (+ bias), in fp32 and rounded once, 1 <= M <= 16
    (otter_gemv_w8_gated, csrc/w8.hip): the second FFN product of a gated cross-attention block with its tanh-gate residual.  gate: one fp32
    value on the device, or None (y = v + R); R bf16 / fp32 [M, N] with a unit column stride, not overlapping y.  The rest as gemv_w8."""
    return _w8_gated("gemv_w8_gated", GEMV_W8_MAX_ROWS, x, qweight, scale, gate, R, bias, out_dtype, out)


def gemm_w8_rows_gated(x, qweight, scale, gate, R, bias=None, out_dtype=torch.bfloat16, out=None):
    """gemv_w8_gated for 1 <= M <= 64 (otter_gemm_w8_rows_gated): row m of the result has the same bits whatever M is and whatever the other
    rows of x and R hold."""
    return _w8_gated("gemm_w8_rows_gated", GEMM_W8_ROWS_MAX_ROWS, x, qweight, scale, gate, R, bias, out_dtype, out)


GEMM_W8_PANEL_MAX_ROWS = 256          # include/otter_hip.h: 1 <= M <= 256


def gemm_w8_panel_workspace_bytes(M: int, N: int, K: int) -> int:
    """OTTER_GEMM_W8_PANEL_WORKSPACE_BYTES of include/otter_hip.h: at most min(8, 256 // ceil(N / 128)) K ranges (at least 1)."""
    return min(8, max(1, 256 // ((N + 127) // 128))) * M * N * 4


def gemm_w8_panel(x, qweight, scale, bias=None, act: int = 0, out_dtype=torch.bfloat16, out=None):
    """gemv_w8's product, arguments, `act` codes (0, 1, 3) and rules for 1 <= M <= 256 (otter_gemm_w8_panel, csrc/w8_panel.hip): the one-token
    steps of 65 to 256 rows.  Row m of the result has the same bits whatever M is, whatever the other rows of x hold and wherever it sits."""
    name = "gemm_w8_panel"
    K.require_cuda(x, qweight, scale, bias, out)
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
        raise K.OtterHipError(f"{name}: x must be bf16 [M, K] with a unit column stride")
    if not _w8_weight_ok(qweight, scale):
        raise K.OtterHipError(f"{name}: qweight int8 [N, K] (K % 16 == 0, row stride % 16 == 0, 16-B aligned), scale contiguous fp32 [N]")
    M, Kd = x.shape
    N = qweight.shape[0]
    if Kd != qweight.shape[1] or not 1 <= M <= GEMM_W8_PANEL_MAX_ROWS:
        raise K.OtterHipError(f"{name}: x {tuple(x.shape)} against qweight {tuple(qweight.shape)} (1 <= M <= {GEMM_W8_PANEL_MAX_ROWS})")
    if bias is not None and (bias.numel() != N or not bias.is_contiguous()):
        raise K.OtterHipError(f"{name}: bias must be contiguous [N]")
    y = torch.empty((M, N), dtype=out_dtype, device=x.device) if out is None else out
    if tuple(y.shape) != (M, N) or y.stride(1) != 1 or y.device != x.device:
        raise K.OtterHipError(f"{name}: out must be [M, N] with a unit column stride on x's device")
    ldx, ldy = (x.stride(0), y.stride(0)) if M > 1 else (Kd, N)      # (the row stride of a one-row view is arbitrary)
    ws = _ws.get(gemm_w8_panel_workspace_bytes(M, N, Kd), x.device)
    K.check(K.lib().otter_gemm_w8_panel(x.data_ptr(), ldx, qweight.data_ptr(), qweight.stride(0), scale.data_ptr(), K.ptr(bias),
                                        K.dt(bias) if bias is not None else K.F32, y.data_ptr(), ldy, K.dt(y), M, N, Kd, int(act),
                                        ws.data_ptr(), ws.numel(), K.stream()), name)
    return y


def gemm_w8_panel_gated(x, qweight, scale, gate, R, bias=None, out_dtype=torch.bfloat16, out=None):
    """gemv_w8_gated for 1 <= M <= 256 (otter_gemm_w8_panel_gated), with gemm_w8_panel's independence of row m from M and from the other
    rows of x and R."""
    return _w8_gated("gemm_w8_panel_gated", GEMM_W8_PANEL_MAX_ROWS, x, qweight, scale, gate, R, bias, out_dtype, out)


def dequant_w8(qweight, scale, out=None):
    """out [N, K] bf16 = bf16(float(qweight) * scale[:, None]) (otter_dequant_w8, csrc/w8.hip); `out`: a caller-owned bf16 [N, K] view with
    unit column stride and a row stride that is a multiple of 8."""
    K.require_cuda(qweight, scale, out)
    if not _w8_weight_ok(qweight, scale):
        raise K.OtterHipError("dequant_w8: qweight int8 [N, K] (K % 16 == 0, row stride % 16 == 0, 16-B aligned), scale contiguous fp32 [N]")
    N, Kd = qweight.shape
    if out is None:
        out = torch.empty((N, Kd), dtype=torch.bfloat16, device=qweight.device)
    if out.dtype != torch.bfloat16 or tuple(out.shape) != (N, Kd) or out.stride(1) != 1 or out.device != qweight.device:
        raise K.OtterHipError("dequant_w8: out must be bf16 [N, K] with a unit column stride on qweight's device")
    K.check(K.lib().otter_dequant_w8(qweight.data_ptr(), qweight.stride(0), scale.data_ptr(), out.data_ptr(), out.stride(0), N, Kd, K.stream()),
            "dequant_w8")
    return out


LOGITS_PROCESS_MAX_VOCAB = 262144     # include/otter_hip.h: the V-bit ownership bitmap of otter_logits_process


def _i32_list(name, t, device, op="logits_process"):
    """(pointer, length) of an optional contiguous int32 1-d list on `device`; `op` names the operator in the error."""
    if t is None or t.numel() == 0:
        return None, 0
    if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != device:
        raise K.OtterHipError(f"{op}: {name} must be a contiguous int32 1-d tensor on the scores' device")
    return t.data_ptr(), t.numel()


def logits_process(scores, ids, repetition_penalty=1.0, no_repeat_ngram=0, ban=None, eos=None, suppress_eos=False, word_tokens=None,
                   word_offsets=None):
    """The logits processors of generate() in one launch, IN PLACE on scores fp32 [N, V] (unit column stride, V <= LOGITS_PROCESS_MAX_VOCAB)
    from the token history ids int64 [N, L] on the same device (otter_logits_process, csrc/logits.hip): repetition penalty (1 = off), no-repeat
    n-gram (0 = off), the always-banned int32 list `ban`, the multi-token bad words (`word_tokens` int32 flat, `word_offsets` int32
    [words + 1]) and the int32 `eos` list when `suppress_eos`.  Nothing here synchronises.  Returns scores."""
    K.require_cuda(scores, ids, ban, eos, word_tokens, word_offsets)
    if scores.dim() != 2 or ids.dim() != 2 or scores.shape[0] != ids.shape[0] or scores.device != ids.device:
        raise K.OtterHipError("logits_process: scores [N, V] and ids [N, L] of equal N on one device")
    if scores.dtype != torch.float32 or ids.dtype != torch.int64 or scores.stride(1) != 1 or ids.stride(1) != 1:
        raise K.OtterHipError("logits_process: scores fp32 and ids int64, both with a unit column stride")
    N, V = scores.shape
    L = ids.shape[1]
    if N < 1 or L < 1 or not 1 <= V <= LOGITS_PROCESS_MAX_VOCAB:
        raise K.OtterHipError(f"logits_process: N={N}, L={L} must be >= 1 and V={V} within 1..{LOGITS_PROCESS_MAX_VOCAB}")
    dev = scores.device
    ban_p, n_ban = _i32_list("ban", ban, dev)
    eos_p, n_eos = _i32_list("eos", eos, dev)
    tok_p, _ = _i32_list("word_tokens", word_tokens, dev)
    off_p, n_off = _i32_list("word_offsets", word_offsets, dev)
    if (tok_p is None) != (off_p is None) or n_off == 1:
        raise K.OtterHipError("logits_process: word_tokens and word_offsets (int32 [words + 1]) are given together or not at all")
    s_rs = scores.stride(0) if N > 1 else max(scores.stride(0), V)      # (the row stride of a one-row view is arbitrary)
    i_rs = ids.stride(0) if N > 1 else max(ids.stride(0), L)
    K.check(K.lib().otter_logits_process(scores.data_ptr(), s_rs, ids.data_ptr(), i_rs, N, V, L, float(repetition_penalty), int(no_repeat_ngram),
                                         ban_p, n_ban, eos_p, n_eos, int(bool(suppress_eos)), tok_p, off_p, max(n_off - 1, 0), K.stream()),
            "logits_process")
    return scores


BEAM_STEP_MAX_CANDIDATES = 64         # include/otter_hip.h: OTTER_BEAM_STEP_MAX_CANDIDATES, the candidates one wave of otter_beam_step ranks


def beam_step_workspace_bytes(B, nb, V, n_cand):
    """The workspace otter_beam_step needs for B sentences of nb beams over V tokens with n_cand candidates (host arithmetic only)."""
    n = K.lib().otter_beam_step_workspace_bytes(int(B), int(nb), int(V), int(n_cand))
    if n < 0:
        raise K.OtterHipError(f"beam_step: B={B}, nb={nb}, V={V}, n_cand={n_cand} out of range (n_cand <= {BEAM_STEP_MAX_CANDIDATES})")
    return n


def beam_step(logp, beam_scores, ids, ids_next, beam_idx, eos, pad_token_id, nb, n_cand, L0, max_len, early_stopping, length_penalty_positive,
              len_pow, done, hyp_score, hyp_tokens, hyp_len, hyp_slot, hyp_count, hyp_worst, all_done, workspace):
    """One beam-search step in two launches (otter_beam_step, csrc/beam.hip; include/otter_hip.h states the semantics and the tie rule): from
    logp fp32 [B * nb, V] (unit column stride), beam_scores fp32 [B * nb] (in and out) and ids int64 [B * nb, L], the n_cand best continuations
    per sentence, the scorer with its hypothesis state (hyp_* / done / all_done, the caller's buffers, updated in place) and the outputs
    ids_next int64 [B * nb, L + 1] (not overlapping ids) and beam_idx int64 [B * nb].  `eos`: int32 list tensor or None; `early_stopping`:
    True, False or "never".  Nothing here synchronises or allocates."""
    f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64
    state = (beam_scores, beam_idx, len_pow, done, hyp_score, hyp_tokens, hyp_len, hyp_slot, hyp_count, hyp_worst, all_done, workspace)
    K.require_cuda(logp, ids, ids_next, eos, *state)
    if logp.dim() != 2 or ids.dim() != 2 or ids_next.dim() != 2 or logp.shape[0] != ids.shape[0] or ids_next.shape[0] != ids.shape[0]:
        raise K.OtterHipError("beam_step: logp [N, V], ids [N, L] and ids_next [N, L + 1] of equal N")
    if logp.dtype != f32 or ids.dtype != i64 or ids_next.dtype != i64 or logp.stride(1) != 1 or ids.stride(1) != 1 or ids_next.stride(1) != 1:
        raise K.OtterHipError("beam_step: logp fp32, ids and ids_next int64, all with a unit column stride")
    N, V = logp.shape
    L = ids.shape[1]
    nb, n_cand, L0, max_len = int(nb), int(n_cand), int(L0), int(max_len)
    if nb < 1 or N < 1 or N % nb != 0 or ids_next.shape[1] != L + 1:
        raise K.OtterHipError(f"beam_step: N={N} rows must be a positive multiple of nb={nb}, and ids_next [N, L + 1 = {L + 1}]")
    B = N // nb
    dev = logp.device
    want = ((beam_scores, f32, N), (beam_idx, i64, N), (len_pow, f64, max_len - L0 + 1), (done, i32, B), (hyp_score, f64, N),
            (hyp_tokens, i64, N * max_len), (hyp_len, i32, N), (hyp_slot, i32, N), (hyp_count, i32, B), (hyp_worst, f64, B), (all_done, i32, 2))
    for t, dtype, numel in want:
        if t.dtype != dtype or t.numel() != numel or not t.is_contiguous() or t.device != dev:
            raise K.OtterHipError("beam_step: state and output buffers must be contiguous, on logp's device, of the dtypes and sizes "
                                  "include/otter_hip.h states (got %s of %d elements where %s of %d is needed)" % (t.dtype, t.numel(), dtype, numel))
    if ids.device != dev or ids_next.device != dev or workspace.device != dev or not workspace.is_contiguous():
        raise K.OtterHipError("beam_step: ids, ids_next and the workspace must be on logp's device (the workspace contiguous)")
    eos_p, n_eos = _i32_list("eos", eos, dev)
    early = 1 if early_stopping is True else 0 if early_stopping is False else 2
    lp_rs = logp.stride(0) if N > 1 else max(logp.stride(0), V)      # (the row stride of a one-row view is arbitrary)
    i_rs = ids.stride(0) if N > 1 else max(ids.stride(0), L)
    n_rs = ids_next.stride(0) if N > 1 else max(ids_next.stride(0), L + 1)
    K.check(K.lib().otter_beam_step(logp.data_ptr(), lp_rs, beam_scores.data_ptr(), ids.data_ptr(), i_rs, ids_next.data_ptr(), n_rs,
                                    beam_idx.data_ptr(), eos_p, n_eos, int(pad_token_id), B, nb, V, n_cand, L, L0, max_len, early,
                                    int(bool(length_penalty_positive)), len_pow.data_ptr(), done.data_ptr(), hyp_score.data_ptr(),
                                    hyp_tokens.data_ptr(), hyp_len.data_ptr(), hyp_slot.data_ptr(), hyp_count.data_ptr(), hyp_worst.data_ptr(),
                                    all_done.data_ptr(), workspace.data_ptr(), workspace.numel() * workspace.element_size(), K.stream()),
            "beam_step")
    return ids_next, beam_idx


SELECT_STEP_MAX_VOCAB = 262144        # include/otter_hip.h: OTTER_SELECT_STEP_MAX_VOCAB, the cap otter_logits_process has


def select_step(scores, ids_buf, L, unfinished, n_unfinished, eos=None, pad_token_id=0, sample=False, inv_temperature=1.0, top_k=0, top_p=1.0,
                q=None):
    """The step's token of every row in one launch (otter_select_step, csrc/select.hip; include/otter_hip.h states the rule and the tie
    rules): from scores fp32 [N, V] (unit column stride, V <= SELECT_STEP_MAX_VOCAB, never written) the row maximum, or with `sample` the
    draw under inv_temperature / top_k (0 = off) / top_p (1 = off) against the exponential draws q fp32 [N, V], written into column L of
    ids_buf int64 [N, max_len]; unfinished (bool or uint8 [N]) and n_unfinished (int32 [1]) are updated from the int32 `eos` list tensor (or
    None).  Nothing here synchronises or allocates.  Returns ids_buf."""
    K.require_cuda(scores, ids_buf, unfinished, n_unfinished, eos, q)
    if scores.dim() != 2 or ids_buf.dim() != 2 or scores.shape[0] != ids_buf.shape[0] or scores.device != ids_buf.device:
        raise K.OtterHipError("select_step: scores [N, V] and ids_buf [N, max_len] of equal N on one device")
    if scores.dtype != torch.float32 or ids_buf.dtype != torch.int64 or scores.stride(1) != 1 or ids_buf.stride(1) != 1:
        raise K.OtterHipError("select_step: scores fp32 and ids_buf int64, both with a unit column stride")
    N, V = scores.shape
    max_len, L = ids_buf.shape[1], int(L)
    if N < 1 or not 1 <= V <= SELECT_STEP_MAX_VOCAB or not 0 <= L < max_len:
        raise K.OtterHipError(f"select_step: N={N} must be >= 1, V={V} within 1..{SELECT_STEP_MAX_VOCAB} and L={L} within 0..max_len-1={max_len - 1}")
    dev = scores.device
    if (unfinished.dtype not in (torch.bool, torch.uint8) or unfinished.numel() != N or not unfinished.is_contiguous() or unfinished.device != dev
            or n_unfinished.dtype != torch.int32 or n_unfinished.numel() != 1 or n_unfinished.device != dev):
        raise K.OtterHipError("select_step: unfinished must be a contiguous bool / uint8 [N] and n_unfinished an int32 [1], on the scores' device")
    q_p, q_rs = None, 0
    if sample:
        if q is None or q.dtype != torch.float32 or tuple(q.shape) != (N, V) or q.stride(1) != 1 or q.device != dev:
            raise K.OtterHipError("select_step: sample mode needs q, fp32 [N, V] with a unit column stride on the scores' device")
        q_p, q_rs = q.data_ptr(), (q.stride(0) if N > 1 else max(q.stride(0), V))
    eos_p, n_eos = _i32_list("eos", eos, dev, "select_step")
    s_rs = scores.stride(0) if N > 1 else max(scores.stride(0), V)      # (the row stride of a one-row view is arbitrary)
    i_rs = ids_buf.stride(0) if N > 1 else max(ids_buf.stride(0), max_len)
    K.check(K.lib().otter_select_step(scores.data_ptr(), s_rs, N, V, ids_buf.data_ptr(), i_rs, L, max_len, 1 if sample else 0,
                                      float(inv_temperature), int(top_k), float(top_p), q_p, q_rs, unfinished.data_ptr(),
                                      n_unfinished.data_ptr(), eos_p, n_eos, int(pad_token_id), K.stream()), "select_step")
    return ids_buf


def qk_norm_rope_fwd(qkv, gq, bq, gk, bk, cos, sin, H, rot, eps, width=128, copy_v=True):
    """qkv [B,S,H*3*64] bf16 (per head q|k|v) -> q', k', v as [B,S,H,width] bf16, stats [B*S,H,2,2].  width 128: upper 64 columns zero
    (the 128-wide flash kernels); width 64: compact heads (the head-pair kernels), and with copy_v=False v is returned as the strided
    [B,S,H,64] view of qkv's v slots that those kernels read in place."""
    K.require_cuda(qkv, gq, bq, gk, bk, cos, sin)
    B, S, W = qkv.shape
    if qkv.dtype != torch.bfloat16 or not qkv.is_contiguous() or W != H * 3 * 64:
        raise K.OtterHipError("qk_norm_rope: contiguous bf16 [B,S,H*3*64]")
    if width not in (64, 128):
        raise K.OtterHipError("qk_norm_rope: width 64 or 128")
    for t in (gq, bq, gk, bk):
        if t.dtype != torch.float32 or t.numel() != 64 or not t.is_contiguous():
            raise K.OtterHipError("qk_norm_rope: gamma / beta must be contiguous fp32 [64]")
    if cos.dtype != torch.float32 or not cos.is_contiguous() or tuple(cos.shape) != (S, rot) or tuple(sin.shape) != (S, rot) or not sin.is_contiguous():
        raise K.OtterHipError("qk_norm_rope: cos / sin must be contiguous fp32 [S, rot]")
    q = torch.empty((B, S, H, width), dtype=torch.bfloat16, device=qkv.device)
    k = torch.empty_like(q)
    v = torch.empty_like(q) if copy_v else None
    stats = torch.empty((B * S, H, 2, 2), dtype=torch.float32, device=qkv.device)
    K.check(K.lib().otter_qk_norm_rope_fwd(qkv.data_ptr(), gq.data_ptr(), bq.data_ptr(), gk.data_ptr(), bk.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                           q.data_ptr(), k.data_ptr(), K.ptr(v), stats.data_ptr(), B * S, S, H, rot, float(eps), width, K.stream()),
            "qk_norm_rope_fwd")
    if v is None:
        v = qkv.view(B, S, H, 3, 64)[:, :, :, 2]
    return q, k, v, stats


def qk_norm_rope_bwd(dq, dk, dv, qkv, stats, gq, gk, cos, sin, H, rot, dqkv=None):
    """-> (dqkv like qkv, dgamma_q, dbeta_q, dgamma_k, dbeta_k fp32 [64]).  dq / dk (/ dv) contiguous [B,S,H,64] or [B,S,H,128]; dv None:
    the caller's dqkv already holds the v gradients in its v slots (written in place by the attention backward)."""
    K.require_cuda(dq, dk, dv, qkv, stats, dqkv)
    B, S, _ = qkv.shape
    width = dq.shape[-1]
    for t in (dq, dk, dv):
        if t is not None and (t.dtype != torch.bfloat16 or not t.is_contiguous() or tuple(t.shape) != (B, S, H, width) or width not in (64, 128)):
            raise K.OtterHipError("qk_norm_rope_bwd: dq / dk / dv must be contiguous bf16 [B,S,H,64] or [B,S,H,128]")
    if dv is None and dqkv is None:
        raise K.OtterHipError("qk_norm_rope_bwd: dv=None needs the dqkv buffer whose v slots hold the v gradients")
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    elif dqkv.dtype != torch.bfloat16 or not dqkv.is_contiguous() or dqkv.shape != qkv.shape:
        raise K.OtterHipError("qk_norm_rope_bwd: dqkv must be contiguous bf16 like qkv")
    nb = int(K.lib().otter_qk_norm_rope_bwd_blocks(B * S, H))
    partial = torch.empty((nb, 4, 64), dtype=torch.float32, device=qkv.device)
    K.check(K.lib().otter_qk_norm_rope_bwd(dq.data_ptr(), dk.data_ptr(), K.ptr(dv), qkv.data_ptr(), stats.data_ptr(), gq.data_ptr(), gk.data_ptr(),
                                           cos.data_ptr(), sin.data_ptr(), dqkv.data_ptr(), partial.data_ptr(), B * S, S, H, rot, width, K.stream()),
            "qk_norm_rope_bwd")
    p = partial.sum(0)
    return dqkv, p[0], p[1], p[2], p[3]


def sqrelu_fwd(x):
    K.require_cuda(x)
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or x.numel() % 8:
        raise K.OtterHipError("sqrelu: contiguous bf16 tensor with numel % 8 == 0")
    y = torch.empty_like(x)
    K.check(K.lib().otter_sqrelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), K.stream()), "sqrelu_fwd")
    return y


def sqrelu_bwd(x, dy):
    K.require_cuda(x, dy)
    if dy.dtype != torch.bfloat16 or not dy.is_contiguous() or dy.shape != x.shape:
        raise K.OtterHipError("sqrelu_bwd: dy must be contiguous bf16 like x")
    dx = torch.empty_like(x)
    K.check(K.lib().otter_sqrelu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), K.stream()), "sqrelu_bwd")
    return dx


def scatter_rows(word, patch, idx):
    """word [B,S,D], patch [B,P,D] (f32 or bf16 each), idx int64 [B,S] -> out like word."""
    K.require_cuda(word, patch, idx)
    B, S, D = word.shape
    P = patch.shape[1]
    if not (word.is_contiguous() and patch.is_contiguous() and idx.is_contiguous()) or idx.dtype != torch.int64 or tuple(idx.shape) != (B, S) \
            or patch.shape[0] != B or patch.shape[2] != D:
        raise K.OtterHipError("scatter_rows: contiguous word [B,S,D], patch [B,P,D], int64 idx [B,S]")
    out = torch.empty_like(word)
    K.check(K.lib().otter_scatter_rows(word.data_ptr(), K.dt(word), patch.data_ptr(), K.dt(patch), idx.data_ptr(), out.data_ptr(), B, S, P, D, K.stream()),
            "scatter_rows")
    return out


def add_frame_embs_(x5, emb):
    """x5 [b,T,F,v,D] (contiguous, modified in place) += emb[:F] broadcast (modeling_otter.py:224-226)."""
    b, T, F, v, D = x5.shape
    assert x5.is_contiguous() and emb.dtype == torch.float32 and emb.is_contiguous()
    K.check(K.lib().otter_add_frame_embs(x5.data_ptr(), K.dt(x5), emb.data_ptr(), b * T, F, v, D, K.stream()), "add_frame_embs")
    return x5


def add_rows_(dst2d, src2d, src_map: RowMap):
    """dst2d[r] += src2d[map(r)] (same dtype, same D)."""
    rows, D = dst2d.shape
    assert dst2d.is_contiguous() and src2d.is_contiguous() and dst2d.dtype == src2d.dtype
    K.check(K.lib().otter_add_rows(dst2d.data_ptr(), src2d.data_ptr(), src_map, rows, D, K.dt(dst2d), K.stream()), "add_rows")
    return dst2d


def set_attn_variant(v: int):
    """0 = MFMA attention cores for bf16 (default), 1 = fp32 VALU kernels (A/B hook)."""
    K.check(K.lib().otter_attn_set_variant(int(v)), "attn_set_variant")


def set_flash_variant(v: int):
    """0 = default (LDS-DMA tiles, longest-first block order, persistent dK/dV where it applies), 1 = register-staged tiles, 2 = LDS-DMA tiles
    on the plain grid, 3-5 = dK/dV occupancy / order variants, 6 = forward version 3, 7 = per-key-block dK/dV, 8 = persistent dK/dV wherever
    it can run (A/B hook of the decoder-host flash attention; csrc/flash.hip, include/otter_hip.h)."""
    K.check(K.lib().otter_flash_set_variant(int(v)), "flash_set_variant")


def set_gemm_variant(v: int):
    K.check(K.lib().otter_gemm_set_variant(int(v)), "gemm_set_variant")


def gemm_variant_available(v: int) -> bool:
    """True when schedule `v` is compiled into the loaded library: 0-3, 13, 25, 26, 30.  The numbers of the earlier kernel
    generations (4-12, 14-23, 27-29) are retired; set_gemm_variant refuses them."""
    return bool(K.lib().otter_gemm_variant_available(int(v)))


# Grid shape of the large-grid GEMM launches issued while a `gemm_grid_mode(...)` scope is open (otter_grid_mode in include/otter_hip.h).
# The scope is a module variable, not a thread-local: the backward products are launched from autograd's device thread, not from the thread
# that called TrainStep.__call__.  It is set for the duration of ONE training step by the TrainStep that owns a DP reducer and restored
# when the step returns -- nothing is left behind in the library.  It is PROCESS-WIDE while that step runs:
# any other thread that launches GEMMs during the window (an eval thread, a second TrainStep) inherits the mode, and overlapping scopes
# from two threads restore in LIFO order only if they nest.  The mode affects the grid shape (performance), never results; one training
# thread per process (the reference's own model: one rank = one Python thread) is what the scope is designed for.
_grid_mode = K.GRID_DEFAULT


class gemm_grid_mode:
    """with ops.gemm_grid_mode(K.GRID_PER_TILE): ...  -- every otter_gemm / otter_gemm_nt launch inside asks for that grid shape."""

    def __init__(self, mode: int):
        if mode not in (K.GRID_DEFAULT, K.GRID_PERSISTENT, K.GRID_PER_TILE):
            raise ValueError("gemm_grid_mode: %r" % (mode,))
        self.mode, self.prev = mode, None

    def __enter__(self):
        global _grid_mode
        self.prev, _grid_mode = _grid_mode, self.mode
        return self

    def __exit__(self, *exc):
        global _grid_mode
        _grid_mode = self.prev
        return False


def set_gemm_persistent(on: bool) -> None:
    """False: variant 26 runs one workgroup per tile (robust when RCCL kernels hold CUs during the backward GEMMs)."""
    K.check(K.lib().otter_gemm_set_persistent(1 if on else 0), "gemm_set_persistent")


def set_gemm_cu_budget(cus: int) -> int:
    """Cap the persistent GEMM grids at `cus` workgroups (0 = all CUs); returns the grid size in effect."""
    n = K.lib().otter_gemm_set_cu_budget(int(cus))
    if n < 0:
        K.check(n, "gemm_set_cu_budget")
    return int(n)


def prof_arm_gemm(M, N, Kd, max_events=4096):
    K.check(K.lib().otter_prof_arm_gemm(M, N, Kd, max_events), "prof_arm")


def prof_collect():
    n = C.c_int(0)
    ms = C.c_double(0.0)
    K.check(K.lib().otter_prof_collect(C.byref(n), C.byref(ms)), "prof_collect")
    return n.value, ms.value


def prof_collect_split():
    """(launches, total ms, launches with a K-major operand, their ms)."""
    n, nk = C.c_int(0), C.c_int(0)
    ms, mk = C.c_double(0.0), C.c_double(0.0)
    K.check(K.lib().otter_prof_collect_split(C.byref(n), C.byref(ms), C.byref(nk), C.byref(mk)), "prof_collect_split")
    return n.value, ms.value, nk.value, mk.value


def prof_disarm():
    K.check(K.lib().otter_prof_disarm(), "prof_disarm")
