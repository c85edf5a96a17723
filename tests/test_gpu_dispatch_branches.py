"""GPU parity tests, kernel level: the host-side dispatch branches of the older row-wise, element-wise, attention, decode, loss and
optimizer kernels (template instantiation / kernel chosen from shape, alignment and dtype) that no test compared with a reference.
Every reference is numpy / torch-CPU in fp64; for bf16 data it runs on the values after rounding to bf16.

| File | Branch | Test that reaches it |
|---|---|---|
| csrc/elementwise.hip otter_rope_strided | rope_vec_kernel<1>, <2>, <4>, <8>; both sides of the <8>/<4> and <4>/<2> thresholds | test_rope_strided_per_group |
| csrc/elementwise.hip otter_cast | scalar tail (n % 8 != 0), all four dtype pairs | test_cast_tail_and_dtype_pairs |
| csrc/elementwise.hip otter_rope | f32 / bf16 with partial rotary, inverse, in place | test_rope_scalar_partial_rotary |
| csrc/elementwise.hip otter_add_frame_embs | both dtypes | test_add_frame_embs |
| csrc/attn.hip VALU kernels | SPLITK = true with a mask (EQ / GE) in attn_fwd_kernel and attn_bwd_dq_kernel: merge of waves that saw no allowed key, zeroed rows, uniform rows, an M % 32 != 0 tail chunk | tests/test_gpu_kernels.py::test_attention_core, the ATTN_CASES with M >= 256 |
| csrc/attn_mfma.hip | a masked row whose allowed media follows several fully masked 64-key tiles | tests/test_gpu_kernels.py::test_attention_core[bf16], cases (2, 2, 40, 320, 64, 1 / 2) and (1, 4, 300, 256, 64, 1) |
| csrc/norm.hip otter_colsum | accumulate = 1; bf16 source; D < 512 and D % 512 != 0; rows < 32; rows > 32 * 256 (the rch cap, trailing empty row chunks); a row map | test_colsum_shapes_and_accumulate |
| csrc/norm.hip otter_layernorm_bwd | accumulate = 1 on dgamma and dbeta | test_layernorm_bwd_accumulates_weight_gradients |
| csrc/norm.hip norm_fwd_kernel / norm_bwd_dx_kernel<NCH, RMS> | generic NCH = 1, 2, 4 (1024 < D <= 2048), 8, 16; D = 8 (one lane of 64); D = 504, 520, 1032, 2056, 4104, 8184 (lanes of the last live chunk past D, statistics divided by a D that is no power of two), exact answers | tests/test_gpu_norm_exact.py::test_forward_at_chunk_edges_every_route_and_option, ::test_backward_at_chunk_edges_every_route_and_option |
| csrc/norm.hip dtype routes | fp32 -> bf16 on the generic kernels (D % 512 != 0; D = 4608 and 8192: NCH = 16), bf16 -> fp32, bf16 gamma / beta (ld4 and load8 on weights), otter_rmsnorm_bwd / _ex with a bf16 x (round_to in the dx and the dw kernel), add_rmsnorm_fwd without delta, rmsnorm_bwd_ex without dres, every other optional argument present and absent | the same two tests; through the wrappers: tests/test_gpu_norm_exact.py::test_ops_wrappers_every_optional_argument |
| csrc/norm.hip norm_fwd_c_kernel / norm_bwd_dx_c_kernel<NCH, RMS> | coalesced NCH = 1, 2, 4, 8 at D = 512, 1024, 2048, 3584, 4096; bf16 weights | tests/test_gpu_norm_exact.py::test_coalescable_cases_forward_and_backward |
| csrc/norm.hip norm_variant | OTTER_NORM_VARIANT=0 (read once per process): the generic kernels at the coalescable shapes | tests/test_gpu_norm_exact.py::test_generic_kernels_meet_the_coalesced_shapes_in_a_fresh_process |
| csrc/norm.hip row kernels, rows < 4 | rows = 1, 2, 3, 4, 5 at D = 520 and 1024: blocks whose waves return early | tests/test_gpu_norm_exact.py::test_blocks_with_waves_that_return_early |
| csrc/norm.hip norm_bwd_dw_partial_kernel / norm_bwd_dw_final_kernel, pick_rch | rows = 31, 32, 33, 63, 64, 65 (one row chunk becomes two, short last chunk), 127, 8191, 8192, 8193 (the cap: per = 33, empty trailing chunks over a stale workspace); accumulate, no dbeta, a dy row map, RMSNorm with a bf16 x | tests/test_gpu_norm_exact.py::test_dgamma_dbeta_at_row_chunk_edges |
| csrc/norm.hip colsum_partial_kernel / colsum_final_kernel | the same row counts, bf16 and fp32 sources, count / one-row / one-hot forms, accumulate, a row map | tests/test_gpu_norm_exact.py::test_colsum_at_row_chunk_edges |
| otter_amd/ops.py rmsnorm_bwd | dy of another dtype than x raises | tests/test_norm_cases_cpu.py::test_rmsnorm_bwd_rejects_a_dy_of_another_dtype, tests/test_gpu_norm_exact.py::test_ops_rmsnorm_bwd_rejects_a_dy_of_another_dtype |
| csrc/attn.hip otter_text_time | T of exactly 64 / 128, T < 64, media at positions 63 and 64 (carry between the 64-wide scans), an all-media row | test_text_time_scan_boundaries |
| csrc/decode.hip | Sk <= 256 boundary of the LDS floor, Sk = 1, a fully masked batch row, q as a strided slice | test_decode_attn_small_sk_and_masked_row |
| csrc/loss.hip | scalar tails of both vector widths, ld > V, ldd != ld | test_cross_entropy_tails_and_padded_strides |
| csrc/optim.hip | sumsq_kernel and the AdamW kernel on p / g that are not 16-byte aligned (vec_ok false), tensors of several 8192-element chunks that end in a tail | test_fused_adamw_misaligned_views |
| csrc/gemm.hip pick_cfg, forced | variants 1, 2 (K tail: K % 64 != 0), 3, 13, 25, 30, 26 (cross-tile form at 4 K-tiles and more, its tail-trip-only loop at K = 384, K = 128 without it, plain K order, cross-tile form off) on both sides of every tile edge, exact answers | tests/test_gpu_gemm_exact.py::test_forced_variant_at_tile_and_k_tile_edges |
| csrc/gemm_tail.h epilogue4 / epilogue8 / tail_apply | STORE, accumulate, sum-of-squares partials, SCALE_RES (R fp32 / bf16), GATE_BWD (identity, squared ReLU, stashed derivative; partials), GELU (C2 = acc, C2 = GELU'), each with a gate where it takes one, full-tile and masked tails, both output dtypes | tests/test_gpu_gemm_exact.py::test_every_epilogue_form |
| csrc/gemm.hip gemm_impl `wide` | N, ldc, ldc2, ldr, ldaux % 8 one at a time: 4-wide against 8-wide tail | tests/test_gpu_gemm_exact.py::test_wide_tail_switch_one_leading_dimension_at_a_time |
| csrc/gemm_tiled.hip gemm_f32_kernel | 64 x 64 x 32 tile edges, K % 32 != 0, every epilogue form | tests/test_gpu_gemm_exact.py::test_fp32_kernel_at_its_tile_edges |
| otter_amd/ops.py gemm_nt `k=` | operands wider than the reduction, NaN behind column k | tests/test_gpu_gemm_exact.py::test_k_argument_reduces_over_the_first_k_columns |
| csrc/gemm.hip launch_cfg and the launch functions of csrc/gemm_*.hip: persistent grids, OTTER_GRID_PER_TILE | two and more ragged tiles per workgroup under a CU budget of 8 (every persistent kernel); variant 26 with one workgroup per tile, same bits | tests/test_gpu_gemm_exact.py::test_several_tiles_per_workgroup |
| csrc/gemm_t4.hip gemm_bf16_t4_kernel<EPI, TA, TB, XT> by default dispatch | >= 192 tiles of 256 x 256, full and ragged; K-contiguous (cross-tile form), A / B / both K-major with padded leading dimensions, both K-major at K % 128 != 0 (rows behind K read as zeros) | tests/test_gpu_gemm_exact.py::test_default_dispatch_large_grid_and_k_major |
"""

import numpy as np
import pytest
import torch

from oracle import otter_oracle as O
from tests.test_gpu_kernels import DEV, bf16_round, host, ops, relmax, rng, to_dev  # noqa: F401  (ops: the module-scoped fixture)

pytestmark = pytest.mark.gpu

SENT = 0xA5     # byte of the sentinel frames
PAD = 256       # bytes on either side of a framed buffer (keeps the payload 16-byte aligned)


def _framed(nbytes):
    """(whole uint8 buffer, address of the payload): `nbytes` of payload between two sentinel pads."""
    buf = torch.full((nbytes + 2 * PAD,), SENT, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + PAD


def _frame_intact(buf, nbytes):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + nbytes:] == SENT).all())


def _bf16_elementwise_ok(got, ref, x1, x2):
    """fp32 arithmetic rounded once to bf16: |got - ref| <= 2**-8 |ref| + 2**-20 (|x1| + |x2|) -- the bf16 rounding (8 significant bits:
    half an ulp is at most 2**-8 of the value, reached just above a power of two) plus slack for the two fp32 products and their sum
    (|cos|, |sin| <= 1).  Returns the largest ratio error / bound (must be <= 1)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = 2.0 ** -8 * np.abs(ref) + 2.0 ** -20 * (np.abs(x1) + np.abs(x2))
    return float((err / (bound + 1e-300)).max())


def _tables(r, S, width):
    """fp32 cos / sin tables [S, width] whose two halves differ (a kernel that takes the first-half value for the second half fails)."""
    ang = r.uniform(-np.pi, np.pi, size=(S, width))
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _rope_ref(x, cos, sin, pos, rot, inverse):
    """fp64 RoPE, half-split layout: x [tokens, H, d], cos / sin [S, rot], pos [tokens] -> (y, partner of every rotated element)."""
    x = x.astype(np.float64)
    c, s = cos.astype(np.float64)[pos][:, None, :], sin.astype(np.float64)[pos][:, None, :]
    xr, h = x[..., :rot], rot // 2
    if not inverse:
        yr = xr * c + np.concatenate([-xr[..., h:], xr[..., :h]], -1) * s
    else:
        t = xr * s
        yr = xr * c + np.concatenate([t[..., h:], -t[..., :h]], -1)
    partner = np.concatenate([xr[..., h:], xr[..., :h]], -1)
    return np.concatenate([yr, x[..., rot:]], -1), partner


# ----------------------------------------------------------------------------------------------------------------------
# 1. otter_rope_strided: one case per G
# ----------------------------------------------------------------------------------------------------------------------

ROPE_STRIDED = [
    # H, tokens, S, d       the dispatch: G = 8 if H % 8 == 0 and tokens*(H/8)*(d/16) >= 65536; else G = 4 if H % 4 == 0 and
    #                       tokens*(H/4)*(d/16) >= 65536; else G = 2 if H % 2 == 0; else G = 1
    (3, 5, 3, 128),         # H odd -> <1>
    (3, 5, 3, 16),          # <1>, one 8-element chunk per half
    (3, 5, 3, 32),          # <1>, two chunks per half
    (6, 74, 37, 128),       # H % 4 != 0 -> <2>
    (12, 2752, 1376, 128),  # H % 8 != 0; 2752*(12/4)*8 = 66048 >= 65536 -> <4>
    (16, 4096, 2048, 128),  # 4096*(16/8)*8 = 65536 >= 65536 -> <8>
    (8, 8192, 4096, 128),   # 8192*(8/8)*8 = 65536 -> <8>, exactly on the threshold
    (8, 8184, 4092, 128),   # 8184*1*8 = 65472 < 65536 but 8184*(8/4)*8 = 130944 -> <4>, just below the <8> threshold
    (8, 4096, 2048, 128),   # 4096*1*8 = 32768 < 65536, 4096*2*8 = 65536 -> <4>, exactly on its threshold
    (8, 4095, 1365, 128),   # 4095*2*8 = 65520 < 65536 -> <2>, just below the <4> threshold
]


@pytest.mark.parametrize("H,tokens,S,d", ROPE_STRIDED)
def test_rope_strided_per_group(ops, H, tokens, S, d):
    """x with a padded token stride (H*d + 64) -> packed y, forward; inverse in place on a second padded buffer whose 64 elements
    between one token's heads and the next token's must keep their bits.  S < tokens, so tok % S wraps."""
    r = rng(H * 1000 + tokens + d)
    xs = H * d + 64
    cos, sin = _tables(r, S, d)
    pos = np.arange(tokens) % S
    dcos, dsin = to_dev(cos), to_dev(sin)
    xbuf = bf16_round(r.standard_normal((tokens, xs)))
    x = xbuf[:, :H * d].reshape(tokens, H, d)
    ref, partner = _rope_ref(x, cos, sin, pos, d, False)
    dx = to_dev(xbuf, torch.bfloat16)
    y = torch.zeros((tokens, H * d), dtype=torch.bfloat16, device=DEV)
    ops.rope_strided(dx, y, dcos, dsin, tokens, S, H, d, xs, H * d)
    worst = _bf16_elementwise_ok(host(y).reshape(tokens, H, d), ref, x, partner)
    print("rope_strided fwd H=%d tokens=%d d=%d: worst error / bound = %.3f" % (H, tokens, d, worst))
    assert worst <= 1.0
    assert torch.equal(dx, to_dev(xbuf, torch.bfloat16))          # the source is only read
    gbuf = bf16_round(r.standard_normal((tokens, xs)))
    g = gbuf[:, :H * d].reshape(tokens, H, d)
    gref, gpartner = _rope_ref(g, cos, sin, pos, d, True)
    dg = to_dev(gbuf, torch.bfloat16)
    ops.rope_strided(dg, dg, dcos, dsin, tokens, S, H, d, xs, xs, inverse=True)
    got = host(dg)
    worst = _bf16_elementwise_ok(got[:, :H * d].reshape(tokens, H, d), gref, g, gpartner)
    print("rope_strided inverse in place: worst error / bound = %.3f" % worst)
    assert worst <= 1.0
    assert np.array_equal(got[:, H * d:].view(np.uint32), gbuf[:, H * d:].view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------------
# 2. otter_cast
# ----------------------------------------------------------------------------------------------------------------------

_SPECIAL_BITS = np.array([
    0x00000000, 0x80000000,               # +-0
    0x00011C71, 0x80011C71, 0x00000001,   # fp32 denormals (1e-40, -1e-40, the smallest)
    0x00400000, 0x80010000,               # values that are denormal in bf16 as well
    0x7F800000, 0xFF800000,               # +-inf
    0x3F808000, 0x3F818000,               # exact bf16 ties: even mantissa (rounds down to 0x3F80), odd mantissa (rounds up to 0x3F82)
    0xC1A08000, 0xC1A18000,               # the same two, negative
    0x7F7FFFFF, 0xFF7FFFFF,               # the largest finite fp32 (rounds to inf in bf16)
    0x7FC00000, 0x7F800001,               # NaNs
    0x3F7FFFFF,                           # rounds up across a binade
], dtype=np.uint32)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 16387])
@pytest.mark.parametrize("sdt,ddt", [("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16"), ("f32", "f32")])
def test_cast_tail_and_dtype_pairs(ops, sdt, ddt, n):
    """One thread converts 8 elements; the thread that owns the last n % 8 elements runs the scalar loop.  Bit-equal to torch's CPU
    conversion (NaN positions compared as NaN), and exactly n elements written (sentinel frame)."""
    from otter_amd import _capi as K

    r = rng(n)
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16}
    bits = (r.standard_normal(n) * 3).astype(np.float32).view(np.uint32).copy()
    ns = len(_SPECIAL_BITS)
    m = min(n, ns)
    bits[:m] = _SPECIAL_BITS[:m]
    tail = np.arange(n - m, n)
    bits[tail] = _SPECIAL_BITS[(tail + n) % ns]          # ... and in the last elements, where the scalar loop runs
    src = torch.from_numpy(bits.view(np.float32).copy()).to(tdt[sdt])   # CPU, source dtype
    want = src.to(tdt[ddt])
    dsrc = src.to(DEV)
    es = 2 if ddt == "bf16" else 4
    buf, out_ptr = _framed(n * es)
    K.check(K.lib().otter_cast(dsrc.data_ptr(), K.dt(dsrc), out_ptr, K.dt_of(tdt[ddt]), n, K.stream()), "cast")
    torch.cuda.synchronize()
    assert _frame_intact(buf, n * es)
    got = buf[PAD:PAD + n * es].cpu().view(tdt[ddt])
    nan_w, nan_g = torch.isnan(want.float()), torch.isnan(got.float())
    assert torch.equal(nan_w, nan_g)
    ity = torch.int16 if ddt == "bf16" else torch.int32
    gi, wi = got.view(ity)[~nan_w], want.view(ity)[~nan_w]
    bad = (gi != wi).nonzero().flatten().tolist()
    assert not bad, [(i, hex(int(gi[i]) & 0xFFFFFFFF), hex(int(wi[i]) & 0xFFFFFFFF)) for i in bad[:8]]


# ----------------------------------------------------------------------------------------------------------------------
# 3. otter_rope, the scalar kernel
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("rot", [64, 32, 16])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rope_scalar_partial_rotary(ops, dt, rot):
    """d = 64 with full and partial rotary, forward and inverse against fp64, out of place and in place (y == x); the pass-through
    columns [rot, d) keep their bits.  f32: 2e-5 relative-to-max; bf16: the per-element bound of the strided kernel."""
    r = rng(300 + rot)
    B, S, H, d = 2, 5, 3, 64
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    x = r.standard_normal((B, S, H, d)).astype(np.float32)
    if dt == "bf16":
        x = bf16_round(x)
    cos, sin = _tables(r, S, rot)
    pos = np.tile(np.arange(S), B)
    dcos, dsin = to_dev(cos), to_dev(sin)
    for inverse in (False, True):
        ref, partner = _rope_ref(x.reshape(B * S, H, d), cos, sin, pos, rot, inverse)
        ref = ref.reshape(B, S, H, d)
        dx = to_dev(x, tdt)
        y = ops.rope(dx, dcos, dsin, rot_dim=rot, inverse=inverse)
        z = dx.clone()
        assert ops.rope(z, dcos, dsin, rot_dim=rot, inverse=inverse, out=z).data_ptr() == z.data_ptr()
        assert torch.equal(y, z)                                      # in place: same bits as out of place
        assert torch.equal(dx, to_dev(x, tdt))                        # out of place: x untouched
        if rot < d:
            assert torch.equal(y[..., rot:], dx[..., rot:])
        if dt == "f32":
            e = relmax(host(y), ref)
            print("rope f32 rot=%d inverse=%d: relmax = %.3g" % (rot, inverse, e))
            assert e < 2e-5
        else:
            xr = x.reshape(B * S, H, d)[..., :rot]
            worst = _bf16_elementwise_ok(host(y).reshape(B * S, H, d)[..., :rot], ref.reshape(B * S, H, d)[..., :rot], xr, partner)
            print("rope bf16 rot=%d inverse=%d: worst error / bound = %.3f" % (rot, inverse, worst))
            assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# 4. otter_add_frame_embs
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_add_frame_embs(ops, dt):
    """x [outer, F, inner, D] += emb[f] in fp32: bit-equal to numpy's fp32 sum (f32 x) / to its bf16 rounding (bf16 x)."""
    r = rng(404)
    outer, F, inner, D = 3, 4, 5, 72
    x = r.standard_normal((outer, F, inner, D)).astype(np.float32)
    emb = r.standard_normal((F, D)).astype(np.float32)
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    if dt == "bf16":
        x = bf16_round(x)
    want = x + emb[None, :, None, :]
    if dt == "bf16":
        want = bf16_round(want)
    dx = to_dev(x.reshape(1, outer, F, inner, D), tdt)
    out = ops.add_frame_embs_(dx, to_dev(emb))
    assert out.data_ptr() == dx.data_ptr()
    assert np.array_equal(host(out).reshape(outer, F, inner, D).view(np.uint32), want.astype(np.float32).view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------------
# 6. otter_colsum, otter_layernorm_bwd with accumulate = 1
# ----------------------------------------------------------------------------------------------------------------------

COLSUM = [
    # rows, D, dtype, row map (grp_rows, grp_stride, row_off) or None      rch = clamp(rows / 32, 1, 256) row chunks, ceil(D/512) column blocks
    (1, 8, "f32", None),                   # rch = 1: three of the four waves see no row; one lane active
    (31, 520, "f32", None),                # rows < 32 -> rch = 1; D = 512 + 8: a second column block with one active lane
    (33, 520, "bf16", None),               # rch = 1, bf16 source
    (8300, 64, "bf16", None),              # 8300/32 = 259 -> capped at 256; ceil(8300/256) = 33 rows per chunk, 252*33 = 8316 > 8300: chunks 252..255 are empty
    (257, 1024, "f32", (257, 300, 7)),     # rows 7..263 of a 300-row buffer; rch = 8
]


@pytest.mark.parametrize("rows,D,dt,rmap", COLSUM)
def test_colsum_shapes_and_accumulate(ops, rows, D, dt, rmap):
    from otter_amd._capi import RowMap

    r = rng(rows + D)
    nrows = rows if rmap is None else rmap[1]
    src = r.standard_normal((nrows, D)).astype(np.float32)
    if dt == "bf16":
        src = bf16_round(src)
    used = src if rmap is None else src[rmap[2]:rmap[2] + rows]
    ref = used.astype(np.float64).sum(0)
    dsrc = to_dev(src, torch.float32 if dt == "f32" else torch.bfloat16)
    m = None if rmap is None else RowMap(*rmap)
    out = torch.full((D,), float("nan"), device=DEV)
    assert ops.colsum(dsrc, m, rows, out=out).data_ptr() == out.data_ptr()
    e1 = relmax(host(out), ref)
    ops.colsum(dsrc, m, rows, out=out, accumulate=True)
    e2 = relmax(host(out), 2 * ref)
    print("colsum rows=%d D=%d %s: relmax = %.3g, accumulated %.3g" % (rows, D, dt, e1, e2))
    assert e1 < 1e-5 and e2 < 1e-5


@pytest.mark.parametrize("rows,D", [(70, 1024),      # fp32 x, bf16 dy, D % 512 == 0: the coalesced dx kernel
                                    (33, 136)])      # D % 512 != 0: the generic dx kernel
def test_layernorm_bwd_accumulates_weight_gradients(ops, rows, D):
    """accumulate = 1: dgamma / dbeta += their sums (ops.layernorm_bwd always passes 0, so through ctypes).  preload + fp64 reference,
    1e-4 relative-to-max; the same call with accumulate = 0 overwrites the preload."""
    from otter_amd import _capi as K
    from otter_amd._capi import RowMap

    r = rng(rows * D)
    eps = 1e-5
    x = (r.standard_normal((rows, D)) * 2 + 0.5).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(D)).astype(np.float32)
    b = (0.1 * r.standard_normal(D)).astype(np.float32)
    dy = bf16_round(r.standard_normal((rows, D)))
    pre_g = r.standard_normal(D).astype(np.float32) * 5
    pre_b = r.standard_normal(D).astype(np.float32) * 5
    x64 = x.astype(np.float64)
    mu = x64.mean(-1, keepdims=True)
    xhat = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + eps)
    dg_ref, db_ref = (dy.astype(np.float64) * xhat).sum(0), dy.astype(np.float64).sum(0)
    dx_x, dx_w, dx_dy = to_dev(x), to_dev(w), to_dev(dy, torch.bfloat16)
    _, mean, rstd = ops.layernorm_fwd(dx_x, dx_w, to_dev(b), torch.bfloat16, eps=eps)
    ws = torch.empty(K.lib().otter_layernorm_bwd_workspace_bytes(rows, D), dtype=torch.uint8, device=DEV)
    dx = torch.empty((rows, D), dtype=torch.float32, device=DEV)
    for accumulate in (1, 0):
        dg, db = to_dev(pre_g), to_dev(pre_b)
        K.check(K.lib().otter_layernorm_bwd(dx_dy.data_ptr(), K.BF16, RowMap(0, 0, 0), dx_x.data_ptr(), K.F32, dx_w.data_ptr(), K.F32,
                                            mean.data_ptr(), rstd.data_ptr(), None, dx.data_ptr(), K.F32, None, dg.data_ptr(), db.data_ptr(),
                                            accumulate, ws.data_ptr(), rows, D, K.stream()), "layernorm_bwd")
        eg = relmax(host(dg), accumulate * pre_g.astype(np.float64) + dg_ref)
        eb = relmax(host(db), accumulate * pre_b.astype(np.float64) + db_ref)
        print("layernorm_bwd rows=%d D=%d accumulate=%d: dgamma %.3g dbeta %.3g" % (rows, D, accumulate, eg, eb))
        assert eg < 1e-4 and eb < 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# 7. otter_text_time
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("attend_previous", [True, False])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 128, 333])
def test_text_time_scan_boundaries(ops, T, attend_previous):
    """One wave scans 64 positions at a time and carries the count into the next 64: T below, at and just above one and two scans,
    media on either side of the first carry (positions 63 and 64), no media, only media."""
    r = rng(700 + T)
    ml = np.zeros((6, T), bool)
    ml[1, :] = True
    for row, idx in ((2, (63,)), (3, (64,)), (4, (63, 64))):
        for i in idx:
            if i < T:
                ml[row, i] = True
    ml[5] = r.random(T) < 0.3
    tt = ops.text_time(torch.from_numpy(ml).to(DEV), attend_previous)
    assert tt.dtype == torch.int32
    assert np.array_equal(tt.cpu().numpy().astype(np.int64), O.text_time(ml, attend_previous))


# ----------------------------------------------------------------------------------------------------------------------
# 8. otter_decode_attn
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("alibi", [False, True])
@pytest.mark.parametrize("Sk", [1, 2, 255, 256, 257])     # dynamic LDS = max(Sk, 2*128) floats: 256 is the last Sk on the floor, 257 the first above it
def test_decode_attn_small_sk_and_masked_row(ops, Sk, alibi):
    """LLaMA layout [B,H,Sk,128], q = qkv[:, 0] of a fused [B,3,H,128] buffer (batch stride 3*H*128), batch row 1 fully masked (output
    exactly 0), row 2 with its first key masked when it has a second one.  fp64 softmax attention, 1e-2 relative-to-max."""
    r = rng(800 + Sk)
    B, H, d = 3, 2, 128
    qkv = bf16_round(r.standard_normal((B, 3, H, d)))
    k = bf16_round(r.standard_normal((B, H, Sk, d)))
    v = bf16_round(r.standard_normal((B, H, Sk, d)))
    slopes = (2.0 ** -np.arange(1, H + 1)).astype(np.float32) if alibi else None
    valid = np.ones((B, Sk), np.uint8)
    valid[1, :] = 0
    if Sk > 1:
        valid[2, 0] = 0
    scale = d ** -0.5
    q = qkv[:, 0].astype(np.float64)
    s = np.einsum("bhd,bhsd->bhs", q, k.astype(np.float64)) * scale
    if alibi:
        s = s + slopes.astype(np.float64)[None, :, None] * (np.arange(Sk) - (Sk - 1))[None, None, :]
    live = [0, 2]
    s = np.where(valid[live][:, None, :] != 0, s[live], -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = np.einsum("bhs,bhsd->bhd", p, v[live].astype(np.float64))
    dqkv = to_dev(qkv, torch.bfloat16)
    tq = dqkv[:, 0]
    assert tq.stride() == (3 * H * d, d, 1)
    o = ops.decode_attn(tq, to_dev(k, torch.bfloat16), to_dev(v, torch.bfloat16), to_dev(slopes) if alibi else None,
                        torch.from_numpy(valid).to(DEV), scale)
    got = host(o)
    e = relmax(got[live], ref)
    print("decode_attn Sk=%d alibi=%d: relmax = %.3g" % (Sk, alibi, e))
    assert e < 1e-2
    assert np.array_equal(got[1].view(np.uint32), np.zeros((H, d), np.uint32))


# ----------------------------------------------------------------------------------------------------------------------
# 9. otter_cross_entropy_fwd / _bwd: scalar tails, padded row strides
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("V,ld,ldd", [(1003, 1008, 1008),     # ld % 8 == 0 -> VEC = 8: 125 chunks + a tail of 3
                                      (1002, 1004, 1004),     # ld % 8 == 4 -> VEC = 4: 250 chunks + a tail of 2
                                      (1001, 1008, 1016),     # VEC = 8 in both passes, tail of 1, ldd != ld
                                      (1000, 1004, 1008)])    # forward and backward VEC = 4 (ld % 8 == 4), no tail, ldd != ld
def test_cross_entropy_tails_and_padded_strides(ops, V, ld, ldd):
    """Logits in a [rows, ld] buffer whose padding columns [V, ld) hold +inf (reading one shows at once), dlogits in a [rows, ldd]
    buffer pre-filled with a sentinel that columns [V, ldd) must keep.  lse / nll within 2e-6 relative of fp64, dlogits within
    rtol 2**-7, atol 1e-9 (one bf16 rounding)."""
    from otter_amd import _capi as K

    r = rng(V)
    rows = 8
    x = bf16_round(3 * r.standard_normal((rows, V)))
    x[7, V - 1] = 60.0           # the row maximum lies in the scalar tail (where there is one)
    x[7, 3] = -60.0
    t0 = (V // 8) * 8 if V % 8 else V - 2          # first element of the VEC = 8 tail (any late column when there is none)
    labels = np.array([0, V - 1, t0, -100, int(r.integers(0, V)), V - 1, int(r.integers(0, V)), 3], np.int64)
    buf = np.full((rows, ld), np.inf, np.float32)
    buf[:, :V] = x
    dlogits = to_dev(buf, torch.bfloat16)
    dlab = torch.from_numpy(labels).to(DEV)
    lse = torch.full((rows,), float("nan"), device=DEV)
    nll = torch.full((rows,), float("nan"), device=DEV)
    K.check(K.lib().otter_cross_entropy_fwd(dlogits.data_ptr(), ld, dlab.data_ptr(), lse.data_ptr(), nll.data_ptr(), rows, V, K.stream()), "ce_fwd")
    x64 = x.astype(np.float64)
    mx = x64.max(-1, keepdims=True)
    lse_ref = (mx + np.log(np.exp(x64 - mx).sum(-1, keepdims=True)))[:, 0]
    ok = labels >= 0
    nll_ref = np.where(ok, lse_ref - x64[np.arange(rows), np.where(ok, labels, 0)], 0.0)
    lse_ref = np.where(ok, lse_ref, 0.0)           # an ignored row reports lse = nll = 0
    e_lse = np.abs(host(lse) - lse_ref) / np.where(ok, np.abs(lse_ref), 1.0)
    e_nll = np.abs(host(nll) - nll_ref) / np.where(ok, np.abs(nll_ref), 1.0)
    print("cross_entropy V=%d ld=%d: lse rel %.3g, nll rel %.3g" % (V, ld, e_lse.max(), e_nll.max()))
    assert e_lse.max() <= 2e-6 and e_nll.max() <= 2e-6
    sentinel = 7.0
    dd = torch.full((rows, ldd), sentinel, dtype=torch.bfloat16, device=DEV)
    dloss, nv = 0.37, float(ok.sum())
    d_dloss, d_nv = to_dev(np.array([dloss], np.float32)), to_dev(np.array([nv], np.float32))
    K.check(K.lib().otter_cross_entropy_bwd(dlogits.data_ptr(), ld, dlab.data_ptr(), lse.data_ptr(), d_dloss.data_ptr(), d_nv.data_ptr(), dd.data_ptr(),
                                            ldd, rows, V, K.stream()), "ce_bwd")
    got = host(dd).astype(np.float64)
    assert np.array_equal(got[:, V:], np.full((rows, ldd - V), sentinel))
    onehot = np.zeros((rows, V))
    onehot[np.arange(rows)[ok], labels[ok]] = 1.0
    d_ref = np.where(ok[:, None], (np.exp(x64 - (mx + np.log(np.exp(x64 - mx).sum(-1, keepdims=True)))) - onehot) * dloss / nv, 0.0)
    excess = np.abs(got[:, :V] - d_ref) - (1e-9 + 2.0 ** -7 * np.abs(d_ref))
    print("cross_entropy dlogits: worst excess over the bound %.3g" % excess.max())
    assert excess.max() <= 0.0
    assert np.array_equal(got[3, :V], np.zeros(V))
    assert torch.equal(dlogits, to_dev(buf, torch.bfloat16))     # the logits are only read


# ----------------------------------------------------------------------------------------------------------------------
# 10. grad-norm + AdamW on tensors that are not 16-byte aligned
# ----------------------------------------------------------------------------------------------------------------------


def test_fused_adamw_misaligned_views():
    """Parameters and gradients are views at element offsets 1, 2, 3 of larger fp32 buffers (4, 8, 12 bytes off 16-byte alignment):
    sumsq_kernel's scalar loop (it looks at g alone) and the update kernel's scalar loop (vec_ok false), over tensors of one element
    group, exactly one 8192-chunk, and several chunks ending in a tail (16384 + 5 = 2 chunks + 5; 333*77 = 25641 = 3 chunks + 1065);
    one tensor carries a bf16 shadow, refreshed by the scalar loop.  Against torch.optim.AdamW + clip_grad_norm_(1.0) on aligned clones,
    the tolerances of test_fused_adamw_matches_torch; everything outside the views keeps its bytes."""
    from otter_amd import _capi as K
    from otter_amd.functional import shadows
    from otter_amd.optim import FusedAdamW

    assert K.lib().otter_device_check() > 0, K.lib().otter_last_error()
    torch.manual_seed(13)
    numels = [5, 8192, 16384 + 5, 333 * 77]
    p_off = [1, 2, 3, 1]
    g_off = [3, 1, 2, 2]
    guard = 16
    pbufs = [torch.full((n + o + guard,), 123.25, device=DEV) for n, o in zip(numels, p_off)]
    gbufs = [torch.full((n + o + guard,), -77.5, device=DEV) for n, o in zip(numels, g_off)]
    init = [torch.randn(n, device=DEV) * 0.1 for n in numels]
    mine = []
    for buf, o, n, x0 in zip(pbufs, p_off, numels, init):
        view = buf[o:o + n]
        view.copy_(x0)
        assert view.data_ptr() % 16 == 4 * o and view.is_contiguous()
        mine.append(view.requires_grad_(True))
    gviews = [buf[o:o + n] for buf, o, n in zip(gbufs, g_off, numels)]
    assert all(g.data_ptr() % 16 == 4 * o for g, o in zip(gviews, g_off))
    ref = [x0.clone().requires_grad_(True) for x0 in init]
    wd_split = 2
    opt_r = torch.optim.AdamW([{"params": ref[:wd_split], "weight_decay": 0.1}, {"params": ref[wd_split:], "weight_decay": 0.0}], lr=1e-3)
    opt_m = FusedAdamW([{"params": mine[:wd_split], "weight_decay": 0.1}, {"params": mine[wd_split:], "weight_decay": 0.0}], lr=1e-3,
                       max_grad_norm=1.0)
    # the bf16 shadow of a misaligned parameter: registered by hand (the cast kernel that would make it wants an aligned source)
    sh0 = mine[2].detach().to(torch.bfloat16)
    shadows.mark_w(mine[2], torch.bfloat16, sh0)
    try:
        for step in range(3):
            grads = [torch.randn(n, device=DEV) * (3.0 if step == 0 else 0.01) for n in numels]   # step 0 clips, later steps do not
            for r_, m_, gv, g in zip(ref, mine, gviews, grads):
                r_.grad = g.clone()
                gv.copy_(g)
                m_.grad = gv
            norm64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
            norm_r = torch.nn.utils.clip_grad_norm_(ref, 1.0)
            opt_r.step()
            opt_m.step()
            cur = shadows.w(mine[2], torch.bfloat16)
            assert cur.data_ptr() == sh0.data_ptr() and torch.equal(cur, mine[2].detach().to(torch.bfloat16))
            got_norm = float(opt_m.last_norm[0])
            print("adamw misaligned step %d: norm %.9g torch %.9g fp64 %.9g" % (step, got_norm, float(norm_r), norm64))
            assert abs(got_norm - float(norm_r)) <= 1e-5 * float(norm_r)
            assert abs(got_norm - norm64) <= 2e-6 * norm64
            for i, (r_, m_) in enumerate(zip(ref, mine)):
                err = float((r_.detach() - m_.detach()).abs().max())
                assert err <= 2e-6 * float(r_.detach().abs().max()) + 1e-9, (step, i, err, float(r_.detach().abs().max()))
        for r_, m_ in zip(ref, mine):
            sr, sm = opt_r.state[r_], opt_m.state[m_]
            assert float((sr["exp_avg"] - sm["exp_avg"]).abs().max()) <= 2e-6 * float(sr["exp_avg"].abs().max()) + 1e-12
            assert float((sr["exp_avg_sq"] - sm["exp_avg_sq"]).abs().max()) <= 3e-5 * float(sr["exp_avg_sq"].abs().max()) + 1e-15
        for buf, o, n in zip(pbufs, p_off, numels):
            assert bool((buf[:o] == 123.25).all()) and bool((buf[o + n:] == 123.25).all())
        for buf, o, n, g in zip(gbufs, g_off, numels, grads):
            assert bool((buf[:o] == -77.5).all()) and bool((buf[o + n:] == -77.5).all()) and torch.equal(buf[o:o + n], g)
    finally:
        shadows.clear()
