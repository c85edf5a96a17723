"""GPU parity tests, kernel level: every entry point of include/otter_hip.h is called through the C ABI (ctypes, via
otter_amd.ops) on seeded inputs and compared with the numpy oracle.

Tolerances (stated per the brief):
  f32 storage : 2e-5 relative-to-max  (fp32 arithmetic, different summation order than numpy)
  bf16 storage: inputs are rounded to bf16 FIRST and the oracle runs on the rounded values, so the only error left is
                fp32 accumulation order + one bf16 rounding of the output: 1e-2 relative-to-max for bf16 outputs,
                1e-4 for fp32 outputs of bf16-operand GEMMs.
"""

import numpy as np
import pytest
import torch

from oracle import otter_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rng(seed):
    return np.random.default_rng(seed)


def to_dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def host(t):
    return t.detach().float().cpu().numpy()


def relmax(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def ops():
    from otter_amd import _capi, ops as _ops

    assert _capi.lib().otter_device_check() > 0, _capi.lib().otter_last_error()
    return _ops


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm / RMSNorm / colsum
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("rows,D", [(7, 64), (33, 128), (130, 1024), (64, 4096), (5, 8192)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_layernorm_fwd_bwd(ops, rows, D, dt):
    r = rng(rows * D)
    x = r.standard_normal((rows, D)).astype(np.float32) * 2 + 0.5
    w = (1 + 0.1 * r.standard_normal(D)).astype(np.float32)
    b = (0.1 * r.standard_normal(D)).astype(np.float32)
    dy = r.standard_normal((rows, D)).astype(np.float32)
    dres = r.standard_normal((rows, D)).astype(np.float32)
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    if dt == "bf16":
        x, dy = bf16_round(x), bf16_round(dy)
    y_ref, cache = O.layer_norm_fwd(x, w, b)
    y, mean, rstd = ops.layernorm_fwd(to_dev(x, tdt), to_dev(w), to_dev(b), tdt)
    tol = 2e-5 if dt == "f32" else 1e-2
    assert relmax(host(y), y_ref) < tol
    assert relmax(host(mean), x.mean(-1)) < 1e-5 and relmax(host(rstd), cache[1][:, 0]) < 1e-4
    dx_ref, dw_ref, db_ref = O.layer_norm_bwd(dy, cache)
    dx, dg, db = ops.layernorm_bwd(to_dev(dy, tdt), to_dev(x, tdt), to_dev(w), mean, rstd, torch.float32, dres=to_dev(dres))
    assert relmax(host(dx), dx_ref + dres) < 5e-5
    assert relmax(host(dg), dw_ref) < 1e-4 and relmax(host(db), db_ref) < 1e-4


@pytest.mark.parametrize("rows,D", [(37, 512), (130, 1024), (70, 4096), (4097, 1536), (4096, 4096), (67, 3584)])
def test_norm_training_config_vs_oracle(ops, rows, D):
    """The coalesced row kernels (fp32 stream, bf16 branch tensors, D % 512 == 0: norm_fwd_c / norm_bwd_dx_c_kernel; incl. the C2 stream shape and
    row counts that are not multiples of four) against the oracle:
    LayerNorm forward (plain, with fused residual add, through a row map + second output), backward with and without the residual
    gradient / bf16 copy / weight gradients; RMSNorm forward + backward.  Tolerances: bf16 outputs 1e-2, fp32 results 5e-5."""
    from otter_amd._capi import RowMap

    r = rng(rows + D)
    x = (r.standard_normal((rows, D)) * 2 + 0.5).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(D)).astype(np.float32)
    b = (0.1 * r.standard_normal(D)).astype(np.float32)
    dy = bf16_round(r.standard_normal((rows, D)))
    dres = r.standard_normal((rows, D)).astype(np.float32)
    delta = bf16_round(r.standard_normal((rows, D)))
    # forward
    y_ref, cache = O.layer_norm_fwd(x, w, b)
    y, mean, rstd = ops.layernorm_fwd(to_dev(x), to_dev(w), to_dev(b), torch.bfloat16)
    assert y.dtype == torch.bfloat16 and relmax(host(y), y_ref) < 1e-2
    assert relmax(host(mean), x.mean(-1)) < 1e-5 and relmax(host(rstd), cache[1][:, 0]) < 1e-4
    xs, y2, mean2, rstd2 = ops.add_layernorm_fwd(to_dev(x), to_dev(delta, torch.bfloat16), to_dev(w), to_dev(b), torch.bfloat16)
    ys_ref, cache_s = O.layer_norm_fwd(x + delta, w, b)
    assert np.array_equal(host(xs), x + delta) and relmax(host(y2), ys_ref) < 1e-2
    if rows % 2 == 0:   # row-mapped output + the second (contiguous) copy
        half = rows // 2
        buf = torch.zeros((rows + 6, D), dtype=torch.bfloat16, device=DEV)
        ycopy = torch.empty((rows, D), dtype=torch.bfloat16, device=DEV)
        ops.layernorm_fwd(to_dev(x), to_dev(w), to_dev(b), torch.bfloat16, y=buf, ymap=RowMap(half, half + 3, 3), y2=ycopy)
        got = host(buf).reshape(2, half + 3, D)[:, 3:, :].reshape(rows, D)
        assert np.array_equal(got, host(y)) and torch.equal(ycopy, y)
    # backward: dx (+ residual gradient), bf16 copy, weight gradients
    dx_ref, dw_ref, db_ref = O.layer_norm_bwd(dy, cache)
    dxb = torch.empty((rows, D), dtype=torch.bfloat16, device=DEV)
    dx, dg, db = ops.layernorm_bwd(to_dev(dy, torch.bfloat16), to_dev(x), to_dev(w), mean, rstd, torch.float32, dres=to_dev(dres), dx_bf16=dxb)
    assert relmax(host(dx), dx_ref + dres) < 5e-5 and torch.equal(dxb, dx.to(torch.bfloat16))
    assert relmax(host(dg), dw_ref) < 1e-4 and relmax(host(db), db_ref) < 1e-4
    dx0, _, _ = ops.layernorm_bwd(to_dev(dy, torch.bfloat16), to_dev(x), to_dev(w), mean, rstd, torch.float32, need_dw=False)
    assert relmax(host(dx0), dx_ref) < 5e-5
    dxn, _, _ = ops.layernorm_bwd(to_dev(dy, torch.bfloat16), to_dev(x), None, mean, rstd, torch.float32, need_dw=False)   # no affine
    assert relmax(host(dxn), O.layer_norm_bwd(dy, (cache[0], cache[1], None))[0]) < 5e-5
    # RMSNorm (LLaMA host): fp32 stream, bf16 out; backward with residual gradient and weight gradient
    xs2, yr, rs = ops.add_rmsnorm_fwd(to_dev(x), to_dev(delta, torch.bfloat16), to_dev(w), torch.bfloat16)
    yr_ref, c = O.rms_norm_fwd(x + delta, w, 1e-6)
    assert np.array_equal(host(xs2), x + delta) and relmax(host(yr), yr_ref) < 1e-2
    dxr_ref, dwr_ref = O.rms_norm_bwd(dy, c)
    dxr, dwr = ops.rmsnorm_bwd_ex(to_dev(dy, torch.bfloat16), xs2, to_dev(w), rs, torch.float32, dres=to_dev(dres), need_dw=True)
    assert relmax(host(dxr), dxr_ref + dres) < 5e-5 and relmax(host(dwr), dwr_ref) < 1e-4


def test_layernorm_rowmap_and_nobias(ops):
    from otter_amd._capi import RowMap

    r = rng(5)
    G, n1, n2, D = 3, 10, 4, 128
    x = r.standard_normal((G * n1, D)).astype(np.float32)
    l = r.standard_normal((G * n2, D)).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(D)).astype(np.float32)
    buf = torch.full((G * (n1 + n2), D), float("nan"), device=DEV)
    ops.layernorm_fwd(to_dev(x), to_dev(w), None, torch.float32, y=buf, ymap=RowMap(n1, n1 + n2, 0))
    y2 = torch.empty((G * n2, D), device=DEV)
    _, mean_l, rstd_l = ops.layernorm_fwd(to_dev(l), to_dev(w), None, torch.float32, y=buf, ymap=RowMap(n2, n1 + n2, n1), y2=y2)
    yx, _ = O.layer_norm_fwd(x, w, None)
    yl, cl = O.layer_norm_fwd(l, w, None)
    ref = np.concatenate([yx.reshape(G, n1, D), yl.reshape(G, n2, D)], axis=1).reshape(-1, D)
    assert relmax(host(buf), ref) < 2e-5 and relmax(host(y2), yl) < 2e-5
    # backward reading dy through the same map
    dbuf = r.standard_normal((G * (n1 + n2), D)).astype(np.float32)
    dyl = dbuf.reshape(G, n1 + n2, D)[:, n1:, :].reshape(-1, D)
    dx_ref, dw_ref, _ = O.layer_norm_bwd(dyl, cl)
    dx, dg, db = ops.layernorm_bwd(to_dev(dbuf), to_dev(l), to_dev(w), mean_l, rstd_l, torch.float32,
                                   dymap=RowMap(n2, n1 + n2, n1), need_dbeta=False)
    assert relmax(host(dx), dx_ref) < 5e-5 and relmax(host(dg), dw_ref) < 1e-4 and db is None
    # add_rows / colsum through the same map
    dst = r.standard_normal((G * n2, D)).astype(np.float32)
    out = ops.add_rows_(to_dev(dst), to_dev(dbuf), RowMap(n2, n1 + n2, n1))
    assert relmax(host(out), dst + dyl) < 1e-6
    cs = ops.colsum(to_dev(dbuf), RowMap(n2, n1 + n2, n1), G * n2)
    assert relmax(host(cs), dyl.sum(0)) < 1e-5


def test_add_layernorm_fused(ops):
    """xsum = x + delta (fp32 residual, bf16 delta), y = LN(xsum) in bf16 -- the MPT block's residual-add + norm_2 pair."""
    r = rng(123)
    rows, D = 70, 4096
    x = r.standard_normal((rows, D)).astype(np.float32)
    delta = bf16_round(r.standard_normal((rows, D)).astype(np.float32))
    w = (1 + 0.1 * r.standard_normal(D)).astype(np.float32)
    xsum, y, mean, rstd = ops.add_layernorm_fwd(to_dev(x), to_dev(delta, torch.bfloat16), to_dev(w), None, torch.bfloat16)
    assert np.array_equal(host(xsum), x + delta)  # fp32 add of the same operands: bit-exact
    y_ref, _ = O.layer_norm_fwd(x + delta, w, None)
    assert relmax(host(y), y_ref) < 1e-2 and y.dtype == torch.bfloat16
    # backward with the fused bf16 copy of dx (the branch gradient): identical to casting dx afterwards
    dy = to_dev(bf16_round(r.standard_normal((rows, D)).astype(np.float32)), torch.bfloat16)
    dres = to_dev(r.standard_normal((rows, D)).astype(np.float32))
    dx2 = torch.empty(rows, D, dtype=torch.bfloat16, device=DEV)
    dx, _, _ = ops.layernorm_bwd(dy, xsum, to_dev(w), mean, rstd, torch.float32, dres=dres, need_dw=False, dx_bf16=dx2)
    dx_plain, _, _ = ops.layernorm_bwd(dy, xsum, to_dev(w), mean, rstd, torch.float32, dres=dres, need_dw=False)
    assert torch.equal(dx, dx_plain) and torch.equal(dx2, dx.to(torch.bfloat16))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rmsnorm(ops, dt):
    r = rng(9)
    rows, D = 37, 4096
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    x = r.standard_normal((rows, D)).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(D)).astype(np.float32)
    dy = r.standard_normal((rows, D)).astype(np.float32)
    if dt == "bf16":
        x, dy, w = bf16_round(x), bf16_round(dy), bf16_round(w)
    y, rstd = ops.rmsnorm_fwd(to_dev(x, tdt), to_dev(w, tdt))
    if dt == "f32":
        y_ref, c = O.rms_norm_fwd(x, w, 1e-6)
        assert relmax(host(y), y_ref) < 2e-5
        dx_ref, dw_ref = O.rms_norm_bwd(dy, c)
        dx, dw = ops.rmsnorm_bwd(to_dev(dy), to_dev(x), to_dev(w), rstd)
        assert relmax(host(dx), dx_ref) < 5e-5 and relmax(host(dw), dw_ref) < 1e-4
    else:
        var = (x.astype(np.float64) ** 2).mean(-1, keepdims=True)
        xn = bf16_round((x / np.sqrt(var + 1e-6)).astype(np.float32))
        assert relmax(host(y), bf16_round(w * xn)) < 1e-2


def test_llama_ops_golden(ops):
    """RMSNorm + RoPE against the fixture produced by transformers' LlamaRMSNorm / apply_rotary_pos_emb."""
    from oracle import synth
    from tests import _golden as G

    m = G.meta()["llama_ops"]
    gold = G.load("llama_ops")
    s = m["seed"]
    x = synth.tensor(s, "rms.x", (2 * m["S"], m["D"]))
    w = synth.tensor(s, "rms.w", (m["D"],), 0.1, 1.0)
    y, rstd = ops.rmsnorm_fwd(to_dev(x), to_dev(w))
    assert relmax(host(y), gold["rms_y"].reshape(-1, m["D"])) < 2e-5
    dx, dw = ops.rmsnorm_bwd(to_dev(synth.tensor(s, "rms.R", (2 * m["S"], m["D"]))), to_dev(x), to_dev(w), rstd)
    assert relmax(host(dx), gold["rms_dx"].reshape(-1, m["D"])) < 5e-5 and relmax(host(dw), gold["rms_dw"]) < 1e-4
    cos, sin = O.rope_tables(m["S"], m["d"])
    q = synth.tensor(s, "rope.q", (2, m["H"], m["S"], m["d"])).transpose(0, 2, 1, 3).copy()
    qe = ops.rope(to_dev(q), to_dev(cos), to_dev(sin))
    assert relmax(host(qe).transpose(0, 2, 1, 3), gold["rope_q"]) < 1e-5
    R = synth.tensor(s, "rope.R", (2, m["H"], m["S"], m["d"])).transpose(0, 2, 1, 3).copy()
    dq = ops.rope(to_dev(R), to_dev(cos), to_dev(sin), inverse=True)
    assert relmax(host(dq).transpose(0, 2, 1, 3), gold["rope_dq"]) < 1e-5
    # partial rotary (Persimmon): rot_dim = d/2, bf16, round trip forward -> inverse = identity on every element
    xb = to_dev(bf16_round(q), torch.bfloat16)
    c2, s2 = O.rope_tables(m["S"], m["d"] // 2)
    yb = ops.rope(xb, to_dev(c2), to_dev(s2), rot_dim=m["d"] // 2)
    assert relmax(host(yb), O.rope_fwd(host(xb), c2, s2, m["d"] // 2)) < 1e-2
    assert torch.equal(yb[..., m["d"] // 2:], xb[..., m["d"] // 2:])


# ----------------------------------------------------------------------------------------------------------------------
# GEMM (all variants, all epilogues)
# ----------------------------------------------------------------------------------------------------------------------

# The library carries the schedules pick_cfg can choose (1-3, 13, 25, 26, 30); the kernel generations that led to them (rounds 1-2:
# 4-12, 14-23, 27-29) are retired and refused by otter_gemm_set_variant.
LIVE_VARIANTS = [1, 2, 3, 13, 25, 26, 30]


GEMM_SHAPES = [(48, 128, 48), (200, 136, 328), (257, 512, 64), (64, 384, 1024), (520, 264, 200), (300, 520, 256), (513, 260, 128)]


@pytest.mark.parametrize("variant", LIVE_VARIANTS)
@pytest.mark.parametrize("M,N,Kd", GEMM_SHAPES)
def test_gemm_bf16_store(ops, variant, M, N, Kd):
    ops.set_gemm_variant(variant)
    try:
        r = rng(M + N + Kd)
        A = bf16_round(r.standard_normal((M, Kd)))
        B = bf16_round(r.standard_normal((N, Kd)))
        ref = A.astype(np.float64) @ B.astype(np.float64).T
        C = ops.gemm_nt(to_dev(A, torch.bfloat16), to_dev(B, torch.bfloat16), out_dtype=torch.float32)
        assert relmax(host(C), ref) < 1e-4  # asymmetric random A/B: a transposed or permuted tile cannot pass
        Cb = ops.gemm_nt(to_dev(A, torch.bfloat16), to_dev(B, torch.bfloat16))
        assert Cb.dtype == torch.bfloat16 and relmax(host(Cb), ref) < 1e-2
    finally:
        ops.set_gemm_variant(0)


@pytest.mark.parametrize("M,N,Kd", GEMM_SHAPES + [(4, 4, 4), (65, 68, 36)])
def test_gemm_f32_store(ops, M, N, Kd):
    r = rng(M * 3 + N + Kd)
    A = r.standard_normal((M, Kd)).astype(np.float32)
    B = r.standard_normal((N, Kd)).astype(np.float32)
    ref = A.astype(np.float64) @ B.astype(np.float64).T
    C = ops.gemm_nt(to_dev(A), to_dev(B))
    assert relmax(host(C), ref) < 2e-6 * max(1, Kd ** 0.5)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("variant", [1, 2, 13, 25, 26, 30])
def test_gemm_epilogues(ops, dt, variant):
    from otter_amd._capi import EPI_GATE_BWD, EPI_GELU, EPI_SCALE_RES, EPI_STORE

    ops.set_gemm_variant(variant)
    try:
        r = rng(77 + variant)
        M, N, Kd = 300, 264, (256 if variant >= 17 else 136)  # variants 17/18 need K % 128 == 0 (else it defers to 13)
        tdt = torch.float32 if dt == "f32" else torch.bfloat16
        A = r.standard_normal((M, Kd)).astype(np.float32) * 0.3
        B = r.standard_normal((N, Kd)).astype(np.float32) * 0.3
        R = r.standard_normal((M, N)).astype(np.float32)
        aux = r.standard_normal((M, N)).astype(np.float32)
        if dt == "bf16":
            A, B, aux = bf16_round(A), bf16_round(B), bf16_round(aux)
        acc = A.astype(np.float64) @ B.astype(np.float64).T
        gate = np.array([0.7], np.float32)
        s = np.tanh(0.7)
        dA, dB, dgate = to_dev(A, tdt), to_dev(B, tdt), to_dev(gate)
        tol = 3e-5 if dt == "f32" else 1e-4
        # GELU with pre-activation copy
        C2 = torch.empty((M, N), dtype=torch.float32, device=DEV)
        C = ops.gemm_nt(dA, dB, out_dtype=torch.float32, kind=EPI_GELU, C2=C2)
        assert relmax(host(C2), acc) < tol and relmax(host(C), O.gelu_fwd(acc)) < tol
        # SCALE_RES with and without a gate, f32 residual/out
        C = ops.gemm_nt(dA, dB, out_dtype=torch.float32, kind=EPI_SCALE_RES, gate=dgate, R=to_dev(R))
        assert relmax(host(C), acc * s + R) < tol
        C = ops.gemm_nt(dA, dB, out_dtype=torch.float32, kind=EPI_SCALE_RES, R=to_dev(R))
        assert relmax(host(C), acc + R) < tol
        # STORE scaled by the gate, and accumulate
        C = ops.gemm_nt(dA, dB, out_dtype=torch.float32, kind=EPI_STORE, gate=dgate)
        assert relmax(host(C), acc * s) < tol
        ops.gemm_nt(dA, dB, out=C, kind=EPI_STORE, accumulate=True)
        assert relmax(host(C), acc * s + acc) < tol
        # GATE_BWD, the three aux activations (identity, erf GELU, squared ReLU)
        for aux_gelu in (False, True, "sqrelu"):
            part = torch.zeros(ops.gemm_num_partials(M, N, tdt), dtype=torch.float32, device=DEV)
            C = ops.gemm_nt(dA, dB, out_dtype=torch.float32, kind=EPI_GATE_BWD, gate=dgate, aux=to_dev(aux, tdt), aux_gelu=aux_gelu,
                            partial=part)
            if aux_gelu == "sqrelu":
                f, fp = np.maximum(aux, 0.0) ** 2, 2.0 * np.maximum(aux, 0.0)
            else:
                f = O.gelu_fwd(aux.astype(np.float64)) if aux_gelu else aux
                fp = O.gelu_grad(aux.astype(np.float64)) if aux_gelu else 1.0
            assert relmax(host(C), s * acc * fp) < tol
            dg = ops.reduce_partials(part, gate=dgate)
            assert abs(float(dg[0]) - (acc * f).sum() * (1 - s * s)) < 1e-3 * abs((acc * f).sum() * (1 - s * s)) + 1e-3
    finally:
        ops.set_gemm_variant(0)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(300, 264, 256), (1024, 2048, 512), (4096, 16384, 256)])
def test_gemm_gelu_derivative_stash(ops, dt, shape):
    """Round 6c, otter_epilogue_args::aux_is_gelu_input == 3: a GELU launch writes C = GELU(acc) and C2 = GELU'(acc) (instead of acc), a
    GATE_BWD launch whose aux holds that derivative only multiplies.  Every kernel family the shapes select (ring, large-grid incl. the
    cross-tile form, edge tiles), fp32 and bf16 results; the pair composes to what the plain pair (C2 = acc, aux = acc with the GELU flag)
    gives, within the rounding of the stashed value."""
    from otter_amd._capi import EPI_GATE_BWD, EPI_GELU

    M, N, Kd = shape
    r = rng(601 + M)
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    A = r.standard_normal((M, Kd)).astype(np.float32) * 0.12
    B = r.standard_normal((N, Kd)).astype(np.float32) * 0.12
    if dt == "bf16":
        A, B = bf16_round(A), bf16_round(B)
    dA, dB = to_dev(A, tdt), to_dev(B, tdt)
    acc = torch.from_numpy(A).double().to(DEV) @ torch.from_numpy(B).double().to(DEV).T
    gelu = 0.5 * acc * (1 + torch.erf(acc * 0.5 ** 0.5))
    grad = 0.5 * (1 + torch.erf(acc * 0.5 ** 0.5)) + acc * torch.exp(-0.5 * acc * acc) * (1.0 / (2 * np.pi) ** 0.5)
    for odt in ([torch.float32] if dt == "f32" else [torch.float32, torch.bfloat16]):
        tol = (3e-5 if dt == "f32" else 1e-4) if odt == torch.float32 else 6e-3
        C2 = torch.empty((M, N), dtype=odt, device=DEV)
        C = ops.gemm_nt(dA, dB, out_dtype=odt, kind=EPI_GELU, C2=C2, aux_gelu="stash")
        assert float((C.double() - gelu).abs().max()) < tol * float(gelu.abs().max()) + tol
        assert float((C2.double() - grad).abs().max()) < tol * 1.13 + tol       # GELU' lies in [-0.13, 1.13]
        # the plain pair on the same operands: same C bit for bit (the stash only changes what lands in C2)
        U = torch.empty((M, N), dtype=odt, device=DEV)
        Cp = ops.gemm_nt(dA, dB, out_dtype=odt, kind=EPI_GELU, C2=U)
        assert torch.equal(C, Cp)
        # backward: a product times the stash, against the plain tail on the stored pre-activation
        if odt == tdt:
            dU_s = ops.gemm_nt(dA, dB, out_dtype=odt, kind=EPI_GATE_BWD, aux=C2, aux_gelu="stash")
            dU_p = ops.gemm_nt(dA, dB, out_dtype=odt, kind=EPI_GATE_BWD, aux=U, aux_gelu=True)
            want = acc * grad
            scale = float(want.abs().max())
            e_s, e_p = float((dU_s.double() - want).abs().max()) / scale, float((dU_p.double() - want).abs().max()) / scale
            assert e_s < (1e-4 if odt == torch.float32 else 1.2e-2), (e_s, e_p)
            assert e_s < 2.0 * e_p + 1e-4, (e_s, e_p)          # not worse than the plain form beyond the one extra rounding
    with pytest.raises(Exception):     # no gate partial from a stashed derivative
        part = torch.zeros(ops.gemm_num_partials(M, N, tdt), dtype=torch.float32, device=DEV)
        ops.gemm_nt(dA, dB, out_dtype=tdt, kind=EPI_GATE_BWD, aux=to_dev(np.zeros((M, N), np.float32), tdt), aux_gelu="stash", partial=part)


@pytest.mark.parametrize("variant", [25, 26, 30])
@pytest.mark.parametrize("out_dt", ["bf16", "f32"])
def test_gemm_full_tile_fast_tail(ops, variant, out_dt):
    """The one-wave-per-SIMD kernels take an unrolled, double-buffered tail on full in-bounds tiles: every epilogue kind and
    both output dtypes against the 8-wave kernel (variant 13, generic tail) on a 512 x 768 x 256 problem -- same per-element
    accumulation order, so the results must agree to the last bit -- and against the fp64 product."""
    from otter_amd._capi import EPI_GATE_BWD, EPI_GELU, EPI_SCALE_RES, EPI_STORE

    r = rng(900 + variant)
    M, N, Kd = 512, 768, 256
    odt = torch.bfloat16 if out_dt == "bf16" else torch.float32
    A = to_dev(bf16_round(r.standard_normal((M, Kd)) * 0.3), torch.bfloat16)
    B = to_dev(bf16_round(r.standard_normal((N, Kd)) * 0.3), torch.bfloat16)
    R = to_dev(r.standard_normal((M, N)).astype(np.float32))
    aux = to_dev(bf16_round(r.standard_normal((M, N))), torch.bfloat16)
    gate = to_dev(np.array([0.7], np.float32))
    ref = host(A).astype(np.float64) @ host(B).astype(np.float64).T

    def run(v):
        ops.set_gemm_variant(v)
        out = {}
        out["store"] = ops.gemm_nt(A, B, out_dtype=odt, kind=EPI_STORE, gate=gate)
        C2 = torch.empty((M, N), dtype=odt, device=DEV)
        out["gelu"] = ops.gemm_nt(A, B, out_dtype=odt, kind=EPI_GELU, C2=C2)
        out["gelu_pre"] = C2
        out["res"] = ops.gemm_nt(A, B, out_dtype=odt, kind=EPI_SCALE_RES, gate=gate, R=R)
        for ag in (False, True):
            part = torch.zeros(ops.gemm_num_partials(M, N, torch.bfloat16), dtype=torch.float32, device=DEV)
            out["gbwd%d" % ag] = ops.gemm_nt(A, B, out_dtype=odt, kind=EPI_GATE_BWD, gate=gate, aux=aux, aux_gelu=ag, partial=part)
            out["gpart%d" % ag] = ops.reduce_partials(part, gate=gate)
        if out_dt == "f32":
            acc = out["store"].clone()
            ops.gemm_nt(A, B, out=acc, kind=EPI_STORE, accumulate=True)
            out["accum"] = acc
        return out

    from otter_amd import _capi as K_

    try:
        # variant 26 walks a tile's K-tiles rotated by the tile's XCD since round 6 (another fp32 summation order than variant 13's): the
        # bit-for-bit comparison of the TAILS runs it with the plain K order (otter_gemm_set_debug bit 23 = take bits 16-22 as the order: 0)
        K_.gemm_set_debug(1 << 23)
        mine, base = run(variant), run(13)
    finally:
        K_.gemm_set_debug(0)
        ops.set_gemm_variant(0)
    for k in base:
        if k.startswith("gpart"):   # block partials are summed in a different order (4 vs 8 waves)
            assert abs(float(mine[k][0]) - float(base[k][0])) <= 1e-4 * abs(float(base[k][0])) + 1e-4, k
        else:
            assert torch.equal(mine[k], base[k]), k
    tol = 1e-2 if out_dt == "bf16" else 1e-4
    assert relmax(host(mine["store"]), ref * np.tanh(0.7)) < tol
    assert relmax(host(mine["gelu_pre"]), ref) < tol


@pytest.mark.parametrize("variant", [26])
def test_gemm_persistent_blocks_with_several_tiles(ops, variant):
    """More tiles than CUs (17 x 16 = 272 tiles of 256 x 256, K = 384 -> the tail-trip-only K loop of nk = 6): the persistent blocks
    walk 2 tiles each for 16 of them, which is where the cross-tile form requests the next tile's first K-tiles from inside the K loop.  Bit-exact
    against the 8-wave kernel for a plain and a residual epilogue, and against fp64."""
    from otter_amd._capi import EPI_SCALE_RES

    r = rng(333)
    M, N, Kd = 4352, 4096, 384
    A = to_dev(bf16_round(r.standard_normal((M, Kd)) * 0.5), torch.bfloat16)
    B = to_dev(bf16_round(r.standard_normal((N, Kd)) * 0.5), torch.bfloat16)
    R = to_dev(r.standard_normal((M, N)).astype(np.float32))
    from otter_amd import _capi as K_

    outs = {}
    try:
        K_.gemm_set_debug(1 << 23)   # plain K order (variant 26 rotates it by the tile's N panel: another summation order)
        for v in (13, variant):
            ops.set_gemm_variant(v)
            outs[v] = (ops.gemm_nt(A, B), ops.gemm_nt(A, B, out_dtype=torch.float32, kind=EPI_SCALE_RES, R=R))
    finally:
        K_.gemm_set_debug(0)
        ops.set_gemm_variant(0)
    assert torch.equal(outs[13][0], outs[variant][0]) and torch.equal(outs[13][1], outs[variant][1])
    ref = host(A[:300]).astype(np.float64) @ host(B).astype(np.float64).T
    assert relmax(host(outs[variant][0][:300]), ref) < 1e-2


BENCH_GEMMS = [
    # (M, N, K, kind, out dtype, operand layout): every launch of the gated cross-attention block at config C2 (B*T = 4096 tokens, D = 4096,
    # FFN 16384, inner 512) AS THE BENCHMARK ISSUES IT since round 3 -- T4 (variant 26) for the FFN shapes, S4 (variant 25) for the
    # projections; "nt" = both operands K-contiguous (otter_gemm_nt: the forward products), "ab" = both K-major (the weight gradients
    # dW = dy^T x: token rows are the reduction index of both operands as they lie), "b" = B K-major (the input gradients dx = dy W with
    # W as stored [out, in]).  roofline.by_layout of the bench line counts 320 of 480 FFN-shape launches in the K-major forms.
    (4096, 16384, 4096, "gelu", "bf16", "nt"),        # FF1 forward: h = gelu(f W1^T), u stored beside it
    (4096, 4096, 16384, "res", "f32", "nt"),          # FF2 forward: y = (h W2^T) tanh(g) + x1, fp32 stream
    (4096, 16384, 4096, "gate_bwd", "bf16", "b"),     # dU = (dy W2) tanh(g) gelu'(u), W2 [4096, 16384] as stored = [K][N]
    (4096, 4096, 16384, "store", "bf16", "b"),        # df = dU W1, W1 [16384, 4096] as stored
    (16384, 4096, 4096, "store", "f32", "ab"),        # dW1 = dU^T f        (fp32 weight gradient; dU [tokens, 16384], f [tokens, 4096])
    (4096, 16384, 4096, "store_gate", "f32", "ab"),   # dW2 = tanh(g) dy^T h (fp32 weight gradient with the gate folded in)
    (4096, 16384, 4096, "gate_bwd", "bf16", "nt"),    # round-2 forms of the same four products (OTTER_NO_KMAJOR=1, and what C4 / C5 fall
    (4096, 4096, 16384, "store", "bf16", "nt"),       # back to when a shape is not K-major capable): transposed copies + otter_gemm_nt
    (16384, 4096, 4096, "store_gate", "f32", "nt"),
    (4096, 16384, 4096, "store_gate", "f32", "nt"),
    (4096, 512, 4096, "store", "bf16", "nt"),         # to_q
    (4096, 4096, 512, "res", "f32", "nt"),            # to_out + gate + residual
    (512, 4096, 4096, "store_gate", "f32", "nt"),     # dWq
    (4096, 512, 4096, "store_gate", "f32", "nt"),     # dWo
]


@pytest.mark.parametrize("M,N,Kd,kind,out_dt,layout", BENCH_GEMMS)
def test_gemm_bench_shapes(ops, M, N, Kd, kind, out_dt, layout):
    """the kernels the benchmark times, at the benchmark's shapes AND operand layouts, with the fused tails
    and the fp32-output weight-gradient form -- default dispatch (variant 0).  The K-major launches are judged against the fp64 product
    like the others (not against the K-contiguous kernel).  A full fp64 product of 4096 x 16384 x 4096 is too slow for the host, so:
    (a) 96 sampled rows and 96 sampled columns (incl. first / last of every 256-tile edge) against the fp64 product of those rows /
    columns; (b) a checksum over EVERY element through linearity: C 1 = A (B^T 1) for the plain store (fp64 on the host, O(MK + NK))."""
    from otter_amd._capi import EPI_GATE_BWD, EPI_GELU, EPI_SCALE_RES, EPI_STORE

    r = rng(M // 7 + N + Kd)
    A = bf16_round(r.standard_normal((M, Kd)).astype(np.float32) * 0.25)
    B = bf16_round(r.standard_normal((N, Kd)).astype(np.float32) * 0.25)
    ta, tb = layout == "ab", layout in ("ab", "b")
    # a K-major operand is handed over as it lies in the backward pass: [K rows][M or N columns]
    dA = to_dev(np.ascontiguousarray(A.T) if ta else A, torch.bfloat16)
    dB = to_dev(np.ascontiguousarray(B.T) if tb else B, torch.bfloat16)
    if ta or tb:
        assert ops.gemm_kmajor_supported(M, N, Kd, dA.stride(0), dB.stride(0), ta, tb, torch.bfloat16)
    _nt = ops.gemm_nt

    def gemm_nt(a, b, **kw):
        return _nt(a, b, a_kmajor=ta, b_kmajor=tb, **kw)

    odt = torch.bfloat16 if out_dt == "bf16" else torch.float32
    gate = np.array([0.6], np.float32)
    s = float(np.tanh(0.6))
    rows = np.unique(np.concatenate([[0, 255, 256, M - 257, M - 1], r.integers(0, M, 91)]))
    cols = np.unique(np.concatenate([[0, 255, 256, N - 257, N - 1], r.integers(0, N, 91)]))
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    acc_r = A64[rows] @ B64.T              # [rows, N]
    acc_c = A64 @ B64[cols].T              # [M, cols]
    tol = 1e-2 if out_dt == "bf16" else 2e-4

    def check(C, f, tol_=tol):
        Ch = host(C)
        assert relmax(Ch[rows], f(acc_r, rows, slice(None))) < tol_
        assert relmax(Ch[:, cols], f(acc_c, slice(None), cols)) < tol_

    if kind == "store":
        C = gemm_nt(dA, dB, out_dtype=odt)
        check(C, lambda a, i, j: a)
    elif kind == "store_gate":
        C = gemm_nt(dA, dB, out_dtype=odt, kind=EPI_STORE, gate=to_dev(gate))
        check(C, lambda a, i, j: a * s)
        # checksum of every element: row sums of C == s * A (sum_n B[n, :])
        rs = host(C).astype(np.float64).sum(1)
        want = s * (A64 @ B64.sum(0))
        assert np.abs(rs - want).max() < 1e-3 * np.abs(want).max() + 1e-3 * np.sqrt(N)
    elif kind == "gelu":
        C2 = torch.empty((M, N), dtype=odt, device=DEV)
        C = gemm_nt(dA, dB, out_dtype=odt, kind=EPI_GELU, C2=C2)
        check(C2, lambda a, i, j: a)
        check(C, lambda a, i, j: O.gelu_fwd(a))
    elif kind == "res":
        R = r.standard_normal((M, N)).astype(np.float32)
        C = gemm_nt(dA, dB, out_dtype=odt, kind=EPI_SCALE_RES, gate=to_dev(gate), R=to_dev(R))
        check(C, lambda a, i, j: a * s + R[i, j].astype(np.float64))
    else:
        aux = bf16_round(r.standard_normal((M, N)).astype(np.float32))
        part = torch.zeros(ops.gemm_num_partials(M, N, torch.bfloat16), dtype=torch.float32, device=DEV)
        C = gemm_nt(dA, dB, out_dtype=odt, kind=EPI_GATE_BWD, gate=to_dev(gate), aux=to_dev(aux, torch.bfloat16), aux_gelu=True, partial=part)
        check(C, lambda a, i, j: s * a * O.gelu_grad(aux[i, j].astype(np.float64)))
        # the gate gradient = (1 - s^2) sum(acc * gelu(aux)) over EVERY element: against an independent fp32 product (torch / rocBLAS on
        # the same device, fp64 reduction) -- the per-tile partials + reduce kernel see all 64 M accumulators
        dg = float(ops.reduce_partials(part, gate=to_dev(gate))[0])
        acc_t = torch.matmul(dA.float().t() if ta else dA.float(), dB.float() if tb else dB.float().t())
        want = float((acc_t.double() * torch.nn.functional.gelu(to_dev(aux).double())).sum()) * (1 - s * s)
        scale = float((acc_t.double() * torch.nn.functional.gelu(to_dev(aux).double())).abs().sum()) * (1 - s * s)
        assert abs(dg - want) < 1e-5 * scale + 1e-3


@pytest.mark.parametrize("M,N,Kd", [(4096, 512, 4096), (512, 4096, 4096), (512, 1024, 4096), (520, 384, 1024), (72, 128, 512)])
def test_gemm_half_height_ring_equals_ring(ops, M, N, Kd):
    """Round 4, variant 30 (64 x 128 tiles of the small-grid ring kernel: the skinny projections of the gated block / the resampler's
    512-row products on twice the workgroups).  Same fragments and per-element accumulation order as variant 25 -> bit-identical results
    for every epilogue kind and both output dtypes, ragged M / N edges included; fp64 product on sampled rows; and the default dispatch
    (variant 0) takes it exactly for the few-tile shapes."""
    from otter_amd._capi import EPI_GATE_BWD, EPI_GELU, EPI_SCALE_RES, EPI_STORE

    r = rng(M + N + Kd)
    A = to_dev(bf16_round(r.standard_normal((M, Kd)) * 0.3), torch.bfloat16)
    B = to_dev(bf16_round(r.standard_normal((N, Kd)) * 0.3), torch.bfloat16)
    R = to_dev(r.standard_normal((M, N)).astype(np.float32))
    aux = to_dev(bf16_round(r.standard_normal((M, N))), torch.bfloat16)
    gate = to_dev(np.array([0.7], np.float32))

    def run(v):
        ops.set_gemm_variant(v)
        out = {}
        for odt, tag in ((torch.bfloat16, "b"), (torch.float32, "f")):
            out["store" + tag] = ops.gemm_nt(A, B, out_dtype=odt, kind=EPI_STORE, gate=gate)
            C2 = torch.empty((M, N), dtype=odt, device=DEV)
            out["gelu" + tag] = ops.gemm_nt(A, B, out_dtype=odt, kind=EPI_GELU, C2=C2)
            out["pre" + tag] = C2
            out["res" + tag] = ops.gemm_nt(A, B, out_dtype=odt, kind=EPI_SCALE_RES, gate=gate, R=R)
            out["gbwd" + tag] = ops.gemm_nt(A, B, out_dtype=odt, kind=EPI_GATE_BWD, gate=gate, aux=aux, aux_gelu=True)    # (no partials: stays on 30)
        acc = out["storef"].clone()
        ops.gemm_nt(A, B, out=acc, kind=EPI_STORE, accumulate=True)
        out["accum"] = acc
        return out

    try:
        half, ring, auto = run(30), run(25), run(0)
    finally:
        ops.set_gemm_variant(0)
    for k in ring:
        assert torch.equal(half[k], ring[k]), k
        assert torch.equal(auto[k], ring[k]), k
    rows = np.unique(np.concatenate([[0, 63, 64, M - 1], r.integers(0, M, 40)]))
    ref = host(A)[rows].astype(np.float64) @ host(B).astype(np.float64).T
    assert relmax(host(half["storef"])[rows], ref * np.tanh(0.7)) < 2e-4
    assert relmax(host(half["preb"])[rows], ref) < 1e-2


KMAJOR_CASES = [
    # (M, N, K, a_kmajor, b_kmajor, extra leading-dimension padding): >= 192 tiles of 256 x 256, K % 128 == 0
    (4096, 4096, 256, True, True, 0),       # wgrad form, square grid
    (4096, 4096, 256, False, True, 0),      # dgrad form (W as stored)
    (4096, 4096, 256, True, False, 0),
    (3592, 3600, 384, True, True, 8),       # ragged M / N edges (multiples of 8, not of 256) + padded leading dimensions
    (3592, 3600, 384, False, True, 24),
    (4096, 16384, 512, True, True, 0),      # the FFN weight-gradient aspect ratio
    (4096, 4096, 328, True, True, 0),       # both K-major: ANY reduction length (config C5: 8 x 1396 = 11168 token rows); rows past K read as zeros
    (3592, 3600, 1400, True, True, 8),      # (the K-contiguous comparison call needs K % 8 == 0; the K-major kernel itself takes any K: see below)
]


@pytest.mark.parametrize("M,N,Kd,ta,tb,pad", KMAJOR_CASES)
def test_gemm_kmajor_operands(ops, M, N, Kd, ta, tb, pad):
    """otter_gemm with K-major operands (round 3: transpose reads in the kernel instead of transpose kernels in HBM) against the SAME
    product issued on explicitly transposed copies through otter_gemm_nt -- identical fragments and accumulation order, so the fp32
    results must agree bit for bit -- and against the fp64 product on sampled rows; asymmetric random operands (a swapped or
    mis-swizzled block cannot pass); fp32 and bf16 outputs; the fused gate and accumulate forms of the weight-gradient call."""
    from otter_amd._capi import EPI_GATE_BWD, EPI_STORE

    r = rng(M + 3 * N + Kd + ta + 2 * tb)
    A = bf16_round(r.standard_normal((M, Kd)).astype(np.float32) * 0.5)     # logical [M, K]
    B = bf16_round(r.standard_normal((N, Kd)).astype(np.float32) * 0.5)     # logical [N, K]

    def operand(X, kmajor):
        t = to_dev(X, torch.bfloat16)
        if not kmajor:
            return t
        rows, cols = X.shape[1], X.shape[0]                  # stored [K, rows_of_X]
        buf = torch.full((rows, cols + pad), float("nan"), dtype=torch.bfloat16, device=DEV)   # NaN padding: never read into a valid output
        buf[:, :cols] = t.t()
        return buf[:, :cols]

    dA, dB = operand(A, ta), operand(B, tb)
    assert ops.gemm_kmajor_supported(M, N, Kd, dA.stride(0), dB.stride(0), ta, tb, torch.bfloat16)
    C = ops.gemm(dA, dB, ta, tb, out_dtype=torch.float32)
    base = ops.gemm_nt(to_dev(A, torch.bfloat16), to_dev(B, torch.bfloat16), out_dtype=torch.float32)
    if Kd % 128 == 0:
        assert torch.equal(C, base)          # same kernel, same fragments, same order
    else:
        assert relmax(host(C), host(base)) < 1e-5     # the K-contiguous side runs another schedule (variant 13) for this K
    rows = np.unique(np.concatenate([[0, 255, 256, M - 1], r.integers(0, M, 60)]))
    ref = A[rows].astype(np.float64) @ B.astype(np.float64).T
    assert relmax(host(C)[rows], ref) < 1e-4
    Cb = ops.gemm(dA, dB, ta, tb)
    assert Cb.dtype == torch.bfloat16
    if Kd % 128 == 0:
        assert torch.equal(Cb, ops.gemm_nt(to_dev(A, torch.bfloat16), to_dev(B, torch.bfloat16)))
    gate = to_dev(np.array([0.4], np.float32))
    acc = ops.gemm(dA, dB, ta, tb, out_dtype=torch.float32, kind=EPI_STORE, gate=gate)
    ops.gemm(dA, dB, ta, tb, out=acc, kind=EPI_STORE, accumulate=True)
    want = ops.gemm_nt(to_dev(A, torch.bfloat16), to_dev(B, torch.bfloat16), out_dtype=torch.float32, kind=EPI_STORE, gate=gate)
    ops.gemm_nt(to_dev(A, torch.bfloat16), to_dev(B, torch.bfloat16), out=want, kind=EPI_STORE, accumulate=True)
    assert torch.equal(acc, want) if Kd % 128 == 0 else relmax(host(acc), host(want)) < 1e-5
    if not ta and tb and pad == 0:       # the dgrad-with-GELU-backward launch (dU = (dy W2) tanh(g) gelu'(u))
        aux = to_dev(bf16_round(r.standard_normal((M, N)).astype(np.float32)), torch.bfloat16)
        p1 = torch.zeros(ops.gemm_num_partials(M, N, torch.bfloat16), dtype=torch.float32, device=DEV)
        p2 = torch.zeros_like(p1)
        x1 = ops.gemm(dA, dB, ta, tb, kind=EPI_GATE_BWD, gate=gate, aux=aux, aux_gelu=True, partial=p1)
        x2 = ops.gemm_nt(to_dev(A, torch.bfloat16), to_dev(B, torch.bfloat16), kind=EPI_GATE_BWD, gate=gate, aux=aux, aux_gelu=True, partial=p2)
        assert torch.equal(x1, x2) and torch.equal(p1, p2)
        # the Persimmon MLP's launch: dh = (dy W) . 2 relu(h), no gate, no partial sums; against the unfused pair (GEMM, then otter_sqrelu_bwd)
        x3 = ops.gemm(dA, dB, ta, tb, kind=EPI_GATE_BWD, aux=aux, aux_gelu="sqrelu")
        plain = ops.gemm(dA, dB, ta, tb, out_dtype=torch.float32)
        want3 = plain * 2.0 * torch.relu(aux.float())
        assert relmax(host(x3), host(want3)) < 1e-2 and relmax(host(x3), host(ops.sqrelu_bwd(aux, plain.to(torch.bfloat16)))) < 2e-2


@pytest.mark.parametrize("M,N,Kd,km", [(4096, 16384, 512, True),     # the FFN weight-gradient launch: both operands K-major, 1024 tiles (variant 26)
                                        (4104, 12304, 256, True),     # ragged edge tiles of the same kernel
                                        (4096, 16384, 256, False),    # K-contiguous operands: the cross-tile form's tail
                                        (1024, 512, 512, False),      # ring kernel (128 x 128 tiles; half-height tiles are not taken with partials)
                                        (200, 136, 64, False)])       # generic kernel, partial tiles
def test_gemm_store_sum_of_squares_partials(ops, M, N, Kd, km):
    """Round 6b: a plain-store launch with an fp32 C also writes sum(C^2) per output tile (otter_epilogue_args::partial) -- the
    clip_grad_norm_ reduction of a weight gradient taken in the launch that produces it.  Against the stored C itself in fp64, with the
    gate scale and in the accumulate form (the sum is of the values as STORED); the stored C is bit-identical to the launch without
    partials; bf16 outputs refuse partials."""
    from otter_amd._capi import EPI_STORE, OtterHipError

    r = rng(M + N + Kd)
    A = to_dev(bf16_round(r.standard_normal((M, Kd)).astype(np.float32) * 0.5), torch.bfloat16)
    B = to_dev(bf16_round(r.standard_normal((N, Kd)).astype(np.float32) * 0.5), torch.bfloat16)
    if km:
        A, B = A.t().contiguous(), B.t().contiguous()
        assert ops.gemm_kmajor_supported(M, N, Kd, A.stride(0), B.stride(0), True, True, torch.bfloat16)
    n = ops.gemm_num_partials(M, N, torch.bfloat16)
    gate = to_dev(np.array([0.4], np.float32))

    def launch(**kw):
        return ops.gemm(A, B, km, km, out_dtype=torch.float32, kind=EPI_STORE, **kw) if km else ops.gemm_nt(A, B, out_dtype=torch.float32, kind=EPI_STORE, **kw)

    for g in (None, gate):
        part = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
        C = launch(gate=g, partial=part)
        assert torch.equal(C, launch(gate=g))
        want = float((C.double() ** 2).sum())
        got = float(part.double().sum())
        assert np.isfinite(got) and abs(got - want) <= 2e-6 * want, (got, want)
    # accumulate: the partials are those of the sum
    part = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    C2 = launch()
    if km:
        ops.gemm(A, B, True, True, out=C2, kind=EPI_STORE, accumulate=True, partial=part)
    else:
        ops.gemm_nt(A, B, out=C2, kind=EPI_STORE, accumulate=True, partial=part)
    want = float((C2.double() ** 2).sum())
    assert abs(float(part.double().sum()) - want) <= 2e-6 * want
    with pytest.raises(OtterHipError):
        (ops.gemm(A, B, True, True, partial=part) if km else ops.gemm_nt(A, B, partial=part))


def test_gemm_kmajor_any_reduction_length(ops):
    """Both operands K-major: K is a row count -- odd values included (rows past K lie outside both descriptors and read as zeros)."""
    r = rng(5)
    M, N, Kd = 4096, 4096, 333
    At = to_dev(bf16_round(r.standard_normal((Kd, M)).astype(np.float32) * 0.5), torch.bfloat16)    # stored [K, M]
    Bt = to_dev(bf16_round(r.standard_normal((Kd, N)).astype(np.float32) * 0.5), torch.bfloat16)
    C = ops.gemm(At, Bt, True, True, out_dtype=torch.float32)
    rows = np.unique(r.integers(0, M, 64))
    ref = host(At).astype(np.float64).T[rows] @ host(Bt).astype(np.float64)
    assert relmax(host(C)[rows], ref) < 1e-4


def test_gemm_kmajor_unsupported_shapes_are_refused(ops):
    from otter_amd import _capi

    A = torch.zeros((256, 512), dtype=torch.bfloat16, device=DEV)      # [K=256, M=512]: 2 x 2 tiles -> small grid
    assert not ops.gemm_kmajor_supported(512, 512, 256, 512, 512, True, True, torch.bfloat16)
    with pytest.raises(_capi.OtterHipError, match="K-major operands need"):
        ops.gemm(A, A, True, True)
    assert not ops.gemm_kmajor_supported(4096, 4096, 192, 4096, 4096, False, True, torch.bfloat16)    # K % 128 with a K-contiguous operand
    assert ops.gemm_kmajor_supported(4096, 4096, 192, 4096, 4096, True, True, torch.bfloat16)         # ... any K when both are K-major
    assert not ops.gemm_kmajor_supported(4096, 4092, 256, 4096, 4092, True, True, torch.bfloat16)     # N % 8


def test_gemm_big_variants_agree(ops):
    """All three bf16 schedules produce the same numbers on the FFN shape class (256-multiple tiles, K=1024)."""
    r = rng(3)
    M, N, Kd = 1024, 2048, 1024
    A = to_dev(r.standard_normal((M, Kd)), torch.bfloat16)
    B = to_dev(r.standard_normal((N, Kd)), torch.bfloat16)
    ref = host(A).astype(np.float64) @ host(B).astype(np.float64).T
    outs = []
    for v in LIVE_VARIANTS:
        ops.set_gemm_variant(v)
        outs.append(ops.gemm_nt(A, B, out_dtype=torch.float32))
    ops.set_gemm_variant(0)
    for o in outs:
        assert relmax(host(o), ref) < 1e-4
    # same tile shape + same per-tile K rotation -> same accumulation order -> bit-identical (register- vs LDS-DMA-staged)
    assert torch.equal(outs[1], outs[2])


def test_transpose_cast(ops):
    r = rng(11)
    a = r.standard_normal((70, 200)).astype(np.float32)
    t, same = ops.transpose(to_dev(a), torch.bfloat16, want_same=True)
    assert t.shape == (200, 72) and torch.equal(t[:, 70:], torch.zeros_like(t[:, 70:]))
    assert np.array_equal(host(t[:, :70]), bf16_round(a).T) and np.array_equal(host(same), bf16_round(a))
    assert np.array_equal(host(ops.cast(to_dev(a), torch.bfloat16)), bf16_round(a))
    t32 = ops.transpose(to_dev(a[:64]), torch.float32)
    assert np.array_equal(host(t32), a[:64].T)
    # vectorised path (everything a multiple of 8), ragged tile edges, both dtype directions
    b = r.standard_normal((200, 136)).astype(np.float32)
    tb, sb = ops.transpose(to_dev(b), torch.bfloat16, want_same=True)
    assert np.array_equal(host(tb), bf16_round(b).T) and np.array_equal(host(sb), bf16_round(b))
    tbb = ops.transpose(to_dev(b, torch.bfloat16), torch.bfloat16)
    assert np.array_equal(host(tbb), bf16_round(b).T)
    tbf = ops.transpose(to_dev(b, torch.bfloat16), torch.float32)
    assert np.array_equal(host(tbf), bf16_round(b).T)


# ----------------------------------------------------------------------------------------------------------------------
# text_time + attention core
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("attend_previous", [True, False])
def test_text_time(ops, attend_previous):
    r = rng(4)
    ml = r.random((5, 333)) < 0.02
    ml[0, :] = False
    ml[1, 0] = True
    tt = ops.text_time(torch.from_numpy(ml).to(DEV), attend_previous)
    assert np.array_equal(host(tt).astype(np.int64), O.text_time(ml, attend_previous))


def _attn_ref(q, k, v, H, tt, n, mode, scale):
    """numpy reference of the attention core with the exact mask semantics (fwd + grads for a given dO)."""
    B, Tq, _ = q.shape
    M = k.shape[1]
    qh = O._split_heads(q, H) * scale
    kh, vh = O._split_heads(k, H), O._split_heads(v, H)
    sim = qh @ np.swapaxes(kh, -1, -2)
    allowed = None
    zero = None
    if mode != 0:
        mt = np.repeat(np.arange(M // n) + 1, n)
        allowed = (tt[:, None, :, None] == mt) if mode == 1 else (tt[:, None, :, None] >= mt)
        sim = np.where(allowed, sim, -np.finfo(np.float32).max)
    p = O.softmax_lastdim(sim)
    if mode == 1:
        zero = (tt == 0)[:, None, :, None]
        p = np.where(zero, 0, p)
    o = O._merge_heads(p @ vh)

    def bwd(do):
        doh = O._split_heads(do, H)
        dv = np.swapaxes(p, -1, -2) @ doh
        dp = doh @ np.swapaxes(vh, -1, -2)
        ds = p * (dp - (dp * p).sum(-1, keepdims=True))
        if allowed is not None:
            ds = np.where(allowed, ds, 0)
        dq = O._merge_heads((ds @ kh) * scale)
        dk = O._merge_heads(np.swapaxes(ds, -1, -2) @ qh)
        return dq, dk, O._merge_heads(dv)

    return o, bwd


ATTN_CASES = [
    # B, H, Tq, M, n, mode            (split-Q: many queries / few keys; split-K: <=64 queries / many keys)
    (2, 8, 24, 24, 8, 1),
    (2, 8, 24, 24, 8, 2),
    (2, 2, 300, 128, 64, 1),
    (1, 8, 16, 26, 1, 0),
    (2, 8, 64, 320, 1, 0),
    (1, 4, 40, 2112, 1, 0),
    (3, 8, 520, 64, 64, 1),
    (2, 4, 200, 192, 64, 2),
    (1, 2, 70, 96, 32, 1),
    # masked split-K on the VALU kernels (Tq <= 64 and M > 256), 5 key tiles of 64 on the MFMA kernels: waves / tiles that see no allowed key
    (2, 2, 40, 320, 64, 1),
    (2, 2, 40, 320, 64, 2),
    # split-K with Tq > 64 (B*H*ceil(Tq/256) = 1*4*2 = 8 < 64, M = 256 >= 256): 5 query blocks of 64, the last with 300 - 256 = 44 live rows
    (1, 4, 300, 256, 64, 1),
    # n % 32 != 0: all three dtypes run the VALU split-K kernels; 33 media, M % 32 = 8 -> a tail chunk of 8 keys
    (1, 2, 70, 264, 8, 2),
    (1, 2, 70, 264, 8, 1),
    # unmasked split-K, M % 32 = 12: ceil(300/32) = 10 chunks over 4 waves -> waves 2 and 3 idle in the third iteration
    (1, 2, 16, 300, 1, 0),
]

# seed offsets of the cases whose default draw (seed = sum(case)) lacks a zeroed row (tt == 0) or a uniform row (tt == t_img + 1)
ATTN_SEED_OFFSET = {(1, 2, 70, 264, 8, 2): 2, (1, 2, 70, 264, 8, 1): 3}


@pytest.mark.parametrize("case", ATTN_CASES)
@pytest.mark.parametrize("dt", ["f32", "bf16", "bf16-valu"])
def test_attention_core(ops, case, dt):
    """bf16 runs the MFMA kernels (attn_mfma.hip) where eligible, "bf16-valu" forces the fp32 VALU kernels on bf16 data."""
    ops.set_attn_variant(1 if dt == "bf16-valu" else 0)
    dt = "bf16" if dt == "bf16-valu" else dt
    try:
        _attention_core_case(ops, case, dt)
    finally:
        ops.set_attn_variant(0)


def _attention_core_case(ops, case, dt):
    B, H, Tq, M, n, mode = case
    r = rng(sum(case) + ATTN_SEED_OFFSET.get(case, 0))
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    inner = H * 64
    q = r.standard_normal((B, Tq, inner)).astype(np.float32)
    kv = r.standard_normal((B, M, 2 * inner)).astype(np.float32)
    do = r.standard_normal((B, Tq, inner)).astype(np.float32)
    if dt == "bf16":
        q, kv, do = bf16_round(q), bf16_round(kv), bf16_round(do)
    tt = None
    if mode != 0:
        t_img = M // n
        ttn = r.integers(0, t_img + 2, size=(B, Tq))  # includes 0 (zeroed rows) and t_img+1 (fully masked -> uniform)
        ttn = np.sort(ttn, axis=1)
        if M >= 256:    # the split-K / many-tile cases: zeroed rows, uniform rows and rows whose media follows fully masked tiles are all present
            assert (ttn == 0).any() and (ttn == t_img + 1).any() and (ttn >= 3).any(), case
        tt = torch.from_numpy(ttn.astype(np.int32)).to(DEV)
    else:
        ttn = None
    scale = 0.125
    o_ref, bwd = _attn_ref(q, kv[..., :inner], kv[..., inner:], H, ttn, n, mode, scale)
    dkv3 = to_dev(kv, tdt)
    dq3 = to_dev(q, tdt)
    o, lse = ops.attn_fwd(dq3, dkv3[..., :inner], dkv3[..., inner:], H, tt, n, mode, scale)
    tol = 3e-5 if dt == "f32" else 1e-2
    assert relmax(host(o), o_ref) < tol
    if dt == "bf16":
        o_used = bf16_round(host(o))  # the backward consumes the stored (rounded) o
    dq_ref, dk_ref, dv_ref = bwd(do)
    dq, dkv = ops.attn_bwd(dq3, dkv3[..., :inner], dkv3[..., inner:], o, to_dev(do, tdt), lse, H, tt, n, mode, scale)
    tolb = 1e-4 if dt == "f32" else 2e-2
    assert relmax(host(dq), dq_ref) < tolb
    assert relmax(host(dkv[..., :inner]), dk_ref) < tolb and relmax(host(dkv[..., inner:]), dv_ref) < tolb


# ----------------------------------------------------------------------------------------------------------------------
# LLaMA host kernels (config C4): fused add + RMSNorm with its own output dtype, strided RoPE, SwiGLU
# ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("with_delta", [False, True])
def test_add_rmsnorm_fwd_bwd(ops, with_delta):
    """fp32 residual stream, bf16 branch: y = bf16(w * x_norm) and the backward (dx + dres, bf16 copy, dw) against the oracle's
    RMSNorm (xformers_model/llama.py:95-112) evaluated in fp32 on x + delta."""
    r = rng(41)
    rows, D = 70, 256
    x = r.standard_normal((rows, D)).astype(np.float32)
    delta = bf16_round(r.standard_normal((rows, D)) * 0.5) if with_delta else None
    w = (1.0 + 0.1 * r.standard_normal(D)).astype(np.float32)
    xs_ref = x + delta if with_delta else x
    y_ref, cache = O.rms_norm_fwd(xs_ref, w)
    xsum, y, rstd = ops.add_rmsnorm_fwd(to_dev(x), to_dev(delta, torch.bfloat16) if with_delta else None, to_dev(w), torch.bfloat16)
    if with_delta:
        assert relmax(host(xsum), xs_ref) < 1e-6
    else:
        assert xsum is None
    assert relmax(host(y), y_ref) < 8e-3            # bf16 rounding of the output
    dy = bf16_round(r.standard_normal((rows, D)))
    dres = r.standard_normal((rows, D)).astype(np.float32)
    dx_ref, dw_ref = O.rms_norm_bwd(dy.astype(np.float32), cache)
    xs_dev = xsum if with_delta else to_dev(x)
    dxb = torch.empty((rows, D), dtype=torch.bfloat16, device=DEV)
    dx, dw = ops.rmsnorm_bwd_ex(to_dev(dy, torch.bfloat16), xs_dev, to_dev(w), rstd, torch.float32, dres=to_dev(dres), need_dw=True,
                                dx_bf16=dxb)
    assert relmax(host(dx), dx_ref + dres) < 1e-5
    assert relmax(host(dxb), dx_ref + dres) < 8e-3
    assert relmax(host(dw), dw_ref) < 1e-4
    dx2, dw2 = ops.rmsnorm_bwd_ex(to_dev(dy, torch.bfloat16), xs_dev, to_dev(w), rstd, torch.float32)   # frozen decoder: no dw, no dres
    assert dw2 is None and relmax(host(dx2), dx_ref) < 1e-5


def test_rope_strided_qkv_buffer(ops):
    """RoPE on the q and k heads inside a fused [B,S,3,H,128] projection buffer -> packed [B,S,2,H,128]; inverse in place.
    Reference: oracle rope (xformers_model/llama.py:158-166) on the bf16 values, fp32 arithmetic."""
    r = rng(43)
    B, S, H, d = 2, 37, 3, 128
    qkv = bf16_round(r.standard_normal((B, S, 3, H, d)))
    cos, sin = O.rope_tables(S, d)
    q_ref = O.rope_fwd(qkv[:, :, 0], cos, sin)
    k_ref = O.rope_fwd(qkv[:, :, 1], cos, sin)
    dq = to_dev(qkv, torch.bfloat16)
    out = torch.zeros((B, S, 2, H, d), dtype=torch.bfloat16, device=DEV)
    ops.rope_strided(dq, out, to_dev(cos), to_dev(sin), B * S, S, 2 * H, d, 3 * H * d, 2 * H * d)
    assert relmax(host(out[:, :, 0]), q_ref) < 8e-3 and relmax(host(out[:, :, 1]), k_ref) < 8e-3
    # in place + inverse on a gradient buffer: q|k parts rotated back, the v part untouched
    g = bf16_round(r.standard_normal((B, S, 3, H, d)))
    dg = to_dev(g, torch.bfloat16)
    ops.rope_strided(dg, dg, to_dev(cos), to_dev(sin), B * S, S, 2 * H, d, 3 * H * d, 3 * H * d, inverse=True)
    assert relmax(host(dg[:, :, 0]), O.rope_bwd(g[:, :, 0], cos, sin)) < 8e-3
    assert relmax(host(dg[:, :, 1]), O.rope_bwd(g[:, :, 1], cos, sin)) < 8e-3
    assert np.array_equal(host(dg[:, :, 2]), g[:, :, 2])


def test_gelu_fwd_bwd(ops):
    """Decoder-MLP GELU kernels vs the oracle's exact-erf GELU (float64): fp32 to 1e-6 of the range, bf16 to output rounding;
    in-place forms; the tails (|x| up to 12) must come out as 0 / x exactly like erf's saturation."""
    from oracle import otter_oracle as O

    r = rng(53)
    x = np.concatenate([r.standard_normal(4096 - 16) * 3, np.array([0.0, -0.0, 12.0, -12.0, 6.5, -6.5, 1e-4, -1e-4, 40.0, -40.0, 0.5, -0.5, 2.0, -2.0, 8.0, -8.0])])
    dy = r.standard_normal(4096)
    ref, gref = O.gelu_fwd(x.astype(np.float64)), O.gelu_grad(x.astype(np.float64))
    xf, df = to_dev(x, torch.float32), to_dev(dy, torch.float32)
    assert np.abs(host(ops.gelu_fwd(xf)) - ref).max() < 2e-6 * 40
    assert np.abs(host(ops.gelu_bwd(xf, df)) - dy * gref).max() < 5e-6
    xb, db = bf16_round(x), bf16_round(dy)
    refb, grefb = O.gelu_fwd(xb.astype(np.float64)), O.gelu_grad(xb.astype(np.float64))
    assert relmax(host(ops.gelu_fwd(to_dev(xb, torch.bfloat16))), refb) < 5e-3
    assert relmax(host(ops.gelu_bwd(to_dev(xb, torch.bfloat16), to_dev(db, torch.bfloat16))), db * grefb) < 5e-3
    # autograd wrapper == torch's GELU on the same bf16 input (values and gradient), 3-D shape
    from otter_amd import functional as OF
    u = to_dev(bf16_round(r.standard_normal((2, 24, 64)) * 2), torch.bfloat16).requires_grad_(True)
    u2 = u.detach().clone().requires_grad_(True)
    g = to_dev(bf16_round(r.standard_normal((2, 24, 64))), torch.bfloat16)
    OF.gelu(u).backward(g)
    torch.nn.functional.gelu(u2).backward(g)
    assert relmax(host(OF.gelu(u)), host(torch.nn.functional.gelu(u2))) < 8e-3
    assert relmax(host(u.grad), host(u2.grad)) < 8e-3


def test_swiglu_fwd_bwd(ops):
    r = rng(47)
    rows, I = 53, 176
    gu = bf16_round(r.standard_normal((rows, 2 * I)) * 2)
    dh = bf16_round(r.standard_normal((rows, I)))
    g, u = gu[:, :I].astype(np.float64), gu[:, I:].astype(np.float64)
    sg = 1.0 / (1.0 + np.exp(-g))
    h = ops.swiglu_fwd(to_dev(gu, torch.bfloat16))
    assert relmax(host(h), g * sg * u) < 8e-3
    dgu = ops.swiglu_bwd(to_dev(gu, torch.bfloat16), to_dev(dh, torch.bfloat16))
    assert relmax(host(dgu[:, :I]), dh * u * (sg * (1 + g * (1 - sg)))) < 8e-3
    assert relmax(host(dgu[:, I:]), dh * g * sg) < 8e-3


def test_quick_gelu_and_clip_attention_core(ops):
    """CLIP tower pieces on HIP: in-place quick-GELU, and the attention core on strided q/k/v views of one fused projection
    buffer with CLIP's shape (16 heads x 64, 257 tokens, no mask) against an fp64 softmax attention."""
    from otter_amd._capi import MASK_NONE

    r = rng(51)
    x = bf16_round(r.standard_normal((37, 4096)) * 3)
    y = ops.quick_gelu_(to_dev(x, torch.bfloat16))
    assert relmax(host(y), x / (1 + np.exp(-1.702 * x.astype(np.float64)))) < 8e-3
    N, S, H, d = 3, 257, 16, 64
    D = H * d
    qkv = bf16_round(r.standard_normal((N, S, 3 * D)))
    t = to_dev(qkv, torch.bfloat16)
    o, _ = ops.attn_fwd(t[..., :D], t[..., D:2 * D], t[..., 2 * D:], H, None, S, MASK_NONE, d ** -0.5, need_lse=False)
    q = qkv[..., :D].reshape(N, S, H, d).transpose(0, 2, 1, 3).astype(np.float64)
    k = qkv[..., D:2 * D].reshape(N, S, H, d).transpose(0, 2, 1, 3).astype(np.float64)
    v = qkv[..., 2 * D:].reshape(N, S, H, d).transpose(0, 2, 1, 3).astype(np.float64)
    sc = q @ k.transpose(0, 1, 3, 2) * d ** -0.5
    p = np.exp(sc - sc.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = (p @ v).transpose(0, 2, 1, 3).reshape(N, S, D)
    assert relmax(host(o), ref) < 1e-2


# ----------------------------------------------------------------------------------------------------------------------
# OtterHD / Fuyu kernels (config C5)
# ----------------------------------------------------------------------------------------------------------------------


def _np_layernorm(x, g, b, eps):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


@pytest.mark.parametrize("rot", [32, 64, 16])
def test_qk_norm_rope_fwd_bwd(ops, rot):
    """q/k LayerNorm over head_dim 64 + partial rotary + padding to 128 (fuyu/modeling_persimmon.py:262-304) against fp64 numpy,
    forward and backward (dqkv, dgamma, dbeta) -- the backward reference is a torch.autograd evaluation of the same formula."""
    r = rng(61 + rot)
    B, S, H, d = 2, 13, 3, 64
    qkv = bf16_round(r.standard_normal((B, S, H, 3, d)))
    gq, bq = (1 + 0.2 * r.standard_normal(d)).astype(np.float32), (0.1 * r.standard_normal(d)).astype(np.float32)
    gk, bk = (1 + 0.2 * r.standard_normal(d)).astype(np.float32), (0.1 * r.standard_normal(d)).astype(np.float32)
    cos, sin = O.rope_tables(S, rot, base=25000.0)
    eps = 1e-5
    T = torch.float64
    tq = torch.tensor(qkv, dtype=T, requires_grad=True)
    tg = [torch.tensor(a, dtype=T, requires_grad=True) for a in (gq, bq, gk, bk)]

    def ref(tq, gq_, bq_, gk_, bk_):
        outs = []
        for sel, (g_, b_) in enumerate(((gq_, bq_), (gk_, bk_))):
            x = tq[..., sel, :]
            y = torch.nn.functional.layer_norm(x, (d,), g_, b_, eps)
            c = torch.tensor(cos, dtype=T)[None, :, None, :]
            s_ = torch.tensor(sin, dtype=T)[None, :, None, :]
            yr = y[..., :rot]
            h = rot // 2
            rh = torch.cat((-yr[..., h:], yr[..., :h]), -1)
            outs.append(torch.cat((yr * c + rh * s_, y[..., rot:]), -1))
        return outs[0], outs[1], tq[..., 2, :]

    q_ref, k_ref, v_ref = ref(tq, *tg)
    dev = lambda a: to_dev(a)
    q, k, v, stats = ops.qk_norm_rope_fwd(to_dev(qkv.reshape(B, S, H * 3 * d), torch.bfloat16), dev(gq), dev(bq), dev(gk), dev(bk), dev(cos), dev(sin),
                                          H, rot, eps)
    assert q.shape == (B, S, H, 128)
    for got, want in ((q, q_ref), (k, k_ref), (v, v_ref)):
        assert relmax(host(got[..., :64]), want.detach().numpy()) < 1e-2
        assert float(got[..., 64:].abs().max()) == 0.0
    dq, dk, dv = (bf16_round(r.standard_normal((B, S, H, d))) for _ in range(3))
    (q_ref * torch.tensor(dq, dtype=T)).sum().backward(retain_graph=True)
    (k_ref * torch.tensor(dk, dtype=T)).sum().backward(retain_graph=True)
    (v_ref * torch.tensor(dv, dtype=T)).sum().backward()

    def pad(a):
        t = torch.zeros((B, S, H, 128), dtype=torch.bfloat16, device=DEV)
        t[..., :64] = to_dev(a, torch.bfloat16)
        t[..., 64:] = 3.0          # the upper columns of the incoming gradients must be ignored
        return t

    dqkv, dgq, dbq, dgk, dbk = ops.qk_norm_rope_bwd(pad(dq), pad(dk), pad(dv), to_dev(qkv.reshape(B, S, H * 3 * d), torch.bfloat16), stats, dev(gq), dev(gk),
                                                    dev(cos), dev(sin), H, rot)
    assert relmax(host(dqkv).reshape(B, S, H, 3, d), tq.grad.numpy()) < 1.5e-2
    for got, want in ((dgq, tg[0]), (dbq, tg[1]), (dgk, tg[2]), (dbk, tg[3])):
        assert relmax(host(got), want.grad.numpy()) < 1e-3
    # round 3's layout for the head-pair attention kernels: compact 64-wide q / k, v left in place (a strided view of qkv), and a backward
    # that fills only the q / k slots of a dqkv whose v slots the attention backward has written
    qkv_d = to_dev(qkv.reshape(B, S, H * 3 * d), torch.bfloat16)
    q2, k2, v2, stats2 = ops.qk_norm_rope_fwd(qkv_d, dev(gq), dev(bq), dev(gk), dev(bk), dev(cos), dev(sin), H, rot, eps, width=64, copy_v=False)
    assert q2.shape == (B, S, H, 64) and q2.is_contiguous() and v2.data_ptr() == qkv_d.data_ptr() + 2 * 128 and v2.stride() == (S * H * 192, H * 192, 192, 1)
    assert torch.equal(q2, q[..., :64]) and torch.equal(k2, k[..., :64]) and torch.equal(v2, v[..., :64]) and torch.equal(stats2, stats)
    dqkv2 = torch.full_like(qkv_d, float("nan"))
    dqkv2.view(B, S, H, 3, d)[:, :, :, 2] = to_dev(dv, torch.bfloat16)
    out2, dgq2, dbq2, dgk2, dbk2 = ops.qk_norm_rope_bwd(to_dev(dq, torch.bfloat16), to_dev(dk, torch.bfloat16), None, qkv_d, stats2, dev(gq), dev(gk), dev(cos),
                                                        dev(sin), H, rot, dqkv=dqkv2)
    assert out2.data_ptr() == dqkv2.data_ptr() and torch.equal(dqkv2, dqkv)
    for a_, b_ in ((dgq2, dgq), (dbq2, dbq), (dgk2, dgk), (dbk2, dbk)):     # same terms, another blocking of the fp32 partial sums
        assert relmax(host(a_), host(b_)) < 1e-5


def test_sqrelu_and_scatter_rows(ops):
    r = rng(67)
    x = bf16_round(r.standard_normal((19, 256)) * 2)
    dy = bf16_round(r.standard_normal((19, 256)))
    y = ops.sqrelu_fwd(to_dev(x, torch.bfloat16))
    assert relmax(host(y), np.maximum(x, 0) ** 2) < 8e-3
    dx = ops.sqrelu_bwd(to_dev(x, torch.bfloat16), to_dev(dy, torch.bfloat16))
    assert relmax(host(dx), 2 * np.maximum(x, 0) * dy) < 8e-3
    B, S, P, D = 2, 11, 5, 64
    word = r.standard_normal((B, S, D)).astype(np.float32)
    patch = bf16_round(r.standard_normal((B, P, D)))
    idx = np.full((B, S), -1, np.int64)
    idx[0, 2:7] = [0, 1, 2, 3, 4]
    idx[1, 0:3] = [4, 0, 2]
    ref = word.copy()
    for b in range(B):
        for s in range(S):
            if idx[b, s] >= 0:
                ref[b, s] = patch[b, idx[b, s]]
    for wdt, pdt in ((torch.float32, torch.bfloat16), (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)):
        out = ops.scatter_rows(to_dev(word, wdt), to_dev(patch, pdt), torch.from_numpy(idx).to(DEV))
        assert relmax(host(out), ref) < (1e-6 if wdt == torch.float32 else 8e-3)


def test_scatter_rows_out_of_range_index_is_never_dereferenced(ops):
    """an index >= P must not read another sample's rows (or past the buffer): the kernel writes NaN for it (the host
    wrapper of the module raises IndexError before launching -- tests/test_fuyu_host.py); every other row is untouched."""
    r = rng(68)
    B, S, P, D = 2, 9, 4, 64
    word = r.standard_normal((B, S, D)).astype(np.float32)
    patch = r.standard_normal((B, P, D)).astype(np.float32)
    idx = np.full((B, S), -1, np.int64)
    idx[0, 1:4] = [0, 3, 4]          # 4 == P: out of range (would alias patch[1, 0] without the check)
    idx[1, 8] = 1 << 40              # far out of range
    out = host(ops.scatter_rows(to_dev(word), to_dev(patch), torch.from_numpy(idx).to(DEV)))
    assert np.isnan(out[0, 3]).all() and np.isnan(out[1, 8]).all()
    assert np.array_equal(out[0, 1], patch[0, 0]) and np.array_equal(out[0, 2], patch[0, 3]) and np.array_equal(out[0, 0], word[0, 0])
    assert np.array_equal(out[1, :8], word[1, :8])


def test_gemm_cu_budget_and_variant_availability(ops):
    """otter_gemm_set_cu_budget: the persistent kernels run on fewer workgroups (CUs left to a concurrent RCCL kernel) with identical
    results; the library rejects the retired schedules loudly."""
    from otter_amd import _capi

    r = rng(91)
    M, N, Kd = 4096, 4096, 512            # 256 tiles of 256^2 (the T4 kernel) walked by 240 / 8 persistent workgroups
    A = to_dev(bf16_round(r.standard_normal((M, Kd)) * 0.3), torch.bfloat16)
    B = to_dev(bf16_round(r.standard_normal((N, Kd)) * 0.3), torch.bfloat16)
    base = ops.gemm_nt(A, B, out_dtype=torch.float32)
    try:
        for budget in (240, 8, 1):
            eff = ops.set_gemm_cu_budget(budget)
            assert eff == max(budget, 8)
            assert torch.equal(ops.gemm_nt(A, B, out_dtype=torch.float32), base), budget
            # small-grid ring kernel and the 128^2 kernel as well
            assert torch.equal(ops.gemm_nt(A[:512], B[:512], out_dtype=torch.float32), base[:512, :512])
    finally:
        total = ops.set_gemm_cu_budget(0)
    assert total == _capi.lib().otter_device_check()
    assert all(ops.gemm_variant_available(v) for v in LIVE_VARIANTS) and not ops.gemm_variant_available(24)
    assert not ops.gemm_variant_available(18)
    with pytest.raises(_capi.OtterHipError, match="retired"):
        ops.set_gemm_variant(18)


def test_decode_attention_at_the_lds_limit(ops):
    """Sk = 16384 needs 64 KiB of dynamic LDS (above the default allowance): the launcher opts in; one step beyond is
    refused with a message, not a launch failure."""
    from otter_amd import _capi

    r = rng(72)
    B, H, d = 1, 2, 128
    for Sk in (16384, 8193):
        q = bf16_round(r.standard_normal((B, H, d)))
        k = bf16_round(r.standard_normal((B, H, Sk, d)) * 0.5)
        v = bf16_round(r.standard_normal((B, H, Sk, d)))
        o = ops.decode_attn(to_dev(q, torch.bfloat16), to_dev(k, torch.bfloat16), to_dev(v, torch.bfloat16), None, None, d ** -0.5)
        sc = np.einsum("bhd,bhsd->bhs", q.astype(np.float64), k.astype(np.float64)) * d ** -0.5
        p = np.exp(sc - sc.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        ref = np.einsum("bhs,bhsd->bhd", p, v.astype(np.float64))
        assert relmax(host(o), ref) < 2e-2, Sk
    big = torch.zeros((1, 1, 16392, d), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_capi.OtterHipError, match="exceeds the LDS score buffer"):
        ops.decode_attn(torch.zeros((1, 1, d), dtype=torch.bfloat16, device=DEV), big, big, None, None, 1.0)


@pytest.mark.parametrize("layout", ["mpt", "llama"])
def test_decode_attention_over_kv_cache(ops, layout):
    """csrc/decode.hip: one query over a KV cache in the reference's MPT layout (k [B,H,d,S], v [B,H,S,d]) and in the LLaMA host's
    [B,H,S,d] layout, with ALiBi, a padding mask and a ragged Sk, against an fp64 softmax attention."""
    r = rng(71)
    B, H, Sk, d = 3, 5, 77, 128
    q = bf16_round(r.standard_normal((B, H, d)))
    k = bf16_round(r.standard_normal((B, H, Sk, d)))
    v = bf16_round(r.standard_normal((B, H, Sk, d)))
    slopes = (2.0 ** -np.arange(1, H + 1)).astype(np.float32) if layout == "mpt" else None
    valid = np.ones((B, Sk), np.uint8)
    valid[1, :9] = 0
    scale = d ** -0.5
    s = np.einsum("bhd,bhsd->bhs", q.astype(np.float64), k.astype(np.float64)) * scale
    if slopes is not None:
        s = s + slopes[None, :, None] * (np.arange(Sk) - (Sk - 1))[None, None, :]
    s = np.where(valid[:, None, :] != 0, s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = np.einsum("bhs,bhsd->bhd", p, v.astype(np.float64))
    tq, tv = to_dev(q, torch.bfloat16), to_dev(v, torch.bfloat16)
    if layout == "mpt":
        tk = to_dev(k.transpose(0, 1, 3, 2).copy(), torch.bfloat16).transpose(2, 3)      # storage [B,H,d,S], indexed [b,h,s,d]
        assert tk.stride(2) == 1
    else:
        tk = to_dev(k, torch.bfloat16)
    o = ops.decode_attn(tq, tk, tv, to_dev(slopes) if slopes is not None else None, torch.from_numpy(valid).to(DEV), scale)
    assert relmax(host(o), ref) < 1e-2
    o2 = ops.decode_attn(tq, tk, tv, to_dev(slopes) if slopes is not None else None, None, scale)     # no mask
    s2 = np.einsum("bhd,bhsd->bhs", q.astype(np.float64), k.astype(np.float64)) * scale
    if slopes is not None:
        s2 = s2 + slopes[None, :, None] * (np.arange(Sk) - (Sk - 1))[None, None, :]
    p2 = np.exp(s2 - s2.max(-1, keepdims=True))
    p2 /= p2.sum(-1, keepdims=True)
    assert relmax(host(o2), np.einsum("bhs,bhsd->bhd", p2, v.astype(np.float64))) < 1e-2
