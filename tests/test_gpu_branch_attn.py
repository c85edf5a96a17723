"""Candidate rows over a cached prompt on HIP: csrc/branch_attn.hip (`ops.branch_attn_merge`), `StaticKVCache.attend_branches` (flash forward
over the cache in place + the merge kernel) and `score_candidates` on 2-layer full-width MPT and LLaMA hosts.

Shapes: H = 4, B in {1, 2}, C in {1, 3}, T in {1, 2, 63, 64}, P in {1, 127, 128, 129}.  Rows are n = (b C + c) T + t.

No case takes the plain-torch path: `attend_branches_reference` raises for the whole of this file, and the launches are counted."""
import copy
import gc
import itertools
import math

import pytest
import torch

from tests._decode_cases import TOL_ORACLE          # 2^-8 + 2^-12: one bf16 rounding of the output + fp32 scores, __expf and the merges

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x5A5A          # bf16 bit pattern of the frame around o
FLOOR = 2.0 ** -8      # one bf16 rounding of the output
H = 4
BS, CS, TS, PS = (1, 2), (1, 3), (1, 2, 63, 64), (1, 127, 128, 129)
LN2 = math.log(2.0)


@pytest.fixture(autouse=True)
def _kernel_path_only(monkeypatch):
    from otter_amd.kv_cache import StaticKVCache

    def refuse(*a, **k):
        raise AssertionError("a GPU case took attend_branches_reference")

    monkeypatch.setattr(StaticKVCache, "attend_branches_reference", refuse)


def _rows(B, C, T, device=DEV):
    n = torch.arange(B * C * T, device=device)
    return n // (C * T), (n // T) % C, n % T            # b, c, t of every row


def _qkv(N, g, fused=True):
    """q, k_new, v_new [N, H, 128] bf16: the three slices of one projection buffer (read in place), or three tensors."""
    if fused:
        buf = torch.randn(N, 3, H, 128, generator=g, device=DEV).bfloat16()
        return buf[:, 0], buf[:, 1], buf[:, 2]
    return tuple(torch.randn(N, H, 128, generator=g, device=DEV).bfloat16() for _ in range(3))


def _merge_oracle(q, kn, vn, o1, lse1, scale, slopes, B, C, T):
    """fp64 on the kernel's own inputs: the formula of include/otter_hip.h, dense over (t, u)."""
    N = B * C * T
    q5, k5, v5 = (x.double().view(B, C, T, H, 128) for x in (q, kn, vn))
    tpos = torch.arange(T, device=DEV)
    rel = (tpos.view(1, T) - tpos.view(T, 1)).double()                                   # [t, u] = u - t
    a = slopes.double() if slopes is not None else torch.zeros(H, dtype=torch.float64, device=DEV)
    e = torch.einsum("bcthd,bcuhd->bchtu", q5, k5) * scale + a.view(1, 1, H, 1, 1) * rel
    e = e.masked_fill((rel > 0).view(1, 1, 1, T, T), float("-inf"))
    L1 = lse1.double().view(B, H, C, T).permute(0, 2, 1, 3) - a.view(1, 1, H, 1) * (tpos + 1).double().view(1, 1, 1, T)
    M = torch.maximum(L1, e.amax(-1))
    w1, pu = torch.exp(L1 - M), torch.exp(e - M.unsqueeze(-1))
    o1_ = torch.nan_to_num(o1.double().view(B, C, T, H, 128).permute(0, 1, 3, 2, 4), nan=0.0)
    o1_ = torch.where((w1 > 0).unsqueeze(-1), o1_, torch.zeros_like(o1_))
    v5 = torch.nan_to_num(v5, nan=0.0)
    o = (w1.unsqueeze(-1) * o1_ + torch.einsum("bchtu,bcuhd->bchtd", pu, v5)) / (w1 + pu.sum(-1)).unsqueeze(-1)
    return o.permute(0, 1, 3, 2, 4).reshape(N, H, 128)


def _framed(N):
    buf = torch.full((N * H * 128 + 512,), SENT, dtype=torch.int16, device=DEV)
    return buf, buf[256:256 + N * H * 128].view(torch.bfloat16).view(N, H, 128)


def _frames_intact(buf):
    return bool((buf[:256] == SENT).all()) and bool((buf[-256:] == SENT).all())


# ---- count inputs: exact ------------------------------------------------------------------------------------------------------------------
# q = 0, so every score is its ALiBi term alone and every weight a power of two (or 1 / P' for the prompt).  v_new of row (b, c, u) is
# 2^(c + 3 b) in dim u and 0 elsewhere: output dim u of row (b, c, t) shows whether own key u was counted, with which weight, and whether
# it came from this candidate of this sentence.  The expected value is computed in fp64, asserted to be a bf16 number, and the kernel must
# return exactly it: its fp32 result is within ~1e-5 relative (two roundings of lse1, __expf) of a value that has at most 8 significant bits,
# a rounding boundary of bf16 is 2^-9 relative away, so the one rounding of the output lands on it.

def _count_case(B, C, T, slope_mult):
    """slope_mult None: no slopes, lse1 = log(128 - t - 1), o1 = 1: the denominator P' + t + 1 = 128.
    Otherwise slopes a_h = ln 2 * slope_mult[h]: own key u weighs 2^(-s (t - u)); lse1 is set so that the prompt weighs Pw = 2 - (the own keys'
    sum), the denominator is 2; o1 = 1 in dims 64.. and 0 in dims ..63.
    Built on the CPU, where 2.0 ** integer is exact in fp64 (a device pow may be an ulp off), then moved."""
    N = B * C * T
    b, c, t = _rows(B, C, T, "cpu")
    q = torch.zeros(N, H, 128, dtype=torch.bfloat16, device="cpu")
    kn = torch.randn(N, H, 128, device="cpu").bfloat16()                                   # (q = 0: the keys' values do not matter)
    vn = torch.zeros(N, H, 128, dtype=torch.float64, device="cpu")
    vn[torch.arange(N, device="cpu"), :, t] = (2.0 ** (c + 3 * b)).double().view(N, 1)
    own = (torch.arange(128, device="cpu").view(1, 128) <= t.view(N, 1)).double()          # [N, dim]: own key `dim` is visible
    val = (2.0 ** (c + 3 * b)).double().view(N, 1, 1)
    if slope_mult is None:
        slopes = None
        lse1_rows = torch.log((128 - t - 1).double()).view(N, 1).expand(N, H)
        o1 = torch.ones(N, H, 128, dtype=torch.float64, device="cpu")
        expected = (((128 - t - 1).double().view(N, 1, 1) + val * own.view(N, 1, 128)) / 128.0).expand(N, H, 128).contiguous()
    else:
        s = torch.tensor(slope_mult, dtype=torch.float64, device="cpu")                    # [H]
        slopes = (s * LN2).float().contiguous()
        u = torch.arange(128, device="cpu").double()
        w = own.view(N, 1, 128) * 2.0 ** (-s.view(1, H, 1) * (t.double().view(N, 1, 1) - u.view(1, 1, 128)).clamp(min=0))   # [N, H, dim u]
        # [N, H]; s = 1: 2 - (2 - 2^-t) in closed form (fp64 cannot hold 2 - 2^-63), s = 2 comes with T <= 2 only
        Pw = torch.where(s.view(1, H) == 1, 2.0 ** -t.double().view(N, 1), 2.0 - w.sum(-1))
        assert bool((Pw > 0).all())
        lse1_rows = torch.log(Pw) + slopes.double().view(1, H) * (t + 1).double().view(N, 1)
        o1 = torch.zeros(N, H, 128, dtype=torch.float64, device="cpu")
        o1[:, :, 64:] = 1.0
        expected = (Pw.unsqueeze(-1) * o1 + w * val) / 2.0
    assert torch.equal(expected.bfloat16().double(), expected), "the expected values are not bf16 numbers"
    lse1 = lse1_rows.float().view(B, C * T, H).permute(0, 2, 1).contiguous()             # [B, H, C T]
    dev = lambda x: None if x is None else x.to(DEV)
    return dev(q), dev(kn), dev(vn.bfloat16()), dev(o1.float()), dev(lse1), dev(slopes), dev(expected)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
def test_count_inputs_are_exact(B, C):
    from otter_amd import ops

    n = 0
    for T in TS:
        for slope_mult in (None, (1.0, 1.0, 1.0, 1.0)) + (((1.0, 2.0, 1.0, 2.0),) if T <= 2 else ()):
            q, kn, vn, o1, lse1, slopes, expected = _count_case(B, C, T, slope_mult)
            o = ops.branch_attn_merge(q, kn, vn, o1, lse1, 128 ** -0.5, T, C * T, slopes=slopes)
            bad = (o.double() != expected).nonzero()
            assert bad.numel() == 0, ("first wrong (row, head, dim)", (B, C, T, slope_mult), bad[0].tolist(),
                                      float(o[tuple(bad[0])]), float(expected[tuple(bad[0])]))
            n += 1
    assert n == 2 * len(TS) + 2


# ---- the merge kernel against fp64 ----------------------------------------------------------------------------------------------------------

def _merge_inputs(B, C, T, g, fused):
    N = B * C * T
    q, kn, vn = _qkv(N, g, fused)
    o1 = torch.randn(N, H, 128, generator=g, device=DEV)                                 # fp32, as the flash forward hands it over
    lse1 = (torch.randn(B, H, C * T, generator=g, device=DEV) * 3 + 4).float()
    dead = torch.rand(B, H, C * T, generator=g, device=DEV) < 0.15                       # no visible prompt key: lse1 = -inf, o1 unused
    lse1 = lse1.masked_fill(dead, float("-inf"))
    o1 = torch.where(dead.permute(0, 2, 1).reshape(N, H, 1), torch.full_like(o1, float("nan")), o1).contiguous()   # NaN where it must not be read
    return q, kn, vn, o1, lse1


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
def test_merge_kernel_against_the_fp64_oracle(B, C):
    """Random operands, with and without slopes, fused and separate inputs; lse1 = -inf on ~15 % of the (row, head) with NaN in their o1.
    |o - ref| <= TOL_ORACLE x the row's largest |ref|.  The frame around o stays, and a second call gives the same bits."""
    from otter_amd import ops

    g = torch.Generator(device=DEV).manual_seed(100 * B + C)
    scale = 128 ** -0.5
    slopes_t = (2.0 ** -(8.0 * torch.arange(1, H + 1, device=DEV, dtype=torch.float32) / H)).contiguous()
    worst, n = 0.0, 0
    for T, alibi, fused in itertools.product(TS, (False, True), (False, True)):
        q, kn, vn, o1, lse1 = _merge_inputs(B, C, T, g, fused)
        slopes = slopes_t if alibi else None
        ref = _merge_oracle(q, kn, vn, o1, lse1, scale, slopes, B, C, T)
        buf, out = _framed(B * C * T)
        o = ops.branch_attn_merge(q, kn, vn, o1, lse1, scale, T, C * T, slopes=slopes, out=out)
        assert o.data_ptr() == out.data_ptr() and _frames_intact(buf), ("frame around o", (B, C, T, alibi, fused))
        assert not bool(torch.isnan(o).any()), ("NaN: an o1 that must not be read was read", (B, C, T, alibi, fused))
        o2 = ops.branch_attn_merge(q, kn, vn, o1, lse1, scale, T, C * T, slopes=slopes)
        assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), ("not deterministic", (B, C, T, alibi, fused))
        err, bound = (o.double() - ref).abs().amax(-1), TOL_ORACLE * ref.abs().amax(-1)
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), ((B, C, T, alibi, fused), float((err / bound).max()))
        n += 1
    print("[branch-attn] merge kernel B=%d C=%d: %d cases, worst err / bound %.3f" % (B, C, n, worst), flush=True)
    assert n == 4 * len(TS)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
def test_a_row_reads_only_its_own_slots(B, C):
    """For a chosen row: NaN in every k_new / v_new row of the other candidates and of later positions of its own (and NaN in o1 where
    lse1 = -inf, from `_merge_inputs`): the row's output is what it was."""
    from otter_amd import ops

    g = torch.Generator(device=DEV).manual_seed(7 * B + C)
    for T in TS:
        N = B * C * T
        q, kn, vn, o1, lse1 = _merge_inputs(B, C, T, g, fused=False)
        slopes = torch.full((H,), 0.125, device=DEV)
        base = ops.branch_attn_merge(q, kn, vn, o1, lse1, 0.1, T, C * T, slopes=slopes)
        for n in sorted({0, T // 2, N // 2, N - T, N - 1}):
            t = n % T
            mine = torch.zeros(N, dtype=torch.bool, device=DEV)
            mine[n - t:n + 1] = True
            kp, vp = kn.clone(), vn.clone()
            kp[~mine] = float("nan")
            vp[~mine] = float("nan")
            got = ops.branch_attn_merge(q, kp, vp, o1, lse1, 0.1, T, C * T, slopes=slopes)
            assert torch.equal(got[n].view(torch.int16), base[n].view(torch.int16)), (B, C, T, n)


def test_binding_refuses_bad_arguments_on_the_device():
    from otter_amd import ops
    from otter_amd._capi import OtterHipError

    q, kn, vn = _qkv(12, torch.Generator(device=DEV).manual_seed(0))
    o1, lse1 = torch.zeros(12, H, 128, device=DEV), torch.zeros(2, H, 6, device=DEV)
    assert tuple(ops.branch_attn_merge(q, kn, vn, o1, lse1, 0.1, 3, 6).shape) == (12, H, 128)
    for kw, text in ((dict(T=5), "not whole candidates"), (dict(T=65), "outside"), (dict(rows_per_sentence=9), "rows_per_sentence")):
        a = dict(T=3, rows_per_sentence=6)
        a.update(kw)
        with pytest.raises(OtterHipError, match=text):
            ops.branch_attn_merge(q, kn, vn, o1, lse1, 0.1, a["T"], a["rows_per_sentence"])


# ---- attend_branches end to end: flash over the cache in place + the merge -------------------------------------------------------------------

def _full_oracle(q, kn, vn, kp, vp, valid, scale, slopes, B, C, T):
    """fp64: ONE softmax per (row, head) over [the visible prompt keys of the row's sentence + own keys u <= t], ALiBi origin at the row's own
    key.  kp / vp [B, H, P, 128]; valid bool [B, P] or None."""
    N, P = B * C * T, kp.shape[2]
    q4 = q.double().view(B, C * T, H, 128)
    k5, v5 = kn.double().view(B, C, T, H, 128), vn.double().view(B, C, T, H, 128)
    tpos = torch.arange(T, device=DEV)
    a = slopes.double() if slopes is not None else torch.zeros(H, dtype=torch.float64, device=DEV)
    s1 = torch.einsum("bnhd,bhjd->bhnj", q4, kp.double()) * scale                        # [B, H, CT, P]
    t_of = tpos.repeat(C).double().view(1, 1, C * T, 1)
    s1 = s1 + a.view(1, H, 1, 1) * (torch.arange(P, device=DEV).double().view(1, 1, 1, P) - (P + t_of))
    if valid is not None:
        s1 = s1.masked_fill(~valid.view(B, 1, 1, P), float("-inf"))
    rel = (tpos.view(1, T) - tpos.view(T, 1)).double()
    e = torch.einsum("bcthd,bcuhd->bchtu", q4.view(B, C, T, H, 128), k5) * scale + a.view(1, 1, H, 1, 1) * rel
    e = e.masked_fill((rel > 0).view(1, 1, 1, T, T), float("-inf"))
    s = torch.cat([s1.view(B, H, C, T, P).permute(0, 2, 1, 3, 4), e], dim=-1)            # [B, C, H, T, P + T]
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("bchtj,bhjd->bchtd", p[..., :P], vp.double()) + torch.einsum("bchtu,bcuhd->bchtd", p[..., P:], v5)
    return o.permute(0, 1, 3, 2, 4).reshape(N, H, 128)


def _steps_of_the_existing_kernel(q, kn, vn, kp, vp, valid, scale, slopes, B, C, T):
    """The same rows on `ops.decode_attn_cached`, row by row in t: a scratch cache of B*C rows holds the prompt of the row's sentence; step t
    appends own key t at slot P + t and attends, as a user's loop of cached steps does."""
    from otter_amd import ops

    P = kp.shape[2]
    kc = torch.zeros(B * C, H, P + T + 1, 128, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    kc[:, :, :P], vc[:, :, :P] = kp.repeat_interleave(C, dim=0), vp.repeat_interleave(C, dim=0)
    kv = torch.ones(B * C, P + T, dtype=torch.uint8, device=DEV)
    if valid is not None:
        kv[:, :P] = valid.repeat_interleave(C, dim=0).to(torch.uint8)
    q5, k5, v5 = (x.view(B * C, T, H, 128) for x in (q, kn, vn))
    out = torch.empty(B * C, T, H, 128, dtype=torch.bfloat16, device=DEV)
    for t in range(T):
        out[:, t] = ops.decode_attn_cached(q5[:, t].contiguous(), k5[:, t].contiguous(), v5[:, t].contiguous(), kc, vc, P + t, scale,
                                           key_valid=kv[:, :P + t + 1].contiguous(), slopes=slopes).view(B * C, H, 128)
    return out.view(B * C * T, H, 128)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("B", BS)
def test_attend_branches_against_the_fp64_softmax_and_the_existing_kernel(B, C, monkeypatch):
    """Every T x P x {ALiBi} x {all valid, left-padded with the last sentence's prompt fully masked (lse1 = -inf)}.  err_new <= max(1.25
    err_old, 2^-8 max|ref|) with err_old the error of `ops.decode_attn_cached` on the same operands, as in tests/test_gpu_decode_cached.py.
    The cache is read in place and comes back bit-identical; each call is exactly one flash forward and one merge launch.

    Measured on an MI355X: err_new = err_old in the worst case of every parameter set (worst err_new / bound 0.800 = 1 / 1.25, 0 of 256 cases
    over the bound).  That rests on two properties of the prompt stage, each found by this test: o1 crosses to the merge kernel in fp32 (in
    bf16 the answer is rounded twice: 33 of the 256 cases missed, by up to 1.62 x), and the fp32-output flash instance feeds its probabilities
    to the second product as a bf16 hi + lo pair (with bf16 probabilities alone its fp32 o1 was 0.8e-03 to 3.4e-03 from fp64 at max|ref| 0.5 to
    1.3, and 4 cases still missed, by up to 1.39 x; now 3e-06).  The merge kernel on an exact prompt part has exactly the existing kernel's
    error."""
    from otter_amd import ops
    from otter_amd.kv_cache import StaticKVCache

    calls = {"flash": 0, "merge": 0}
    for name, key in (("flash_attn_fwd_f32", "flash"), ("branch_attn_merge", "merge")):
        def spy(*a, _f=getattr(ops, name), _k=key, **k):
            calls[_k] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    g = torch.Generator(device=DEV).manual_seed(31 * B + C)
    scale = 128 ** -0.5
    slopes_t = (2.0 ** -(8.0 * torch.arange(1, H + 1, device=DEV, dtype=torch.float32) / H)).contiguous()
    worst, n, misses = 0.0, 0, []
    for T, P in itertools.product(TS, PS):
        cache = StaticKVCache(2, B, H, 128, P + 2, DEV)
        kp, vp = (torch.randn(B, H, P, 128, generator=g, device=DEV).bfloat16() for _ in range(2))
        cache.k.view(torch.int16).fill_(SENT)
        cache.v.view(torch.int16).fill_(SENT)
        cache.fill(1, kp, vp)
        cache.length = P
        k0, v0 = cache.k.clone(), cache.v.clone()
        padded = torch.ones(B, P, dtype=torch.bool, device=DEV)
        for b in range(B):
            padded[b, :min(3 * b + 1, P - 1)] = False                                   # left padding
        padded[B - 1] = False                                                            # a fully masked prompt: lse1 = -inf for its rows
        for alibi, masked in itertools.product((False, True), (False, True)):
            q, kn, vn = _qkv(B * C * T, g)
            slopes, valid = (slopes_t if alibi else None), (padded if masked else None)
            tag = (B, C, T, P, alibi, masked)
            before = dict(calls)
            o = cache.attend_branches(1, q, kn, vn, scale, C, T, key_valid=valid, slopes=slopes).view(-1, H, 128)
            assert (calls["flash"] - before["flash"], calls["merge"] - before["merge"]) == (1, 1), tag
            assert torch.equal(cache.k.view(torch.int16), k0.view(torch.int16)) and torch.equal(cache.v.view(torch.int16), v0.view(torch.int16)), tag
            assert cache.length == P and cache.src is None
            ref = _full_oracle(q, kn, vn, kp, vp, valid, scale, slopes, B, C, T)
            old = _steps_of_the_existing_kernel(q, kn, vn, kp, vp, valid, scale, slopes, B, C, T)
            mag = float(ref.abs().max())
            err_new, err_old = float((o.double() - ref).abs().max()), float((old.double() - ref).abs().max())
            bound = max(1.25 * err_old, FLOOR * mag)
            worst = max(worst, err_new / bound)
            if err_new > bound:
                misses.append((tag, err_new, err_old, mag))
                print("[branch-attn] attend_branches MISS %s: err_new %.3e, err_old %.3e, 2^-8 max|ref| %.3e (err_new / bound %.3f)"
                      % (tag, err_new, err_old, FLOOR * mag, err_new / bound), flush=True)
            n += 1
    print("[branch-attn] attend_branches B=%d C=%d: %d cases, %d over the bound, worst err_new / bound %.3f" % (B, C, n, len(misses), worst),
          flush=True)
    assert n == len(TS) * len(PS) * 4
    assert not misses, misses


# ---- the hosts --------------------------------------------------------------------------------------------------------------------------------

P_LEN = 24


def _host_case(model, bench, B, pads, C, T, seed):
    vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN, DEV, seed=99, frames=1)
    if pads is not None:
        for r, n in enumerate(pads):
            mask[r, :n] = 0
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(5, 1000, (B, C, T), generator=g)
    lens = torch.randint(1, T + 1, (B, C), generator=g)
    lens[:, 0] = T
    cmask = torch.arange(T).expand(B, C, T) < lens.unsqueeze(-1)
    assert model.media_token_id >= 1000
    return vx, ids, (mask if pads is not None else None), cand.to(DEV), cmask.to(DEV)


def _reforward(model, vx, ids, mask, cand, cmask, bf16):
    """The oracle: one uncached forward per (b, c) over prompt + candidate, log-softmax in fp32, the candidate's tokens gathered."""
    B, C, T = cand.shape
    ref = torch.zeros(B, C, T, device=DEV)
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if bf16 else torch.autocast("cuda", enabled=False)
    with torch.no_grad(), ctx:
        for b in range(B):
            for c in range(C):
                L = int(cmask[b, c].sum())
                full = torch.cat([ids[b], cand[b, c, :L]])[None]
                fm = torch.cat([mask[b], torch.ones(L, dtype=mask.dtype, device=DEV)])[None] if mask is not None else None
                v = vx[b:b + 1].to(torch.bfloat16) if bf16 else vx[b:b + 1]
                logits = model(vision_x=v, lang_x=full, attention_mask=fm, use_cache=False).logits[0].float()
                ref[b, c, :L] = torch.log_softmax(logits, -1)[P_LEN - 1:P_LEN + L - 1].gather(1, cand[b, c, :L, None])[:, 0]
    return ref


def _score(model, vx, ids, mask, cand, cmask, **kw):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        return model.score_candidates(vx.to(torch.bfloat16), ids, mask, candidates=cand, candidate_mask=cmask, return_token_logprobs=True, **kw)[1]


def _to_twin(model, qmodel):
    """`model` (fp32) takes the q * scale of every Int8FrozenLinear of `qmodel` (tests/test_gpu_w8_gated.py: MPT's tied table keeps the lookup)."""
    from otter_amd.quant import Int8FrozenLinear, Int8Unembedding, dequantize_weight_int8

    mods = dict(model.named_modules())
    with torch.no_grad():
        for name, m in qmodel.named_modules():
            if not isinstance(m, Int8FrozenLinear):
                continue
            w = dequantize_weight_int8(m.qweight, m.scale, torch.float32)
            if isinstance(m, Int8Unembedding) and name.endswith("wte.unembed_int8"):
                wte = mods[name[:-len(".unembed_int8")]]
                wte.forward = lambda input, unembed=False, _w=w, _f=wte.forward: (
                    torch.nn.functional.linear(input, _w.to(input.dtype)) if unembed else _f(input))
            else:
                mods[name].weight.copy_(w)


@pytest.mark.parametrize("kind", ["mpt", "llama"])
def test_hosts_stay_within_twice_the_bf16_reforward_drift(kind, monkeypatch):
    """2-layer full-width hosts, a left-padded batch of 2, 3 ragged candidates of up to 4 tokens, bf16 and then the int8 decoder (gated blocks
    and un-embedding included, against its fp32 fake-quantised twin): the token log-probabilities of `score_candidates` are within 2 x the
    distance of the bf16 re-forward from the fp32 re-forward.  One candidate per pass gives the scores of one pass (the prompt cache is
    reusable: a second call too); the branch pass runs clean under torch's sync debug mode "error"; every layer's branch attention is one
    flash forward + one merge launch."""
    from otter_amd import ops
    from tests.test_gpu_media_cache import _build

    model, bench = _build(kind)
    merges = [0]
    inner = ops.branch_attn_merge

    def spy(*a, **k):
        merges[0] += 1
        return inner(*a, **k)

    monkeypatch.setattr(ops, "branch_attn_merge", spy)
    B, C, T = 2, 3, 4
    vx, ids, mask, cand, cmask = _host_case(model, bench, B, (0, 3), C, T, seed=4)

    def check(m, ref32_model, tag):
        ref = _reforward(ref32_model, vx, ids, mask, cand, cmask, bf16=False)
        d_ref = float(((_reforward(m, vx, ids, mask, cand, cmask, bf16=True) - ref) * cmask).abs().max())
        merges[0] = 0
        tok = _score(m, vx, ids, mask, cand, cmask)
        assert merges[0] == 2, merges                                   # one pass, two layers
        d_new = float(((tok - ref) * cmask).abs().max())
        print("[branch-attn] %s %s: token log-prob distance from the fp32 re-forward: bf16 re-forward %.3e, score_candidates %.3e (ratio %.2f)"
              % (kind, tag, d_ref, d_new, d_new / d_ref), flush=True)
        assert d_ref > 0 and d_new <= 2 * d_ref, (kind, tag, d_new, d_ref)
        assert torch.equal(tok == 0, ~cmask) and not m.lang_encoder.is_conditioned()
        return tok, ref, d_ref

    tok, ref, d_ref = check(model, model, "bf16")
    # one candidate per pass: the same yardstick (the passes have other row counts, so their GEMMs may round differently); the prompt cache
    # is only read, so a second call gives the same bits
    merges[0] = 0
    one_each = _score(model, vx, ids, mask, cand, cmask, max_rows=B * (T - 1))
    assert merges[0] == 2 * C
    assert float(((one_each - ref) * cmask).abs().max()) <= 2 * d_ref
    assert torch.equal(_score(model, vx, ids, mask, cand, cmask), tok)
    # the branch pass synchronises nothing
    lm = model.lang_encoder
    fb = lm.forward_branches

    def strict(*a, **k):
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fb(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode(prev)

    lm.forward_branches = strict
    try:
        assert torch.equal(_score(model, vx, ids, mask, cand, cmask), tok)
    finally:
        del lm.forward_branches
    # the int8 decoder
    qmodel = copy.deepcopy(model)
    qmodel.quantize_decoder_int8(gated_blocks=True, lm_head=True)
    _to_twin(model, qmodel)
    check(qmodel, model, "int8")
    del model, qmodel
    gc.collect()
    torch.cuda.empty_cache()
