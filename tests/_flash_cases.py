"""Inputs with exactly known answers for the flash attention kernels (csrc/flash.hip: forward, dQ, dK/dV; head_dim 128 and 64), an fp64
reference and the checkers that go with them.  Pure torch, device-agnostic: tests/test_gpu_flash_exact.py feeds the checkers with
ops.flash_attn_fwd / ops.flash_attn_bwd, tests/test_flash_cases_cpu.py with a plain fp64 step and with deliberately wrong ones.

A *case* is a SimpleNamespace: q [B, Sq, H, hd], k / v [B, Sk, H, hd] and dout [B, Sq, H, hd] as bf16, `slopes` [H] fp32 or None, `key_valid`
[B, Sk] uint8 or None, `causal`, `scale`, the layout that the GPU harness allocates (`fused`, `compact`, `interleaved`), and what the builder
knows about the answer.  A *step* maps a case to Result(o [B, Sq, H, hd], lse [B, H, Sq], dq, dk, dv), in the layout of the inputs.

The reference is softmax(scale q k^T + slope (j - (Sk - 1)) + masks) v in fp64; key j is visible to query i iff it is valid and, under the
causal mask, j <= i + Sk - Sq.  A row without a visible key has o = 0, lse = -inf and zero gradients (include/otter_hip.h).  The backward
reference takes the step's OWN o and lse, as the backward kernels do: P = exp(s - lse), delta = dout . o, dS = P (dP - delta).  The forward
is judged separately, so both bounds are per element:

    |got - ref| <= (r 2^-8 + FP32_SLACK) A        (+ UNDERFLOW where A > 0)

with A the sum of the absolute values of the element's terms (for dQ / dK with dP and delta expanded into their own terms) and r the number
of bf16 roundings on the output's path.  A = 0 therefore demands an exact zero.

Kinds of input:
  count     q = 0 (every score exactly 0, no ALiBi), V holds only 0 and 1: o[i, d] = (visible keys owning d) / n_i, lse_i = ln n_i.  lse
            carries the number of keys, o their placement.  No (row, dim) count exceeds 32, so one key moves an element by >= 1 / 32 of it.
  onekey    q = 0, V nonzero at ONE key j* per (b, h): every row that must not see j* is exactly 0 (with ALiBi: V[j*] P_ij* otherwise).
  onequery  random q / k / v, dout nonzero at ONE row i* per head of ONE batch row: every key gradient has one term, dQ is exactly 0 off row
            i*, dK / dV are exactly 0 at masked keys, above i* + off and in every other batch row.
  ramp      q = 8 (e0 + e1), k_j = c_j e0 + f_j e1: the row maximum moves from one 64-key tile to the next by a stated amount, on either
            side of the forward's lazy-rescale threshold (8 in log2 units = 5.545).
  oracle    randn * 0.8.
"""
import math
from types import SimpleNamespace

import torch

SCALE = 0.125
TILE, WAVE, BLOCK = 64, 32, 128
KMASK_TILES = 128              # csrc/flash.hip: above 128 key tiles the v2 forward / dQ kernel read the mask bytes per tile
PERS_MAX_BLOCKS = 32           # dkv_persistent: one mask bit per 128-key block in a 32-bit word
RESCALE_LOG2 = 8.0             # the forward rescales its accumulator when a row's maximum grew by more than this (log2 units)
COUNT_LIMIT = 32

BF16 = 2.0 ** -8
# bf16 roundings on each output's path, from csrc/flash.hip:
R_O = 2     # forward: pack8(s) rounds P (the row sum adds the unrounded p), store_rows_lds / store_dt round o * inv
R_DV = 2    # dK/dV kernel: pack8(s) rounds P, the store rounds dV
R_DQ = 2    # dQ kernel: pack8(dp) rounds dS, the store rounds scale * dQ
R_DK = 2    # dK/dV kernel: pack8(dp) rounds dS, the store rounds scale * dK
# fp32: a score in log2 units stays below 2^9 in every case here (the steepest ramp ends at 210 / ln 2 = 303), where fp32 numbers are 2^-15
# apart; scale, bias and the subtraction of the maximum (or lse) round it three times, and an error e in the exponent is a relative error
# e ln 2 in P: 3 * 2^-15 * 0.69 < 2^-13.  The row sum, 1 / l, logf and the products add a few 2^-24.  2^-12 covers both with a factor 2.
FP32_SLACK = 2.0 ** -12
# bf16 and fp32 end at 2^-126: a P or dS below that may be flushed to 0.  At most 2^13 terms, each times a factor below 2^13.  Only where A > 0.
UNDERFLOW = 2.0 ** -100

ALL_S = [1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 255, 256, 257, 321]
PADS = [0, 1, 31, 32, 33, 64, 127, 128, 129, 200]
PAD_S = 260
SQSK = [(1, 129), (33, 200), (128, 321), (200, 130), (65, 1)]
RAMPS = {"up5.0": 5.0, "up5.6": 5.6, "up30": 30.0, "jump60": 60.0, "down60": -60.0}
LAYOUTS = ["fused", "compact", "interleaved"]

WORST = {}                     # (kind, output) -> largest error / bound seen by the checkers


class Result(SimpleNamespace):
    pass


class CheckFailure(AssertionError):
    def __init__(self, reason, detail):
        super().__init__("%s: %s" % (reason, detail))
        self.reason = reason


def alibi(H):
    """mpt.alibi_slopes(H, 8) for a power-of-two head count."""
    return torch.tensor([2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32)


def bh(t):
    """[B, S, H, hd] -> fp64 [B, H, S, hd]."""
    return t.double().permute(0, 2, 1, 3)


def sbh(t):
    return t.permute(0, 2, 1, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------- reference

def visible(case, rows):
    """bool [B, 1, R, Sk]: key j visible to query rows[r]."""
    vis = torch.ones(case.B, 1, len(rows), case.Sk, dtype=torch.bool)
    if case.key_valid is not None:
        vis = vis & case.key_valid.bool()[:, None, None, :]
    if case.causal:
        vis = vis & (torch.arange(case.Sk)[None, :] <= (rows + (case.Sk - case.Sq))[:, None])[None, None]
    return vis


def _rows(case, rows):
    return torch.arange(case.Sq) if rows is None else torch.as_tensor(rows, dtype=torch.long)


def scores(case, rows, vis_fn=None):
    s = case.scale * (bh(case.q)[:, :, rows] @ bh(case.k).transpose(-1, -2))
    if case.slopes is not None:
        s = s + case.slopes.double()[None, :, None, None] * (torch.arange(case.Sk, dtype=torch.float64) - (case.Sk - 1))[None, None, None, :]
    vis = (vis_fn or visible)(case, rows)
    return s.masked_fill(~vis, -math.inf), vis


def ref_forward(case, rows=None, vis_fn=None, round_p=False):
    """o, A [B, H, R, hd], lse, n [B, H, R] of the query rows `rows` (all by default)."""
    rows = _rows(case, rows)
    s, vis = scores(case, rows, vis_fn)
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    lse = torch.where(l > 0, torch.log(l) + m, torch.full_like(l, -math.inf)).squeeze(-1)
    l1 = torch.where(l > 0, l, torch.ones_like(l))
    P = e / l1
    Pn = e.bfloat16().double() / l1 if round_p else P     # the forward rounds exp(s - m), not the normalised P
    v = bh(case.v)
    return SimpleNamespace(o=Pn @ v, A=P @ v.abs(), lse=lse, n=vis.expand(-1, case.H, -1, -1).sum(-1), rows=rows)


def ref_backward(case, o, lse, rows=None, vis_fn=None, rounded=False):
    """Gradients [B, H, S, hd] and their A from the step's own o [B, Sq, H, hd] and lse [B, H, Sq]; `rows`: the query rows that carry a
    nonzero dout (all by default)."""
    rows = _rows(case, rows)
    s, vis = scores(case, rows, vis_fn)
    l = lse.double()[:, :, rows, None]
    dead = torch.isinf(l) | ~vis
    P = torch.where(dead, torch.zeros_like(s), torch.exp(torch.where(dead, torch.zeros_like(s), s - l)))
    do, oo, q = bh(case.dout)[:, :, rows], bh(o)[:, :, rows], bh(case.q)[:, :, rows]
    k, v = bh(case.k), bh(case.v)
    dP, adP = do @ v.transpose(-1, -2), do.abs() @ v.abs().transpose(-1, -2)
    delta, adelta = (do * oo).sum(-1, keepdim=True), (do * oo).abs().sum(-1, keepdim=True)
    dS, adS = P * (dP - delta), P * (adP + adelta)
    Pn = P
    if rounded:
        Pn, dS = P.bfloat16().double(), dS.bfloat16().double()
    dq = torch.zeros(case.B, case.H, case.Sq, case.hd, dtype=torch.float64)
    Adq = torch.zeros_like(dq)
    dq[:, :, rows] = case.scale * (dS @ k)
    Adq[:, :, rows] = case.scale * (adS @ k.abs())
    dST, adST, PT = dS.transpose(-1, -2), adS.transpose(-1, -2), Pn.transpose(-1, -2)
    return SimpleNamespace(dq=dq, Adq=Adq, dk=case.scale * (dST @ q), Adk=case.scale * (adST @ q.abs()), dv=PT @ do,
                           Adv=P.transpose(-1, -2) @ do.abs())


def zero_score_forward(case):
    """Closed form of a case whose scores are all 0 (q = 0, no ALiBi), from cumulative sums over the keys: n_i = valid keys <= i + off,
    o_i = sum of their V / n_i.  No S x S matrix."""
    assert case.slopes is None and not bool(case.q.any())
    B, H, Sq, Sk = case.B, case.H, case.Sq, case.Sk
    valid = torch.ones(B, Sk, dtype=torch.float64) if case.key_valid is None else case.key_valid.double()
    v = bh(case.v)
    vv = valid[:, None, :, None] * v
    if case.causal:
        idx = torch.arange(Sq) + (Sk - Sq)
        live = (idx >= 0).double()
        idx = idx.clamp_min(0)
        n = valid.cumsum(-1)[:, idx] * live[None]
        num = vv.cumsum(2)[:, :, idx] * live[None, None, :, None]
        absnum = vv.abs().cumsum(2)[:, :, idx] * live[None, None, :, None]
    else:
        n = valid.sum(-1, keepdim=True).expand(B, Sq)
        num = vv.sum(2, keepdim=True).expand(B, H, Sq, case.hd)
        absnum = vv.abs().sum(2, keepdim=True).expand(B, H, Sq, case.hd)
    n = n[:, None, :].expand(B, H, Sq)
    d = n.clamp_min(1.0)[..., None]
    lse = torch.where(n > 0, torch.log(n.clamp_min(1.0)), torch.full_like(n, -math.inf))
    return SimpleNamespace(o=num / d, A=absnum / d, lse=lse, n=n, num=num, rows=torch.arange(Sq))


def zero_score_dv(case, n):
    """dV of a zero-score case: P_ij = 1 / n_i on the visible keys, so dV_j = valid_j sum over the rows i >= j - off of dout_i / n_i."""
    B, H, Sq, Sk = case.B, case.H, case.Sq, case.Sk
    valid = torch.ones(B, Sk, dtype=torch.float64) if case.key_valid is None else case.key_valid.double()
    w = torch.where(n > 0, 1.0 / n.clamp_min(1.0), torch.zeros_like(n))[..., None]
    do = bh(case.dout)
    out = []
    for t in (do * w, do.abs() * w):
        if case.causal:
            rc = t.flip(2).cumsum(2).flip(2)
            t = rc[:, :, (torch.arange(Sk) - (Sk - Sq)).clamp_min(0)]
        else:
            t = t.sum(2, keepdim=True).expand(B, H, Sk, case.hd)
        out.append(t * valid[:, None, :, None])
    return out[0], out[1]


def plain_step(case, vis_fn=None, rounded=False):
    """The reference as a step.  rounded: with the bf16 roundings that the kernels make (P, dS and every stored output)."""
    f = ref_forward(case, None, vis_fn, round_p=rounded)
    o = sbh(f.o).bfloat16() if rounded else sbh(f.o)
    g = ref_backward(case, o, f.lse, case.rows_bwd, vis_fn, rounded)
    r = Result(o=o, lse=f.lse, dq=sbh(g.dq), dk=sbh(g.dk), dv=sbh(g.dv))
    if rounded:
        r.dq, r.dk, r.dv = r.dq.bfloat16(), r.dk.bfloat16(), r.dv.bfloat16()
    return r


def closed_step(case):
    """A step for the long zero-score cases without an S x S matrix: the closed forward, dV from it, dK = 0 (q = 0).  dQ (random k) has no
    closed form of this size; the count checks do not read it and it is left 0."""
    f = zero_score_forward(case)
    dv, _ = zero_score_dv(case, f.n)
    z = torch.zeros(case.B, case.Sk, case.H, case.hd, dtype=torch.float64)
    return Result(o=sbh(f.o), lse=f.lse, dq=torch.zeros(case.B, case.Sq, case.H, case.hd, dtype=torch.float64), dk=z, dv=sbh(dv))


def online_forward(case, bug=None):
    """The forward as the kernels walk it: 64-key tiles, running maximum (log2 units), accumulator rescaled only when a row's maximum grew
    by more than RESCALE_LOG2.  bug = 'sum_not_rescaled': the rescale skips the row sum.  bug = 'stale_forever': no rescale after tile 0,
    P taken in fp32 and rounded to bf16 against that stale maximum."""
    rows = torch.arange(case.Sq)
    s, _ = scores(case, rows)
    s = s * math.log2(math.e)
    v = bh(case.v)
    m = torch.full(s.shape[:-1] + (1,), -math.inf, dtype=torch.float64)
    l = torch.zeros_like(m)
    o = torch.zeros(case.B, case.H, case.Sq, case.hd, dtype=torch.float64)
    for t in range((case.Sk + TILE - 1) // TILE):
        st = s[..., t * TILE:(t + 1) * TILE]
        mx = st.amax(-1, keepdim=True)
        grow = (mx > m + RESCALE_LOG2) if bug != "stale_forever" else torch.full_like(mx, t == 0, dtype=torch.bool)
        mnew = torch.where(grow, torch.maximum(m, mx), m)
        muse = torch.where(torch.isinf(mnew), torch.zeros_like(mnew), mnew)
        alpha = torch.where(grow, torch.exp2(m - muse), torch.ones_like(m))
        o = o * alpha
        if bug != "sum_not_rescaled":
            l = l * alpha
        m = mnew
        p = torch.exp2(st - muse)
        if bug == "stale_forever":
            p = p.float().bfloat16().double()
        l = l + p.sum(-1, keepdim=True)
        o = o + p @ v[:, :, t * TILE:(t + 1) * TILE]
    muse = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    lse = torch.where(l > 0, muse * math.log(2.0) + torch.log(l), torch.full_like(l, -math.inf)).squeeze(-1)
    return sbh(o / torch.where(l > 0, l, torch.ones_like(l))), lse


# ---------------------------------------------------------------------------------------------------------------- masks

def make_valid(kind, B, Sk, pads=None, seed=0):
    """uint8 [B, Sk] or None.  'none'.  'left': row b loses its first pads[b] keys.  'right': its last pads[b].  'holes': 'left' with 30 % of
    the keys masked at random and a masked key at both ends of every 64-key tile.  'edges': 'left' with only those tile-end keys masked."""
    if kind == "none":
        return None
    pads = [pads[b % len(pads)] for b in range(B)]
    valid = torch.ones(B, Sk, dtype=torch.uint8)
    for b, p in enumerate(pads):
        p = min(p, Sk)
        if kind == "right":
            valid[b, Sk - p:] = 0
        else:
            valid[b, :p] = 0
    if kind == "holes":
        valid[torch.rand(B, Sk, generator=torch.Generator().manual_seed(seed + Sk)) < 0.3] = 0
    if kind in ("holes", "edges"):
        j = torch.arange(Sk)
        valid[:, (j % TILE == 0) | (j % TILE == TILE - 1)] = 0
    return valid


# ---------------------------------------------------------------------------------------------------------------- builders

def _case(kind, name, B, H, Sq, Sk, hd, causal, key_valid, slopes, layout, q, k, v, dout, **known):
    c = SimpleNamespace(kind=kind, name=name, B=B, H=H, Sq=Sq, Sk=Sk, hd=hd, causal=bool(causal), key_valid=key_valid, slopes=slopes,
                        scale=SCALE, layout=layout, q=q, k=k, v=v, dout=dout, rows_fwd=None, rows_bwd=None, long=max(Sq, Sk) > 2048)
    c.__dict__.update(known)
    return c


def _name(kind, B, H, Sq, Sk, hd, causal, mask, extra=""):
    return "%s%s B%d H%d Sq%d Sk%d hd%d %s mask=%s" % (kind, extra, B, H, Sq, Sk, hd, "causal" if causal else "full", mask)


def _rand(gen, *shape, mul=0.8):
    return (torch.randn(*shape, generator=gen) * mul).bfloat16()


def _edge_keys(valid_row, Sk):
    """First and last valid key of a batch row ([] if none)."""
    if valid_row is None:
        return [0, Sk - 1]
    nz = torch.nonzero(valid_row).flatten()
    return [int(nz[0]), int(nz[-1])] if len(nz) else []


def marked_keys(b, Sq, Sk, key_valid):
    """The keys that own a dim when Sk > 32 hd: first and last key of each 64-key tile, the keys beside the diagonal at each 32-row wave edge
    (i + off and i + off + 1 for i = 32 w - 1, 32 w), the first and last valid key of the row."""
    off = Sk - Sq
    ks = set()
    for t in range(0, Sk, TILE):
        ks.update((t, min(t + TILE - 1, Sk - 1)))
    for w in range(0, Sq + 1, WAVE):
        for i in (w - 1, w):
            if 0 <= i < Sq:
                ks.update(j for j in (i + off, i + off + 1) if 0 <= j < Sk)
    ks.update(_edge_keys(None if key_valid is None else key_valid[b], Sk))
    return sorted(ks)


def count_case(B, H, Sq, Sk, hd, causal, mask="none", key_valid=None, layout="fused", seed=0):
    g = torch.Generator().manual_seed(1000 + seed + Sq + 7 * Sk)
    v = torch.zeros(B, Sk, H, hd)
    for b in range(B):
        keys = list(range(Sk)) if Sk <= COUNT_LIMIT * hd else marked_keys(b, Sq, Sk, key_valid)
        kt = torch.tensor(keys)
        for h in range(H):
            v[b, kt, h, (torch.arange(len(keys)) + 5 * h + 3 * b) % hd] = 1.0
    assert int(v.sum(-1).max()) == 1                                  # one owner dim per (marked) key
    top = int(v.sum(1).max())
    assert top <= COUNT_LIMIT, (top, Sk, hd)                          # no (row, dim) count can exceed the limit
    return _case("count", _name("count", B, H, Sq, Sk, hd, causal, mask), B, H, Sq, Sk, hd, causal, key_valid, None, layout,
                 torch.zeros(B, Sq, H, hd).bfloat16(), _rand(g, B, Sk, H, hd), v.bfloat16(), _rand(g, B, Sq, H, hd, mul=1.0), top=top)


def onekey_targets(B, H, Sq, Sk, key_valid):
    """The keys j* that a shape visits, as lists of B * H keys (one case each)."""
    off = Sk - Sq
    js = [0, 63, 64, 127, 128, Sk - 1, 31 + off, 32 + off, 33 + off]
    for b in range(B):
        js += _edge_keys(None if key_valid is None else key_valid[b], Sk)
    js = sorted({j for j in js if 0 <= j < Sk})
    n = B * H
    return [[js[(c * n + i) % len(js)] for i in range(n)] for c in range((len(js) + n - 1) // n)]


def onekey_case(B, H, Sq, Sk, hd, causal, targets, use_alibi=False, mask="none", key_valid=None, layout="fused", seed=0):
    g = torch.Generator().manual_seed(2000 + seed + Sq + 7 * Sk + targets[0])
    v = torch.zeros(B, Sk, H, hd).bfloat16()
    jstar = torch.tensor(targets).reshape(B, H)
    for b in range(B):
        for h in range(H):
            x = _rand(g, hd, mul=1.0)
            v[b, jstar[b, h], h] = torch.where(x == 0, torch.ones_like(x), x)
    return _case("onekey", _name("onekey", B, H, Sq, Sk, hd, causal, mask, "+alibi" if use_alibi else "") + " j*=%s" % targets, B, H, Sq, Sk,
                 hd, causal, key_valid, alibi(H) if use_alibi else None, layout, torch.zeros(B, Sq, H, hd).bfloat16(), _rand(g, B, Sk, H, hd),
                 v, _rand(g, B, Sq, H, hd, mul=1.0), jstar=jstar)


def onequery_targets(b, Sq, Sk, key_valid):
    """The rows i* that a shape visits in batch row b."""
    off = Sk - Sq
    rows = [0, 31, 32, 127, 128, Sq - 1]
    if key_valid is not None:
        e = _edge_keys(key_valid[b], Sk)
        if e:
            rows += [e[0] - off, e[0] - off - 1]              # the first live row behind the left padding, the last dead one
    rows += [-off, -off - 1]                                   # Sq > Sk: the same two rows
    return sorted({i for i in rows if 0 <= i < Sq})


def onequery_case(B, H, Sq, Sk, hd, causal, bstar, targets, use_alibi=False, mask="none", key_valid=None, layout="fused", seed=0, pool=None):
    """targets: H rows, one per head, of batch row bstar.  pool: q / k / v to share between the cases of a shape."""
    g = torch.Generator().manual_seed(3000 + seed + Sq + 7 * Sk + 13 * bstar + targets[0])
    q, k, v = pool if pool is not None else (_rand(g, B, Sq, H, hd), _rand(g, B, Sk, H, hd), _rand(g, B, Sk, H, hd))
    dout = torch.zeros(B, Sq, H, hd).bfloat16()
    for h in range(H):
        x = _rand(g, hd, mul=1.0)
        dout[bstar, targets[h], h] = torch.where(x == 0, torch.ones_like(x), x)
    c = _case("onequery", _name("onequery", B, H, Sq, Sk, hd, causal, mask, "+alibi" if use_alibi else "") + " b*=%d i*=%s" % (bstar, targets),
              B, H, Sq, Sk, hd, causal, key_valid, alibi(H) if use_alibi else None, layout, q, k, v, dout, bstar=bstar,
              istar=torch.tensor(targets))
    c.rows_bwd = torch.tensor(sorted(set(targets)))
    if c.long:
        c.rows_fwd = torch.tensor(sorted(set(targets) | {0, Sq // 2 + 1, Sq - 1}))
    return c


def oracle_case(B, H, Sq, Sk, hd, causal, use_alibi=False, mask="none", key_valid=None, layout="fused", seed=0):
    g = torch.Generator().manual_seed(4000 + seed + Sq + 7 * Sk)
    return _case("oracle", _name("oracle", B, H, Sq, Sk, hd, causal, mask, "+alibi" if use_alibi else ""), B, H, Sq, Sk, hd, causal, key_valid,
                 alibi(H) if use_alibi else None, layout, _rand(g, B, Sq, H, hd), _rand(g, B, Sk, H, hd), _rand(g, B, Sk, H, hd),
                 _rand(g, B, Sq, H, hd, mul=1.0))


def ramp_case(ramp, hd, use_alibi, causal, layout="fused"):
    """Eight 64-key tiles whose maximum score moves by RAMPS[ramp] per tile ('jump60': once, at tile 4; 'down60': tile 0 holds the maximum
    and every later tile lies 60 below).  Within a tile one key holds the maximum, the others lie up to 3 below it.  s_j = c_j + f_j with
    c the bf16 rounding of the target and f that of the remainder, so the growth holds to 2^-15."""
    B, H, S, step = 1, 2, 8 * TILE, RAMPS[ramp]
    g = torch.Generator().manual_seed(5000 + int(abs(step) * 10) + hd)
    t = torch.arange(S) // TILE
    top = {"jump60": step * (t >= 4), "down60": step * (t >= 1)}.get(ramp, step * t).double()
    u = 3.0 * torch.rand(S, generator=g).double()
    u[torch.arange(8) * TILE + (17 * torch.arange(8) + 5) % TILE] = 0.0
    target = top - u
    c = target.bfloat16()
    f = (target - c.double()).bfloat16()
    q = torch.zeros(B, S, H, hd).bfloat16()
    q[..., 0] = 8.0
    q[..., 1] = 8.0
    k = torch.zeros(B, S, H, hd).bfloat16()
    k[..., 0] = c[None, :, None]
    k[..., 1] = f[None, :, None]
    case = _case("ramp", _name("ramp", B, H, S, S, hd, causal, "none", " %s%s" % (ramp, "+alibi" if use_alibi else "")), B, H, S, S, hd, causal,
                 None, alibi(H) if use_alibi else None, layout, q, k, _rand(g, B, S, H, hd), _rand(g, B, S, H, hd, mul=1.0), ramp=ramp)
    # the builder's condition: the growth of the tile maximum of scale q.k is the stated one, on the stated side of the rescale threshold
    s = (c.double() + f.double()).reshape(8, TILE).amax(-1)
    grow = s[1:] - s[:-1]
    want = {"jump60": torch.tensor([0, 0, 0, step, 0, 0, 0.0]), "down60": torch.tensor([step, 0, 0, 0, 0, 0, 0.0])}.get(ramp, torch.full((7,), step))
    assert float((grow - want.double()).abs().max()) < 2.0 ** -12, (ramp, grow)
    case.growth_log2 = grow * math.log2(math.e)
    if ramp == "up5.0":
        assert bool((case.growth_log2 < RESCALE_LOG2).all()) and bool((case.growth_log2 > RESCALE_LOG2 - 1).all())
    if ramp == "up5.6":
        assert bool((case.growth_log2 > RESCALE_LOG2).all()) and bool((case.growth_log2 < RESCALE_LOG2 + 0.1).all())
    return case


# ---------------------------------------------------------------------------------------------------------------- case lists

def shape_cases(B, H, Sq, Sk, hd, causal, mask="none", pads=None, layout="fused", backward=True, kinds=("count", "onekey", "onequery", "oracle"),
                onekey_alibi=True):
    """Every case of one shape and mask, inputs built once."""
    kv = make_valid(mask, B, Sk, pads, seed=Sq)
    kw = dict(mask=mask, key_valid=kv, layout=layout)
    out = []
    if "count" in kinds:
        out.append(count_case(B, H, Sq, Sk, hd, causal, **kw))
    if "onekey" in kinds:
        for n, tg in enumerate(onekey_targets(B, H, Sq, Sk, kv)):
            out.append(onekey_case(B, H, Sq, Sk, hd, causal, tg, use_alibi=(onekey_alibi and n % 2 == 1), **kw))
        if onekey_alibi and not any(c.slopes is not None for c in out):
            out.append(onekey_case(B, H, Sq, Sk, hd, causal, onekey_targets(B, H, Sq, Sk, kv)[0], use_alibi=True, **kw))
    if "onequery" in kinds and backward:
        g = torch.Generator().manual_seed(6000 + Sq + 7 * Sk)
        pool = (_rand(g, B, Sq, H, hd), _rand(g, B, Sk, H, hd), _rand(g, B, Sk, H, hd))
        n = 0
        for b in range(B):
            rows = onequery_targets(b, Sq, Sk, kv)
            if B > 2:        # padded batches: the rows at the padding's edge first, then two of the general list in turn
                e = [i for i in rows if i not in (0, 31, 32, 127, 128, Sq - 1)] or rows
                rest = [i for i in rows if i not in e] or rows
                rows = (e + [rest[b % len(rest)]])[:2] + [rest[(b + 1) % len(rest)], rest[(b + 3) % len(rest)]]
            for c0 in range(0, len(rows), H):
                tg = [rows[(c0 + h) % len(rows)] for h in range(H)]
                out.append(onequery_case(B, H, Sq, Sk, hd, causal, b, tg, use_alibi=(n % 2 == 1), pool=pool, **kw))
                n += 1
    if "oracle" in kinds:
        out.append(oracle_case(B, H, Sq, Sk, hd, causal, use_alibi=False, **kw))
        out.append(oracle_case(B, H, Sq, Sk, hd, causal, use_alibi=True, seed=1, **kw))
    return out


def narrow_cases(S, hd, layout="fused"):
    return [c for causal in (True, False) for c in shape_cases(2, 2, S, S, hd, causal, layout=layout)]


def padded_cases(mask, hd, layout="fused"):
    """B = 10, S = 260: 'left', 'holes' or 'right' with PADS keys lost per row."""
    return shape_cases(len(PADS), 2, PAD_S, PAD_S, hd, True, mask=mask, pads=PADS, layout=layout)


def sqsk_cases(Sq, Sk, hd, layout="fused"):
    out = []
    for causal in (True, False):
        for mask in ("none", "left"):
            if mask == "left" and Sk < 8:
                continue
            out += shape_cases(2, 2, Sq, Sk, hd, causal, mask=mask, pads=[0, 5], layout=layout)
    return out


def ramp_cases():
    return [ramp_case(r, hd, al, causal) for r in RAMPS for (hd, al) in ((128, False), (128, True), (64, False)) for causal in (False, True)]


def long_cases(Sq, Sk, hd=128, mask="edges", pad=200, backward=True, causal=True, layout="fused"):
    """B = 1, H = 2 at the lengths where the kernels change form: a count case and the one-query cases, answers from cumulative sums and
    single score rows."""
    kinds = ("count", "onequery") if backward else ("count", "onekey")
    return shape_cases(1, 2, Sq, Sk, hd, causal, mask=mask, pads=[pad], layout=layout, backward=backward, kinds=kinds, onekey_alibi=False)


# ---------------------------------------------------------------------------------------------------------------- checkers

def _judge(case, reason, got, ref, tol):
    got = got.double()
    tol = torch.where(tol > 0, tol + UNDERFLOW, tol)
    err = (got - ref).abs()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        i = tuple(int(x) for x in torch.nonzero(ratio == ratio.max())[0])
        raise CheckFailure(reason, "%s at %s: got %r, reference %r, bound %r" % (case.name, i, float(got[i]), float(ref[i]), float(tol[i])))
    WORST[(case.kind, reason)] = max(WORST.get((case.kind, reason), 0.0), worst)      # of the checks that passed
    return worst


def _exact_zero(case, reason, got, where, what):
    if where.any():
        bad = (got.double() != 0) & where
        bad = bad | (torch.isnan(got.double()) & where)
        if bad.any():
            i = tuple(int(x) for x in torch.nonzero(bad)[0])
            raise CheckFailure(reason, "%s: %s must be exactly 0, got %r at %s" % (case.name, what, float(got.double()[i]), i))


def forward_reference(case):
    if getattr(case, "_fwd", None) is None:
        if case.long and case.kind in ("count", "onekey"):
            case._fwd = zero_score_forward(case)
        else:
            case._fwd = ref_forward(case, case.rows_fwd)
    return case._fwd


def check_forward(case, res):
    """The forward's o and lse.  Returns the largest error / bound."""
    f = forward_reference(case)
    rows = f.rows
    o, lse = bh(res.o)[:, :, rows], res.lse.double()[:, :, rows]
    dead = f.n == 0
    _exact_zero(case, "dead.o", o, dead[..., None].expand_as(o), "o of a row without a visible key")
    if bool((dead & ~(torch.isinf(lse) & (lse < 0))).any()):
        raise CheckFailure("dead.lse", "%s: lse of a row without a visible key must be -inf" % case.name)
    live = ~dead
    lse_l = torch.where(live, lse, torch.zeros_like(lse))
    ref_l = torch.where(live, f.lse, torch.zeros_like(lse))
    worst = 0.0
    if case.kind == "count":
        n = f.n.double().clamp_min(1.0)
        worst = max(worst, _judge(case, "count.lse", lse_l, ref_l, torch.where(live, 0.25 / n, torch.ones_like(n))))
        worst = max(worst, _judge(case, "count.o", o, f.o, BF16 * f.o))
        return worst
    if case.kind == "onekey":
        sees = visible(case, rows).expand(-1, case.H, -1, -1).gather(-1, case.jstar[:, :, None, None].expand(-1, -1, len(rows), 1))
        _exact_zero(case, "onekey.zero", o, (~sees).expand_as(o), "a row that must not see j*")
    worst = max(worst, _judge(case, "%s.o" % _family(case), o, f.o, (R_O * BF16 + FP32_SLACK) * f.A))
    # lse = m ln 2 + logf(l): the row sum carries the relative fp32 slack of its terms, the sum itself a few spacings of its value
    worst = max(worst, _judge(case, "%s.lse" % _family(case), lse_l, ref_l, FP32_SLACK + 2.0 ** -21 * ref_l.abs()))
    return worst


def _family(case):
    return {"onekey": "onekey", "ramp": "ramp"}.get(case.kind, "oracle")


def check_backward(case, res):
    """dQ, dK and dV against the reference backward of the step's own o and lse.  Returns the largest error / bound."""
    B, H, Sq, Sk = case.B, case.H, case.Sq, case.Sk
    dq, dk, dv = bh(res.dq), bh(res.dk), bh(res.dv)
    if case.key_valid is not None:
        masked = (case.key_valid == 0)[:, None, :, None].expand_as(dk)
        _exact_zero(case, "bwd.dk.zero", dk, masked, "dK of a masked key")
        _exact_zero(case, "bwd.dv.zero", dv, masked, "dV of a masked key")
    dead = torch.isinf(res.lse.double())[..., None].expand_as(dq)
    _exact_zero(case, "dead.dq", dq, dead, "dQ of a row without a visible key")
    worst = 0.0
    if case.kind == "count":           # q = 0: dK is exactly 0; dV in closed form
        rdv, adv = zero_score_dv(case, forward_reference(case).n.double())
        _exact_zero(case, "bwd.dk.zero", dk, torch.ones_like(dk, dtype=torch.bool), "dK with q = 0")
        return _judge(case, "bwd.dv", dv, rdv, (R_DV * BF16 + FP32_SLACK) * adv)
    if case.kind == "onequery":
        hot = torch.zeros(B, H, Sq, dtype=torch.bool)
        hot[case.bstar, torch.arange(H), case.istar] = True
        _exact_zero(case, "bwd.dq.zero", dq, (~hot)[..., None].expand_as(dq), "dQ off the row i*")
        cold = torch.ones(B, H, Sk, dtype=torch.bool)
        lim = case.istar + (Sk - Sq) if case.causal else torch.full((H,), Sk - 1)
        cold[case.bstar] = torch.arange(Sk)[None, :] > lim[:, None]
        _exact_zero(case, "bwd.dk.zero", dk, cold[..., None].expand_as(dk), "dK above i* + off or in another batch row")
        _exact_zero(case, "bwd.dv.zero", dv, cold[..., None].expand_as(dv), "dV above i* + off or in another batch row")
    g = ref_backward(case, res.o, res.lse, case.rows_bwd)
    worst = max(worst, _judge(case, "bwd.dq", dq, g.dq, (R_DQ * BF16 + FP32_SLACK) * g.Adq))
    worst = max(worst, _judge(case, "bwd.dk", dk, g.dk, (R_DK * BF16 + FP32_SLACK) * g.Adk))
    worst = max(worst, _judge(case, "bwd.dv", dv, g.dv, (R_DV * BF16 + FP32_SLACK) * g.Adv))
    return worst


def check(case, res, backward=True):
    w = check_forward(case, res)
    return max(w, check_backward(case, res)) if backward else w


def worst_table():
    return "\n".join("[flash-cases] %-9s %-12s worst error / bound %.3f" % (k[0], k[1], v) for k, v in sorted(WORST.items()))
