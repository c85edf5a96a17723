"""Round 6: the cross-tile form of variant 26 (XT: the DMA ring keeps running across the tiles of a persistent workgroup, csrc/gemm.hip T4_XT_*)
and its K-order modes against the round-5 kernel and hipBLASLt, on COLD operands (launches rotate over NSET operand sets, as the step's layers do).
One process, legs interleaved, `reps` rounds, min and median per leg.  Also checks that XT with the plain K order is BIT-IDENTICAL to the round-5
kernel on every leg, and that a permuted K order stays within bf16 rounding of it.
Usage: gemm_xt_ab.py [reps] [korder,korder,...]      (korder: bits 0-1 rotation 0 none / 1 XCD halves+quarters / 2 XCD eighths / 3 per tile;
                                                       bits 2-3 in-group permutation 0 none / 1 groups of 4 / 2 groups of 8 / 3 pairs;
                                                       bits 4-6 start phase step d: workgroup b starts ((b >> 3) & 3) * d * 1024 cycles late)"""
import os, statistics, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from otter_amd import ops
from otter_amd import _capi as K
from otter_amd._capi import EPI_GELU, EPI_GATE_BWD, EPI_STORE

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
korders = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [0, 1, 2, 4, 5, 8, 12]
M, D, FF = 4096, 4096, 16384
NSET = int(os.environ.get("NSET", "8"))
bf = torch.bfloat16
amp = float(os.environ.get("AMP", "0.05"))


def rnd(*s):
    return (torch.randn(*s, device="cuda") * amp).to(bf)


xs = [rnd(M, D) for _ in range(NSET)]          # activations [tokens, D]
W1 = [rnd(FF, D) for _ in range(NSET)]         # up projection [16384, 4096]
hs = [rnd(M, FF) for _ in range(NSET)]         # hidden [tokens, 16384]
W2 = [rnd(D, FF) for _ in range(NSET)]         # down projection [4096, 16384]
ubuf = torch.empty(M, FF, device="cuda", dtype=bf)
obuf = torch.empty(M, FF, device="cuda", dtype=bf)
obuf_d = torch.empty(M, D, device="cuda", dtype=bf)
o32 = torch.empty(D, FF, device="cuda")
gate = torch.full((1,), 0.5, device="cuda")
part = torch.empty(ops.gemm_num_partials(M, FF, bf), device="cuda")


def set_mode(xt, korder=0):
    # otter_gemm_set_debug: bits 14-15 = 1 off / 2 on; bit 23 + bits 16-22 = K order / start phase override
    K.gemm_set_debug(((2 if xt else 1) << 14) | (1 << 23) | ((korder & 127) << 16))


legs = {
    "up     x W1^T            bf16 ": lambda i: ops.gemm_nt(xs[i], W1[i], out=obuf),
    "up     x W1^T + GELU     bf16 ": lambda i: ops.gemm_nt(xs[i], W1[i], out=obuf, kind=EPI_GELU, C2=ubuf),
    "down   h W2^T (K=16384)  bf16 ": lambda i: ops.gemm_nt(hs[i], W2[i], out=obuf_d),
    "dW2    dy^T h  (A^T B^T) f32  ": lambda i: ops.gemm(xs[i], hs[i], True, True, out=o32, kind=EPI_STORE, gate=gate),
    "dU     dy W2 GELU' (B^T) bf16 ": lambda i: ops.gemm(xs[i], W2[i], False, True, out=obuf, kind=EPI_GATE_BWD, gate=gate, aux=hs[i], aux_gelu=True, partial=part),
    "df     dU W1   (B^T)     bf16 ": lambda i: ops.gemm(hs[i], W1[i], False, True, out=obuf_d),
}
lib_legs = {
    "up     x W1^T            bf16 ": lambda i: F.linear(xs[i], W1[i]),
    "down   h W2^T (K=16384)  bf16 ": lambda i: F.linear(hs[i], W2[i]),
}

# ---- correctness: XT (plain K order) must equal the round-5 kernel bit for bit; permuted orders within bf16 rounding ----
ref = {}
set_mode(False)
for k, fn in legs.items():
    ref[k] = fn(1).float().clone()
    if "GELU " in k:
        ref[k + "/u"] = ubuf.float().clone()
    if "GELU'" in k:
        ref[k + "/p"] = part.clone()
bad = 0
for ko in [0] + [k for k in korders if k]:
    set_mode(True, ko)
    for k, fn in legs.items():
        for rep in range(2):          # twice: the second launch finds a warm chip and different timing of the ring
            got = fn(1).float()
            outs = [(k, got, ref[k])]
            if "GELU " in k:
                outs.append((k + "/u", ubuf.float(), ref[k + "/u"]))
            if "GELU'" in k:
                outs.append((k + "/p", part, ref[k + "/p"]))
            for name, a, b in outs:
                if ko == 0:
                    ok = torch.equal(a, b)
                else:
                    ok = float((a - b).norm() / b.norm()) < (1e-4 if ("f32" in name or name.endswith("/p")) else 1e-2)
                if not ok:
                    bad += 1
                    print("MISMATCH korder=%d %s rep %d: max abs diff %.4g, rel l2 %.3g, nan %d" %
                          (ko, name, rep, float((a - b).abs().max()), float((a - b).norm() / b.norm()), int(torch.isnan(a).sum())))
print("correctness: %s (XT bit-identical to the round-5 kernel at korder 0; permuted orders within rounding)" % ("OK" if bad == 0 else "%d MISMATCHES" % bad))


def timeit(fn, iters=16):
    for i in range(4):
        fn(i % NSET)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i % NSET)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


modes = [("r5 ", False, 0)] + [("xt%-3d" % ko, True, ko) for ko in korders]
res = {}
for rep in range(reps):
    for k, fn in legs.items():
        if k in lib_legs:
            res.setdefault((k, "lib "), []).append(timeit(lib_legs[k]))
        for name, xt, ko in modes:
            set_mode(xt, ko)
            res.setdefault((k, name), []).append(timeit(fn))
K.gemm_set_debug(0)
print("cold operands (%d sets in rotation), us per launch: min / median of %d rounds" % (NSET, reps))
for k in legs:
    row = []
    for name in (["lib "] if k in lib_legs else []) + [m[0] for m in modes]:
        v = res[(k, name)]
        row.append("%s %6.1f/%6.1f" % (name, min(v), statistics.median(v)))
    print(k, " | ".join(row))
sys.exit(1 if bad else 0)
