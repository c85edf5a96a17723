"""Build libotter_hip.so (gfx950 only) in-tree with hipcc.  `python -m otter_amd.build [--force]`.

The .so is git-ignored but travels with the gpurun snapshot; the product refuses to run without it (no fallback)."""
from __future__ import annotations

import concurrent.futures as cf
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libotter_hip.so")
# The GEMM: the host half (gemm.hip) and one unit per kernel family; variant 26 and the ring kernels share one (csrc/gemm_t4_s4.hip says why).
# First in SOURCES: the longest compile starts first.
GEMM = ["gemm_t4_s4.hip", "gemm_tiled.hip", "gemm_ph.hip", "gemm.hip"]
SOURCES = GEMM + ["lib.hip", "norm.hip", "attn.hip", "elementwise.hip", "flash.hip", "optim.hip", "attn_mfma.hip", "loss.hip", "fuyu.hip", "decode.hip", "persimmon_decode.hip", "persimmon_decode_cache.hip", "decode_cache.hip", "decode_cache_i8.hip", "decode_cache_shared.hip", "decode_cache_shared_i8.hip", "branch_attn.hip", "xattn_decode.hip", "w8.hip", "logits.hip", "beam.hip", "select.hip", "probe.hip"]
PIECES = {"gemm_t4_s4.hip": ["gemm_t4.hip", "gemm_s4.hip"], "w8.hip": ["w8_panel.hip"]}   # .hip files a unit includes: they rebuild that unit only (a header or .inc rebuilds all)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-Wno-unused-result", "-Wno-unused-value"]
# the GEMM units: the K-major instantiations of variant 26 keep their accumulators in explicit AGPRs behind asm MFMAs; hipcc must not use the
# AGPR half as spill space of its own there (it would, between the K loop and the tail's read-back: measured as wrong blocks)
EXTRA = {s: ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"] for s in GEMM}


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def build_variant(sources, defines, suffix: str, verbose: bool = True) -> str:
    """Tools-only A/B or diagnostics library: every unit of `sources` compiled with extra -D `defines`, linked with the product's other objects
    -> lib/libotter_hip_<suffix>.so.  Loaded through OTTER_LIB_PATH; the product never does (some of these give wrong results by construction)."""
    build(verbose=verbose)  # the other objects
    cc = hipcc()
    objs = []
    for source in sources:
        objs.append(os.path.join(LIBDIR, "%s_%s.o" % (source.replace(".hip", ""), suffix)))
        subprocess.check_call([cc, *FLAGS, *EXTRA.get(source, []), *["-D" + d for d in defines], "-c", os.path.join(CSRC, source), "-o", objs[-1]])
    out = os.path.join(LIBDIR, "libotter_hip_%s.so" % suffix)
    others = [os.path.join(LIBDIR, s.replace(".hip", ".o")) for s in SOURCES if s not in sources]
    subprocess.check_call([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, *objs, *others])
    return out


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    # every header and every included piece of a source (gemm_t4.hip includes its generated K-tile schedules)
    hdrs = [os.path.join(os.path.dirname(HERE), "include", "otter_hip.h")]
    for d, _, names in os.walk(CSRC):
        hdrs += [os.path.join(d, n) for n in names if n.endswith((".h", ".inc"))]
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    pieces = {os.path.join(CSRC, s): [os.path.join(CSRC, p) for p in ps] for s, ps in PIECES.items()}
    if not force and _newer(LIB, srcs + sum(pieces.values(), []) + hdrs):
        return LIB
    cc = hipcc()
    objs = [os.path.join(LIBDIR, s.replace(".hip", ".o")) for s in SOURCES]

    def one(pair):
        src, obj = pair
        if not force and _newer(obj, [src] + pieces.get(src, []) + hdrs):
            return obj
        cmd = [cc, *FLAGS, *EXTRA.get(os.path.basename(src), []), "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return obj

    with cf.ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(one, zip(srcs, objs)))
    cmd = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    arg = lambda flag, k: sys.argv[sys.argv.index(flag) + k]
    if "--define" in sys.argv:          # --define OTTER_T4_ABL=4 abl4
        print(build_variant(["gemm_t4_s4.hip"], [arg("--define", 1)], arg("--define", 2)))   # (the unit of variant 26)
    elif "--flash-define" in sys.argv:  # --flash-define OTTER_FLASH_SAFE_DMA safedma
        print(build_variant(["flash.hip"], [arg("--flash-define", 1)], arg("--flash-define", 2)))
    elif "--src-define" in sys.argv:    # --src-define norm.hip OTTER_NORM_NT=1 normnt
        print(build_variant([arg("--src-define", 1)], [arg("--src-define", 2)], arg("--src-define", 3)))
    elif "--flash-timing" in sys.argv:  # the in-kernel timeline of the flash forward (tools/flash_timeline.py)
        print(build_variant(["flash.hip"], ["OTTER_FLASH_TIMING"], "flashtiming"))
    elif "--diag" in sys.argv:          # --diag 4: the tail diagnostics of csrc/gemm_tail.h (OTTER_DIAG): every GEMM unit
        print(build_variant(GEMM, ["OTTER_DIAG=%d" % int(arg("--diag", 1))], "diag%d" % int(arg("--diag", 1))))
    else:
        print(build(force="--force" in sys.argv))
