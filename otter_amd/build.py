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
SOURCES = ["lib.hip", "gemm.hip", "norm.hip", "attn.hip", "elementwise.hip", "flash.hip", "optim.hip", "attn_mfma.hip", "loss.hip", "fuyu.hip", "decode.hip", "persimmon_decode.hip", "persimmon_decode_cache.hip", "decode_cache.hip", "decode_cache_i8.hip", "decode_cache_shared.hip", "xattn_decode.hip", "w8.hip", "logits.hip", "beam.hip", "select.hip", "probe.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-Wno-unused-result", "-Wno-unused-value"]
# gemm.hip: the K-major instantiations of variant 26 keep their accumulators in explicit AGPRs behind asm MFMAs; hipcc must not use the
# AGPR half as spill space of its own there (it would, between the K loop and the tail's read-back: measured as wrong blocks)
EXTRA = {"gemm.hip": ["-mllvm", "-amdgpu-spill-vgpr-to-agpr=0"]}


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


def build_variant(source: str, defines, suffix: str, verbose: bool = True) -> str:
    """Tools-only A/B or diagnostics library: `source` compiled with extra -D `defines`, linked with the product's other objects ->
    lib/libotter_hip_<suffix>.so.  Loaded through OTTER_LIB_PATH; the product never does (some of these give wrong results by construction)."""
    build(verbose=verbose)  # the other objects
    cc = hipcc()
    obj = os.path.join(LIBDIR, "%s_%s.o" % (source.replace(".hip", ""), suffix))
    out = os.path.join(LIBDIR, "libotter_hip_%s.so" % suffix)
    subprocess.check_call([cc, *FLAGS, *EXTRA.get(source, []), *["-D" + d for d in defines], "-c", os.path.join(CSRC, source), "-o", obj])
    others = [os.path.join(LIBDIR, s.replace(".hip", ".o")) for s in SOURCES if s != source]
    subprocess.check_call([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, obj, *others])
    return out


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    # every header and every included piece of a source (gemm.hip includes its generated K-tile schedules)
    hdrs = [os.path.join(os.path.dirname(HERE), "include", "otter_hip.h")]
    for d, _, names in os.walk(CSRC):
        hdrs += [os.path.join(d, n) for n in names if n.endswith((".h", ".inc"))]
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    if not force and _newer(LIB, srcs + hdrs):
        return LIB
    cc = hipcc()
    objs = [os.path.join(LIBDIR, s.replace(".hip", ".o")) for s in SOURCES]

    def one(pair):
        src, obj = pair
        if not force and _newer(obj, [src] + hdrs):
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
        print(build_variant("gemm.hip", [arg("--define", 1)], arg("--define", 2)))
    elif "--flash-define" in sys.argv:  # --flash-define OTTER_FLASH_SAFE_DMA safedma
        print(build_variant("flash.hip", [arg("--flash-define", 1)], arg("--flash-define", 2)))
    elif "--src-define" in sys.argv:    # --src-define norm.hip OTTER_NORM_NT=1 normnt
        print(build_variant(arg("--src-define", 1), [arg("--src-define", 2)], arg("--src-define", 3)))
    elif "--flash-timing" in sys.argv:  # the in-kernel timeline of the flash forward (tools/flash_timeline.py)
        print(build_variant("flash.hip", ["OTTER_FLASH_TIMING"], "flashtiming"))
    elif "--diag" in sys.argv:          # --diag 4: the tail diagnostics of csrc/gemm.hip (OTTER_DIAG)
        print(build_variant("gemm.hip", ["OTTER_DIAG=%d" % int(arg("--diag", 1))], "diag%d" % int(arg("--diag", 1))))
    else:
        print(build(force="--force" in sys.argv))
