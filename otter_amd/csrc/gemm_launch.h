// gemm_launch.h -- host only: how the dispatch (gemm.hip) reaches the kernel files.  Each kernel file exports one launch function per kernel
// family; what a launch needs from the process state (CU budget, grid mode, cross-tile switch) comes in as arguments.
#pragma once
#include "gemm_args.h"
#include <type_traits>

namespace {

// Launch of a kernel with dynamic LDS: the attribute that admits more than 64 KB is set once per kernel instantiation (the function-local
// static of this template, which is keyed on the kernel).
template <auto Kernel>
int launch_lds(unsigned blocks, unsigned threads, int smem, hipStream_t st, const GemmArgs& g) {
    static bool once = false;
    if (!once) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) OTTER_FAIL(OTTER_ERR_LAUNCH, "hipFuncSetAttribute(%d B LDS): %s", smem, hipGetErrorString(e));
        once = true;
    }
    hipLaunchKernelGGL(Kernel, dim3(blocks), dim3(threads), smem, st, g);
    return OTTER_OK;
}

// The epilogue kind is a template argument of every kernel: f(std::integral_constant<int, kind>)
template <typename F>
int with_epi(int kind, F f) {
    switch (kind) {
        case OTTER_EPI_STORE: return f(std::integral_constant<int, OTTER_EPI_STORE>{});
        case OTTER_EPI_GELU: return f(std::integral_constant<int, OTTER_EPI_GELU>{});
        case OTTER_EPI_SCALE_RES: return f(std::integral_constant<int, OTTER_EPI_SCALE_RES>{});
        default: return f(std::integral_constant<int, OTTER_EPI_GATE_BWD>{});
    }
}

}  // namespace

// kind: the epilogue (otter_epilogue_kind); tiles: output tiles of the kernel's tile size (cfg_tiles); cus: the CUs a persistent grid may use
// (otter_gemm_set_cu_budget).  Not exported from the library.
#define GEMM_LOCAL __attribute__((visibility("hidden")))
GEMM_LOCAL int gemm_launch_f32(int kind, unsigned tiles, hipStream_t st, const GemmArgs& g);                                      // gemm_tiled.hip
GEMM_LOCAL int gemm_launch_tiled(int kind, int bm, bool glds, unsigned tiles, unsigned cus, hipStream_t st, const GemmArgs& g);   // gemm_tiled.hip: 128^2, 256^2, 256^2 with LDS-DMA
GEMM_LOCAL int gemm_launch_ph(int kind, unsigned tiles, unsigned cus, hipStream_t st, const GemmArgs& g);                         // gemm_ph.hip
// per_tile: one workgroup per tile instead of a persistent grid; xt: the cross-tile form is on (it runs where the kernel file says it applies)
GEMM_LOCAL int gemm_launch_t4(int kind, unsigned tiles, unsigned cus, bool per_tile, bool xt, hipStream_t st, const GemmArgs& g);   // gemm_t4.hip
GEMM_LOCAL int gemm_launch_s4(int kind, unsigned tiles, unsigned cus, hipStream_t st, const GemmArgs& g);                         // gemm_s4.hip
GEMM_LOCAL int gemm_launch_s4h(int kind, unsigned tiles, unsigned cus, hipStream_t st, const GemmArgs& g);                        // gemm_s4.hip
