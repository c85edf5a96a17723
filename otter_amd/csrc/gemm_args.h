// gemm_args.h -- what the host half of the GEMM (gemm.hip) hands to every kernel, and the vector types the kernels share.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

struct GemmArgs {
    const void* A; int64_t lda;
    const void* B; int64_t ldb;
    void* C; int64_t ldc; int cdt;
    int64_t M, N, K;
    int kind, accumulate;
    const float* gate;
    const void* R; int64_t ldr; int rdt;
    void* C2; int64_t ldc2;
    const void* aux; int64_t ldaux; int auxdt; int aux_gelu;
    float* partial;
    int gm, gn;
    int dbg;  // diagnostics only (otter_gemm_set_debug): bit0 = skip K-loop global loads, bit1 = skip MFMAs
    int order;  // tile order override (diagnostics, see tile_of_block)
    int wide;  // bf16 output and every tensor the fused tail touches allows 8-element accesses (N, ldc, ldc2, ldr, ldaux % 8 == 0)
    int ta, tb;  // operand A / B is K-major ([K rows][M or N columns]); variant 26 only (otter_gemm)
    int grid_mode;  // host side only: 0 = process default (otter_gemm_set_persistent), 1 = persistent grid, 2 = one workgroup per tile
    int korder;  // cross-tile form of variant 26: K-tile order of a tile (bits 0-1 rotation by XCD / tile, bits 2-3 in-group permutation; see xt_tile);
                 // bits 4-6: start phase step (units of 1024 cycles) between the four workgroup phases
};
