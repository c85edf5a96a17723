// gemm_tiled.hip -- the tiled kernels of the GEMM and their launches: gemm_bf16_kernel (variants 1-3; the map of the variants is in gemm.hip)
// and gemm_f32_kernel (fp32 operands).
//
// bf16 kernel (the MFMA-bound kernel of the path: the gated cross-attention FFN is 96.8 % of a block's FLOPs):
//   * block tile BM x BN x 64, WM x WN waves; each wave owns a (BM/WM) x (BN/WN) sub-tile as MI x NI blocks of
//     32x32 accumulated by v_mfma_f32_32x32x16_bf16 (fp32 accumulate).
//   * operands are fed SWAPPED (a-operand = B rows, b-operand = A rows) so that a lane's 16 accumulator registers
//     hold, for ONE output row m, four runs of 4 consecutive n: the epilogue then reads/writes 8-byte (bf16) or
//     16-byte (f32) vectors of C / residual / aux instead of 2-byte scalars.
//   * LDS image per operand tile: [rows][64] bf16 = 128 B rows, 16-B slot index XOR-swizzled with (row>>1)&7, so a
//     ds_read_b128 lane group (16 lanes = 16 distinct rows, one k-slot) touches 16 distinct 16-B slots of the two
//     256-B bank rows -> conflict-free (MI355X guide, LDS section).
//   * double-buffered LDS, ONE barrier per K-tile: global loads for tile t+1 are issued before the MFMAs of tile t
//     and written to the other buffer after them (register staging), or -- variant 3 -- go straight to LDS with
//     global_load_lds_dwordx4 (the swizzle then lives on the per-lane SOURCE address; LDS destination is lane-linear).
//   * XCD-aware block order: consecutive (swizzled) ids sweep M inside one N panel, and each XCD gets a contiguous
//     chunk of that order, so a weight panel is fetched into one XCD's L2 once.
// f32 kernel (parity mode, exact f32): v_mfma_f32_32x32x2_f32, 64x64x32 tile, padded LDS rows.
#include "gemm_tail.h"
#include "gemm_launch.h"

namespace {

// ------------------------------------------------------------------------------------------------------------
// bf16 MFMA kernel
// ------------------------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, bool GLDS, int EPI>
__global__ __launch_bounds__(WM* WN * 64) void gemm_bf16_kernel(GemmArgs g) {
    static_assert(BN / WN == 64, "the epilogue stripe is 64 columns wide");
    constexpr int NT = WM * WN * 64;
    constexpr int TM = BM / WM, TN = BN / WN;
    constexpr int MI = TM / 32, NI = TN / 32;
    constexpr int A_CH = BM * 8 / NT, B_CH = BN * 8 / NT;
    constexpr int TILE_BYTES = (BM + BN) * 128;
    static_assert(BM * 8 % NT == 0 && BN * 8 % NT == 0, "tile/threads mismatch");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const bf16_t* __restrict__ A = (const bf16_t*)g.A;
    const bf16_t* __restrict__ B = (const bf16_t*)g.B;
    const int64_t K = g.K;
    const int nk = (int)((K + 63) >> 6);
    const float s = g.gate ? tanhf(*g.gate) : 1.0f;
    // Persistent over output tiles: a block keeps its CU and walks virtual block ids vb = blockIdx.x + i*gridDim.x
    // (gridDim.x is a multiple of 8, so vb stays on this block's XCD chunk).  The epilogue stores of tile i drain while
    // the K loop of tile i+1 is already running -- with one block per tile a CU sat idle until its 128 KB of C had been
    // acknowledged (the ablation showed the stores costing 4x their stand-alone time).
    const int ntiles = g.gm * g.gn;
    for (int vb = blockIdx.x; vb < ntiles; vb += gridDim.x) {
    int tile_m, tile_n;
    tile_of_block(g, vb, tile_m, tile_n);
    const int64_t m0 = (int64_t)tile_m * BM, n0 = (int64_t)tile_n * BN;

    // per-thread chunk coordinates (constant over the K loop)
    const bf16_t* pa[A_CH];
    const bf16_t* pb[B_CH];
    int la[A_CH], lb[B_CH], ka[A_CH], kb[B_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        const int c = i * NT + tid, row = c >> 3, phys = c & 7;
        const int slot = (GLDS && !(g.dbg & 64)) ? (phys ^ ((row >> 1) & 7)) : phys;        // logical k-slot this lane fetches (dbg 64: linear, wrong results)
        const int dst = GLDS ? phys : (phys ^ ((row >> 1) & 7));        // physical slot it lands in
        int64_t gr = m0 + row;
        if (gr > g.M - 1) gr = g.M - 1;
        pa[i] = A + gr * g.lda + slot * 8;
        ka[i] = slot * 8;
        la[i] = row * 128 + dst * 16;
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
        const int c = i * NT + tid, row = c >> 3, phys = c & 7;
        const int slot = (GLDS && !(g.dbg & 64)) ? (phys ^ ((row >> 1) & 7)) : phys;
        const int dst = GLDS ? phys : (phys ^ ((row >> 1) & 7));
        int64_t gr = n0 + row;
        if (gr > g.N - 1) gr = g.N - 1;
        pb[i] = B + gr * g.ldb + slot * 8;
        kb[i] = slot * 8;
        lb[i] = BM * 128 + row * 128 + dst * 16;
    }

    f32x16_t acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    // (A per-tile rotation of the K walk -- meant to spread the power-of-two operand strides over L2/HBM channels -- was
    // measured 10 % SLOWER in interleaved A/B rounds: tiles that share an A or B panel hit the same lines at the same time
    // when they walk k in lock step, and that temporal L2 sharing is worth more than the channel spread.  Not used.)
    auto krot = [&](int t) { return t; };

    auto compute = [&](int buf) {
        const char* At = smem + buf * TILE_BYTES;
        const char* Bt = At + BM * 128;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int slot = 2 * ks + (lane >> 5);
            bf16x8_t fa[NI], fb[MI];
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int row = wn * TN + ni * 32 + (lane & 31);
                fa[ni] = *reinterpret_cast<const bf16x8_t*>(Bt + row * 128 + ((slot ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int row = wm * TM + mi * 32 + (lane & 31);
                fb[mi] = *reinterpret_cast<const bf16x8_t*>(At + row * 128 + ((slot ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ni], fb[mi], acc[mi][ni], 0, 0, 0);
        }
    };

    if constexpr (GLDS) {
        // direct global -> LDS (wave-uniform LDS base + lane*16); requires K % 64 == 0 (checked on the host)
        auto stage = [&](int buf, int kt) {
            const int64_t koff = (int64_t)kt * 64;
#pragma unroll
            for (int i = 0; i < A_CH; ++i) {
                const int wbase = buf * TILE_BYTES + (i * NT + wave * 64) * 16;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pa[i] + koff),
                                                 (__attribute__((address_space(3))) void*)(smem + wbase), 16, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < B_CH; ++i) {
                const int wbase = buf * TILE_BYTES + BM * 128 + (i * NT + wave * 64) * 16;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pb[i] + koff),
                                                 (__attribute__((address_space(3))) void*)(smem + wbase), 16, 0, 0);
            }
        };
        stage(0, krot(0));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int nk_run = (g.dbg & 8) ? 0 : nk;
        for (int t = 0; t < nk_run; ++t) {
            const int cur = t & 1;
            if (t + 1 < nk && !(g.dbg & 1)) stage(cur ^ 1, krot(t + 1));
            if (!(g.dbg & 2)) compute(cur);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    } else {
        uint4 ra[A_CH], rb[B_CH];
        auto gload = [&](int kt) {
            const int64_t koff = (int64_t)kt * 64;
#pragma unroll
            for (int i = 0; i < A_CH; ++i)
                ra[i] = (koff + ka[i] < K) ? *reinterpret_cast<const uint4*>(pa[i] + koff) : make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < B_CH; ++i)
                rb[i] = (koff + kb[i] < K) ? *reinterpret_cast<const uint4*>(pb[i] + koff) : make_uint4(0, 0, 0, 0);
        };
        auto lstore = [&](int buf) {
            char* base = smem + buf * TILE_BYTES;
#pragma unroll
            for (int i = 0; i < A_CH; ++i) *reinterpret_cast<uint4*>(base + la[i]) = ra[i];
#pragma unroll
            for (int i = 0; i < B_CH; ++i) *reinterpret_cast<uint4*>(base + lb[i]) = rb[i];
        };
        gload(krot(0));
        lstore(0);
        __syncthreads();
        for (int t = 0; t < nk; ++t) {
            const int cur = t & 1;
            if (t + 1 < nk && !(g.dbg & 1)) gload(krot(t + 1));   // in flight under the MFMAs below
            if (!(g.dbg & 2)) compute(cur);
            if (t + 1 < nk) lstore(cur ^ 1);
            __syncthreads();
        }
    }

    // ---- epilogue: accumulators -> wave-private LDS block -> row-major read-back + fused tail ----
    // (the last K-loop barrier has already retired every read of the operand tiles this aliases)
    float part = 0.f;
    float* blk = reinterpret_cast<float*>(smem) + wave * (32 * EPI_LD);
    if (!(g.dbg & 4)) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) park_block(blk, acc[mi][ni], lane, ni * 32);
        // the stripe is wave-private and a wave's LDS instructions execute in program order: no workgroup barrier needed,
        // the 8 waves run their epilogues independently (wave_barrier only pins the compiler's instruction order)
        __builtin_amdgcn_wave_barrier();
        part += epilogue_stripe<EPI>(g, s, blk, m0 + wm * TM + mi * 32, n0 + wn * TN, lane);
        __builtin_amdgcn_wave_barrier();
    }
    }  // !(dbg & 4)
    if ((g.dbg & 16) && part == 12345.678f) reinterpret_cast<float*>(g.C)[0] = part;
    block_partial<WM * WN, EPI>(g, part, reinterpret_cast<float*>(smem), vb);
    __syncthreads();  // every wave is done with the LDS it parked in before the next tile's staging overwrites it
    }  // persistent tile loop
}

// ------------------------------------------------------------------------------------------------------------
// exact-f32 MFMA kernel (parity mode): 64x64x32 tile, 4 waves (2x2), one 32x32 accumulator block per wave
// ------------------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmArgs g) {
    constexpr int BM = 64, BN = 64, BK = 32, LD = BK + 1;
    __shared__ __attribute__((aligned(16))) float sm[2 * 32 * EPI_LD > (BM + BN) * LD ? 2 * 32 * EPI_LD : (BM + BN) * LD];
    float* As = sm;
    float* Bs = sm + BM * LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int tile_m, tile_n;
    tile_of_block(g, (int)blockIdx.x, tile_m, tile_n);
    const int64_t m0 = (int64_t)tile_m * BM, n0 = (int64_t)tile_n * BN;
    const float* __restrict__ A = (const float*)g.A;
    const float* __restrict__ B = (const float*)g.B;
    const int64_t K = g.K;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int64_t k0 = 0; k0 < K; k0 += BK) {
        // 64 rows x 32 floats = 512 float4 chunks per operand; 2 per thread
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = i * 256 + tid, row = c >> 3, q = c & 7;
            const int64_t k = k0 + q * 4;
            int64_t ga = m0 + row; if (ga > g.M - 1) ga = g.M - 1;
            int64_t gb = n0 + row; if (gb > g.N - 1) gb = g.N - 1;
            float4 va = make_float4(0, 0, 0, 0), vb = make_float4(0, 0, 0, 0);
            if (k < K) {  // K % 4 == 0 is enforced on the host
                va = *reinterpret_cast<const float4*>(A + ga * g.lda + k);
                vb = *reinterpret_cast<const float4*>(B + gb * g.ldb + k);
            }
            float* da = As + row * LD + q * 4;
            float* db = Bs + row * LD + q * 4;
            da[0] = va.x; da[1] = va.y; da[2] = va.z; da[3] = va.w;
            db[0] = vb.x; db[1] = vb.y; db[2] = vb.z; db[3] = vb.w;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float a = Bs[(wn * 32 + (lane & 31)) * LD + kk + (lane >> 5)];  // a-operand = B rows (n)
            const float b = As[(wm * 32 + (lane & 31)) * LD + kk + (lane >> 5)];  // b-operand = A rows (m)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const float s = g.gate ? tanhf(*g.gate) : 1.0f;
    // the two waves of a row pair (wn = 0, 1) share one 64-column stripe
    float* blk = sm + wm * (32 * EPI_LD);
    park_block(blk, acc, lane, wn * 32);
    __syncthreads();
    float part = 0.f;
    {
        // 32 rows x 64 columns handled by the pair's 128 lanes: lane id within the pair = wn*64 + lane
        const int pl = wn * 64 + lane;
#pragma unroll 1
        for (int it = 0; it < 4; ++it) {
            const int r = (pl >> 4) + 8 * it;
            const int c = (pl & 15) * 4;
            const int64_t m = m0 + wm * 32 + r, n = n0 + c;
            if (m < g.M && n < g.N) {
                const float4 t = *reinterpret_cast<const float4*>(blk + r * EPI_LD + c);
                float v[4] = {t.x, t.y, t.z, t.w};
                part += epilogue4<EPI>(g, s, m, n, v);
            }
        }
    }
    block_partial<4, EPI>(g, part, sm, (int)blockIdx.x);
}

// variants 1-3.  Persistent grid: one resident wave of blocks (two per CU of the 128^2 tile, one of the 256^2 tile), or one per tile if fewer
template <int BM, int BN, int WM, int WN, bool GLDS, int EPI>
int launch_tiled(unsigned tiles, unsigned cus, hipStream_t st, const GemmArgs& g) {
    const unsigned pg = cus * ((BM == 256) ? 1u : 2u);
    return launch_lds<gemm_bf16_kernel<BM, BN, WM, WN, GLDS, EPI>>(tiles < pg ? tiles : pg, WM * WN * 64, 2 * (BM + BN) * 128, st, g);
}

}  // namespace

int gemm_launch_tiled(int kind, int bm, bool glds, unsigned tiles, unsigned cus, hipStream_t st, const GemmArgs& g) {
    return with_epi(kind, [&](auto epi) {
        constexpr int EPI = decltype(epi)::value;
        if (bm == 128) return launch_tiled<128, 128, 2, 2, false, EPI>(tiles, cus, st, g);
        if (!glds) return launch_tiled<256, 256, 2, 4, false, EPI>(tiles, cus, st, g);
        return launch_tiled<256, 256, 2, 4, true, EPI>(tiles, cus, st, g);
    });
}

int gemm_launch_f32(int kind, unsigned tiles, hipStream_t st, const GemmArgs& g) {
    return with_epi(kind, [&](auto epi) -> int {
        hipLaunchKernelGGL(gemm_f32_kernel<decltype(epi)::value>, dim3(tiles), dim3(256), 0, st, g);
        return OTTER_OK;
    });
}
