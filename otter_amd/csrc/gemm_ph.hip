// gemm_ph.hip -- the phased 8-wave kernel of the GEMM (gemm_bf16_ph_kernel, variant 13; the map of the variants is in gemm.hip) and its launch.
#include "gemm_tail.h"
#include "gemm_launch.h"

namespace {

// ------------------------------------------------------------------------------------------------------------
// bf16 phased kernel (variant 13, the fallback for K % 128 != 0): the 256x256x64 / 8-wave / LDS-DMA tile of gemm_bf16_kernel
// with the K-tile split into four quadrant phases and the two wave rows STAGGERED by one barrier:
//   wave (wr, wc) owns rows wr*128.. x cols wc*64..; phase (mh, nh) = its 64x32 quadrant x the whole BK = 8 MFMAs.
//   per phase:  LOAD part (ds_read the quadrant's new fragments + two DMA pieces of the next K-tile)
//               | s_barrier | lgkmcnt(0) | setprio(1) 8x MFMA setprio(0) | s_barrier
//   waves 4-7 (wr = 1) execute one extra s_barrier up front, so at every moment one wave row sits in its MFMA cluster
//   while the other sits in its LOAD part.  A SIMD hosts wave s (wr 0) and wave s+4 (wr 1): its matrix pipe is fed by
//   the two alternately and LDS reads / DMA issue of one always run under the MFMAs of the other.
// Hazards (barrier instance k of row 0 pairs with instance k+1 of row 1):
//   RAW  DMA(t+1) -> ds_read: counted vmcnt in the LOAD part of the phase before the one that reads the half-tile, i.e.
//        before a barrier that both its own row and (one instance later) the other row pass before their first read.
//   WAR  ds_read(t-1) -> DMA(t+1) into the same buffer: phase 3 reads nothing new (both nh fragments of B stay in
//        registers) and every phase's reads are retired by lgkmcnt(0) before its MFMAs, so a half-tile is refilled only
//        after its last read has completed, on both rows.
// (The six other schedules this kernel once carried, with and without buffer addressing -- variants 6, 7, 9-11, 14-16 -- are retired: DESIGN_HISTORY.md.)
// ------------------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512) void gemm_bf16_ph_kernel(GemmArgs g) {
    constexpr int BM = 256, BN = 256, NT = 512;
    constexpr int TILE_BYTES = (BM + BN) * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const bf16_t* __restrict__ A = (const bf16_t*)g.A;
    const bf16_t* __restrict__ B = (const bf16_t*)g.B;
    const int nk = (int)(g.K >> 6);
    const float sgate = g.gate ? tanhf(*g.gate) : 1.0f;
    // buffer addressing for the DMA (SGPR resource descriptor + 32-bit per-lane offset + scalar K offset): no per-piece
    // 64-bit VALU address arithmetic, and the hardware range check clamps reads past the end of the operand (the host
    // guarantees the operands span < 4 GB)
    const __amdgpu_buffer_rsrc_t rsrc_a =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(A), 0, (int)(uint32_t)((g.M - 1) * g.lda * 2 + g.K * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_b =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(B), 0, (int)(uint32_t)((g.N - 1) * g.ldb * 2 + g.K * 2), 0x00020000);
    const int ntiles = g.gm * g.gn;
#define RAW_BARRIER()                       \
    do {                                    \
        __builtin_amdgcn_sched_barrier(0);  \
        __builtin_amdgcn_s_barrier();       \
        __builtin_amdgcn_sched_barrier(0);  \
    } while (0)
    for (int vb = blockIdx.x; vb < ntiles; vb += gridDim.x) {
        int tile_m, tile_n;
        tile_of_block(g, vb, tile_m, tile_n);
        const int64_t m0 = (int64_t)tile_m * BM, n0 = (int64_t)tile_n * BN;
        // The K-tile is fed as four half-tiles of 128 rows -- A_h(mh) = rows {wr*128 + mh*64 + 0..63 : wr},
        // B_h(nh) = rows {wc*64 + nh*32 + 0..31 : wc} -- i.e. exactly the rows ONE quadrant phase reads.  Two DMA pieces per
        // thread per half-tile; they are issued one or two per phase and retired with COUNTED vmcnt (never drained in
        // steady state): A_h0,B_h0(t+1) in phase 0, B_h1(t+1) in phase 1, A_h1(t+1) in phase 2 -> every half-tile has three
        // phases to land and the wait in phase q-1 for the rows phase q reads leaves the 2-3 newest half-tiles in flight.
        uint32_t oah[2][2], obh[2][2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = i * NT + tid, rl = c >> 3, phys = c & 7;
                const int ra = (rl >> 6) * 128 + h * 64 + (rl & 63);
                const int rb = (rl >> 5) * 64 + h * 32 + (rl & 31);
                int64_t ga = m0 + ra; if (ga > g.M - 1) ga = g.M - 1;
                int64_t gb = n0 + rb; if (gb > g.N - 1) gb = g.N - 1;
                oah[h][i] = (uint32_t)((ga * g.lda + (phys ^ ((ra >> 1) & 7)) * 8) * 2);
                obh[h][i] = (uint32_t)((gb * g.ldb + (phys ^ ((rb >> 1) & 7)) * 8) * 2);
            }
        auto stage_ah = [&](int buf, int kt, int h) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int wbase = buf * TILE_BYTES + (i * 128 + h * 64 + wave * 8) * 128;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, (__attribute__((address_space(3))) void*)(smem + wbase), 16,
                                                         (int)oah[h][i], kt * 128, 0, 0);
            }
        };
        auto stage_bh = [&](int buf, int kt, int h) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int wbase = buf * TILE_BYTES + BM * 128 + ((2 * i + (wave >> 2)) * 64 + h * 32 + (wave & 3) * 8) * 128;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (__attribute__((address_space(3))) void*)(smem + wbase), 16,
                                                         (int)obh[h][i], kt * 128, 0, 0);
            }
        };
        // LDS side: the swizzle term (row>>1)&7 only depends on lane&31 (every row offset used below is a multiple of 32),
        // so ONE base per k-step and operand (8 VGPRs) + compile-time immediates reach every fragment of the wave.
        const int swz = ((lane & 31) >> 1) & 7;
        int la[4], lb[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int slot = (2 * ks + (lane >> 5)) ^ swz;
            la[ks] = (wr * 128 + (lane & 31)) * 128 + (slot << 4);
            lb[ks] = BM * 128 + (wc * 64 + (lane & 31)) * 128 + (slot << 4);
        }
        auto ld_a = [&](int buf, int mh, bf16x8_t (&fa)[2][4]) {
            const char* base = smem + buf * TILE_BYTES + mh * (64 * 128);
#pragma unroll
            for (int mi2 = 0; mi2 < 2; ++mi2)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    fa[mi2][ks] = *reinterpret_cast<const bf16x8_t*>(base + la[ks] + mi2 * (32 * 128));
        };
        auto ld_b = [&](int buf, int nh, bf16x8_t (&fb)[4]) {
            const char* base = smem + buf * TILE_BYTES + nh * (32 * 128);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) fb[ks] = *reinterpret_cast<const bf16x8_t*>(base + lb[ks]);
        };
        f32x16_t acc[4][2];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
        // one quadrant: 8 MFMAs, operands swapped (a = B rows, b = A rows)
#define QUAD(MH, NH, FA, FB)                                                                                            \
    do {                                                                                                                \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                              \
        __builtin_amdgcn_s_setprio(1);                                                                                  \
        _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                                                              \
            acc[(MH)*2 + 0][NH] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FB[ks], FA[0][ks], acc[(MH)*2 + 0][NH], 0, 0, 0); \
            acc[(MH)*2 + 1][NH] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(FB[ks], FA[1][ks], acc[(MH)*2 + 1][NH], 0, 0, 0); \
        }                                                                                                               \
        __builtin_amdgcn_s_setprio(0);                                                                                  \
    } while (0)

        stage_ah(0, 0, 0); stage_bh(0, 0, 0); stage_bh(0, 0, 1); stage_ah(0, 0, 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (wr == 1) RAW_BARRIER();  // stagger the second wave row by one barrier
        bf16x8_t fa[2][4], fb[4], fb1[4];
        // LOAD-part-only balanced schedule: fb/fb1 resident (phase 3 reads nothing), two DMA pieces per phase:
        //   phase 0: A_h0(t+1), 1: B_h0(t+1), 2: B_h1(t+1), 3: A_h1(t+1); reads/pieces = 12/2, 4/2, 8/2, 0/2.
        for (int t = 0; t < nk; ++t) {
            const int cur = t & 1;
            const bool more = t + 1 < nk;
            ld_a(cur, 0, fa);
            ld_b(cur, 0, fb);
            __builtin_amdgcn_sched_barrier(0);
            if (more) stage_ah(cur ^ 1, t + 1, 0);
            if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            RAW_BARRIER();
            QUAD(0, 0, fa, fb);
            RAW_BARRIER();
            ld_b(cur, 1, fb1);
            __builtin_amdgcn_sched_barrier(0);
            if (more) stage_bh(cur ^ 1, t + 1, 0);
            if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            RAW_BARRIER();
            QUAD(0, 1, fa, fb1);
            RAW_BARRIER();
            ld_a(cur, 1, fa);
            __builtin_amdgcn_sched_barrier(0);
            if (more) stage_bh(cur ^ 1, t + 1, 1);
            RAW_BARRIER();
            QUAD(1, 1, fa, fb1);
            RAW_BARRIER();
            if (more) { stage_ah(cur ^ 1, t + 1, 1); asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }
            RAW_BARRIER();
            QUAD(1, 0, fa, fb);
            RAW_BARRIER();
        }
        if (wr == 0) RAW_BARRIER();  // undo the stagger
        __syncthreads();
#undef QUAD

        // ---- epilogue (same as the 8-wave kernel: 64-column wave-private stripes) ----
        float part = 0.f;
        float* blk = reinterpret_cast<float*>(smem) + wave * (32 * EPI_LD);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) park_block(blk, acc[mi][ni], lane, ni * 32);
            __builtin_amdgcn_wave_barrier();
            part += epilogue_stripe<EPI>(g, sgate, blk, m0 + wr * 128 + mi * 32, n0 + wc * 64, lane);
            __builtin_amdgcn_wave_barrier();
        }
        block_partial<8, EPI>(g, part, reinterpret_cast<float*>(smem), vb);
        __syncthreads();
    }
#undef RAW_BARRIER
}

}  // namespace

int gemm_launch_ph(int kind, unsigned tiles, unsigned cus, hipStream_t st, const GemmArgs& g) {
    // persistent: one workgroup per CU left to the GEMMs (otter_gemm_set_cu_budget), or one per tile if fewer
    const unsigned pg = tiles < cus ? tiles : cus;
    return with_epi(kind, [&](auto epi) { return launch_lds<gemm_bf16_ph_kernel<decltype(epi)::value>>(pg, 512, 2 * (256 + 256) * 128, st, g); });
}
