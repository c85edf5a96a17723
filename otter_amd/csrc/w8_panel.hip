// w8_panel.hip -- otter_gemm_w8_panel: the int8 weight-only product for one-token steps of 65 to 256 rows.
// A piece of w8.hip (included inside its anonymous namespace): W8Args, cvt8, w8_epilogue, the reduce kernel and the host checks are shared.
//
// Panel decomposition.  At 256 rows the rows kernel's layout (one 16-row weight tile per wave) reads 4 x 128 KB of x from LDS for every
// 16 KB of weights: the LDS reads, not the weight stream, would set the time.  Here a wave owns TWO 16-row weight tiles (32 output columns,
// 128 per workgroup) and every x fragment it reads from LDS feeds the MFMAs of both, which halves the LDS bytes and the x re-reads per
// weight byte.  K advances in chunks of 128 (two 64-wide steps).  Per chunk a wave loads its 2 x 2 x 16 weight bytes per lane straight
// into VGPRs (the weight is streamed once and shared with nobody); the workgroup loads the chunk of x, rows 0 .. 16 MB - 1 (rows >= M are
// zero-filled, not read), as full 256-byte row pieces and writes them to one of two LDS images [16 MB rows][16 slots of 16 B], slot c of
// row r stored at c ^ (r & 15): a row is exactly one 256-byte bank row, and the 16 rows that one lane group of a 16-byte LDS read covers
// fall on 16 different slots of it.  One barrier per chunk, the loads of chunk c + 1 issued before chunk c is consumed, as in the rows
// kernel.  Each converted weight fragment (cvt8, once per weight element) feeds the MFMAs of all MB column blocks.  MB is the smallest
// instantiated block count >= ceil(M / 16); the blocks beyond M hold zeros and are never stored.
// Split-K ACROSS workgroups only, the split count and every K range functions of (N, K) alone: every output element is one MFMA chain per
// K range in ascending K and the ranges are added in order by gemv_w8_reduce_kernel, so row m of y has the same bits whatever M is,
// whatever the other rows hold (NaN included: an x row is one column of the MFMA's B operand) and wherever it sits in the batch.  The
// split rule is this kernel's own (one workgroup per CU at most): bit-equality with the rows kernel is not promised.

constexpr int PANEL_MAX_M = 256;
constexpr int PANEL_TILES = 2;                                  // 16-row weight tiles per wave
constexpr int PANEL_BN = 16 * PANEL_TILES * WAVES;              // output columns (weight rows) per workgroup: 128
constexpr int PANEL_STEPS = 2;                                  // 64-wide K steps per chunk
constexpr int PANEL_KC = PANEL_STEPS * KSTEP;                   // K elements per chunk: 128
constexpr int PANEL_SLOTS = PANEL_KC / 8;                       // 16-byte slots per x row of a chunk (16: one 256-byte bank row)
constexpr int PANEL_MAX_SPLIT = 8;                              // OTTER_GEMM_W8_PANEL_MAX_SPLIT of the header restates the rule below
constexpr int64_t PANEL_WG_TARGET = 256;                        // K is split only while the grid stays within one workgroup per CU of a 256-CU part
constexpr int64_t PANEL_MIN_K_PER_WG = 256;                     // ... and each workgroup keeps two chunks

template <int MB, bool GATED>
__global__ __launch_bounds__(NT) void gemm_w8_panel_kernel(W8Args a) {         // a.T: chunks in all, a.q: chunks per K range
    __shared__ uint4 xs[2][16 * MB * PANEL_SLOTS];                             // 2 x 4 MB KB (MB = 16: 2 x 64 KB, one workgroup per CU)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * PANEL_BN + 16 * PANEL_TILES * wv;
    const int s = blockIdx.y;
    const int c0 = s * a.q, c1 = min(c0 + a.q, a.T);

    // Every load of the K loop is unconditional: a lane that has nothing to fetch (a weight row >= N, an x row >= M, K elements >= K) reads
    // a valid address instead (row 0, the last 16 / 8 elements of the row) and the value is replaced by zero.  With the loads under
    // conditions the compiler turns each into a branch and the loop into a chain of waits.
    bool row_ok[PANEL_TILES];
    const int8_t* wp[PANEL_TILES];
#pragma unroll
    for (int t = 0; t < PANEL_TILES; ++t) {
        const int64_t n = n0 + 16 * t + r16;
        row_ok[t] = n < a.N;
        wp[t] = a.w + (row_ok[t] ? n : 0) * a.ldw;
    }
    auto load_w = [&](uint4 (&w)[PANEL_STEPS][PANEL_TILES], int c) {
#pragma unroll
        for (int u = 0; u < PANEL_STEPS; ++u) {
            const int k = c * PANEL_KC + u * KSTEP + 16 * g;                   // K % 16 == 0: a lane's 16 elements are all inside or all outside
#pragma unroll
            for (int t = 0; t < PANEL_TILES; ++t) w[u][t] = *reinterpret_cast<const uint4*>(wp[t] + min(k, a.K - 16));
        }
    };
    auto mask_w = [&](uint4 (&w)[PANEL_STEPS][PANEL_TILES], int c) {           // (after the wait for the loads, in front of cvt8)
#pragma unroll
        for (int u = 0; u < PANEL_STEPS; ++u)
#pragma unroll
            for (int t = 0; t < PANEL_TILES; ++t)
                if (!(row_ok[t] && c * PANEL_KC + u * KSTEP + 16 * g < a.K)) w[u][t] = make_uint4(0, 0, 0, 0);
    };
    // x chunk: 16 MB rows x 16 slots, MB slots per thread, staged through registers in two halves (h = 0, 1) of XH slots; 16 consecutive
    // threads read one 256-byte row piece.  Rows >= M are never read: their lanes fetch row 0 and store zeros.
    constexpr int XH = (MB + 1) / 2, XROWS = NT / PANEL_SLOTS;                 // (a trip of the workgroup covers XROWS = 16 rows)
    const int xrow0 = tid / PANEL_SLOTS, xcc = tid % PANEL_SLOTS;
    const bf16_t* xp = a.x + (int64_t)xrow0 * a.ldx;
    auto load_x = [&](uint4 (&xr)[XH], int c, int h) {
        const int k = c * PANEL_KC + 8 * xcc;                                  // (K % 8 == 0: the 8 elements are all inside or all outside)
#pragma unroll
        for (int j = 0; j < XH; ++j) {
            if (h * XH + j >= MB) continue;
            const bool row_in = (h * XH + j) * XROWS + xrow0 < a.M;
            const bf16_t* p = row_in ? xp + (int64_t)((h * XH + j) * XROWS) * a.ldx : a.x;
            xr[j] = *reinterpret_cast<const uint4*>(p + min(k, a.K - 8));
        }
    };
    auto store_x = [&](int buf, const uint4 (&xr)[XH], int c, int h) {
        const bool k_in = c * PANEL_KC + 8 * xcc < a.K;
#pragma unroll
        for (int j = 0; j < XH; ++j) {
            if (h * XH + j >= MB) continue;
            const int row = (h * XH + j) * XROWS + xrow0;
            uint4 v = xr[j];
            if (!(k_in && row < a.M)) v = make_uint4(0, 0, 0, 0);
            xs[buf][row * PANEL_SLOTS + (xcc ^ (row & 15))] = v;
        }
    };

    // a tile is [weight row, x row] as in the rows kernel: acc[t][mb][i] of a lane = weight row 16 t + 4 (lane >> 4) + i of the wave's 32,
    // x row 16 mb + (lane & 15)
    w8_f32x4_t acc[PANEL_TILES][MB];
#pragma unroll
    for (int t = 0; t < PANEL_TILES; ++t)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[t][mb] = w8_f32x4_t{0.f, 0.f, 0.f, 0.f};

    // K step u (0, 1) of a chunk.  The x fragments of column block mb + 1 are requested from LDS before the MFMAs of block mb are issued
    // (two 16-byte reads per four MFMAs); the scheduling groups keep the compiler from moving the reads back in front of their use.
    auto consume = [&](const uint4 (&w)[PANEL_STEPS][PANEL_TILES], int buf, int u) {
        w8_bf16x8_t wa[PANEL_TILES], wb[PANEL_TILES];
#pragma unroll
        for (int t = 0; t < PANEL_TILES; ++t) {
            wa[t] = cvt8(w[u][t].x, w[u][t].y);
            wb[t] = cvt8(w[u][t].z, w[u][t].w);
        }
        const uint4* xcol = &xs[buf][r16 * PANEL_SLOTS];
        const int sa = (8 * u + 2 * g) ^ r16, sb = (8 * u + 2 * g + 1) ^ r16;
        uint4 xa[2], xb[2];
        xa[0] = xcol[sa];
        xb[0] = xcol[sb];
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            if (mb + 1 < MB) {
                xa[(mb + 1) & 1] = xcol[16 * (mb + 1) * PANEL_SLOTS + sa];
                xb[(mb + 1) & 1] = xcol[16 * (mb + 1) * PANEL_SLOTS + sb];
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
            const w8_bf16x8_t fa = __builtin_bit_cast(w8_bf16x8_t, xa[mb & 1]), fb = __builtin_bit_cast(w8_bf16x8_t, xb[mb & 1]);
#pragma unroll
            for (int t = 0; t < PANEL_TILES; ++t) {                            // each x fragment read from LDS feeds both weight tiles
                acc[t][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[t], fa, acc[t][mb], 0, 0, 0);
                acc[t][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[t], fb, acc[t][mb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * PANEL_TILES, 0);
        }
    };

    // chunk c + 1 is requested while chunk c is consumed: its weights at the start, its x in two halves, each written to the other LDS
    // image one K step after it was requested.  One barrier per chunk; the last chunk of the range requests nothing.
    uint4 wc[PANEL_STEPS][PANEL_TILES], wn[PANEL_STEPS][PANEL_TILES], xr[XH];
    if (c0 < c1) {                                                              // (uniform over the workgroup, as everything below)
        load_w(wc, c0);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            load_x(xr, c0, h);
            store_x(0, xr, c0, h);
        }
        mask_w(wc, c0);
        __syncthreads();
        int buf = 0;
        for (int c = c0; c + 1 < c1; ++c, buf ^= 1) {
            // (the memory counter retires loads in order: the first half of x goes out in front of the weights, so that the wait before
            // its LDS stores leaves the weights in flight.  The scheduling barriers keep the requests where they are written.)
            load_x(xr, c + 1, 0);
            load_w(wn, c + 1);
            __builtin_amdgcn_sched_barrier(0);
            consume(wc, buf, 0);
            __builtin_amdgcn_sched_barrier(0);
            store_x(buf ^ 1, xr, c + 1, 0);
            load_x(xr, c + 1, 1);
            __builtin_amdgcn_sched_barrier(0);
            consume(wc, buf, 1);
            __builtin_amdgcn_sched_barrier(0);
            store_x(buf ^ 1, xr, c + 1, 1);
            mask_w(wn, c + 1);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < PANEL_STEPS; ++u)
#pragma unroll
                for (int t = 0; t < PANEL_TILES; ++t) wc[u][t] = wn[u][t];
        }
        consume(wc, buf, 0);
        consume(wc, buf, 1);
    }

    const float sg = w8_gate<GATED>(a);
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int m = 16 * mb + r16;
#pragma unroll
        for (int t = 0; t < PANEL_TILES; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t n = n0 + 16 * t + 4 * g + i;
                if (m >= a.M || n >= a.N) continue;
                if (a.S == 1) st_from_f32(a.y, (int64_t)m * a.ldy + n, a.y_dtype, w8_epilogue<GATED>(acc[t][mb][i], sg, m, n, a));
                else a.part[((int64_t)s * a.M + m) * a.N + n] = acc[t][mb][i];
            }
    }
}

template <int MB>
void launch_panel_mb(bool gated, dim3 grid, hipStream_t st, const W8Args& a) {
    if (gated) hipLaunchKernelGGL((gemm_w8_panel_kernel<MB, true>), grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((gemm_w8_panel_kernel<MB, false>), grid, dim3(NT), 0, st, a);
}

// the instantiated block counts: 4 (up to 64 rows), 5 (72 = 24 sentences x 3 beams), 6, 8, 12, 16.  A larger MB than ceil(M / 16) only adds
// zero blocks: it changes no bit of any row.
void launch_panel(int mb, bool gated, dim3 grid, hipStream_t st, const W8Args& a) {
    if (mb <= 4) launch_panel_mb<4>(gated, grid, st, a);
    else if (mb == 5) launch_panel_mb<5>(gated, grid, st, a);
    else if (mb == 6) launch_panel_mb<6>(gated, grid, st, a);
    else if (mb <= 8) launch_panel_mb<8>(gated, grid, st, a);
    else if (mb <= 12) launch_panel_mb<12>(gated, grid, st, a);
    else launch_panel_mb<16>(gated, grid, st, a);
}

int gemm_w8_panel_run(const W8Call& c, const char* what, const char* what_reduce) {
    const int rc = w8_check(c, what, PANEL_MAX_M);
    if (rc != OTTER_OK) return rc;
    const int64_t N = c.N, K = c.K;
    // the split is a function of (N, K) only -- never of M -- so that a row's summation order does not depend on what it is batched with
    const int64_t base = cdiv64(N, PANEL_BN);
    int S = 1;
    while (base * 2 * S <= PANEL_WG_TARGET && S < PANEL_MAX_SPLIT && K / (2 * S) >= PANEL_MIN_K_PER_WG) S *= 2;
    OTTER_REQUIRE(base <= 0x7fffffff && S <= OTTER_GEMM_W8_PANEL_MAX_SPLIT(N), "%s: internal grid", what);

    W8Args a = w8_args(c);
    a.S = S;
    a.T = (int)cdiv64(K, PANEL_KC);
    a.q = (int)cdiv64(a.T, S);
    hipStream_t st = (hipStream_t)c.stream;
    launch_panel((int)cdiv64(c.M, 16), c.gated, dim3((unsigned)base, (unsigned)S), st, a);
    OTTER_CHECK_LAUNCH(what);
    return S > 1 ? w8_reduce(a, st, what_reduce) : OTTER_OK;
}
