// gemm.hip -- C[M,N] = epilogue(A[M,K] . B[N,K]^T) on gfx950 MFMA: the host half.  Argument checks, the choice of a kernel (pick_cfg), the
// process-wide switches, the profiling hook and the C entry points; plus reduce_partials_kernel.  The kernels live in files of their own, each
// with its launch function (gemm_launch.h); what they share on the device is gemm_tail.h, what the host hands them is gemm_args.h.
//
// Variant numbers (otter_gemm_set_variant; 0 = auto = pick_cfg) -> kernel -> when pick_cfg chooses it:
//   1   gemm_bf16_kernel<128,128,2,2,false>  fewer than 192 tiles of 256x256 and the ring does not apply; fallback of 25 / 30      gemm_tiled.hip
//   2   gemm_bf16_kernel<256,256,2,4,false>  never by itself: fallback of 3 / 13 / 26 for K % 64 != 0                               gemm_tiled.hip
//   3   gemm_bf16_kernel<256,256,2,4,true>   never by itself: fallback of 13 / 26 for an operand of >= 4 GB (K % 64 == 0)           gemm_tiled.hip
//   13  gemm_bf16_ph_kernel                  >= 192 tiles of 256x256 and K % 128 != 0 (K % 64 == 0)                                  gemm_ph.hip
//   25  gemm_bf16_s4_kernel                  fewer than 192 such tiles, K % 256 == 0, K >= 512, at most 512 tiles of 128x128         gemm_s4.hip
//   30  gemm_bf16_s4h_kernel                 as 25 with at most 160 tiles of 128x128 and no gate partials (gemm_impl)                gemm_s4.hip
//   26  gemm_bf16_t4_kernel<EPI,TA,TB,XT>    >= 192 tiles of 256x256 and K % 128 == 0: the default of the FFN shapes.  XT (cross-tile ring) for
//                                            K-contiguous operands with K >= 256; TA / TB for K-major operands (otter_gemm)          gemm_t4.hip
//   fp32 operands: gemm_f32_kernel (gemm_tiled.hip), always.  Numbers 4-12, 14-23 and 27-29 are retired (DESIGN_HISTORY.md).
//   (gemm_t4.hip and gemm_s4.hip are compiled as one translation unit, gemm_t4_s4.hip, which says why.)
#include "gemm_launch.h"

namespace {

__global__ void reduce_partials_kernel(const float* __restrict__ partial, int64_t n, const float* __restrict__ gate,
                                       float* __restrict__ out, int accumulate) {
    __shared__ float red[4];
    float t = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) t += partial[i];
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = red[0] + red[1] + red[2] + red[3];
        if (gate) {
            const float th = tanhf(*gate);
            s *= (1.0f - th * th);
        }
        out[0] = accumulate ? out[0] + s : s;
    }
}

// ---- configuration choice (shared by the launcher and otter_gemm_num_partials) ----
int g_variant = 0;
int g_debug = 0;
int g_order = 0;
int g_narrow_epilogue = 0;  // A/B hook (otter_gemm_set_debug bit 256): force the 4-wide fused tail
// Cross-tile form of variant 26 (round 6): otter_gemm_set_debug bits 14-15 = 0 default / 1 off / 2 on, bits 16-22 = K order + start phase (GemmArgs::korder), bit 23 = use them
int g_xt_force = 0;
int g_korder_force = -1;
bool t4_xt_on() { return g_xt_force ? g_xt_force == 2 : true; }
// default 3: K-tiles of a tile walked from a quarter given by its N panel: -1..-4 % on cold operands (profiles/r06_xt_ab*.txt);
// mode 3 and not the XCD modes: a row of C keeps one summation order wherever it sits in the batch (DP invariant)
int t4_korder() { return g_korder_force >= 0 ? g_korder_force : 3; }
// The numbers are public (otter_gemm_set_variant; bench.py and the tests pass them).  4-12, 14-23 and 27-29 were the kernel generations and
// schedule placements that led to 13 and 26: retired, DESIGN_HISTORY.md names the last commit that holds them.
enum Cfg { CFG_128 = 1, CFG_256 = 2, CFG_256_GLDS = 3, CFG_PHLB = 13, CFG_S4 = 25, CFG_T4 = 26, CFG_S4H = 30, CFG_F32 = 100 };

// wide: an operand spans >= 4 GB, so the kernels that address it with 32-bit byte offsets are out
int pick_cfg(int64_t M, int64_t N, int64_t K, int ab_dtype, bool wide = false) {
    if (ab_dtype == OTTER_F32) return CFG_F32;
    int v = g_variant;
    if (v == 0) {
        // interleaved A/B medians on MI355X (tools/gemm_ab.py): the one-wave-per-SIMD kernel with the register-resident
        // K-tile (variant 26) beats the balanced 8-wave phased schedule (variant 13) on all three FFN shapes; it needs K % 128 == 0,
        // else 13 stays
        if (cdiv64(M, 256) * cdiv64(N, 256) >= 192) v = (K % 128 == 0 && !wide) ? CFG_T4 : CFG_PHLB;
        else if (K % 256 == 0 && K >= 512 && !wide && cdiv64(M, 128) * cdiv64(N, 128) <= 512) v = CFG_S4;   // few tiles, long reduction: the ring
        else v = CFG_128;
    }
    if (v == CFG_PHLB && (K % 64 != 0 || wide)) v = (K % 64 == 0) ? CFG_256_GLDS : CFG_256;
    if (v == CFG_T4 && (K % 128 != 0 || wide)) v = (K % 64 == 0 && !wide) ? CFG_PHLB : ((K % 64 == 0) ? CFG_256_GLDS : CFG_256);
    if ((v == CFG_S4 || v == CFG_S4H) && (K % 256 != 0 || wide)) v = CFG_128;
    if (v == CFG_256_GLDS && (K % 64 != 0)) v = CFG_256;
    return v;
}
void cfg_tiles(int cfg, int& bm, int& bn) {
    if (cfg == CFG_F32) { bm = 64; bn = 64; }
    else if (cfg == CFG_128 || cfg == CFG_S4) { bm = 128; bn = 128; }
    else if (cfg == CFG_S4H) { bm = 64; bn = 128; }
    else { bm = 256; bn = 256; }
}

// Persistent grids: one workgroup per CU of THIS device (hipDeviceProp_t::multiProcessorCount, read once per process -- one
// process drives one GPU), capped by otter_gemm_set_cu_budget: with a DP reducer live the GEMMs leave a few CUs to RCCL's
// kernels so the all-reduce of bucket i runs beside the dgrad GEMMs of the layers below instead of waiting for the gaps
// between launches (every persistent GEMM otherwise pins all CUs with one 512-register wave per SIMD).
int g_cu_budget = 0;   // 0 = all
int g_persistent = 1;  // 0: the large-grid kernel (variant 26) runs one workgroup per tile (otter_gemm_set_persistent)
unsigned device_cus() {
    static unsigned n = 0;
    if (n == 0) {
        int dev = 0;
        hipDeviceProp_t p;
        n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0)
                ? (unsigned)p.multiProcessorCount : 256u;
    }
    return n;
}
unsigned persistent_cus() {
    const unsigned n = device_cus();
    return (g_cu_budget > 0 && (unsigned)g_cu_budget < n) ? (unsigned)g_cu_budget : n;
}

// ---- profiling hook (bench.py roofline object) ----
struct Prof {
    bool armed = false;
    int64_t M = 0, N = 0, K = 0;
    int max_events = 0, n = 0;
    hipEvent_t* start = nullptr;
    hipEvent_t* stop = nullptr;
    unsigned char* kmajor = nullptr;   // per event: the launch had a K-major operand
} g_prof;

// the launch functions of the kernel files (gemm_launch.h), by configuration
int launch_cfg(int cfg, unsigned tiles, hipStream_t st, const GemmArgs& g) {
    const unsigned cus = persistent_cus();
    if (cfg == CFG_F32) return gemm_launch_f32(g.kind, tiles, st, g);
    if (cfg == CFG_128) return gemm_launch_tiled(g.kind, 128, false, tiles, cus, st, g);
    if (cfg == CFG_256) return gemm_launch_tiled(g.kind, 256, false, tiles, cus, st, g);
    if (cfg == CFG_PHLB) return gemm_launch_ph(g.kind, tiles, cus, st, g);
    if (cfg == CFG_T4) {
        // one workgroup per tile: asked for by this call (otter_epilogue_args::grid_mode = 2), by the process default
        // (otter_gemm_set_persistent(0)) when the call leaves it open, or by debug bit 13
        const bool per_tile = g.grid_mode == OTTER_GRID_PER_TILE || (g.grid_mode == OTTER_GRID_DEFAULT && !g_persistent);
        return gemm_launch_t4(g.kind, tiles, cus, (g_order & 0x10) || per_tile, t4_xt_on(), st, g);
    }
    if (cfg == CFG_S4H) return gemm_launch_s4h(g.kind, tiles, cus, st, g);
    if (cfg == CFG_S4) return gemm_launch_s4(g.kind, tiles, cus, st, g);
    return gemm_launch_tiled(g.kind, 256, true, tiles, cus, st, g);   // CFG_256_GLDS
}

}  // namespace

extern "C" {

int otter_gemm_set_cu_budget(int cus) {
    if (cus < 0) OTTER_FAIL(OTTER_ERR_ARG, "gemm cu budget %d", cus);
    g_cu_budget = (cus > 0 && cus < 8) ? 8 : cus;   // at least one workgroup per XCD
    return (int)persistent_cus();
}

int otter_gemm_set_persistent(int on) {
    g_persistent = on ? 1 : 0;
    return OTTER_OK;
}

int otter_gemm_variant_available(int variant) {
    // auto (0), the generic 128^2 / 256^2 kernels (1-3), the phased fallback for K % 128 != 0 (13), the small-grid ring (25) and its
    // half-height form (30), and the default (26); every other number belonged to a retired schedule
    return variant >= 0 && (variant <= 3 || variant == CFG_PHLB || variant == CFG_S4 || variant == CFG_T4 || variant == CFG_S4H);
}

int otter_gemm_set_variant(int variant) {
    if (variant < 0 || variant > 30) OTTER_FAIL(OTTER_ERR_ARG, "gemm variant %d", variant);
    if (!otter_gemm_variant_available(variant))
        OTTER_FAIL(OTTER_ERR_UNSUPPORTED, "gemm variant %d was retired or never assigned: this library has 0-3, 13, 25, 26 and 30 (DESIGN_HISTORY.md)", variant);
    g_variant = variant;
    return OTTER_OK;
}

int otter_gemm_set_debug(int flags) {
    g_debug = flags & 255;  // bit 64: tile-phase timeline of variant 26 (otter_gemm_read_timeline)
    g_narrow_epilogue = (flags & 256) ? 1 : 0;
    g_order = (flags >> 9) & 31;  // tile-order override (bits 9-12, see tile_of_block); bit 13: non-persistent launch of variant 26
    g_xt_force = (flags >> 14) & 3;                       // cross-tile form of variant 26: 0 default, 1 off, 2 on
    g_korder_force = (flags & (1 << 23)) ? ((flags >> 16) & 127) : -1;   // bit 23: bits 16-22 override the K order / start phase of that form
    return OTTER_OK;
}

int64_t otter_gemm_num_partials(int64_t M, int64_t N, int ab_dtype) {
    int bm, bn;
    cfg_tiles(pick_cfg(M, N, 64, ab_dtype), bm, bn);
    return cdiv64(M, bm) * cdiv64(N, bn);
}

int otter_gemm_kmajor_supported(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int a_kmajor, int b_kmajor, int ab_dtype) {
    if (ab_dtype != OTTER_BF16 || g_variant != 0) return 0;
    if (K < 128) return 0;
    if (K % 128 != 0 && !(a_kmajor && b_kmajor)) return 0;               // K-contiguous operands: whole K-tile pairs (variant 26's pipeline);
                                                                         // both K-major: any K (rows past K read as zeros)
    if (cdiv64(M, 256) * cdiv64(N, 256) < 192) return 0;                 // small grids run the ring kernel on K-contiguous operands
    if (a_kmajor && (M % 8 != 0 || lda % 8 != 0)) return 0;              // 16-byte chunks along the rows
    if (b_kmajor && (N % 8 != 0 || ldb % 8 != 0)) return 0;
    const int64_t span_a = a_kmajor ? ((K - 1) * lda + M) * 2 : ((M - 1) * lda + K) * 2;
    const int64_t span_b = b_kmajor ? ((K - 1) * ldb + N) * 2 : ((N - 1) * ldb + K) * 2;
    return span_a < (int64_t(1) << 32) && span_b < (int64_t(1) << 32);
}

static int gemm_impl(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor, void* C, int64_t ldc, int64_t M, int64_t N,
                     int64_t K, int ab_dtype, int c_dtype, const otter_epilogue_args* epi, void* stream);

int otter_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                  int ab_dtype, int c_dtype, const otter_epilogue_args* epi, void* stream) {
    return gemm_impl(A, lda, 0, B, ldb, 0, C, ldc, M, N, K, ab_dtype, c_dtype, epi, stream);
}

int otter_gemm(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor, void* C, int64_t ldc, int64_t M, int64_t N,
               int64_t K, int ab_dtype, int c_dtype, const otter_epilogue_args* epi, void* stream) {
    if (a_kmajor || b_kmajor)
        OTTER_REQUIRE(otter_gemm_kmajor_supported(M, N, K, lda, ldb, a_kmajor, b_kmajor, ab_dtype),
                      "gemm: K-major operands need bf16, K %% 128 == 0 (any K when both are K-major), >= 192 tiles of 256x256, M / N / ld %% 8 == 0 and < 4 GB per operand "
                      "(M=%ld N=%ld K=%ld): ask otter_gemm_kmajor_supported first and transpose otherwise", (long)M, (long)N, (long)K);
    return gemm_impl(A, lda, a_kmajor ? 1 : 0, B, ldb, b_kmajor ? 1 : 0, C, ldc, M, N, K, ab_dtype, c_dtype, epi, stream);
}

static int gemm_impl(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor, void* C, int64_t ldc, int64_t M, int64_t N,
                     int64_t K, int ab_dtype, int c_dtype, const otter_epilogue_args* epi, void* stream) {
    OTTER_REQUIRE(A && B && C && epi, "gemm: null pointer");
    OTTER_REQUIRE(M > 0 && N > 0 && K > 0, "gemm: empty shape M=%ld N=%ld K=%ld", (long)M, (long)N, (long)K);
    const int kal = ab_dtype == OTTER_BF16 ? 8 : 4;
    OTTER_REQUIRE(((a_kmajor && b_kmajor) || K % kal == 0) && lda % kal == 0 && ldb % kal == 0, "gemm: K=%ld lda=%ld ldb=%ld must be multiples of %d",
                  (long)K, (long)lda, (long)ldb, kal);   // (both operands K-major: K is a row count, any value)
    OTTER_REQUIRE(N % 4 == 0 && ldc % 4 == 0, "gemm: N=%ld ldc=%ld must be multiples of 4", (long)N, (long)ldc);
    OTTER_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0 && ((uintptr_t)C & 15) == 0, "gemm: 16-byte alignment");
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.cdt = c_dtype;
    g.M = M; g.N = N; g.K = K;
    g.kind = epi->kind; g.accumulate = epi->accumulate; g.gate = epi->gate;
    g.R = epi->R; g.ldr = epi->ldr; g.rdt = epi->r_dtype;
    g.C2 = epi->C2; g.ldc2 = epi->ldc2;
    g.aux = epi->aux; g.ldaux = epi->ldaux; g.auxdt = epi->aux_dtype; g.aux_gelu = epi->aux_is_gelu_input;
    g.partial = epi->partial;
    OTTER_REQUIRE(epi->grid_mode >= OTTER_GRID_DEFAULT && epi->grid_mode <= OTTER_GRID_PER_TILE, "gemm: grid_mode %d", epi->grid_mode);
    g.grid_mode = epi->grid_mode;
    switch (g.kind) {
        case OTTER_EPI_STORE:
            OTTER_REQUIRE(!g.accumulate || c_dtype == OTTER_F32, "gemm: accumulate needs an f32 C");
            OTTER_REQUIRE(!g.partial || c_dtype == OTTER_F32, "gemm: sum-of-squares partials of a plain store need an f32 C");
            break;
        case OTTER_EPI_GELU:
            OTTER_REQUIRE(!g.C2 || g.ldc2 % 4 == 0, "gemm: ldc2 %% 4");
            OTTER_REQUIRE(g.aux_gelu == 0 || g.aux_gelu == 3, "gemm: a GELU launch takes aux_is_gelu_input 0 (C2 = pre-activation) or 3 (C2 = GELU'), got %d", g.aux_gelu);
            break;
        case OTTER_EPI_SCALE_RES:
            OTTER_REQUIRE(g.R && g.ldr % 4 == 0, "gemm: SCALE_RES needs R with ldr %% 4 == 0");
            OTTER_REQUIRE(!g.partial, "gemm: partials are written by the STORE (fp32 C) and GATE_BWD epilogues only");
            break;
        case OTTER_EPI_GATE_BWD:
            OTTER_REQUIRE(g.aux && g.ldaux % 4 == 0, "gemm: GATE_BWD needs aux with ldaux %% 4 == 0");
            OTTER_REQUIRE(g.aux_gelu >= 0 && g.aux_gelu <= 3, "gemm: aux activation %d (0 = identity, 1 = erf GELU, 2 = squared ReLU, 3 = aux is the stashed derivative)", g.aux_gelu);
            OTTER_REQUIRE(g.aux_gelu != 3 || !g.partial, "gemm: a stashed derivative (aux_is_gelu_input 3) cannot give the gate partial sum(acc * f(aux))");
            break;
        default:
            OTTER_FAIL(OTTER_ERR_ARG, "gemm: unknown epilogue %d", g.kind);
    }
    const int64_t esz = ab_dtype == OTTER_BF16 ? 2 : 4;
    const bool kmaj = a_kmajor || b_kmajor;
    const bool wide = !kmaj && (((M - 1) * lda + K) * esz >= (int64_t(1) << 32) || ((N - 1) * ldb + K) * esz >= (int64_t(1) << 32));
    int cfg = kmaj ? CFG_T4 : pick_cfg(M, N, K, ab_dtype, wide);
    // round 4: few 128 x 128 tiles of the ring kernel -> half-height tiles (variant 30), so that the skinny products (128 tiles or fewer on
    // 256 CUs) stream on twice the CUs.  Not for a launch that writes per-block gate partials (their count follows otter_gemm_num_partials).
    if (cfg == CFG_S4 && g_variant == 0 && cdiv64(M, 128) * cdiv64(N, 128) <= 160 && !g.partial)
        cfg = CFG_S4H;
    if (cfg == CFG_S4H && g.partial) cfg = CFG_S4;   // (a forced variant 30)
    g.ta = a_kmajor; g.tb = b_kmajor;
    int bm, bn;
    cfg_tiles(cfg, bm, bn);
    g.dbg = g_debug;
    g.order = g_order;
    g.korder = t4_korder();
    // (fp32 outputs stay on the 4-wide tail: there a lane's 4 columns are already a 16-byte store and 16 lanes cover a
    //  whole 256-byte row run; the 8-wide form would split every row into interleaved 16-byte halves: measured +15 %)
    g.wide = (c_dtype == OTTER_BF16 && N % 8 == 0 && ldc % 8 == 0 && (!g.C2 || g.ldc2 % 8 == 0) && (g.kind != OTTER_EPI_SCALE_RES || g.ldr % 8 == 0) &&
              (g.kind != OTTER_EPI_GATE_BWD || g.ldaux % 8 == 0) && !g_narrow_epilogue) ? 1 : 0;
    g.gm = (int)cdiv64(M, bm);
    g.gn = (int)cdiv64(N, bn);
    hipStream_t st = (hipStream_t)stream;
    const bool prof = g_prof.armed && g_prof.M == M && g_prof.N == N && g_prof.K == K && g_prof.n < g_prof.max_events;
    if (prof) hipEventRecord(g_prof.start[g_prof.n], st);
    int rc = launch_cfg(cfg, (unsigned)(g.gm * g.gn), st, g);
    if (rc) return rc;
    if (prof) { g_prof.kmajor[g_prof.n] = (unsigned char)(kmaj ? 1 : 0); hipEventRecord(g_prof.stop[g_prof.n++], st); }
    OTTER_CHECK_LAUNCH("gemm");
    return OTTER_OK;
}

int otter_reduce_partials(const float* partial, int64_t n, const float* gate, float* out, int accumulate, void* stream) {
    OTTER_REQUIRE(partial && out && n > 0, "reduce_partials: bad args");
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, n, gate, out, accumulate);
    OTTER_CHECK_LAUNCH("reduce_partials");
    return OTTER_OK;
}

int otter_prof_arm_gemm(int64_t M, int64_t N, int64_t K, int max_events) {
    otter_prof_disarm();
    OTTER_REQUIRE(max_events > 0 && max_events <= 65536, "prof: max_events");
    g_prof.start = new hipEvent_t[max_events];
    g_prof.stop = new hipEvent_t[max_events];
    g_prof.kmajor = new unsigned char[max_events]();
    for (int i = 0; i < max_events; ++i) {
        hipEventCreate(&g_prof.start[i]);
        hipEventCreate(&g_prof.stop[i]);
    }
    g_prof.M = M; g_prof.N = N; g_prof.K = K;
    g_prof.max_events = max_events;
    g_prof.n = 0;
    g_prof.armed = true;
    return OTTER_OK;
}

int otter_prof_disarm(void) {
    if (g_prof.start) {
        for (int i = 0; i < g_prof.max_events; ++i) {
            hipEventDestroy(g_prof.start[i]);
            hipEventDestroy(g_prof.stop[i]);
        }
        delete[] g_prof.start;
        delete[] g_prof.stop;
        delete[] g_prof.kmajor;
    }
    g_prof = Prof();
    return OTTER_OK;
}

int otter_prof_collect_split(int* count, double* total_ms, int* count_kmajor, double* kmajor_ms) {
    OTTER_REQUIRE(count && total_ms, "prof_collect: null");
    double tot = 0.0, km = 0.0;
    int nk = 0;
    for (int i = 0; i < g_prof.n; ++i) {
        hipEventSynchronize(g_prof.stop[i]);
        float ms = 0.f;
        hipEventElapsedTime(&ms, g_prof.start[i], g_prof.stop[i]);
        tot += ms;
        if (g_prof.kmajor[i]) { km += ms; ++nk; }
    }
    *count = g_prof.n;
    *total_ms = tot;
    if (count_kmajor) *count_kmajor = nk;
    if (kmajor_ms) *kmajor_ms = km;
    g_prof.n = 0;
    return OTTER_OK;
}

int otter_prof_collect(int* count, double* total_ms) { return otter_prof_collect_split(count, total_ms, nullptr, nullptr); }

}  // extern "C"
