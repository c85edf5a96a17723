// w8.hip -- int8 weight-only products of the frozen decoder during generation.
//
// Format (otter_amd/quant.py): qweight int8 [N, K] row-major, scale fp32 [N] (one per output row), |q| <= 127.
//
// otter_gemv_w8   y[M, N] = (x[M, K] . q[N, K]^T) * scale[N] (+ bias[N]) (then exact-erf GELU, act 1, or the squared ReLU of the Persimmon MLP,
//                 act 3), 1 <= M <= 16: one cached decode step sends B x num_beams rows through every decoder linear, so the product is a single pass over the weight.  x is NOT quantised
//                 and the i8 matrix instruction is not used: q is converted to bf16 in registers (exact for |q| <= 127) and fed to
//                 v_mfma_f32_16x16x32_bf16 with x padded to 16 rows; fp32 accumulation, the scale applied to the fp32 sum.
// otter_gemm_w8_rows  the same product for 1 <= M <= 64: one-token steps of 17 to 64 rows (B x num_beams) still stream the weight once.
// otter_gemm_w8_panel  the same product for 1 <= M <= 256: one-token steps of 65 to 256 rows (csrc/w8_panel.hip, included below).
// otter_gemv_w8_gated, otter_gemm_w8_rows_gated, otter_gemm_w8_panel_gated  the same products with y = v tanh(*gate) + R in place of the activation: the second FFN
//                 product of a gated cross-attention block with its tanh-gate residual.  Same kernels, GATED = true.
// otter_dequant_w8  out[n, k] = bf16(float(q[n, k]) * scale[n]): the streaming pass behind the prompt (prefill) path.
//
// GEMV decomposition.  A workgroup of 4 waves owns 16 R output rows (R = 1, or 2 from N = 16384 up) and one of S contiguous K ranges; its
// waves cut that range in four (split-K inside the workgroup, combined through LDS in wave order).  Per 64-wide K step a lane loads 16
// consecutive int8 of ONE weight row (row = lane & 15, K offset 16 (lane >> 4)) straight into VGPRs -- the weight is streamed once and
// shared with nobody, so it never touches LDS -- and the two 8-element halves are the A fragments of two MFMAs; the matching 2 x 8
// bf16 of x row (lane & 15) are the B fragments (x is at most 512 KB and stays in L2; lanes of rows >= M load nothing).  Both operands
// see the same permutation of K inside a step, which a dot product does not notice.  Steps are issued four at a time, the next four
// requested before the current four are consumed.  With S > 1 (few rows, long K: out_proj, down_proj) every workgroup writes its raw
// fp32 sums to the workspace and a second kernel adds the S ranges in order: no floating-point atomics, bit-identical from call to call.
//
// Rows decomposition (gemm_w8_rows).  At 64 rows x is 4 times the GEMV's and fragment-shaped loads of it by every wave would dominate the
// load path, so here the four waves of a workgroup take four DIFFERENT 16-row weight tiles (64 output columns per workgroup) over the SAME
// K range and share x through LDS.  K advances in chunks of 256 (four 64-wide steps).  Per chunk a wave loads its 4 x 16 weight bytes per
// lane straight into VGPRs exactly as the GEMV does; the workgroup loads the chunk of x, rows 0 .. 16 ceil(M / 16) - 1 (rows >= M are
// zero-filled, not read), as full 512-byte row pieces and writes them to one of two LDS images [64 rows][32 slots of 16 B], slot c of row r
// stored at c ^ (r & 15): the 16 rows that one lane group of a 16-byte LDS read covers then fall on 16 different slots of the 256-byte
// bank row.  One barrier per chunk: the loads of chunk c + 1 (weights to registers, x to registers) are issued before chunk c is
// consumed and x is written to the other image after it.  Each converted weight fragment (cvt8, once per weight element) feeds the MFMAs
// of all ceil(M / 16) column blocks.  Split-K as above, but ACROSS workgroups only: the split count S depends on (N, K) alone, every
// output element is one MFMA chain per K range in ascending K and the S ranges are added in order, so row m of y has the same bits
// whatever M is and whatever the other rows hold.  (A wave here sums a whole range where the GEMV's four waves sum quarters of it: for
// M <= 16 the two kernels agree to rounding, not bit for bit.)
#include "common.h"

typedef __bf16 w8_bf16x8_t __attribute__((ext_vector_type(8)));
typedef float w8_f32x4_t __attribute__((ext_vector_type(4)));

namespace {

constexpr int NT = 256, WAVES = 4, KSTEP = 64, UNROLL = 4;
constexpr int MAX_SPLIT = 8;              // OTTER_GEMV_W8_WORKSPACE_BYTES of the header is sized for it
constexpr int64_t WG_TARGET = 512;        // two workgroups (8 waves) per CU of a 256-CU part
constexpr int64_t MIN_K_PER_WG = 1024;    // a K range is split further only while each workgroup keeps this much

struct W8Args {
    const bf16_t* x; int64_t ldx;
    const int8_t* w; int64_t ldw;
    const float* scale;
    const void* bias; int bias_dtype;
    void* y; int64_t ldy; int y_dtype;
    float* part;                          // [S, M, N] fp32 (S > 1)
    int M, N, K, act, S;
    int T, q;                             // K steps in all, K steps per wave
    const float* gate;                    // the GATED kernels only: y = v tanh(*gate) + R, gate NULL: y = v + R (R NULL: a plain entry)
    const void* R; int64_t ldr; int r_dtype;
};

// 8 int8 (two dwords) -> 8 bf16, exact
__device__ __forceinline__ w8_bf16x8_t cvt8(uint32_t lo, uint32_t hi) {
    float f[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[i] = (float)(int)(int8_t)(lo >> (8 * i));
        f[4 + i] = (float)(int)(int8_t)(hi >> (8 * i));
    }
    uint4 r;
    r.x = pack2bf(f[0], f[1]);
    r.y = pack2bf(f[2], f[3]);
    r.z = pack2bf(f[4], f[5]);
    r.w = pack2bf(f[6], f[7]);
    return __builtin_bit_cast(w8_bf16x8_t, r);
}

// GATED (the _gated entries): y = v tanh(*gate) + R, the EPI_SCALE_RES tail of the GEMM family (gemm_tail.h), instead of the activation.  A
// template parameter, not a test of a.R: the plain entries keep, instruction for instruction, the code they had (with a run-time branch
// they measured up to 3 % slower where K is split).  w8_gate: the factor, once per thread.
template <bool GATED>
__device__ __forceinline__ float w8_gate(const W8Args& a) {
    if constexpr (GATED) return a.gate ? tanhf(*a.gate) : 1.0f;
    else return 1.0f;
}

template <bool GATED>
__device__ __forceinline__ float w8_epilogue(float v, float sg, int64_t m, int64_t n, const W8Args& a) {
    v *= a.scale[n];
    if (a.bias) v += ld_as_f32(a.bias, n, a.bias_dtype);
    if constexpr (GATED) {
        return v * sg + ld_as_f32(a.R, m * a.ldr + n, a.r_dtype);
    } else {
        if (a.act == 1) return gelu_erf(v);
        if (a.act == 3) {                 // relu(v)^2 in fp32 on the fp32 sum: one rounding, to the output dtype, in the caller's store
            const float r = fmaxf(v, 0.f);
            return r * r;
        }
        return v;
    }
}

template <int R>
struct Batch {
    uint4 w[UNROLL][R], xa[UNROLL], xb[UNROLL];
};

template <int R, bool GATED>
__global__ __launch_bounds__(NT) void gemv_w8_kernel(W8Args a) {
    __shared__ float red[WAVES][R][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * (16 * R);
    const int s = blockIdx.y;
    const int t0 = (s * WAVES + wv) * a.q, t1 = min(t0 + a.q, a.T);

    const int8_t* wp[R];
    bool row_ok[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t n = n0 + 16 * r + r16;
        row_ok[r] = n < a.N;
        wp[r] = a.w + (row_ok[r] ? n : 0) * a.ldw + 16 * g;
    }
    const bool x_ok = r16 < a.M;
    const bf16_t* xp = a.x + (int64_t)(x_ok ? r16 : 0) * a.ldx + 16 * g;

    auto load = [&](Batch<R>& b, int t) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int64_t k = (int64_t)(t + u) * KSTEP;
            const bool ok = (t + u) < t1 && k + 16 * g < a.K;      // K % 16 == 0: a lane's 16 elements are all inside or all outside
#pragma unroll
            for (int r = 0; r < R; ++r)
                b.w[u][r] = (ok && row_ok[r]) ? *reinterpret_cast<const uint4*>(wp[r] + k) : make_uint4(0, 0, 0, 0);
            if (ok && x_ok) {
                b.xa[u] = *reinterpret_cast<const uint4*>(xp + k);
                b.xb[u] = *reinterpret_cast<const uint4*>(xp + k + 8);
            } else {
                b.xa[u] = make_uint4(0, 0, 0, 0);
                b.xb[u] = make_uint4(0, 0, 0, 0);
            }
        }
    };

    // the weight rows are the MFMA's A operand and the x rows its B operand, so a tile is [weight row, x row]: y transposed (read back below)
    w8_f32x4_t acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = w8_f32x4_t{0.f, 0.f, 0.f, 0.f};

    auto consume = [&](const Batch<R>& b) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const w8_bf16x8_t xa = __builtin_bit_cast(w8_bf16x8_t, b.xa[u]), xb = __builtin_bit_cast(w8_bf16x8_t, b.xb[u]);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8(b.w[u][r].x, b.w[u][r].y), xa, acc[r], 0, 0, 0);
                acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8(b.w[u][r].z, b.w[u][r].w), xb, acc[r], 0, 0, 0);
            }
        }
    };

    Batch<R> cur, nxt;
    if (t0 < t1) load(cur, t0);
    for (int t = t0; t < t1; t += 2 * UNROLL) {                     // ping-pong between the two register batches (all conditions wave-uniform)
        const bool more = t + UNROLL < t1;
        if (more) load(nxt, t + UNROLL);
        consume(cur);
        if (more) {
            if (t + 2 * UNROLL < t1) load(cur, t + 2 * UNROLL);
            consume(nxt);
        }
    }

    // the four waves' partial tiles, added in wave order.  acc[r][i] of a lane = row 16 r + 4 (lane >> 4) + i, column (x row) lane & 15
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[wv][r][i][lane] = acc[r][i];
    __syncthreads();
    const float sg = w8_gate<GATED>(a);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int nn = tid & 15, m = tid >> 4;                      // neighbouring threads write neighbouring columns of y
        const int ln = (nn >> 2) * 16 + m, i = nn & 3;
        const int64_t n = n0 + 16 * r + nn;
        if (m >= a.M || n >= a.N) continue;
        float v = red[0][r][i][ln];
#pragma unroll
        for (int w2 = 1; w2 < WAVES; ++w2) v += red[w2][r][i][ln];
        if (a.S == 1) st_from_f32(a.y, (int64_t)m * a.ldy + n, a.y_dtype, w8_epilogue<GATED>(v, sg, m, n, a));
        else a.part[((int64_t)s * a.M + m) * a.N + n] = v;
    }
}

// S > 1: one thread per output element adds the S ranges in order
template <bool GATED>
__global__ __launch_bounds__(NT) void gemv_w8_reduce_kernel(W8Args a) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= (int64_t)a.M * a.N) return;
    const int64_t m = e / a.N, n = e % a.N;
    float v = a.part[e];
    for (int s = 1; s < a.S; ++s) v += a.part[(int64_t)s * a.M * a.N + e];
    st_from_f32(a.y, m * a.ldy + n, a.y_dtype, w8_epilogue<GATED>(v, w8_gate<GATED>(a), m, n, a));
}

// ---- rows kernel (17 to 64 rows; any 1 <= M <= 64 is accepted) -----------------------------------------------------------------------------

constexpr int ROWS_MAX_M = 64;
constexpr int ROWS_BN = 16 * WAVES;                 // output columns (weight rows) per workgroup
constexpr int ROWS_KC = UNROLL * KSTEP;             // K elements per chunk
constexpr int ROWS_SLOTS = ROWS_KC / 8;             // 16-byte slots per x row of a chunk (32: two 256-byte bank rows)
constexpr int ROWS_MAX_SPLIT = 8;                   // OTTER_GEMM_W8_ROWS_WORKSPACE_BYTES of the header is sized for it
constexpr int64_t ROWS_WG_TARGET = 256;             // K is split further only while there is at most one workgroup per CU of a 256-CU part
constexpr int64_t ROWS_MIN_K_PER_WG = 512;

template <int MB, bool GATED>
__global__ __launch_bounds__(NT) void gemm_w8_rows_kernel(W8Args a) {          // a.T: chunks in all, a.q: chunks per K range
    __shared__ uint4 xs[2][ROWS_MAX_M * ROWS_SLOTS];                           // 2 x 32 KB
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * ROWS_BN + 16 * wv;
    const int s = blockIdx.y;
    const int c0 = s * a.q, c1 = min(c0 + a.q, a.T);

    const bool row_ok = n0 + r16 < a.N;
    const int8_t* wp = a.w + (row_ok ? n0 + r16 : 0) * a.ldw + 16 * g;

    auto load_w = [&](uint4 (&w)[UNROLL], int c) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int64_t k = (int64_t)c * ROWS_KC + u * KSTEP;
            const bool ok = row_ok && k + 16 * g < a.K;                        // K % 16 == 0: a lane's 16 elements are all inside or all outside
            w[u] = ok ? *reinterpret_cast<const uint4*>(wp + k) : make_uint4(0, 0, 0, 0);
        }
    };
    // x chunk: 16 MB rows x 32 slots, 2 MB slots per thread; 32 consecutive threads read one 512-byte row piece
    auto load_x = [&](uint4 (&xr)[2 * MB], int c) {
#pragma unroll
        for (int j = 0; j < 2 * MB; ++j) {
            const int idx = j * NT + tid, row = idx / ROWS_SLOTS, cc = idx % ROWS_SLOTS;
            const int64_t k = (int64_t)c * ROWS_KC + 8 * cc;
            const bool ok = row < a.M && k < a.K;                              // (K % 8 == 0: the 8 elements are all inside or all outside)
            xr[j] = ok ? *reinterpret_cast<const uint4*>(a.x + (int64_t)row * a.ldx + k) : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_x = [&](int buf, const uint4 (&xr)[2 * MB]) {
#pragma unroll
        for (int j = 0; j < 2 * MB; ++j) {
            const int idx = j * NT + tid, row = idx / ROWS_SLOTS, cc = idx % ROWS_SLOTS;
            xs[buf][row * ROWS_SLOTS + (cc ^ (row & 15))] = xr[j];
        }
    };

    // a tile is [weight row, x row] as in the GEMV: acc[mb][i] of a lane = weight row 4 (lane >> 4) + i of the wave's 16, x row 16 mb + (lane & 15)
    w8_f32x4_t acc[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[mb] = w8_f32x4_t{0.f, 0.f, 0.f, 0.f};

    auto consume = [&](const uint4 (&w)[UNROLL], int buf) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const w8_bf16x8_t wa = cvt8(w[u].x, w[u].y), wb = cvt8(w[u].z, w[u].w);
            const int cc = 8 * u + 2 * g;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const uint4* xrow = &xs[buf][(16 * mb + r16) * ROWS_SLOTS];
                const uint4 xa = xrow[cc ^ r16], xb = xrow[(cc + 1) ^ r16];
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, __builtin_bit_cast(w8_bf16x8_t, xa), acc[mb], 0, 0, 0);
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb, __builtin_bit_cast(w8_bf16x8_t, xb), acc[mb], 0, 0, 0);
            }
        }
    };

    uint4 wc[UNROLL], wn[UNROLL], xr[2 * MB];
    if (c0 < c1) {
        load_w(wc, c0);
        load_x(xr, c0);
        store_x(0, xr);
    }
    __syncthreads();
    for (int c = c0; c < c1; c += 2) {                                          // ping-pong between the two register batches / LDS images
        const bool more = c + 1 < c1;                                           // (all conditions uniform over the workgroup)
        if (more) {
            load_w(wn, c + 1);
            load_x(xr, c + 1);
        }
        consume(wc, 0);
        if (more) store_x(1, xr);
        __syncthreads();
        if (more) {
            const bool more2 = c + 2 < c1;
            if (more2) {
                load_w(wc, c + 2);
                load_x(xr, c + 2);
            }
            consume(wn, 1);
            if (more2) store_x(0, xr);
            __syncthreads();
        }
    }

    const float sg = w8_gate<GATED>(a);
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int m = 16 * mb + r16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t n = n0 + 4 * g + i;
            if (m >= a.M || n >= a.N) continue;
            if (a.S == 1) st_from_f32(a.y, (int64_t)m * a.ldy + n, a.y_dtype, w8_epilogue<GATED>(acc[mb][i], sg, m, n, a));
            else a.part[((int64_t)s * a.M + m) * a.N + n] = acc[mb][i];
        }
    }
}

// one workgroup per weight row, 16 elements per thread and trip
__global__ __launch_bounds__(NT) void dequant_w8_kernel(const int8_t* __restrict__ q, int64_t ldw, const float* __restrict__ scale,
                                                        bf16_t* __restrict__ out, int64_t ldo, int K) {
    const int64_t n = blockIdx.x;
    const float sc = scale[n];
    const int8_t* qr = q + n * ldw;
    bf16_t* orow = out + n * ldo;
    for (int k = 16 * threadIdx.x; k < K; k += 16 * NT) {
        const uint4 v = *reinterpret_cast<const uint4*>(qr + k);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint4 o[2];
        uint32_t* op = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float f[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) f[i] = (float)(int)(int8_t)(w[j] >> (8 * i)) * sc;
            op[2 * j] = pack2bf(f[0], f[1]);
            op[2 * j + 1] = pack2bf(f[2], f[3]);
        }
        *reinterpret_cast<uint4*>(orow + k) = o[0];
        *reinterpret_cast<uint4*>(orow + k + 8) = o[1];
    }
}

// ---- host: argument checks and launches shared by the plain and the gated entry of each family --------------------------------------------

struct W8Call {
    const void* x; int64_t ldx; const void* qweight; int64_t ldw; const float* scale; const void* bias; int bias_dtype;
    void* y; int64_t ldy; int y_dtype; int64_t M, N, K; int act; void* workspace; int64_t workspace_bytes; void* stream;
    bool gated; const float* gate; const void* R; int64_t ldr; int r_dtype;       // gated: the tail of otter_gemv_w8_gated (R must be there)
};

// the checks in the order include/otter_hip.h documents them; `what` names the entry in the message, max_m is 16, 64 or 256
int w8_check(const W8Call& c, const char* what, int max_m) {
    OTTER_REQUIRE(c.x && c.qweight && c.scale && c.y && c.workspace && (!c.gated || c.R), "%s: null pointer", what);
    OTTER_REQUIRE(c.M >= 1 && c.M <= max_m, "%s: M=%d outside [1, %d]", what, (int)c.M, max_m);
    OTTER_REQUIRE(c.N >= 1 && c.N <= (int64_t)1 << 30, "%s: N=%ld outside [1, 2^30]", what, (long)c.N);
    OTTER_REQUIRE(c.K >= 16 && c.K % 16 == 0 && c.K <= (int64_t)1 << 30, "%s: K=%d must be a positive multiple of 16", what, (int)c.K);
    OTTER_REQUIRE(c.ldw % 16 == 0 && c.ldx % 8 == 0 && (((uintptr_t)c.x | (uintptr_t)c.qweight | (uintptr_t)c.y) & 15) == 0,
                  "%s: alignment (x, qweight, y 16-byte aligned; ldw %% 16 == 0; ldx %% 8 == 0)", what);
    OTTER_REQUIRE(c.ldw >= c.K && c.ldx >= c.K && c.ldy >= c.N && (!c.gated || c.ldr >= c.N),
                  "%s: a leading dimension is smaller than the row it holds", what);
    if (c.gated) {
        OTTER_REQUIRE((c.y_dtype == OTTER_F32 || c.y_dtype == OTTER_BF16) && (!c.bias || c.bias_dtype == OTTER_F32 || c.bias_dtype == OTTER_BF16) &&
                          (c.r_dtype == OTTER_F32 || c.r_dtype == OTTER_BF16),
                      "%s: y / bias / R dtype must be OTTER_F32 or OTTER_BF16", what);
        // y is written while other threads still read R: the two blocks may not share a byte (the same tensor included)
        const uintptr_t y0 = (uintptr_t)c.y, y1 = y0 + (uintptr_t)((c.M - 1) * c.ldy + c.N) * (c.y_dtype == OTTER_F32 ? 4 : 2);
        const uintptr_t r0 = (uintptr_t)c.R, r1 = r0 + (uintptr_t)((c.M - 1) * c.ldr + c.N) * (c.r_dtype == OTTER_F32 ? 4 : 2);
        OTTER_REQUIRE(y1 <= r0 || r1 <= y0, "%s: y and R overlap", what);
    } else {
        OTTER_REQUIRE((c.y_dtype == OTTER_F32 || c.y_dtype == OTTER_BF16) && (!c.bias || c.bias_dtype == OTTER_F32 || c.bias_dtype == OTTER_BF16),
                      "%s: y / bias dtype must be OTTER_F32 or OTTER_BF16", what);
        OTTER_REQUIRE(c.act == 0 || c.act == 1 || c.act == 3, "%s: act=%d (0 none, 1 GELU, 3 squared ReLU)", what, c.act);
    }
    // (OTTER_GEMM_W8_ROWS_WORKSPACE_BYTES is the GEMV's expression; the panel entries, max_m 256, have their own)
    const int64_t need = max_m > 64 ? OTTER_GEMM_W8_PANEL_WORKSPACE_BYTES(c.M, c.N, c.K) : OTTER_GEMV_W8_WORKSPACE_BYTES(c.M, c.N, c.K);
    OTTER_REQUIRE(c.workspace_bytes >= need, "%s: workspace of %ld bytes, %ld needed", what, (long)c.workspace_bytes, (long)need);
    return OTTER_OK;
}

W8Args w8_args(const W8Call& c) {
    W8Args a;
    a.x = (const bf16_t*)c.x; a.ldx = c.ldx;
    a.w = (const int8_t*)c.qweight; a.ldw = c.ldw;
    a.scale = c.scale; a.bias = c.bias; a.bias_dtype = c.bias_dtype;
    a.y = c.y; a.ldy = c.ldy; a.y_dtype = c.y_dtype;
    a.part = (float*)c.workspace;
    a.M = (int)c.M; a.N = (int)c.N; a.K = (int)c.K; a.act = c.gated ? 0 : c.act;
    a.gate = c.gated ? c.gate : nullptr;
    a.R = c.gated ? c.R : nullptr; a.ldr = c.ldr; a.r_dtype = c.r_dtype;
    return a;
}

template <bool GATED>
void launch_gemv(int R, dim3 grid, hipStream_t st, const W8Args& a) {
    if (R == 2) hipLaunchKernelGGL((gemv_w8_kernel<2, GATED>), grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((gemv_w8_kernel<1, GATED>), grid, dim3(NT), 0, st, a);
}

template <bool GATED>
void launch_rows(int mb, dim3 grid, hipStream_t st, const W8Args& a) {
    switch (mb) {
        case 1: hipLaunchKernelGGL((gemm_w8_rows_kernel<1, GATED>), grid, dim3(NT), 0, st, a); break;
        case 2: hipLaunchKernelGGL((gemm_w8_rows_kernel<2, GATED>), grid, dim3(NT), 0, st, a); break;
        case 3: hipLaunchKernelGGL((gemm_w8_rows_kernel<3, GATED>), grid, dim3(NT), 0, st, a); break;
        default: hipLaunchKernelGGL((gemm_w8_rows_kernel<4, GATED>), grid, dim3(NT), 0, st, a); break;
    }
}

int w8_reduce(const W8Args& a, hipStream_t st, const char* what) {
    const dim3 grid((unsigned)cdiv64((int64_t)a.M * a.N, NT));
    if (a.R) hipLaunchKernelGGL(gemv_w8_reduce_kernel<true>, grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL(gemv_w8_reduce_kernel<false>, grid, dim3(NT), 0, st, a);
    OTTER_CHECK_LAUNCH(what);
    return OTTER_OK;
}

int gemv_w8_run(const W8Call& c, const char* what, const char* what_reduce) {
    const int rc = w8_check(c, what, 16);
    if (rc != OTTER_OK) return rc;
    const int64_t N = c.N, K = c.K;
    const int R = N >= 16384 ? 2 : 1;
    const int64_t base = cdiv64(N, 16 * R);
    int S = 1;
    while (base * S < WG_TARGET && S < MAX_SPLIT && K / (2 * S) >= MIN_K_PER_WG) S *= 2;
    OTTER_REQUIRE(S <= 65535, "%s: internal split", what);

    W8Args a = w8_args(c);
    a.S = S;
    a.T = (int)cdiv64(K, KSTEP);
    a.q = (int)cdiv64(a.T, (int64_t)S * WAVES);
    hipStream_t st = (hipStream_t)c.stream;
    const dim3 grid((unsigned)base, (unsigned)S);
    if (c.gated) launch_gemv<true>(R, grid, st, a);
    else launch_gemv<false>(R, grid, st, a);
    OTTER_CHECK_LAUNCH(what);
    return S > 1 ? w8_reduce(a, st, what_reduce) : OTTER_OK;
}

int gemm_w8_rows_run(const W8Call& c, const char* what, const char* what_reduce) {
    const int rc = w8_check(c, what, ROWS_MAX_M);
    if (rc != OTTER_OK) return rc;
    const int64_t N = c.N, K = c.K;
    // the split is a function of (N, K) only -- never of M -- so that a row's summation order does not depend on what it is batched with
    const int64_t base = cdiv64(N, ROWS_BN);
    int S = 1;
    while (base * S <= ROWS_WG_TARGET && S < ROWS_MAX_SPLIT && K / (2 * S) >= ROWS_MIN_K_PER_WG) S *= 2;
    OTTER_REQUIRE(base <= 0x7fffffff, "%s: internal grid", what);

    W8Args a = w8_args(c);
    a.S = S;
    a.T = (int)cdiv64(K, ROWS_KC);
    a.q = (int)cdiv64(a.T, S);
    hipStream_t st = (hipStream_t)c.stream;
    const dim3 grid((unsigned)base, (unsigned)S);
    if (c.gated) launch_rows<true>((int)cdiv64(c.M, 16), grid, st, a);
    else launch_rows<false>((int)cdiv64(c.M, 16), grid, st, a);
    OTTER_CHECK_LAUNCH(what);
    return S > 1 ? w8_reduce(a, st, what_reduce) : OTTER_OK;
}

#include "w8_panel.hip"   // gemm_w8_panel_kernel and gemm_w8_panel_run: one-token steps of 65 to 256 rows

}  // namespace

extern "C" {

int otter_gemv_w8(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias, int bias_dtype, void* y,
                  int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, int act, void* workspace, int64_t workspace_bytes, void* stream) {
    return gemv_w8_run({x, ldx, qweight, ldw, scale, bias, bias_dtype, y, ldy, y_dtype, M, N, K, act, workspace, workspace_bytes, stream, false,
                        nullptr, nullptr, 0, OTTER_F32},
                       "gemv_w8", "gemv_w8 (reduce)");
}

int otter_gemm_w8_rows(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias, int bias_dtype,
                       void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, int act, void* workspace, int64_t workspace_bytes,
                       void* stream) {
    return gemm_w8_rows_run({x, ldx, qweight, ldw, scale, bias, bias_dtype, y, ldy, y_dtype, M, N, K, act, workspace, workspace_bytes, stream,
                             false, nullptr, nullptr, 0, OTTER_F32},
                            "gemm_w8_rows", "gemm_w8_rows (reduce)");
}

int otter_gemv_w8_gated(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias, int bias_dtype,
                        void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, const float* gate, const void* R, int64_t ldr,
                        int r_dtype, void* workspace, int64_t workspace_bytes, void* stream) {
    return gemv_w8_run({x, ldx, qweight, ldw, scale, bias, bias_dtype, y, ldy, y_dtype, M, N, K, 0, workspace, workspace_bytes, stream, true,
                        gate, R, ldr, r_dtype},
                       "gemv_w8_gated", "gemv_w8_gated (reduce)");
}

int otter_gemm_w8_rows_gated(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias,
                             int bias_dtype, void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, const float* gate,
                             const void* R, int64_t ldr, int r_dtype, void* workspace, int64_t workspace_bytes, void* stream) {
    return gemm_w8_rows_run({x, ldx, qweight, ldw, scale, bias, bias_dtype, y, ldy, y_dtype, M, N, K, 0, workspace, workspace_bytes, stream,
                             true, gate, R, ldr, r_dtype},
                            "gemm_w8_rows_gated", "gemm_w8_rows_gated (reduce)");
}

int otter_gemm_w8_panel(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias, int bias_dtype,
                        void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, int act, void* workspace, int64_t workspace_bytes,
                        void* stream) {
    return gemm_w8_panel_run({x, ldx, qweight, ldw, scale, bias, bias_dtype, y, ldy, y_dtype, M, N, K, act, workspace, workspace_bytes, stream,
                              false, nullptr, nullptr, 0, OTTER_F32},
                             "gemm_w8_panel", "gemm_w8_panel (reduce)");
}

int otter_gemm_w8_panel_gated(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias,
                              int bias_dtype, void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, const float* gate,
                              const void* R, int64_t ldr, int r_dtype, void* workspace, int64_t workspace_bytes, void* stream) {
    return gemm_w8_panel_run({x, ldx, qweight, ldw, scale, bias, bias_dtype, y, ldy, y_dtype, M, N, K, 0, workspace, workspace_bytes, stream,
                              true, gate, R, ldr, r_dtype},
                             "gemm_w8_panel_gated", "gemm_w8_panel_gated (reduce)");
}

int otter_dequant_w8(const void* qweight, int64_t ldw, const float* scale, void* out, int64_t ldo, int64_t N, int64_t K, void* stream) {
    OTTER_REQUIRE(qweight && scale && out, "dequant_w8: null pointer");
    OTTER_REQUIRE(N >= 1 && N <= (int64_t)1 << 30, "dequant_w8: N=%ld outside [1, 2^30]", (long)N);
    OTTER_REQUIRE(K >= 16 && K % 16 == 0 && K <= (int64_t)1 << 30, "dequant_w8: K=%d must be a positive multiple of 16", (int)K);
    OTTER_REQUIRE(ldw % 16 == 0 && ldo % 8 == 0 && (((uintptr_t)qweight | (uintptr_t)out) & 15) == 0,
                  "dequant_w8: alignment (qweight, out 16-byte aligned; ldw %% 16 == 0; ldo %% 8 == 0)");
    OTTER_REQUIRE(ldw >= K && ldo >= K, "dequant_w8: a leading dimension is smaller than the row it holds");
    hipLaunchKernelGGL(dequant_w8_kernel, dim3((unsigned)N), dim3(NT), 0, (hipStream_t)stream, (const int8_t*)qweight, ldw, scale, (bf16_t*)out,
                       ldo, (int)K);
    OTTER_CHECK_LAUNCH("dequant_w8");
    return OTTER_OK;
}

}  // extern "C"
