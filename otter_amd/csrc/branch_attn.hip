// branch_attn.hip -- the self-attention of CANDIDATE rows over a cached prompt (StaticKVCache.attend_branches, otter_amd/kv_cache.py),
// head_dim 128.  N = B * C * T one-token rows, row n = (b C + c) T + t, are the T teacher-forced positions of the C candidates of each of
// the B sentences.  Row (b, c, t) attends over the prompt's keys, which all candidates of sentence b share, and over the t + 1 keys
// (b, c, 0..t) of its own candidate -- nothing of another candidate, nothing later than itself.  The prompt part is a non-causal flash
// forward of all rows of a sentence against the cache (csrc/flash.hip: Sq = C T, Sk = the prompt length), which returns o1 -- in fp32,
// unrounded (otter_flash_attn_fwd_f32), so that the answer is rounded to bf16 once, here, as the one-kernel cached step rounds once -- and lse1; this
// file is the rest: the own keys' scores, and the merge of the two softmax pieces.
//
//   a   = slopes ? slopes[h] : 0
//   L1  = lse1 - a (t + 1)            flash placed the ALiBi origin at the prompt's last key; for this query the newest key lies t + 1 later
//   e_u = scale q . k_new[(b,c,u)] + a (u - t),   u = 0 .. t
//   M   = max(L1, max_u e_u),  w1 = exp(L1 - M),  p_u = exp(e_u - M)
//   o   = (w1 o1 + sum_u p_u v_new[(b,c,u)]) / (w1 + sum_u p_u)           fp32, rounded to bf16 once
//
// lse1 = -inf (no visible prompt key) gives w1 = 0, and o1 is then not used at all (it may hold anything).  Key u = t is always there, so
// the denominator is positive.
//
// Shape: one wave per (row, head), four waves per workgroup, no LDS, no atomics, no workspace; the grid depends on N and H only.  Lane u of
// the wave owns own key u for the score (lanes u > t load nothing); the maximum is a 64-lane butterfly; the sums over u run in ascending u in
// every lane, which owns output dims 2 lane and 2 lane + 1: two calls on the same inputs give the same bits.  Nothing is written but o.
#include "decode_cached_entry.h"

namespace {

constexpr int HD = 128, WAVES = 4, T_MAX = OTTER_BRANCH_ATTN_MAX_T;
static_assert(T_MAX == OTTER_WAVE, "branch_attn: one lane per own key");

struct BranchArgs {
    const bf16_t* q; int64_t q_rs, q_hs;                  // rows [N, H, 128]: row / head strides (elements), dim stride 1
    const bf16_t* kn; int64_t kn_rs, kn_hs;
    const bf16_t* vn; int64_t vn_rs, vn_hs;
    const float* o1;                                      // [N, H, 128] contiguous, fp32: the flash forward's O before any rounding
    const float* lse1;                                    // [N / rows_per_sentence, H, rows_per_sentence]
    const float* slopes;                                  // [H] or null
    bf16_t* o;                                            // [N, H, 128] contiguous
    int64_t NH;                                           // N * H
    int H, T, rps;                                        // rps: rows per sentence, C * T
    float scale;
};

__global__ __launch_bounds__(WAVES * OTTER_WAVE) void branch_attn_merge_kernel(BranchArgs a) {
    const int lane = threadIdx.x & (OTTER_WAVE - 1);
    const int64_t p = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);       // the wave's (row, head)
    if (p >= a.NH) return;                                                    // (wave-uniform; the kernel has no barrier)
    const int64_t n = p / a.H;
    const int h = (int)(p - n * a.H);
    const int t = (int)(n % a.T);
    const int64_t n0 = n - t;                                                 // row (b, c, 0): rows n0 .. n are this row's own keys
    const int64_t b = n / a.rps;
    const float slope = a.slopes ? a.slopes[h] : 0.f;
    const float L1 = a.lse1[(b * a.H + h) * a.rps + (n - b * a.rps)] - slope * (float)(t + 1);

    // 1. lane u <= t: the score of own key u
    float e = -INFINITY;
    if (lane <= t) {
        const bf16_t* qp = a.q + n * a.q_rs + h * a.q_hs;
        const bf16_t* kp = a.kn + (n0 + lane) * a.kn_rs + h * a.kn_hs;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < HD / 8; ++i) {
            float qf[8], kf[8];
            unpack8(*reinterpret_cast<const uint4*>(qp + 8 * i), qf);
            unpack8(*reinterpret_cast<const uint4*>(kp + 8 * i), kf);
#pragma unroll
            for (int j = 0; j < 8; ++j) s = fmaf(qf[j], kf[j], s);
        }
        e = s * a.scale + slope * (float)(lane - t);
    }
    const float M = fmaxf(L1, wave_max(e));                                   // key t is live: M > -inf unless a score is NaN
    const float pu = lane <= t ? __expf(e - M) : 0.f;
    const float w1 = __expf(L1 - M);                                          // L1 = -inf -> 0

    // 2. the own values, u ascending; the lane's two output dims
    float acc0 = 0.f, acc1 = 0.f, den = w1;
    if (w1 > 0.f) {                                                           // (otherwise o1 is not read: it may hold NaN)
        const float2 w = *reinterpret_cast<const float2*>(a.o1 + p * HD + 2 * lane);
        acc0 = w1 * w.x;
        acc1 = w1 * w.y;
    }
    const bf16_t* vp = a.vn + n0 * a.vn_rs + h * a.vn_hs + 2 * lane;
    for (int u = 0; u <= t; ++u) {
        const float pj = __shfl(pu, u, 64);
        const uint32_t w = *reinterpret_cast<const uint32_t*>(vp + u * a.vn_rs);
        acc0 = fmaf(pj, __uint_as_float(w << 16), acc0);
        acc1 = fmaf(pj, __uint_as_float(w & 0xffff0000u), acc1);
        den += pj;
    }
    const float inv = 1.f / den;
    *reinterpret_cast<uint32_t*>(a.o + p * HD + 2 * lane) = pack2bf(acc0 * inv, acc1 * inv);
}

}  // namespace

extern "C" int otter_branch_attn_merge(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                       int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                       const float* o1, const float* lse1, const float* alibi_slopes, void* o, int64_t N, int64_t H, int64_t T,
                                       int64_t rows_per_sentence, int64_t head_dim, float scale, void* stream) {
    static const char name[] = "branch_attn_merge";
    const BranchArgs a = {(const bf16_t*)q, q_row_stride, q_head_stride, (const bf16_t*)k_new, k_new_row_stride, k_new_head_stride,
                          (const bf16_t*)v_new, v_new_row_stride, v_new_head_stride, o1, lse1, alibi_slopes, (bf16_t*)o, N * H,
                          (int)H, (int)T, (int)rows_per_sentence, scale};
    if (int e = require_pointers(name, {q, k_new, v_new, o1, lse1, o})) return e;
    OTTER_REQUIRE(head_dim == HD, "%s: head_dim %ld (%d only)", name, (long)head_dim, HD);
    OTTER_REQUIRE(T >= 1 && T <= T_MAX, "%s: T=%ld outside [1, %d]", name, (long)T, T_MAX);
    OTTER_REQUIRE(N > 0 && H > 0 && H <= 65535 && N <= (int64_t(1) << 31) / H, "%s: bad shape N=%ld H=%ld", name, (long)N, (long)H);
    OTTER_REQUIRE(N % T == 0, "%s: N=%ld rows are not whole candidates of T=%ld", name, (long)N, (long)T);
    OTTER_REQUIRE(rows_per_sentence >= T && rows_per_sentence % T == 0 && N % rows_per_sentence == 0,
                  "%s: rows_per_sentence=%ld must be a multiple of T=%ld that divides N=%ld", name, (long)rows_per_sentence, (long)T, (long)N);
    if (int e = require_aligned16(name, {q, k_new, v_new, o1, o}, "q, k_new, v_new, o1, o")) return e;
    OTTER_REQUIRE((((uintptr_t)lse1 | (uintptr_t)alibi_slopes) & 3) == 0, "%s: lse1, slopes need 4-byte alignment", name);
    OTTER_REQUIRE(mult(8, {q_row_stride, q_head_stride, k_new_row_stride, k_new_head_stride, v_new_row_stride, v_new_head_stride}),
                  "%s: q / k_new / v_new strides must be multiples of 8 elements", name);
    OTTER_REQUIRE(q_row_stride >= 0 && q_head_stride >= 0 && k_new_row_stride >= 0 && k_new_head_stride >= 0 && v_new_row_stride >= 0 &&
                      v_new_head_stride >= 0,
                  "%s: q / k_new / v_new strides must not be negative", name);

    const unsigned blocks = (unsigned)((a.NH + WAVES - 1) / WAVES);
    hipLaunchKernelGGL(branch_attn_merge_kernel, dim3(blocks), dim3(WAVES * OTTER_WAVE), 0, (hipStream_t)stream, a);
    return check_launch(name, "");
}
