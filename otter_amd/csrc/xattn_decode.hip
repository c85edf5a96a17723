// xattn_decode.hip -- the masked cross-attention core of ONE cached generate() step over a media cache (otter_amd/media_cache.py: MediaCache),
// head_dim 64: each of the N rows (batch x beams) has a single query and attends over the projected media of its sentence, which were
// computed once after the prompt pass.  Semantics are those of otter_attn_fwd (csrc/attn.hip) for a Tq = 1 row: masked scores take -FLT_MAX
// (so they add nothing next to an admitted key, and a row whose every key is masked comes out UNIFORM, 1/M over all keys), a row with
// text_time == 0 is zeroed in EQ mode only.  bf16 storage, fp32 arithmetic.
//
// Every case is one CONTIGUOUS key range, because the media index of key j is j / n_per_media and the mask compares it with one number:
//     EQ, 1 <= tt <= T_img      keys [(tt - 1) n, tt n)       -- the n_per_media keys of that media, nothing else is read
//     EQ, tt == 0               no key: o = 0
//     GE, tt >= 1               keys [0, min(tt, T_img) n)
//     every key masked          keys [0, M) with score 0      -- (EQ: tt < 0 or tt > T_img; GE: tt < 1)
//
// Shape: one wave64 per (row, head), four waves per workgroup, no LDS, no workspace, no synchronisation between waves.  The range is walked
// in chunks of 64 keys.  Scores: ONE KEY PER LANE (with the reference's 64 latents an EQ row is exactly one chunk) -- the lane reads its key's
// 64 dims as eight 16-byte loads and the query as eight 16-byte loads of one address (a broadcast); softmax in fp32 with wave reductions, in
// the online form across chunks.  P V: ONE OUTPUT DIM PER LANE -- for each key of the chunk its probability is broadcast from the lane that
// holds it and the 64 lanes read that key's V row as one coalesced 128-byte line.  The order of every sum is fixed: two calls on the same
// inputs give the same bits.
#include "common.h"

#include <math.h>

namespace {

constexpr int HD = 64, WAVES = 4, NT = 64 * WAVES, PV_UNROLL = 16;
constexpr int64_t M_LIMIT = 65536;

struct XdArgs {
    const bf16_t* q; int64_t q_rs;                // [N, H * 64], row stride in elements
    const bf16_t *k, *v; int64_t kv_rs;           // [sentences, M, H * 64] views of one buffer, shared row stride; sentence stride M * kv_rs
    const int32_t* tt;                            // [N]
    bf16_t* o;                                    // [N, H * 64] contiguous
    int64_t pairs;                                // N * H
    int64_t rows_per_media;
    int H, M, n, t_img, mask_mode;
    float scale;
};

__global__ __launch_bounds__(NT) void xattn_decode_kernel(XdArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (pair >= a.pairs) return;                  // (whole waves leave; nothing below synchronises across waves)
    const int64_t r = pair / a.H;
    const int h = (int)(pair - r * a.H);
    bf16_t* op = a.o + r * ((int64_t)a.H * HD) + h * HD + lane;

    // the row's key range [j0, j1) and whether its scores are all zero (every key masked)
    const int tt = a.tt[r];
    int j0 = 0, j1 = a.M;
    bool uniform = false;
    if (a.mask_mode == OTTER_MASK_EQ) {
        if (tt == 0) { *op = 0; return; }         // (bf16 +0)
        if (tt >= 1 && tt <= a.t_img) { j0 = (tt - 1) * a.n; j1 = j0 + a.n; }
        else uniform = true;
    } else {
        if (tt >= 1) j1 = min(tt, a.t_img) * a.n;
        else uniform = true;
    }

    const int64_t sent = r / a.rows_per_media;
    const bf16_t* kb = a.k + sent * a.M * a.kv_rs + h * HD;
    const bf16_t* vb = a.v + sent * a.M * a.kv_rs + h * HD + lane;

    float q[HD];
    if (!uniform) {
        const bf16_t* qp = a.q + r * a.q_rs + h * HD;
#pragma unroll
        for (int c = 0; c < HD / 8; ++c) {
            float t8[8];
            Vec8<bf16_t>::load(qp + 8 * c, t8);
#pragma unroll
            for (int i = 0; i < 8; ++i) q[8 * c + i] = t8[i] * a.scale;
        }
    }

    float m = -INFINITY, l = 0.f, acc = 0.f;      // m, l wave-uniform; acc = output dim `lane`
    for (int jc = j0; jc < j1; jc += 64) {
        const int cnt = min(64, j1 - jc);         // >= 1 keys in this chunk
        const bool live = lane < cnt;
        float s = 0.f;
        if (!uniform) {
            const bf16_t* kp = kb + (int64_t)(jc + (live ? lane : cnt - 1)) * a.kv_rs;   // (a dead lane re-reads the chunk's last key)
#pragma unroll
            for (int c = 0; c < HD / 8; ++c) {
                float t8[8];
                Vec8<bf16_t>::load(kp + 8 * c, t8);
#pragma unroll
                for (int i = 0; i < 8; ++i) s = fmaf(q[8 * c + i], t8[i], s);
            }
        }
        const float mn = fmaxf(m, wave_max(live ? s : -INFINITY));   // finite: the chunk has a live key
        const float alpha = expf(m - mn);                            // (0 for the first chunk)
        const float p = live ? expf(s - mn) : 0.f;
        l = fmaf(l, alpha, wave_sum(p));
        acc *= alpha;
        const bf16_t* vp = vb + (int64_t)jc * a.kv_rs;
        for (int jj = 0; jj < cnt; jj += PV_UNROLL) {
            float vv[PV_UNROLL];
#pragma unroll
            for (int u = 0; u < PV_UNROLL; ++u) vv[u] = jj + u < cnt ? bf2f(vp[(int64_t)(jj + u) * a.kv_rs]) : 0.f;
#pragma unroll
            for (int u = 0; u < PV_UNROLL; ++u) acc = fmaf(__shfl(p, (jj + u) & 63, 64), vv[u], acc);   // (p of a lane >= cnt is 0)
        }
        m = mn;
    }
    *op = f2bf(l > 0.f ? acc / l : 0.f);
}

}  // namespace

extern "C" {

int otter_xattn_decode(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride, const int32_t* text_time, void* o,
                       int64_t N, int64_t H, int64_t T_img, int64_t n_per_media, int64_t rows_per_media, int mask_mode, float scale,
                       void* stream) {
    OTTER_REQUIRE(q && k && v && text_time && o, "xattn_decode: null pointer");
    OTTER_REQUIRE(mask_mode == OTTER_MASK_EQ || mask_mode == OTTER_MASK_GE, "xattn_decode: mask_mode %d (EQ = %d or GE = %d only)", mask_mode,
                  (int)OTTER_MASK_EQ, (int)OTTER_MASK_GE);
    OTTER_REQUIRE(n_per_media >= 1 && T_img >= 1, "xattn_decode: n_per_media=%ld and T_img=%ld must be >= 1", (long)n_per_media, (long)T_img);
    OTTER_REQUIRE(n_per_media <= M_LIMIT && T_img <= M_LIMIT && T_img * n_per_media <= M_LIMIT, "xattn_decode: M = T_img * n_per_media = %ld * %ld exceeds %ld",
                  (long)T_img, (long)n_per_media, (long)M_LIMIT);
    OTTER_REQUIRE(N >= 1 && H >= 1 && H <= 65535 && N <= ((int64_t)1 << 31) / H, "xattn_decode: bad shape N=%ld H=%ld", (long)N, (long)H);
    OTTER_REQUIRE(rows_per_media >= 1 && N % rows_per_media == 0, "xattn_decode: N=%ld is not a multiple of rows_per_media=%ld", (long)N,
                  (long)rows_per_media);
    OTTER_REQUIRE(q_stride % 8 == 0 && kv_stride % 8 == 0, "xattn_decode: q / kv strides must be multiples of 8 elements (q %ld, kv %ld)",
                  (long)q_stride, (long)kv_stride);
    OTTER_REQUIRE(q_stride >= H * HD && kv_stride >= H * HD, "xattn_decode: a row stride below H * 64 (q %ld, kv %ld, H %ld)", (long)q_stride,
                  (long)kv_stride, (long)H);
    OTTER_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0, "xattn_decode: q, k, v need 16-byte alignment");

    XdArgs a;
    a.q = (const bf16_t*)q; a.q_rs = q_stride;
    a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.kv_rs = kv_stride;
    a.tt = text_time; a.o = (bf16_t*)o;
    a.pairs = N * H;
    a.H = (int)H; a.M = (int)(T_img * n_per_media); a.n = (int)n_per_media; a.t_img = (int)T_img; a.rows_per_media = rows_per_media;
    a.mask_mode = mask_mode; a.scale = scale;
    hipLaunchKernelGGL(xattn_decode_kernel, dim3((unsigned)cdiv64(a.pairs, WAVES)), dim3(NT), 0, (hipStream_t)stream, a);
    OTTER_CHECK_LAUNCH("xattn_decode");
    return OTTER_OK;
}

}  // extern "C"
