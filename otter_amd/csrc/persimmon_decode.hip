// persimmon_decode.hip -- one cached generate() step of the OtterHD / Fuyu-8B (Persimmon) attention, config C5
// (fuyu/modeling_persimmon.py:262-312 with past_key_value, S = 1): q / k LayerNorm over the 64-wide head + partial rotary at position
// S_past, the new key / value appended to the cache, and the single query attending over S_past + 1 keys -- in one read of the past
// cache and one write of the new one.  bf16 storage, fp32 arithmetic (the rotate-half convention and the LayerNorm of
// fuyu.hip's qk_norm_rope_fwd_kernel).
//
// Grid (split, head, batch), 256 threads.  Every workgroup normalises and rotates q (and k) of its (batch, head) itself (128 elements:
// cheaper than a launch); the keys of a (batch, head) are cut into `nsplit` contiguous ranges of `kps` keys (flash-decoding), sized so
// that B * H * nsplit is about two workgroups per CU of the device the call runs on, with at least 128 keys per range.
// Inside a workgroup an 8-lane group owns one key at a time (lane l8: dims 8 l8 .. 8 l8 + 7, one 16-byte load each of K and V), two
// keys per group in flight: score by an 8-lane butterfly, online softmax per group (running max m, sum l, o[8]), and the K / V row
// stored to the new cache from the same registers.  The 32 groups are combined through LDS in a fixed order; with nsplit > 1 each
// workgroup writes (m, l, o[64]) to the workspace and a second kernel combines the ranges, again in a fixed order: deterministic.
// Masked keys (key_valid == 0) add nothing; a fully masked row gives o = 0, as csrc/decode.hip.
#include "common.h"

namespace {

constexpr int HD = 64, NT = 256, GROUPS = NT / 8, UNROLL = 2, KEYS_PER_ITER = GROUPS * UNROLL;
constexpr int MIN_KEYS_PER_SPLIT = 128, PART = 2 + HD;   // workspace record per (batch, head, range): m, l, o[64]
constexpr int64_t SK_MAX = 65536;

struct PdArgs {
    const bf16_t* qkv;                                    // [B, H, 3, 64] contiguous: q | k | v of the new token, per head
    const float *gq, *bq, *gk, *bk, *cs, *sn;             // LayerNorm gamma / beta [64]; cos / sin of position S_past [rot]
    const bf16_t* kp; int64_t k_bs, k_hs, k_ss;           // past K [B, H, S_past, 64]: batch / head / key strides, dim stride 1
    const bf16_t* vp; int64_t v_bs, v_hs, v_ss;
    const uint8_t* kvalid;                                // [B, Sk] or null
    bf16_t* kn; bf16_t* vn;                               // new cache [B, H, Sk, 64] contiguous
    bf16_t* o;                                            // [B, H * 64]
    float* part;                                          // [B * H * nsplit, PART] (nsplit > 1)
    int H, Sp, Sk, rot, nsplit, kps;
    float eps, scale;
};

__device__ __forceinline__ float group8_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

__device__ __forceinline__ void unpack8(const uint4& r, float (&v)[8]) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(w[i] << 16);
        v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}

__global__ __launch_bounds__(NT) void persimmon_decode_kernel(PdArgs a) {
    __shared__ float qs[HD];                              // scale * bf16(q')
    __shared__ __attribute__((aligned(16))) bf16_t kv_new[2][HD];   // bf16(k') and v of the new token
    __shared__ float red_m[GROUPS], red_l[GROUPS], red_o[GROUPS][HD];
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int64_t bh = (int64_t)b * a.H + h;

    // 1. wave w < 3 owns vector w of the new token (q, k, v), one element per lane
    const int w = tid >> 6, lane = tid & 63;
    if (w < 3) {
        float x = bf2f(a.qkv[(bh * 3 + w) * HD + lane]);
        if (w < 2) {
            const float mean = wave_sum(x) * (1.0f / HD);
            const float dx = x - mean;
            const float rstd = rsqrtf(wave_sum(dx * dx) * (1.0f / HD) + a.eps);
            x = dx * rstd * (w ? a.gk : a.gq)[lane] + (w ? a.bk : a.bq)[lane];
            // rotate-half on the first `rot` dims: y1 = x1 c - x2 s, y2 = x2 c + x1 s
            const int half = a.rot >> 1;
            const bool in_rot = lane < a.rot, first = lane < half;
            const float xp = __shfl(x, in_rot ? (first ? lane + half : lane - half) : lane, 64);
            if (in_rot) x = x * a.cs[lane] + (first ? -xp : xp) * a.sn[lane];
        }
        const bf16_t xb = f2bf(x);
        if (w == 0) qs[lane] = bf2f(xb) * a.scale;
        else kv_new[w - 1][lane] = xb;
    }
    __syncthreads();

    // 2. the workgroup's key range: scores, online softmax, P V, and the copy into the new cache
    const int l8 = tid & 7, g = tid >> 3;
    float q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = qs[8 * l8 + i];
    const int j0 = split * a.kps, j1 = min(j0 + a.kps, a.Sk);
    const bf16_t* kb = a.kp + b * a.k_bs + h * a.k_hs + 8 * l8;
    const bf16_t* vb = a.vp + b * a.v_bs + h * a.v_hs + 8 * l8;
    bf16_t* knb = a.kn + bh * a.Sk * HD + 8 * l8;
    bf16_t* vnb = a.vn + bh * a.Sk * HD + 8 * l8;
    const uint8_t* kv = a.kvalid ? a.kvalid + (int64_t)b * a.Sk : nullptr;
    float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int jb = j0; jb < j1; jb += KEYS_PER_ITER) {
        uint4 kr[UNROLL], vr[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = jb + u * GROUPS + g;
            if (j < j1 && j < a.Sp) {
                kr[u] = *reinterpret_cast<const uint4*>(kb + (int64_t)j * a.k_ss);
                vr[u] = *reinterpret_cast<const uint4*>(vb + (int64_t)j * a.v_ss);
            } else if (j < j1) {                          // j == S_past: the new token
                kr[u] = *reinterpret_cast<const uint4*>(&kv_new[0][8 * l8]);
                vr[u] = *reinterpret_cast<const uint4*>(&kv_new[1][8 * l8]);
            } else {
                kr[u] = make_uint4(0, 0, 0, 0);
                vr[u] = make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = jb + u * GROUPS + g;
            const bool live = j < j1;
            if (live) {
                *reinterpret_cast<uint4*>(knb + (int64_t)j * HD) = kr[u];
                *reinterpret_cast<uint4*>(vnb + (int64_t)j * HD) = vr[u];
            }
            float k[8], v[8];
            unpack8(kr[u], k);
            unpack8(vr[u], v);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s = fmaf(q[i], k[i], s);
            s = group8_sum(s);                            // (all lanes: the shuffles stay convergent)
            if (!live || (kv && kv[j] == 0)) s = -INFINITY;
            const float mn = fmaxf(m, s);
            if (mn != -INFINITY) {
                const float alpha = __expf(m - mn), p = __expf(s - mn);   // exp(-inf) = 0 for an empty history / a masked key
                l = fmaf(l, alpha, p);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = fmaf(acc[i], alpha, p * v[i]);
                m = mn;
            }
        }
    }

    // 3. the 32 groups, in order
    if (l8 == 0) { red_m[g] = m; red_l[g] = l; }
#pragma unroll
    for (int i = 0; i < 8; ++i) red_o[g][8 * l8 + i] = acc[i];
    __syncthreads();
    if (tid < HD) {
        float M = -INFINITY;
        for (int gg = 0; gg < GROUPS; ++gg) M = fmaxf(M, red_m[gg]);
        float L = 0.f, O = 0.f;
        if (M != -INFINITY) {
            for (int gg = 0; gg < GROUPS; ++gg) {
                const float f = red_m[gg] == -INFINITY ? 0.f : __expf(red_m[gg] - M);
                L = fmaf(red_l[gg], f, L);
                O = fmaf(red_o[gg][tid], f, O);
            }
        }
        if (a.nsplit == 1) {
            a.o[bh * HD + tid] = f2bf(L > 0.f ? O / L : 0.f);
        } else {
            float* pr = a.part + (bh * a.nsplit + split) * PART;
            if (tid < 2) pr[tid] = tid == 0 ? M : L;
            pr[2 + tid] = O;
        }
    }
}

// nsplit > 1: one workgroup of 64 lanes per (head, batch) combines the ranges in order
__global__ __launch_bounds__(64) void persimmon_decode_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ o, int H, int nsplit) {
    const int64_t bh = (int64_t)blockIdx.y * H + blockIdx.x;
    const int d = threadIdx.x;
    const float* p = part + bh * nsplit * PART;
    float M = -INFINITY;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, p[s * PART]);
    float L = 0.f, O = 0.f;
    if (M != -INFINITY) {
        for (int s = 0; s < nsplit; ++s) {
            const float ms = p[s * PART];
            const float f = ms == -INFINITY ? 0.f : __expf(ms - M);
            L = fmaf(p[s * PART + 1], f, L);
            O = fmaf(p[s * PART + 2 + d], f, O);
        }
    }
    o[bh * HD + d] = f2bf(L > 0.f ? O / L : 0.f);
}

int cu_count() {
    static int counts[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (counts[dev] == 0) {
        int n = 0;
        counts[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    return counts[dev];
}

}  // namespace

extern "C" {

int otter_persimmon_decode_attn(const void* qkv, const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k,
                                const float* cos_row, const float* sin_row, const void* k_past, int64_t k_batch_stride, int64_t k_head_stride,
                                int64_t k_key_stride, int64_t k_dim_stride, const void* v_past, int64_t v_batch_stride, int64_t v_head_stride,
                                int64_t v_key_stride, int64_t v_dim_stride, const uint8_t* key_valid, void* k_new, void* v_new, void* o,
                                void* workspace, int64_t workspace_bytes, int64_t B, int64_t H, int64_t S_past, int64_t head_dim, int64_t rot,
                                float eps, float scale, void* stream) {
    OTTER_REQUIRE(qkv && gamma_q && beta_q && gamma_k && beta_k && cos_row && sin_row && k_past && v_past && k_new && v_new && o && workspace,
                  "persimmon_decode_attn: null pointer");
    OTTER_REQUIRE(head_dim == HD, "persimmon_decode_attn: head_dim %ld (64 only)", (long)head_dim);
    OTTER_REQUIRE(B > 0 && H > 0 && S_past > 0 && B <= 65535 && H <= 65535, "persimmon_decode_attn: bad shape B=%ld H=%ld S_past=%ld", (long)B,
                  (long)H, (long)S_past);
    const int64_t Sk = S_past + 1;
    OTTER_REQUIRE(Sk <= SK_MAX, "persimmon_decode_attn: S_past + 1 = %ld keys exceeds the limit (%ld)", (long)Sk, (long)SK_MAX);
    OTTER_REQUIRE(rot > 0 && rot <= HD && rot % 16 == 0, "persimmon_decode_attn: rot=%ld must be a multiple of 16 in (0, 64]", (long)rot);
    OTTER_REQUIRE(k_dim_stride == 1 && v_dim_stride == 1, "persimmon_decode_attn: k_past / v_past need a unit dim stride");
    OTTER_REQUIRE(k_batch_stride % 8 == 0 && k_head_stride % 8 == 0 && k_key_stride % 8 == 0 && v_batch_stride % 8 == 0 && v_head_stride % 8 == 0 &&
                      v_key_stride % 8 == 0,
                  "persimmon_decode_attn: k_past / v_past strides must be multiples of 8 elements");
    OTTER_REQUIRE((((uintptr_t)qkv | (uintptr_t)k_past | (uintptr_t)v_past | (uintptr_t)k_new | (uintptr_t)v_new) & 15) == 0,
                  "persimmon_decode_attn: qkv, k_past, v_past, k_new, v_new need 16-byte alignment");
    const int64_t need = OTTER_PERSIMMON_DECODE_WORKSPACE_BYTES(B, H, Sk);
    OTTER_REQUIRE(workspace_bytes >= need, "persimmon_decode_attn: workspace of %ld bytes, %ld needed", (long)workspace_bytes, (long)need);

    // split rule: about two workgroups per CU over all (batch, head, range), at least MIN_KEYS_PER_SPLIT keys per range
    const int64_t want = cdiv64(2 * (int64_t)cu_count(), B * H);
    int64_t kps = cdiv64(Sk, want > 0 ? want : 1);
    if (kps < MIN_KEYS_PER_SPLIT) kps = MIN_KEYS_PER_SPLIT;
    kps = cdiv64(kps, KEYS_PER_ITER) * KEYS_PER_ITER;
    const int64_t nsplit = cdiv64(Sk, kps);

    PdArgs a;
    a.qkv = (const bf16_t*)qkv;
    a.gq = gamma_q; a.bq = beta_q; a.gk = gamma_k; a.bk = beta_k; a.cs = cos_row; a.sn = sin_row;
    a.kp = (const bf16_t*)k_past; a.k_bs = k_batch_stride; a.k_hs = k_head_stride; a.k_ss = k_key_stride;
    a.vp = (const bf16_t*)v_past; a.v_bs = v_batch_stride; a.v_hs = v_head_stride; a.v_ss = v_key_stride;
    a.kvalid = key_valid;
    a.kn = (bf16_t*)k_new; a.vn = (bf16_t*)v_new; a.o = (bf16_t*)o; a.part = (float*)workspace;
    a.H = (int)H; a.Sp = (int)S_past; a.Sk = (int)Sk; a.rot = (int)rot; a.nsplit = (int)nsplit; a.kps = (int)kps;
    a.eps = eps; a.scale = scale;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(persimmon_decode_kernel, dim3((unsigned)nsplit, (unsigned)H, (unsigned)B), dim3(NT), 0, st, a);
    OTTER_CHECK_LAUNCH("persimmon_decode_attn");
    if (nsplit > 1) {
        hipLaunchKernelGGL(persimmon_decode_combine_kernel, dim3((unsigned)H, (unsigned)B), dim3(64), 0, st, (const float*)workspace, (bf16_t*)o,
                           (int)H, (int)nsplit);
        OTTER_CHECK_LAUNCH("persimmon_decode_attn (combine)");
    }
    return OTTER_OK;
}

}  // extern "C"
