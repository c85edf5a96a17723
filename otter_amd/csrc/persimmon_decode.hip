// persimmon_decode.hip -- one cached generate() step of the OtterHD / Fuyu-8B (Persimmon) attention, config C5
// (fuyu/modeling_persimmon.py:262-312 with past_key_value, S = 1): q / k LayerNorm over the 64-wide head + partial rotary at position
// S_past, the new key / value appended to the cache, and the single query attending over S_past + 1 keys -- in one read of the past
// cache and one write of the new one.  bf16 storage, fp32 arithmetic (the rotate-half convention and the LayerNorm of
// fuyu.hip's qk_norm_rope_fwd_kernel).
//
// Grid (split, head, batch), 256 threads, the split-key step of csrc/decode_split.h: every workgroup normalises and rotates q (and k) of its
// (batch, head) itself (persimmon_new_token, 128 elements: cheaper than a launch); the keys of a (batch, head) are cut into `nsplit`
// contiguous ranges of `kps` keys by split_rule.  An 8-lane group owns one key at a time (lane l8: dims 8 l8 .. 8 l8 + 7, one 16-byte
// load each of K and V), two keys per group in flight, and stores the K / V row to the new cache from the same registers.
// Masked keys (key_valid == 0) add nothing; a fully masked row gives o = 0, as csrc/decode.hip.
#include "decode_split.h"

namespace {

constexpr int HD = 64, LANES = 8, GROUPS = NT / LANES, KEYS_PER_ITER = GROUPS * UNROLL;

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

__global__ __launch_bounds__(NT) void persimmon_decode_kernel(PdArgs a) {
    __shared__ float qs[HD];                              // scale * bf16(q')
    __shared__ __attribute__((aligned(16))) bf16_t kv_new[2][HD];   // bf16(k') and v of the new token
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int64_t bh = (int64_t)b * a.H + h;

    // 1. the new token
    persimmon_new_token(a.qkv, bh, a.gq, a.bq, a.gk, a.bk, a.cs, a.sn, a.rot, a.eps, a.scale, qs, kv_new);
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
            s = group_sum<LANES>(s);                      // (all lanes: the shuffles stay convergent)
            if (!live || (kv && kv[j] == 0)) s = -INFINITY;
            const Softmax r = softmax_update(m, l, acc, s, v);
            m = r.m;
            l = r.l;
        }
    }

    // 3. the 32 groups, in order
    combine_groups<HD, GROUPS>(g, 8 * l8, m, l, acc, a.o, a.part, bh, bh * a.nsplit + split, a.nsplit);
}

// nsplit > 1: one workgroup of 64 lanes per (head, batch) combines the ranges in order.  The statements of combine_ranges, written out: this
// kernel never had them behind a function, and called through one its compiled branch condition has its two operands the other way round.
__global__ __launch_bounds__(64) void persimmon_decode_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ o, int H, int nsplit) {
    const int64_t bh = (int64_t)blockIdx.y * H + blockIdx.x;
    const int d = threadIdx.x;
    const float* p = part + bh * nsplit * PART<HD>;
    float M = -INFINITY;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, p[s * PART<HD>]);
    float L = 0.f, O = 0.f;
    if (M != -INFINITY) {
        for (int s = 0; s < nsplit; ++s) {
            const float ms = p[s * PART<HD>];
            const float f = ms == -INFINITY ? 0.f : __expf(ms - M);
            L = fmaf(p[s * PART<HD> + 1], f, L);
            O = fmaf(p[s * PART<HD> + 2 + d], f, O);
        }
    }
    o[bh * HD + d] = f2bf(L > 0.f ? O / L : 0.f);
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
    OTTER_REQUIRE(Sk <= S_MAX_LIMIT, "persimmon_decode_attn: S_past + 1 = %ld keys exceeds the limit (%ld)", (long)Sk, (long)S_MAX_LIMIT);
    OTTER_REQUIRE(rot > 0 && rot <= HD && rot % 16 == 0, "persimmon_decode_attn: rot=%ld must be a multiple of 16 in (0, 64]", (long)rot);
    OTTER_REQUIRE(k_dim_stride == 1 && v_dim_stride == 1, "persimmon_decode_attn: k_past / v_past need a unit dim stride");
    OTTER_REQUIRE(k_batch_stride % 8 == 0 && k_head_stride % 8 == 0 && k_key_stride % 8 == 0 && v_batch_stride % 8 == 0 && v_head_stride % 8 == 0 &&
                      v_key_stride % 8 == 0,
                  "persimmon_decode_attn: k_past / v_past strides must be multiples of 8 elements");
    OTTER_REQUIRE((((uintptr_t)qkv | (uintptr_t)k_past | (uintptr_t)v_past | (uintptr_t)k_new | (uintptr_t)v_new) & 15) == 0,
                  "persimmon_decode_attn: qkv, k_past, v_past, k_new, v_new need 16-byte alignment");
    const int64_t need = OTTER_PERSIMMON_DECODE_WORKSPACE_BYTES(B, H, Sk);
    OTTER_REQUIRE(workspace_bytes >= need, "persimmon_decode_attn: workspace of %ld bytes, %ld needed", (long)workspace_bytes, (long)need);

    const Split sp = split_rule<KEYS_PER_ITER>(Sk, B * H, cu_count());
    const int64_t nsplit = sp.nsplit;

    PdArgs a;
    a.qkv = (const bf16_t*)qkv;
    a.gq = gamma_q; a.bq = beta_q; a.gk = gamma_k; a.bk = beta_k; a.cs = cos_row; a.sn = sin_row;
    a.kp = (const bf16_t*)k_past; a.k_bs = k_batch_stride; a.k_hs = k_head_stride; a.k_ss = k_key_stride;
    a.vp = (const bf16_t*)v_past; a.v_bs = v_batch_stride; a.v_hs = v_head_stride; a.v_ss = v_key_stride;
    a.kvalid = key_valid;
    a.kn = (bf16_t*)k_new; a.vn = (bf16_t*)v_new; a.o = (bf16_t*)o; a.part = (float*)workspace;
    a.H = (int)H; a.Sp = (int)S_past; a.Sk = (int)Sk; a.rot = (int)rot; a.nsplit = (int)nsplit; a.kps = sp.kps;
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
