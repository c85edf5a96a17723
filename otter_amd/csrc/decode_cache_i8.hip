// decode_cache_i8.hip -- decode_cache.hip's cached generate() step over an INT8 static key / value cache (otter_amd/kv_cache.py:
// StaticKVCache(kv_dtype="int8")), head_dim 128.  A cached vector is 128 int8 codes and one fp32 scale; the step quantises the new token as it
// appends it and dequantises in registers while it attends.  Everything else -- N rows at one position, the beam table `src`, key_valid,
// ALiBi, optional rotary evaluated in fp64 and rounded once, the in-place append at slot `pos` of the row's OWN row, keys < pos read through
// the table, fixed-order reductions, the scalar / device-position pair of entry points -- is decode_cache.hip's, and so is the invariant the
// in-place update rests on: no workgroup reads a slot (codes or scale) that this launch writes.  Scales are per token, so an append never
// rewrites the scale of an earlier position.
//
// THE FORMAT (amax, scale, code, value) is kv_i8_scale / kv_i8_code of csrc/decode_split.h, under its comment there; kv_cache.py states it
// for the project.  DqArgs' fields, the checks of the scales and the launch code are csrc/decode_cached_entry.h's.
//
// The new token is attended in its DEQUANTISED form (codes and scale from LDS), so a step returns what "append, then attend over the cache"
// returns.
//
// Shape: the split-key step of csrc/decode_split.h.  A cached vector is 128 bytes, so an 8-lane group owns one key at a time (lane l8: dims
// 16 l8 .. 16 l8 + 15, one 16-byte load each of K and V codes; the key's two scales are one 4-byte load each, the same address in all 8 lanes),
// 32 groups, two keys per group in flight = 64 keys per iteration: s = k_scale * sum q[i] code_k[i] by an 8-lane butterfly, online softmax per
// group, acc += (p * v_scale) * code_v[i].
#include "decode_cached_entry.h"

namespace {

constexpr int HD = 128, LANES = 8, GROUPS = NT / LANES, KEYS_PER_ITER = GROUPS * UNROLL, DPL = HD / LANES;

struct DqArgs : I8StepArgs {                              // (decode_cached_entry.h: the new token, codes and scales, the tables, o, the ranges)
    float scale;
};

// one workgroup's share of a step: range `split` of row blockIdx.z, head blockIdx.y
__device__ __forceinline__ void decode_cached_i8_body(const DqArgs& a, const int split, const int pos, const int nsplit, const int kps,
                                                      const float* cs_tab, const float* sn_tab) {
    __shared__ float qs[HD];                                        // scale * q'
    __shared__ __attribute__((aligned(16))) int8_t code_new[2][HD]; // the new token's codes: [0] k', [1] v
    __shared__ float scale_new[2], wave_amax[NT / OTTER_WAVE];
    const int h = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const int64_t nh = (int64_t)n * a.H + h;

    // 1. the new token: threads 0..127 own q[d] and v[d] (waves 0, 1), threads 128..255 own k[d] (waves 2, 3).  x = what the bf16 cache
    //    would store; amax over the 128 dims (a max: exact in any order), then divide and round.
    {
        const int d = tid & (HD - 1), which = tid < HD ? 1 : 0;
        const float* cs = cs_tab ? cs_tab + n * a.cs_rs : nullptr;
        const float* sn = cs_tab ? sn_tab + n * a.cs_rs : nullptr;
        float x;
        if (tid < HD) {
            qs[d] = (float)rotated(a.q + n * a.q_rs + h * a.q_hs, cs, sn, d) * a.scale;
            x = bf2f(a.vn[n * a.vn_rs + h * a.vn_hs + d]);
        } else {
            x = bf2f(d2bf(rotated(a.kn + n * a.kn_rs + h * a.kn_hs, cs, sn, d)));
        }
        const float wm = wave_max(fabsf(x));
        if ((tid & (OTTER_WAVE - 1)) == 0) wave_amax[tid / OTTER_WAVE] = wm;
        __syncthreads();
        const float amax = fmaxf(wave_amax[tid < HD ? 0 : 2], wave_amax[tid < HD ? 1 : 3]);
        const float sc = kv_i8_scale(amax);
        const float c = kv_i8_code(x, sc);
        code_new[which][d] = (int8_t)(int)c;
        if (d == 0) scale_new[which] = sc;
    }
    __syncthreads();

    const int l8 = tid & (LANES - 1), g = tid >> 3;
    const int j0 = split * kps, j1 = min(j0 + kps, pos + 1);
    // 2. the append (the workgroup whose range holds `pos`): slot [n, h, pos] of the caller's OWN row -- 8 lanes x 16 bytes each for the K and
    //    the V codes, one lane each for the two scales
    if (pos >= j0 && pos < j1) {
        if (tid < 2 * LANES) {
            int8_t* dst = (tid < LANES ? a.kc + n * a.kc_rs + h * a.kc_hs : a.vc + n * a.vc_rs + h * a.vc_hs) + (int64_t)pos * HD + DPL * l8;
            *reinterpret_cast<Codes<DPL>*>(dst) = *reinterpret_cast<const Codes<DPL>*>(&code_new[tid < LANES ? 0 : 1][DPL * l8]);
        } else if (tid < 2 * LANES + 2) {
            const int w = tid - 2 * LANES;
            float* dst = w == 0 ? a.ks + n * a.ks_rs + h * a.ks_hs : a.vs + n * a.vs_rs + h * a.vs_hs;
            dst[pos] = scale_new[w];
        }
    }

    // 3. the workgroup's key range: scores, online softmax, P V.  Keys j < pos come from the cache (row src[n, j]); key pos from LDS.
    float q[DPL];
#pragma unroll
    for (int i = 0; i < DPL; ++i) q[i] = qs[DPL * l8 + i];
    const int8_t* kb = a.kc + h * a.kc_hs + DPL * l8;
    const int8_t* vb = a.vc + h * a.vc_hs + DPL * l8;
    const float* ksb = a.ks + h * a.ks_hs;
    const float* vsb = a.vs + h * a.vs_hs;
    const int32_t* src = a.src ? a.src + n * a.src_rs : nullptr;
    const uint8_t* kv = a.kvalid ? a.kvalid + n * a.kv_rs : nullptr;
    const float slope = a.slopes ? a.slopes[h] : 0.f;
    float m = -INFINITY, l = 0.f, acc[DPL];
#pragma unroll
    for (int i = 0; i < DPL; ++i) acc[i] = 0.f;
    for (int jb = j0; jb < j1; jb += KEYS_PER_ITER) {
        Codes<DPL> kr[UNROLL], vr[UNROLL];
        float ksc[UNROLL], vsc[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = jb + u * GROUPS + g;
            if (j < j1 && j < pos) {
                // a table entry outside [0, N) is clamped: it can make the result wrong, never an access outside the cache
                const int64_t row = src ? (int64_t)min(max(src[j], 0), a.N - 1) : (int64_t)n;
                kr[u] = *reinterpret_cast<const Codes<DPL>*>(kb + row * a.kc_rs + (int64_t)j * HD);
                vr[u] = *reinterpret_cast<const Codes<DPL>*>(vb + row * a.vc_rs + (int64_t)j * HD);
                ksc[u] = ksb[row * a.ks_rs + j];
                vsc[u] = vsb[row * a.vs_rs + j];
            } else if (j < j1) {                          // j == pos: the new token, as the cache now holds it
                kr[u] = *reinterpret_cast<const Codes<DPL>*>(&code_new[0][DPL * l8]);
                vr[u] = *reinterpret_cast<const Codes<DPL>*>(&code_new[1][DPL * l8]);
                ksc[u] = scale_new[0];
                vsc[u] = scale_new[1];
            } else {
                kr[u] = Codes<DPL>{};
                vr[u] = Codes<DPL>{};
                ksc[u] = 0.f;
                vsc[u] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = jb + u * GROUPS + g;
            const bool live = j < j1;
            float k[DPL], v[DPL];
            unpack_codes(kr[u], k);
            unpack_codes(vr[u], v);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < DPL; ++i) s = fmaf(q[i], k[i], s);
            s = group_sum<LANES>(s);                      // (all lanes: the shuffles stay convergent)
            s = fmaf(s, ksc[u], slope * (float)(j - pos));
            if (!live || (kv && kv[j] == 0)) s = -INFINITY;
            const float mn = fmaxf(m, s);                 // (softmax_update_scaled of decode_split.h, written out; see there)
            if (mn != -INFINITY) {
                const float alpha = __expf(m - mn), p = __expf(s - mn);   // exp(-inf) = 0 for an empty history / a masked key
                const float pv = p * vsc[u];
                l = fmaf(l, alpha, p);
#pragma unroll
                for (int i = 0; i < DPL; ++i) acc[i] = fmaf(acc[i], alpha, pv * v[i]);
                m = mn;
            }
        }
    }

    // 4. the 32 groups, in order (combine_groups of decode_split.h; see there)
    __shared__ float red_m[GROUPS], red_l[GROUPS], red_o[GROUPS][HD];
    if (l8 == 0) { red_m[g] = m; red_l[g] = l; }
#pragma unroll
    for (int i = 0; i < DPL; ++i) red_o[g][DPL * l8 + i] = acc[i];
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
        if (nsplit == 1) {
            a.o[nh * HD + tid] = f2bf(L > 0.f ? O / L : 0.f);
        } else {
            float* pr = a.part + (nh * a.part_stride + split) * PART<HD>;
            if (tid < 2) pr[tid] = tid == 0 ? M : L;
            pr[2 + tid] = O;
        }
    }
}

__global__ __launch_bounds__(NT) void decode_cached_i8_kernel(DqArgs a) {
    decode_cached_i8_body(a, blockIdx.x, a.pos, a.nsplit, a.kps, a.cs, a.sn);
}

// ---- the position in device memory (decode_split.h): grid (max_ranges, H, N) for the capacity --------------------------------------------
__global__ __launch_bounds__(NT) void decode_cached_i8_dyn_kernel(DqArgs a, const int32_t* __restrict__ pos_dev, int S_max, int cus,
                                                                  int64_t table_rs) {
    DYN_POSITION_OR_RETURN(KEYS_PER_ITER, pos, sp, pos_dev, S_max, (int64_t)a.N * a.H, cus);
    if ((int)blockIdx.x >= sp.nsplit) return;
    // row `pos` of the rotary tables, shared by every row (cs_rs = 0)
    decode_cached_i8_body(a, blockIdx.x, pos, sp.nsplit, sp.kps, a.cs ? a.cs + (int64_t)pos * table_rs : nullptr,
                          a.cs ? a.sn + (int64_t)pos * table_rs : nullptr);
}

}  // namespace

// (here the position's check, `pos` or `pos_dev`, follows every check of the layout: the order of this file's entry points since they exist)
extern "C" {

int otter_decode_attn_cached_i8(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                const float* cos_rows, const float* sin_rows, int64_t cos_row_stride, void* k_cache, int64_t k_cache_row_stride,
                                int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride, int64_t v_cache_head_stride,
                                float* k_scale, int64_t k_scale_row_stride, int64_t k_scale_head_stride, float* v_scale,
                                int64_t v_scale_row_stride, int64_t v_scale_head_stride, const int32_t* src, int64_t src_row_stride,
                                const uint8_t* key_valid, int64_t key_valid_row_stride, const float* alibi_slopes, void* o, void* workspace,
                                int64_t workspace_bytes, int64_t N, int64_t H, int64_t pos, int64_t S_max, int64_t head_dim, float scale,
                                void* stream) {
    static const char name[] = "decode_attn_cached_i8";
    DqArgs a = {{{(const bf16_t*)q, q_row_stride, q_head_stride, (const bf16_t*)k_new, k_new_row_stride, k_new_head_stride, (const bf16_t*)v_new,
                  v_new_row_stride, v_new_head_stride, cos_rows, sin_rows, cos_row_stride},
                 (int8_t*)k_cache, k_cache_row_stride, k_cache_head_stride, (int8_t*)v_cache, v_cache_row_stride, v_cache_head_stride,
                 k_scale, k_scale_row_stride, k_scale_head_stride, v_scale, v_scale_row_stride, v_scale_head_stride,
                 src, src_row_stride, key_valid, key_valid_row_stride, alibi_slopes, (bf16_t*)o, (float*)workspace, (int)N, (int)H},
                scale};
    if (int e = require_pointers(name, {q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, o, workspace})) return e;
    if (int e = require_cos_sin_pair(name, cos_rows, sin_rows, "rows")) return e;
    if (int e = require_shape(name, head_dim, HD, N, H)) return e;
    if (int e = require_capacity(name, S_max)) return e;
    if (int e = require_token_and_cache_aligned(name, a)) return e;
    if (int e = require_scales_aligned(name, a)) return e;
    if (int e = require_cache_layout(name, &a, a, 16, S_max, HD)) return e;
    if (int e = require_scale_head_strides(name, a, S_max)) return e;
    if (int e = require_position(name, pos, S_max)) return e;
    if (int e = require_row_strides(name, a, &cos_row_stride, pos)) return e;
    if (int e = require_workspace(name, workspace_bytes, OTTER_DECODE_CACHED_I8_WORKSPACE_BYTES(N, H, pos + 1))) return e;

    return launch_scalar<HD>(name, a, pos, split_rule<KEYS_PER_ITER>(pos + 1, N * H, cu_count()), N, stream,
                             [](dim3 grid, hipStream_t st, const DqArgs& a) { hipLaunchKernelGGL(decode_cached_i8_kernel, grid, dim3(NT), 0, st, a); });
}

int otter_decode_attn_cached_i8_dyn(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                    int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                    const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                    int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                    int64_t v_cache_head_stride, float* k_scale, int64_t k_scale_row_stride, int64_t k_scale_head_stride,
                                    float* v_scale, int64_t v_scale_row_stride, int64_t v_scale_head_stride, const int32_t* src,
                                    int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride, const float* alibi_slopes,
                                    void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, const int32_t* pos_dev,
                                    int64_t S_max, int64_t head_dim, float scale, void* stream) {
    static const char name[] = "decode_attn_cached_i8_dyn";
    DqArgs a = {{{(const bf16_t*)q, q_row_stride, q_head_stride, (const bf16_t*)k_new, k_new_row_stride, k_new_head_stride, (const bf16_t*)v_new,
                  v_new_row_stride, v_new_head_stride, cos_table, sin_table, 0},
                 (int8_t*)k_cache, k_cache_row_stride, k_cache_head_stride, (int8_t*)v_cache, v_cache_row_stride, v_cache_head_stride,
                 k_scale, k_scale_row_stride, k_scale_head_stride, v_scale, v_scale_row_stride, v_scale_head_stride,
                 src, src_row_stride, key_valid, key_valid_row_stride, alibi_slopes, (bf16_t*)o, (float*)workspace, (int)N, (int)H},
                scale};
    if (int e = require_pointers(name, {q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, o, workspace, pos_dev})) return e;
    if (int e = require_cos_sin_pair(name, cos_table, sin_table, "table")) return e;
    if (int e = require_shape(name, head_dim, HD, N, H)) return e;
    if (int e = require_capacity(name, S_max)) return e;
    if (int e = require_token_and_cache_aligned(name, a)) return e;
    if (int e = require_scales_aligned(name, a)) return e;
    if (int e = require_cache_layout(name, &a, a, 16, S_max, HD)) return e;
    if (int e = require_scale_head_strides(name, a, S_max)) return e;
    if (int e = require_pos_dev_aligned(name, pos_dev)) return e;
    if (int e = require_table_strides(name, a, table_row_stride, HD, "128", S_max)) return e;
    if (int e = require_workspace(name, workspace_bytes, OTTER_DECODE_CACHED_I8_DYN_WORKSPACE_BYTES(N, H, S_max))) return e;

    const int cus = cu_count();
    const DynStep d = {pos_dev, (int)S_max, cus, (int)split_max_ranges(S_max, N * H, cus), table_row_stride};
    return launch_dyn(name, a, d, N, stream,
                      [](dim3 grid, hipStream_t st, const DqArgs& a, const DynStep& d) {
                          hipLaunchKernelGGL(decode_cached_i8_dyn_kernel, grid, dim3(NT), 0, st, a, d.pos_dev, d.S_max, d.cus, d.table_rs);
                      },
                      DynCombine<HD, KEYS_PER_ITER>());
}

}  // extern "C"
