// decode_cache.hip -- one cached generate() step over a STATIC key / value cache (otter_amd/kv_cache.py: StaticKVCache), head_dim 128: the
// new key and value are appended in place at slot `pos` of a preallocated cache [row, head, key, 128] and the single query of each of the
// N rows (batch x beams, all at the same position) attends over keys 0..pos -- the keys before `pos` read through a beam indirection table
// (src[n, t] = the cache row that holds sequence n's key / value at position t) instead of a physically reordered cache.  Optional rotary
// embedding of q and k (the rotate_half form of otter_amd/llama.py) and ALiBi (the key-position form of csrc/decode.hip).  bf16 storage,
// fp32 arithmetic; the rotation itself is evaluated in fp64 and rounded ONCE (to bf16 for k, to fp32 for q): the products of a bf16 and an
// fp32 factor are exact there, so the stored key is the correctly rounded rotation, not one of two neighbours.
//
// THE INVARIANT THE IN-PLACE UPDATE RESTS ON: no workgroup reads a slot that this launch writes.  Row n writes slot [n, :, pos, :] only
// (one workgroup per (n, h): the one whose key range contains `pos`); every read of the cache is of a key j < pos (through `src`, of any row);
// key `pos` itself is taken from the workgroup's own copy of the new token (LDS -> registers), never from the cache.  So no ordering between
// workgroups is needed, and a table that points several rows at one ancestor is fine.  Anything that made a workgroup read slot `pos` of
// another row (e.g. attending to pos of a sibling beam) would break this.
//
// Shape: the split-key step of csrc/decode_split.h -- grid (key range, head, row), 256 threads, online softmax per group, fixed-order combines
// of the groups and of the ranges.  A 16-lane group owns one key at a time (lane l16: dims 8 l16 .. 8 l16 + 7, one 16-byte load each of K
// and V), 16 groups, two keys per group in flight.
//
// Two entry points share every line of arithmetic.  otter_decode_attn_cached takes `pos` as a scalar and sizes its grid from it.
// otter_decode_attn_cached_dyn reads `pos` from device memory and launches a grid sized for the cache's CAPACITY: nothing in its launch
// depends on the position, so a captured graph of it can be replayed step after step.  Both derive the key ranges of a position from
// split_rule (host and device); a workgroup of the dyn grid whose range index is not live at the current position returns before it touches
// memory, and the combine kernel merges exactly the live ranges -- so at every position the two entry points give the same bits.
#include "decode_cached_entry.h"

namespace {

constexpr int HD = 128, LANES = 16, GROUPS = NT / LANES, KEYS_PER_ITER = GROUPS * UNROLL;

struct DcArgs : Bf16StepArgs {                            // (decode_cached_entry.h: the new token, the cache, the tables, o, the ranges)
    float scale;
};

// one workgroup's share of a step: range `split` of row blockIdx.z, head blockIdx.y
__device__ __forceinline__ void decode_cached_body(const DcArgs& a, const int split, const int pos, const int nsplit, const int kps,
                                                   const float* cs_tab, const float* sn_tab) {
    __shared__ float qs[HD];                                        // scale * q'
    __shared__ __attribute__((aligned(16))) bf16_t kv_new[2][HD];   // bf16(k') and v of the new token
    const int h = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const int64_t nh = (int64_t)n * a.H + h;

    // 1. the new token: threads 0..127 own q[d] and v[d], threads 128..255 own k[d]
    {
        const int d = tid & (HD - 1);
        const float* cs = cs_tab ? cs_tab + n * a.cs_rs : nullptr;
        const float* sn = cs_tab ? sn_tab + n * a.cs_rs : nullptr;
        if (tid < HD) {
            qs[d] = (float)rotated(a.q + n * a.q_rs + h * a.q_hs, cs, sn, d) * a.scale;
            kv_new[1][d] = a.vn[n * a.vn_rs + h * a.vn_hs + d];
        } else {
            kv_new[0][d] = d2bf(rotated(a.kn + n * a.kn_rs + h * a.kn_hs, cs, sn, d));
        }
    }
    __syncthreads();

    const int l16 = tid & (LANES - 1), g = tid >> 4;
    const int j0 = split * kps, j1 = min(j0 + kps, pos + 1);
    // 2. the append (the workgroup whose range holds `pos`): slot [n, h, pos] of the caller's OWN row, 16 lanes x 16 bytes each for K and V
    if (pos >= j0 && pos < j1 && tid < 2 * LANES) {
        bf16_t* dst = (tid < LANES ? a.kc + n * a.kc_rs + h * a.kc_hs : a.vc + n * a.vc_rs + h * a.vc_hs) + (int64_t)pos * HD + 8 * l16;
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&kv_new[tid < LANES ? 0 : 1][8 * l16]);
    }

    // 3. the workgroup's key range: scores, online softmax, P V.  Keys j < pos come from the cache (row src[n, j]); key pos from kv_new.
    float q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = qs[8 * l16 + i];
    const bf16_t* kb = a.kc + h * a.kc_hs + 8 * l16;
    const bf16_t* vb = a.vc + h * a.vc_hs + 8 * l16;
    const int32_t* src = a.src ? a.src + n * a.src_rs : nullptr;
    const uint8_t* kv = a.kvalid ? a.kvalid + n * a.kv_rs : nullptr;
    const float slope = a.slopes ? a.slopes[h] : 0.f;
    float m = -INFINITY, l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int jb = j0; jb < j1; jb += KEYS_PER_ITER) {
        uint4 kr[UNROLL], vr[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = jb + u * GROUPS + g;
            if (j < j1 && j < pos) {
                // a table entry outside [0, N) is clamped: it can make the result wrong, never an access outside the cache
                const int64_t row = src ? (int64_t)min(max(src[j], 0), a.N - 1) : (int64_t)n;
                kr[u] = *reinterpret_cast<const uint4*>(kb + row * a.kc_rs + (int64_t)j * HD);
                vr[u] = *reinterpret_cast<const uint4*>(vb + row * a.vc_rs + (int64_t)j * HD);
            } else if (j < j1) {                          // j == pos: the new token
                kr[u] = *reinterpret_cast<const uint4*>(&kv_new[0][8 * l16]);
                vr[u] = *reinterpret_cast<const uint4*>(&kv_new[1][8 * l16]);
            } else {
                kr[u] = make_uint4(0, 0, 0, 0);
                vr[u] = make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = jb + u * GROUPS + g;
            const bool live = j < j1;
            float k[8], v[8];
            unpack8(kr[u], k);
            unpack8(vr[u], v);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s = fmaf(q[i], k[i], s);
            s = group_sum<LANES>(s);                      // (all lanes: the shuffles stay convergent)
            s += slope * (float)(j - pos);
            if (!live || (kv && kv[j] == 0)) s = -INFINITY;
            const Softmax r = softmax_update(m, l, acc, s, v);
            m = r.m;
            l = r.l;
        }
    }

    // 4. the 16 groups, in order
    combine_groups<HD, GROUPS>(g, 8 * l16, m, l, acc, a.o, a.part, nh, nh * a.part_stride + split, nsplit);
}

__global__ __launch_bounds__(NT) void decode_cached_kernel(DcArgs a) {
    decode_cached_body(a, blockIdx.x, a.pos, a.nsplit, a.kps, a.cs, a.sn);
}

// ---- the position in device memory (decode_split.h): grid (max_ranges, H, N) for the capacity --------------------------------------------
__global__ __launch_bounds__(NT) void decode_cached_dyn_kernel(DcArgs a, const int32_t* __restrict__ pos_dev, int S_max, int cus, int64_t table_rs) {
    DYN_POSITION_OR_RETURN(KEYS_PER_ITER, pos, sp, pos_dev, S_max, (int64_t)a.N * a.H, cus);
    if ((int)blockIdx.x >= sp.nsplit) return;
    // row `pos` of the rotary tables, shared by every row (cs_rs = 0)
    decode_cached_body(a, blockIdx.x, pos, sp.nsplit, sp.kps, a.cs ? a.cs + (int64_t)pos * table_rs : nullptr,
                       a.cs ? a.sn + (int64_t)pos * table_rs : nullptr);
}

}  // namespace

// (the order of the checks is ABI: the scalar entry point checks `pos` before the alignment checks, the dyn one `pos_dev` between the
// alignment and the stride checks -- decode_cached_entry.h)
extern "C" {

int otter_decode_attn_cached(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                             int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                             const float* cos_rows, const float* sin_rows, int64_t cos_row_stride, void* k_cache, int64_t k_cache_row_stride,
                             int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride, int64_t v_cache_head_stride,
                             const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride,
                             const float* alibi_slopes, void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, int64_t pos,
                             int64_t S_max, int64_t head_dim, float scale, void* stream) {
    static const char name[] = "decode_attn_cached";
    DcArgs a = {{{(const bf16_t*)q, q_row_stride, q_head_stride, (const bf16_t*)k_new, k_new_row_stride, k_new_head_stride, (const bf16_t*)v_new,
                  v_new_row_stride, v_new_head_stride, cos_rows, sin_rows, cos_row_stride},
                 (bf16_t*)k_cache, k_cache_row_stride, k_cache_head_stride, (bf16_t*)v_cache, v_cache_row_stride, v_cache_head_stride, src,
                 src_row_stride, key_valid, key_valid_row_stride, alibi_slopes, (bf16_t*)o, (float*)workspace, (int)N, (int)H},
                scale};
    if (int e = require_pointers(name, {q, k_new, v_new, k_cache, v_cache, o, workspace})) return e;
    if (int e = require_cos_sin_pair(name, cos_rows, sin_rows, "rows")) return e;
    if (int e = require_shape(name, head_dim, HD, N, H)) return e;
    if (int e = require_capacity(name, S_max)) return e;
    if (int e = require_position(name, pos, S_max)) return e;
    if (int e = require_token_and_cache_aligned(name, a)) return e;
    if (int e = require_cache_layout(name, &a, a, 8, S_max, HD)) return e;
    if (int e = require_row_strides(name, a, &cos_row_stride, pos)) return e;
    if (int e = require_workspace(name, workspace_bytes, OTTER_DECODE_CACHED_WORKSPACE_BYTES(N, H, pos + 1))) return e;

    return launch_scalar<HD>(name, a, pos, split_rule<KEYS_PER_ITER>(pos + 1, N * H, cu_count()), N, stream,
                             [](dim3 grid, hipStream_t st, const DcArgs& a) { hipLaunchKernelGGL(decode_cached_kernel, grid, dim3(NT), 0, st, a); });
}

int otter_decode_attn_cached_dyn(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                 int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                 const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                 int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                 int64_t v_cache_head_stride, const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid,
                                 int64_t key_valid_row_stride, const float* alibi_slopes, void* o, void* workspace, int64_t workspace_bytes,
                                 int64_t N, int64_t H, const int32_t* pos_dev, int64_t S_max, int64_t head_dim, float scale, void* stream) {
    static const char name[] = "decode_attn_cached_dyn";
    DcArgs a = {{{(const bf16_t*)q, q_row_stride, q_head_stride, (const bf16_t*)k_new, k_new_row_stride, k_new_head_stride, (const bf16_t*)v_new,
                  v_new_row_stride, v_new_head_stride, cos_table, sin_table, 0},
                 (bf16_t*)k_cache, k_cache_row_stride, k_cache_head_stride, (bf16_t*)v_cache, v_cache_row_stride, v_cache_head_stride, src,
                 src_row_stride, key_valid, key_valid_row_stride, alibi_slopes, (bf16_t*)o, (float*)workspace, (int)N, (int)H},
                scale};
    if (int e = require_pointers(name, {q, k_new, v_new, k_cache, v_cache, o, workspace, pos_dev})) return e;
    if (int e = require_cos_sin_pair(name, cos_table, sin_table, "table")) return e;
    if (int e = require_shape(name, head_dim, HD, N, H)) return e;
    if (int e = require_capacity(name, S_max)) return e;
    if (int e = require_token_and_cache_aligned(name, a)) return e;
    if (int e = require_pos_dev_aligned(name, pos_dev)) return e;
    if (int e = require_cache_layout(name, &a, a, 8, S_max, HD)) return e;
    if (int e = require_table_strides(name, a, table_row_stride, HD, "128", S_max)) return e;
    if (int e = require_workspace(name, workspace_bytes, OTTER_DECODE_CACHED_DYN_WORKSPACE_BYTES(N, H, S_max))) return e;

    const int cus = cu_count();
    const DynStep d = {pos_dev, (int)S_max, cus, (int)split_max_ranges(S_max, N * H, cus), table_row_stride};
    return launch_dyn(name, a, d, N, stream,
                      [](dim3 grid, hipStream_t st, const DcArgs& a, const DynStep& d) {
                          hipLaunchKernelGGL(decode_cached_dyn_kernel, grid, dim3(NT), 0, st, a, d.pos_dev, d.S_max, d.cus, d.table_rs);
                      },
                      DynCombine<HD, KEYS_PER_ITER>());
}

}  // extern "C"
