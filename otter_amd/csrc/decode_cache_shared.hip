// decode_cache_shared.hip -- the cached generate() step of csrc/decode_cache.hip for beam search over a SHARED PROMPT (otter_amd/kv_cache.py:
// StaticKVCache.share_prompt), head_dim 128, bf16.  The N rows are sentences x `group` beams, the beams of a sentence contiguous; keys
// [0, shared_len) of every beam are the keys of the sentence's first row (the LEADER, row (n / group) * group), which alone holds them.  The
// result is exactly what otter_decode_attn_cached returns for a table whose columns [0, shared_len) hold (n / group) * group -- but a shared
// key is fetched once per sentence, not once per beam: ONE workgroup serves a (key range, head, sentence) and carries the `group` queries.
//
//   j <  shared_len          one 16-byte load each of K and V from the leader's row, used for all `group` queries; `src` is not read
//   shared_len <= j < pos    per query, through `src` (NULL: the row's own), entries clamped to [0, N) as in decode_cache.hip
//   j == pos                 the workgroup's own copy of each row's new token (LDS -> registers)
//
// Each row appends into its OWN slot [n, h, pos]; key_valid is read per row; ALiBi and the rotary embedding are decode_cache.hip's (rotated()
// in fp64 with one rounding: the stored key is bit-equal to that kernel's).
//
// THE INVARIANT THE IN-PLACE UPDATE RESTS ON is decode_cache.hip's: no workgroup reads a slot that this launch writes.  The writes are slot
// [n, :, pos, :] of every row n; the reads through `src` are of keys j < pos; the shared reads are of the leaders' keys j < shared_len, and
// the entry points require 1 <= shared_len <= pos, so a leader's write (slot pos >= shared_len) never meets a shared read.  (The dyn kernel
// returns when the position it reads is below shared_len, as it does for one outside [1, S_max).)
//
// Shape: the split-key step of csrc/decode_split.h, included unchanged -- grid (key range, head, SENTENCE), 256 threads, 16 groups of 16 lanes,
// one key per group at a time, two in flight, one online softmax per (group, query); the 16 groups and then the ranges are combined in the
// header's fixed orders, query after query.  The ranges come from split_rule with NH = (N / group) * H, on the host (scalar entry) and on the
// device (dyn entry), so the two entries give the same bits at every position, and two calls on the same inputs give the same bits.
// A range, a 32-key iteration or a group's pair of keys may straddle shared_len: an iteration that lies wholly below it takes the shared
// loader for both of its keys at once; every other iteration decides per key.
//
// What this file has in common with its int8 form, decode_cache_shared_i8.hip, is csrc/decode_cached_entry.h's: the checks of the grouping and
// of shared_len, the switch over the group size (for_group) and the dyn combine kernel (shared_dyn_combine_kernel).  The two key loops are not.
#include "decode_cached_entry.h"

namespace {

constexpr int HD = 128, LANES = 16, GROUPS = NT / LANES, KEYS_PER_ITER = GROUPS * UNROLL;

struct DsArgs : Bf16StepArgs {                            // (decode_cached_entry.h; columns < shared_len of `src` are not read)
    int shared_len;
    float scale;
};

// one key of the G queries: its score against each, ALiBi, the rows' masks, one online-softmax update each
template <int G>
__device__ __forceinline__ void shared_key_update(const uint4 (&kr)[G], const uint4 (&vr)[G], const bool one, const float (&q)[G][8], const int j,
                                                  const bool live, const float bias, const uint8_t* (&kv)[G], float (&m)[G], float (&l)[G],
                                                  float (&acc)[G][8]) {
    float k[8], v[8];
    if (one) {
        unpack8(kr[0], k);
        unpack8(vr[0], v);
    }
#pragma unroll
    for (int b = 0; b < G; ++b) {
        if (!one) {
            unpack8(kr[b], k);
            unpack8(vr[b], v);
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s = fmaf(q[b][i], k[i], s);
        s = group_sum<LANES>(s);                          // (all lanes: the shuffles stay convergent)
        s += bias;
        if (!live || (kv[b] && kv[b][j] == 0)) s = -INFINITY;
        const Softmax r = softmax_update(m[b], l[b], acc[b], s, v);
        m[b] = r.m;
        l[b] = r.l;
    }
}

// one workgroup's share of a step: range `split` of the G rows of sentence blockIdx.z, head blockIdx.y
template <int G>
__device__ __forceinline__ void decode_shared_body(const DsArgs& a, const int split, const int pos, const int nsplit, const int kps,
                                                   const float* cs_tab, const float* sn_tab) {
    __shared__ float qs[G][HD];                                        // scale * q'
    __shared__ __attribute__((aligned(16))) bf16_t kv_new[G][2][HD];   // bf16(k') and v of the new tokens
    const int h = blockIdx.y, n0 = blockIdx.z * G, tid = threadIdx.x;  // n0: the leader
    const int shared_len = a.shared_len;

    // 1. the new tokens: threads 0..127 own q[d] and v[d], threads 128..255 own k[d], row after row
    {
        const int d = tid & (HD - 1);
#pragma unroll
        for (int b = 0; b < G; ++b) {
            const int n = n0 + b;
            const float* cs = cs_tab ? cs_tab + n * a.cs_rs : nullptr;
            const float* sn = cs_tab ? sn_tab + n * a.cs_rs : nullptr;
            if (tid < HD) {
                qs[b][d] = (float)rotated(a.q + n * a.q_rs + h * a.q_hs, cs, sn, d) * a.scale;
                kv_new[b][1][d] = a.vn[n * a.vn_rs + h * a.vn_hs + d];
            } else {
                kv_new[b][0][d] = d2bf(rotated(a.kn + n * a.kn_rs + h * a.kn_hs, cs, sn, d));
            }
        }
    }
    __syncthreads();

    const int l16 = tid & (LANES - 1), g = tid >> 4;
    const int j0 = split * kps, j1 = min(j0 + kps, pos + 1);
    // 2. the append (the workgroup whose range holds `pos`): slot [n, h, pos] of every row's OWN row, 32 threads per row x 16 bytes each
    if (pos >= j0 && pos < j1 && tid < 2 * LANES * G) {
        const int b = tid >> 5, n = n0 + b;
        const bool is_k = (tid & 31) < LANES;
        bf16_t* dst = (is_k ? a.kc + n * a.kc_rs + h * a.kc_hs : a.vc + n * a.vc_rs + h * a.vc_hs) + (int64_t)pos * HD + 8 * l16;
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&kv_new[b][is_k ? 0 : 1][8 * l16]);
    }

    // 3. the workgroup's key range: scores, online softmax, P V for the G queries
    float q[G][8];
    const uint8_t* kv[G];
    const int32_t* src[G];
    float m[G], l[G], acc[G][8];
#pragma unroll
    for (int b = 0; b < G; ++b) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            q[b][i] = qs[b][8 * l16 + i];
            acc[b][i] = 0.f;
        }
        kv[b] = a.kvalid ? a.kvalid + (n0 + b) * a.kv_rs : nullptr;
        src[b] = a.src ? a.src + (n0 + b) * a.src_rs : nullptr;
        m[b] = -INFINITY;
        l[b] = 0.f;
    }
    const bf16_t* kb = a.kc + h * a.kc_hs + 8 * l16;
    const bf16_t* vb = a.vc + h * a.vc_hs + 8 * l16;
    const bf16_t* kl = kb + n0 * a.kc_rs;                 // the leader's row
    const bf16_t* vl = vb + n0 * a.vc_rs;
    const float slope = a.slopes ? a.slopes[h] : 0.f;
    for (int jb = j0; jb < j1; jb += KEYS_PER_ITER) {
        if (jb + KEYS_PER_ITER <= shared_len) {
            // the whole iteration is shared (shared_len <= pos < j1: every key is live): both keys in flight, one load for the G queries
            uint4 kr[UNROLL][G], vr[UNROLL][G];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int j = jb + u * GROUPS + g;
                kr[u][0] = *reinterpret_cast<const uint4*>(kl + (int64_t)j * HD);
                vr[u][0] = *reinterpret_cast<const uint4*>(vl + (int64_t)j * HD);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int j = jb + u * GROUPS + g;
                shared_key_update<G>(kr[u], vr[u], true, q, j, true, slope * (float)(j - pos), kv, m, l, acc);
            }
            continue;
        }
        // an iteration that straddles shared_len, lies above it, or ends the range: the loader is chosen key by key
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = jb + u * GROUPS + g;
            uint4 kr[G], vr[G];
            if (j < j1 && j < shared_len) {               // shared: one load (j < shared_len <= pos)
                kr[0] = *reinterpret_cast<const uint4*>(kl + (int64_t)j * HD);
                vr[0] = *reinterpret_cast<const uint4*>(vl + (int64_t)j * HD);
#pragma unroll
                for (int b = 1; b < G; ++b) {
                    kr[b] = kr[0];
                    vr[b] = vr[0];
                }
            } else if (j < j1 && j < pos) {               // own: per query, through the table
#pragma unroll
                for (int b = 0; b < G; ++b) {
                    // a table entry outside [0, N) is clamped: it can make the result wrong, never an access outside the cache
                    const int64_t row = src[b] ? (int64_t)min(max(src[b][j], 0), a.N - 1) : (int64_t)(n0 + b);
                    kr[b] = *reinterpret_cast<const uint4*>(kb + row * a.kc_rs + (int64_t)j * HD);
                    vr[b] = *reinterpret_cast<const uint4*>(vb + row * a.vc_rs + (int64_t)j * HD);
                }
            } else if (j < j1) {                          // j == pos: the new tokens
#pragma unroll
                for (int b = 0; b < G; ++b) {
                    kr[b] = *reinterpret_cast<const uint4*>(&kv_new[b][0][8 * l16]);
                    vr[b] = *reinterpret_cast<const uint4*>(&kv_new[b][1][8 * l16]);
                }
            } else {
#pragma unroll
                for (int b = 0; b < G; ++b) {
                    kr[b] = make_uint4(0, 0, 0, 0);
                    vr[b] = make_uint4(0, 0, 0, 0);
                }
            }
            shared_key_update<G>(kr, vr, false, q, j, j < j1, slope * (float)(j - pos), kv, m, l, acc);
        }
    }

    // 4. the 16 groups, in order, query after query (one set of LDS buffers: a barrier between two queries' combines)
#pragma unroll
    for (int b = 0; b < G; ++b) {
        if (b) __syncthreads();
        const int64_t nh = (int64_t)(n0 + b) * a.H + h;
        combine_groups<HD, GROUPS>(g, 8 * l16, m[b], l[b], acc[b], a.o, a.part, nh, nh * a.part_stride + split, nsplit);
    }
}

template <int G>
__global__ __launch_bounds__(NT) void decode_shared_kernel(DsArgs a) {
    decode_shared_body<G>(a, blockIdx.x, a.pos, a.nsplit, a.kps, a.cs, a.sn);
}

// ---- the position in device memory (decode_split.h): grid (max_ranges, H, N / G) for the capacity ------------------------------------------
template <int G>
__global__ __launch_bounds__(NT) void decode_shared_dyn_kernel(DsArgs a, const int32_t* __restrict__ pos_dev, int S_max, int cus, int64_t table_rs) {
    DYN_POSITION_OR_RETURN(KEYS_PER_ITER, pos, sp, pos_dev, S_max, (int64_t)(a.N / G) * a.H, cus);
    if (pos < a.shared_len) return;                       // (the in-place invariant needs shared_len <= pos: such a counter does nothing)
    if ((int)blockIdx.x >= sp.nsplit) return;
    // row `pos` of the rotary tables, shared by every row (cs_rs = 0)
    decode_shared_body<G>(a, blockIdx.x, pos, sp.nsplit, sp.kps, a.cs ? a.cs + (int64_t)pos * table_rs : nullptr,
                          a.cs ? a.sn + (int64_t)pos * table_rs : nullptr);
}

}  // namespace

// the checks of both entry points are decode_cache.hip's, in its order (the first failing check names the error), with the two checks of the
// grouping after the shape's and the one of shared_len before the alignment's
extern "C" {

int otter_decode_attn_cached_shared(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                    int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                    const float* cos_rows, const float* sin_rows, int64_t cos_row_stride, void* k_cache,
                                    int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                    int64_t v_cache_head_stride, const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid,
                                    int64_t key_valid_row_stride, const float* alibi_slopes, void* o, void* workspace, int64_t workspace_bytes,
                                    int64_t N, int64_t H, int64_t pos, int64_t S_max, int64_t head_dim, float scale, int64_t group,
                                    int64_t shared_len, void* stream) {
    static const char name[] = "decode_attn_cached_shared";
    DsArgs a = {{{(const bf16_t*)q, q_row_stride, q_head_stride, (const bf16_t*)k_new, k_new_row_stride, k_new_head_stride, (const bf16_t*)v_new,
                  v_new_row_stride, v_new_head_stride, cos_rows, sin_rows, cos_row_stride},
                 (bf16_t*)k_cache, k_cache_row_stride, k_cache_head_stride, (bf16_t*)v_cache, v_cache_row_stride, v_cache_head_stride, src,
                 src_row_stride, key_valid, key_valid_row_stride, alibi_slopes, (bf16_t*)o, (float*)workspace, (int)N, (int)H},
                (int)shared_len, scale};
    if (int e = require_pointers(name, {q, k_new, v_new, k_cache, v_cache, o, workspace})) return e;
    if (int e = require_cos_sin_pair(name, cos_rows, sin_rows, "rows")) return e;
    if (int e = require_shape(name, head_dim, HD, N, H)) return e;
    if (int e = require_capacity(name, S_max)) return e;
    if (int e = require_groups(name, N, group)) return e;
    if (int e = require_position(name, pos, S_max)) return e;
    if (int e = require_shared_len(name, shared_len, pos)) return e;
    if (int e = require_token_and_cache_aligned(name, a)) return e;
    if (int e = require_cache_layout(name, &a, a, 8, S_max, HD)) return e;
    if (int e = require_row_strides(name, a, &cos_row_stride, pos)) return e;
    if (int e = require_workspace(name, workspace_bytes, OTTER_DECODE_CACHED_SHARED_WORKSPACE_BYTES(N, H, pos + 1))) return e;

    // nsplit <= ceil((pos + 1) / 128): the workspace holds N * H * nsplit records
    return launch_scalar<HD>(name, a, pos, split_rule<KEYS_PER_ITER>(pos + 1, (N / group) * H, cu_count()), N / group, stream,
                             [group](dim3 grid, hipStream_t st, const DsArgs& a) {
                                 for_group(group, [&](auto G) { hipLaunchKernelGGL(decode_shared_kernel<decltype(G)::value>, grid, dim3(NT), 0, st, a); });
                             });
}

int otter_decode_attn_cached_shared_dyn(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                        int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                        const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                        int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                        int64_t v_cache_head_stride, const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid,
                                        int64_t key_valid_row_stride, const float* alibi_slopes, void* o, void* workspace,
                                        int64_t workspace_bytes, int64_t N, int64_t H, const int32_t* pos_dev, int64_t S_max, int64_t head_dim,
                                        float scale, int64_t group, int64_t shared_len, void* stream) {
    static const char name[] = "decode_attn_cached_shared_dyn";
    DsArgs a = {{{(const bf16_t*)q, q_row_stride, q_head_stride, (const bf16_t*)k_new, k_new_row_stride, k_new_head_stride, (const bf16_t*)v_new,
                  v_new_row_stride, v_new_head_stride, cos_table, sin_table, 0},
                 (bf16_t*)k_cache, k_cache_row_stride, k_cache_head_stride, (bf16_t*)v_cache, v_cache_row_stride, v_cache_head_stride, src,
                 src_row_stride, key_valid, key_valid_row_stride, alibi_slopes, (bf16_t*)o, (float*)workspace, (int)N, (int)H},
                (int)shared_len, scale};
    if (int e = require_pointers(name, {q, k_new, v_new, k_cache, v_cache, o, workspace, pos_dev})) return e;
    if (int e = require_cos_sin_pair(name, cos_table, sin_table, "table")) return e;
    if (int e = require_shape(name, head_dim, HD, N, H)) return e;
    if (int e = require_capacity(name, S_max)) return e;
    if (int e = require_groups(name, N, group)) return e;
    if (int e = require_shared_len_dyn(name, shared_len, S_max)) return e;
    if (int e = require_token_and_cache_aligned(name, a)) return e;
    if (int e = require_pos_dev_aligned(name, pos_dev)) return e;
    if (int e = require_cache_layout(name, &a, a, 8, S_max, HD)) return e;
    if (int e = require_table_strides(name, a, table_row_stride, HD, "128", S_max)) return e;
    if (int e = require_workspace(name, workspace_bytes, OTTER_DECODE_CACHED_SHARED_DYN_WORKSPACE_BYTES(N, H, S_max))) return e;

    const int cus = cu_count();
    const int64_t NH = (N / group) * H;
    // max_ranges <= ceil(S_max / 128): the workspace holds N * H * max_ranges records
    const DynStep d = {pos_dev, (int)S_max, cus, (int)split_max_ranges(S_max, NH, cus), table_row_stride};
    return launch_dyn(name, a, d, N / group, stream,
                      [group](dim3 grid, hipStream_t st, const DsArgs& a, const DynStep& d) {
                          for_group(group, [&](auto G) {
                              hipLaunchKernelGGL(decode_shared_dyn_kernel<decltype(G)::value>, grid, dim3(NT), 0, st, a, d.pos_dev, d.S_max, d.cus, d.table_rs);
                          });
                      },
                      SharedDynCombine<HD, KEYS_PER_ITER>{NH});
}

}  // extern "C"
