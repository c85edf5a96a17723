// persimmon_decode_cache.hip -- one cached generate() step of the OtterHD / Fuyu-8B (Persimmon) attention over a STATIC key / value cache
// (otter_amd/kv_cache.py: StaticKVCache), head_dim 64.  It is to csrc/persimmon_decode.hip what csrc/decode_cache.hip is to csrc/decode.hip:
// the new key and value are appended in place at slot `pos` of a preallocated cache [row, head, key, 64] and the single query of each of the
// N rows (batch x beams, all at the same position) attends over keys 0..pos -- the keys before `pos` read through a beam indirection table
// (src[n, t] = the cache row that holds sequence n's key / value at position t) instead of a physically reordered cache.
//
// THE ARITHMETIC IS THAT OF persimmon_decode_kernel: the new token by the same persimmon_new_token, the same 8-lane groups (lane l8: dims
// 8 l8 .. 8 l8 + 7, one 16-byte load each of K and V), 32 groups, two keys per group in flight, and the online softmax, the combines and
// the split rule of csrc/decode_split.h.  NOT csrc/decode_cache.hip's fp64 one-rounding rotation: on the same inputs `o` and the stored k'
// are bit-identical to otter_persimmon_decode_attn's `o` and k_new[:, :, S_past], so the static cache returns the tokens of the default cache.
//
// THE INVARIANT THE IN-PLACE UPDATE RESTS ON (csrc/decode_cache.hip, unchanged): no workgroup reads a slot that this launch writes.  Row n
// writes slot [n, :, pos, :] only (one workgroup per (n, h): the one whose key range contains `pos`); every read of the cache is of a key
// j < pos (through `src`, of any row); key `pos` itself is taken from the workgroup's own copy of the new token (LDS -> registers), never
// from the cache.  So no ordering between workgroups is needed, and a table that points several rows at one ancestor is fine.  v is stored
// raw.
//
// Two entry points share every line of arithmetic (persimmon_cached_body).  otter_persimmon_decode_attn_cached takes `pos` as a scalar and
// sizes its grid from it.  otter_persimmon_decode_attn_cached_dyn reads `pos` from device memory and launches a grid sized for the cache's
// CAPACITY: nothing in its launch depends on the position, so a captured graph of it can be replayed step after step.  Both derive the key
// ranges of a position from split_rule (host and device); a workgroup of the dyn grid whose range index is not live at the current position
// returns before it touches memory, and the combine kernel merges exactly the live ranges -- at every position the two give the same bits.
#include "decode_cached_entry.h"

namespace {

constexpr int HD = 64, LANES = 8, GROUPS = NT / LANES, KEYS_PER_ITER = GROUPS * UNROLL;

struct PcArgs {
    const bf16_t* qkv;                                    // [N, H, 3, 64] contiguous: q | k | v of the new token, per head
    const float *gq, *bq, *gk, *bk, *cs, *sn;             // LayerNorm gamma / beta [64]; cos / sin: the row of `pos` [rot] (dyn: the tables)
    bf16_t* kc; int64_t kc_rs, kc_hs;                     // cache [row, h, key, 64]: row / head strides, key stride 64
    bf16_t* vc; int64_t vc_rs, vc_hs;
    const int32_t* src; int64_t src_rs;                   // [N, >= pos] or null (= the row's own)
    const uint8_t* kvalid; int64_t kv_rs;                 // [N, >= pos + 1] or null
    bf16_t* o;                                            // [N, H * 64]
    float* part;                                          // [N * H * part_stride, PART] (nsplit > 1), part_stride >= nsplit
    int N, H, pos, rot, nsplit, kps, part_stride;
    float eps, scale;
};

// one workgroup's share of a step: range `split` of row blockIdx.z, head blockIdx.y; cs / sn = the rotary row of `pos`
__device__ __forceinline__ void persimmon_cached_body(const PcArgs& a, const int split, const int pos, const int nsplit, const int kps,
                                                      const float* cs, const float* sn) {
    __shared__ float qs[HD];                              // scale * bf16(q')
    __shared__ __attribute__((aligned(16))) bf16_t kv_new[2][HD];   // bf16(k') and v of the new token
    const int h = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const int64_t nh = (int64_t)n * a.H + h;

    // 1. the new token
    persimmon_new_token(a.qkv, nh, a.gq, a.bq, a.gk, a.bk, cs, sn, a.rot, a.eps, a.scale, qs, kv_new);
    __syncthreads();

    const int l8 = tid & 7, g = tid >> 3;
    const int j0 = split * kps, j1 = min(j0 + kps, pos + 1);
    // 2. the append (the workgroup whose range holds `pos`): slot [n, h, pos] of the caller's OWN row, 8 lanes x 16 bytes each for K and V
    if (pos >= j0 && pos < j1 && tid < 16) {
        bf16_t* dst = (tid < 8 ? a.kc + n * a.kc_rs + h * a.kc_hs : a.vc + n * a.vc_rs + h * a.vc_hs) + (int64_t)pos * HD + 8 * l8;
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&kv_new[tid < 8 ? 0 : 1][8 * l8]);
    }

    // 3. the workgroup's key range: scores, online softmax, P V.  Keys j < pos come from the cache (row src[n, j]); key pos from kv_new.
    float q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = qs[8 * l8 + i];
    const bf16_t* kb = a.kc + h * a.kc_hs + 8 * l8;
    const bf16_t* vb = a.vc + h * a.vc_hs + 8 * l8;
    const int32_t* src = a.src ? a.src + n * a.src_rs : nullptr;
    const uint8_t* kv = a.kvalid ? a.kvalid + n * a.kv_rs : nullptr;
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

    // 4. the 32 groups, in order
    combine_groups<HD, GROUPS>(g, 8 * l8, m, l, acc, a.o, a.part, nh, nh * a.part_stride + split, nsplit);
}

__global__ __launch_bounds__(NT) void persimmon_cached_kernel(PcArgs a) {
    persimmon_cached_body(a, blockIdx.x, a.pos, a.nsplit, a.kps, a.cs, a.sn);
}

// ---- the position in device memory (decode_split.h): grid (max_ranges, H, N) for the capacity --------------------------------------------
__global__ __launch_bounds__(NT) void persimmon_cached_dyn_kernel(PcArgs a, const int32_t* __restrict__ pos_dev, int S_max, int cus, int64_t table_rs) {
    DYN_POSITION_OR_RETURN(KEYS_PER_ITER, pos, sp, pos_dev, S_max, (int64_t)a.N * a.H, cus);
    if ((int)blockIdx.x >= sp.nsplit) return;
    persimmon_cached_body(a, blockIdx.x, pos, sp.nsplit, sp.kps, a.cs + (int64_t)pos * table_rs, a.sn + (int64_t)pos * table_rs);   // row `pos` of the tables
}

int require_rot(const char* name, int64_t rot) {
    OTTER_REQUIRE(rot > 0 && rot <= HD && rot % 16 == 0, "%s: rot=%ld must be a multiple of 16 in (0, 64]", name, (long)rot);
    return OTTER_OK;
}

}  // namespace

// (the order of the checks is ABI: the scalar entry point checks `pos` before the alignment checks, the dyn one `pos_dev` between the
// alignment and the stride checks -- decode_cached_entry.h)
extern "C" {

int otter_persimmon_decode_attn_cached(const void* qkv, const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k,
                                       const float* cos_row, const float* sin_row, void* k_cache, int64_t k_cache_row_stride,
                                       int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride, int64_t v_cache_head_stride,
                                       const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride, void* o,
                                       void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, int64_t pos, int64_t S_max, int64_t head_dim,
                                       int64_t rot, float eps, float scale, void* stream) {
    static const char name[] = "persimmon_decode_attn_cached";
    PcArgs a = {(const bf16_t*)qkv, gamma_q, beta_q, gamma_k, beta_k, cos_row, sin_row, (bf16_t*)k_cache, k_cache_row_stride, k_cache_head_stride,
                (bf16_t*)v_cache, v_cache_row_stride, v_cache_head_stride, src, src_row_stride, key_valid, key_valid_row_stride, (bf16_t*)o,
                (float*)workspace, (int)N, (int)H, 0, (int)rot, 0, 0, 0, eps, scale};
    if (int e = require_pointers(name, {qkv, gamma_q, beta_q, gamma_k, beta_k, cos_row, sin_row, k_cache, v_cache, o, workspace})) return e;
    if (int e = require_shape(name, head_dim, HD, N, H)) return e;
    if (int e = require_rot(name, rot)) return e;
    if (int e = require_capacity(name, S_max)) return e;
    if (int e = require_position(name, pos, S_max)) return e;
    if (int e = require_aligned16(name, {qkv, k_cache, v_cache}, "qkv, k_cache, v_cache")) return e;
    if (int e = require_cache_layout(name, nullptr, a, 8, S_max, HD)) return e;
    if (int e = require_row_strides(name, a, nullptr, pos)) return e;
    if (int e = require_workspace(name, workspace_bytes, OTTER_PERSIMMON_DECODE_CACHED_WORKSPACE_BYTES(N, H, pos + 1))) return e;

    return launch_scalar<HD>(name, a, pos, split_rule<KEYS_PER_ITER>(pos + 1, N * H, cu_count()), N, stream,
                             [](dim3 grid, hipStream_t st, const PcArgs& a) { hipLaunchKernelGGL(persimmon_cached_kernel, grid, dim3(NT), 0, st, a); });
}

int otter_persimmon_decode_attn_cached_dyn(const void* qkv, const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k,
                                           const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                           int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                           int64_t v_cache_head_stride, const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid,
                                           int64_t key_valid_row_stride, void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H,
                                           const int32_t* pos_dev, int64_t S_max, int64_t head_dim, int64_t rot, float eps, float scale,
                                           void* stream) {
    static const char name[] = "persimmon_decode_attn_cached_dyn";
    PcArgs a = {(const bf16_t*)qkv, gamma_q, beta_q, gamma_k, beta_k, cos_table, sin_table, (bf16_t*)k_cache, k_cache_row_stride, k_cache_head_stride,
                (bf16_t*)v_cache, v_cache_row_stride, v_cache_head_stride, src, src_row_stride, key_valid, key_valid_row_stride, (bf16_t*)o,
                (float*)workspace, (int)N, (int)H, 0, (int)rot, 0, 0, 0, eps, scale};
    if (int e = require_pointers(name, {qkv, gamma_q, beta_q, gamma_k, beta_k, cos_table, sin_table, k_cache, v_cache, o, workspace, pos_dev})) return e;
    if (int e = require_shape(name, head_dim, HD, N, H)) return e;
    if (int e = require_rot(name, rot)) return e;
    if (int e = require_capacity(name, S_max)) return e;
    if (int e = require_aligned16(name, {qkv, k_cache, v_cache}, "qkv, k_cache, v_cache")) return e;
    if (int e = require_pos_dev_aligned(name, pos_dev)) return e;
    if (int e = require_cache_layout(name, nullptr, a, 8, S_max, HD)) return e;
    if (int e = require_table_strides(name, a, table_row_stride, rot, "rot", S_max)) return e;
    if (int e = require_workspace(name, workspace_bytes, OTTER_PERSIMMON_DECODE_CACHED_DYN_WORKSPACE_BYTES(N, H, S_max))) return e;

    const int cus = cu_count();
    const DynStep d = {pos_dev, (int)S_max, cus, (int)split_max_ranges(S_max, N * H, cus), table_row_stride};
    return launch_dyn(name, a, d, N, stream,
                      [](dim3 grid, hipStream_t st, const PcArgs& a, const DynStep& d) {
                          hipLaunchKernelGGL(persimmon_cached_dyn_kernel, grid, dim3(NT), 0, st, a, d.pos_dev, d.S_max, d.cus, d.table_rs);
                      },
                      DynCombine<HD, KEYS_PER_ITER>());
}

}  // extern "C"
