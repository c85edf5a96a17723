// decode_cache_shared_i8.hip -- the grouped step of csrc/decode_cache_shared.hip over the INT8 static cache of csrc/decode_cache_i8.hip
// (otter_amd/kv_cache.py: StaticKVCache(kv_dtype="int8").share_prompt), head_dim 128.  The N rows are sentences x `group` beams, the beams of a
// sentence contiguous; keys [0, shared_len) of every beam are the keys of the sentence's first row (the LEADER, row (n / group) * group), which
// alone holds their codes and scales.  The result is exactly what otter_decode_attn_cached_i8 returns for a table whose columns
// [0, shared_len) hold (n / group) * group -- but a shared key is fetched AND DEQUANTISED once per sentence, not once per beam: ONE workgroup
// serves a (key range, head, sentence) and carries the `group` queries.
//
//   j <  shared_len          one load each of the K codes, V codes, K scale and V scale from the leader's row, unpacked once and used for all
//                            `group` queries; `src` and the other rows' codes and scales [0, shared_len) are not read
//   shared_len <= j < pos    per query, through `src` (NULL: the row's own), entries clamped to [0, N) as in decode_cache_i8.hip
//   j == pos                 the new tokens in their dequantised form: the workgroup's own copy of every row's codes and scales (LDS)
//
// Each row appends its codes and both scales into its OWN slot [n, h, pos]; key_valid is read per row.  THE FORMAT (kv_i8_scale, kv_i8_code),
// the unpacking (Codes, unpack_codes) and the p * v_scale update (softmax_update_scaled) are csrc/decode_split.h's, shared with
// decode_cache_i8.hip; the new-token step around the quantiser (fp64 rotated() with one rounding, the amax over two waves) and the score
// fmaf(s, k_scale, slope * (j - pos)) are written as in that file: the stored codes and scales are bit-equal to that kernel's and to
// quantize_kv_int8.  DsqArgs' fields, every check, the switch over the group size and the combine kernels are csrc/decode_cached_entry.h's.
//
// THE INVARIANT THE IN-PLACE UPDATE RESTS ON is decode_cache_shared.hip's, extended to the scales: no workgroup reads a slot (codes or scale)
// that this launch writes.  The writes are slot [n, :, pos] of every row n; the reads through `src` are of keys j < pos; the shared reads are
// of the leaders' keys j < shared_len, and the entry points require 1 <= shared_len <= pos, so a leader's write (slot pos >= shared_len) never
// meets a shared read.  (The dyn kernel returns when the position it reads is below shared_len, as it does for one outside [1, S_max).)
//
// Shape: the split-key step of csrc/decode_split.h -- grid (key range, head, SENTENCE), 256 threads.  LANE GEOMETRY: 16
// lanes per key, 8 codes per lane (one 8-byte load each of K and V codes), 16 groups, two keys per group in flight = 32 keys per iteration.
// The int8 file's own geometry (8 lanes x 16 codes, 64 keys per iteration) costs 32 VGPRs of q + acc per query: with it the instances for
// groups of 5 and 6 rows do not fit 256 VGPRs without scratch, and the rule is one geometry for every group size (DESIGN.md 4.20 has the
// table).  One online softmax per (group, query); the 16 groups and then the ranges are combined in the header's fixed orders, query after
// query.  The ranges come from split_rule with NH = (N / group) * H, on the host (scalar entry) and on the device (dyn entry), so the two
// entries give the same bits at every position, and two calls on the same inputs give the same bits.  A range, a 32-key iteration or a
// group's pair of keys may straddle shared_len: an iteration that lies wholly below it takes the shared loader for both of its keys at once;
// every other iteration decides per key.  (The iterations wholly below shared_len are the first of a range; they are software-pipelined, the
// keys of a group in the same order as without: the bits do not depend on it.)
#include "decode_cached_entry.h"

namespace {

constexpr int HD = 128, LANES = 16, GROUPS = NT / LANES, KEYS_PER_ITER = GROUPS * UNROLL, DPL = HD / LANES;
constexpr int STAGE = 2;                                  // iterations whose shared loads are issued together, one stage ahead of the arithmetic

struct DsqArgs : I8StepArgs {                             // (decode_cached_entry.h; columns < shared_len of `src` are not read)
    int shared_len;
    float scale;
};

// a key of the leader's row as a lane holds it: its share of the K and V codes, the key's two scales
struct SharedKey { Codes<DPL> k, v; float ks, vs; };

// one key of the G queries: its score against each, the key scale, ALiBi, the rows' masks, one online-softmax update each with the value
// scale.  kr, vr, ksc, vsc: G entries, one per query; ONE: the key is the same vector for every query (one entry), unpacked once
template <int G, bool ONE>
__device__ __forceinline__ void shared_i8_key_update(const Codes<DPL>* kr, const Codes<DPL>* vr, const float* ksc, const float* vsc,
                                                     const float (&q)[G][DPL], const int j, const bool live, const float bias,
                                                     const uint8_t* (&kv)[G], float (&m)[G], float (&l)[G], float (&acc)[G][DPL]) {
    float k[DPL], v[DPL];
    if (ONE) {
        unpack_codes(kr[0], k);
        unpack_codes(vr[0], v);
    }
#pragma unroll
    for (int b = 0; b < G; ++b) {
        if (!ONE) {
            unpack_codes(kr[b], k);
            unpack_codes(vr[b], v);
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < DPL; ++i) s = fmaf(q[b][i], k[i], s);
        s = group_sum<LANES>(s);                          // (all lanes: the shuffles stay convergent)
        s = fmaf(s, ksc[ONE ? 0 : b], bias);
        if (!live || (kv[b] && kv[b][j] == 0)) s = -INFINITY;
        softmax_update_scaled(m[b], l[b], acc[b], s, v, vsc[ONE ? 0 : b]);
    }
}

// one workgroup's share of a step: range `split` of the G rows of sentence blockIdx.z, head blockIdx.y
template <int G>
__device__ __forceinline__ void decode_shared_i8_body(const DsqArgs& a, const int split, const int pos, const int nsplit, const int kps,
                                                      const float* cs_tab, const float* sn_tab) {
    __shared__ float qs[G][HD];                                           // scale * q'
    __shared__ __attribute__((aligned(16))) int8_t code_new[G][2][HD];    // the new tokens' codes: [0] k', [1] v
    __shared__ float scale_new[G][2], wave_amax[G][NT / OTTER_WAVE];
    const int h = blockIdx.y, n0 = blockIdx.z * G, tid = threadIdx.x;     // n0: the leader
    const int shared_len = a.shared_len;

    // 1. the new tokens, row after row: threads 0..127 own q[d] and v[d] (waves 0, 1), threads 128..255 own k[d] (waves 2, 3).  x = what the
    //    bf16 cache would store; amax over the 128 dims (a max: exact in any order), then divide and round.
    {
        const int d = tid & (HD - 1), which = tid < HD ? 1 : 0;
        float x[G];
#pragma unroll
        for (int b = 0; b < G; ++b) {
            const int n = n0 + b;
            const float* cs = cs_tab ? cs_tab + n * a.cs_rs : nullptr;
            const float* sn = cs_tab ? sn_tab + n * a.cs_rs : nullptr;
            if (tid < HD) {
                qs[b][d] = (float)rotated(a.q + n * a.q_rs + h * a.q_hs, cs, sn, d) * a.scale;
                x[b] = bf2f(a.vn[n * a.vn_rs + h * a.vn_hs + d]);
            } else {
                x[b] = bf2f(d2bf(rotated(a.kn + n * a.kn_rs + h * a.kn_hs, cs, sn, d)));
            }
            const float wm = wave_max(fabsf(x[b]));
            if ((tid & (OTTER_WAVE - 1)) == 0) wave_amax[b][tid / OTTER_WAVE] = wm;
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < G; ++b) {
            const float amax = fmaxf(wave_amax[b][tid < HD ? 0 : 2], wave_amax[b][tid < HD ? 1 : 3]);
            const float sc = kv_i8_scale(amax);
            const float c = kv_i8_code(x[b], sc);
            code_new[b][which][d] = (int8_t)(int)c;
            if (d == 0) scale_new[b][which] = sc;
        }
    }
    __syncthreads();

    const int ln = tid & (LANES - 1), g = tid / LANES;
    const int j0 = split * kps, j1 = min(j0 + kps, pos + 1);
    // 2. the append (the workgroup whose range holds `pos`): slot [n, h, pos] of every row's OWN row -- LANES lanes x DPL bytes each for the K
    //    and the V codes of a row, then one lane each for its two scales
    if (pos >= j0 && pos < j1) {
        if (tid < 2 * LANES * G) {
            const int b = tid / (2 * LANES), n = n0 + b;
            const bool is_k = (tid & (2 * LANES - 1)) < LANES;
            int8_t* dst = (is_k ? a.kc + n * a.kc_rs + h * a.kc_hs : a.vc + n * a.vc_rs + h * a.vc_hs) + (int64_t)pos * HD + DPL * ln;
            *reinterpret_cast<Codes<DPL>*>(dst) = *reinterpret_cast<const Codes<DPL>*>(&code_new[b][is_k ? 0 : 1][DPL * ln]);
        } else if (tid < 2 * LANES * G + 2 * G) {
            const int w = tid - 2 * LANES * G, b = w >> 1, n = n0 + b;
            float* dst = (w & 1) == 0 ? a.ks + n * a.ks_rs + h * a.ks_hs : a.vs + n * a.vs_rs + h * a.vs_hs;
            dst[pos] = scale_new[b][w & 1];
        }
    }

    // 3. the workgroup's key range: scores, online softmax, P V for the G queries
    float q[G][DPL];
    const uint8_t* kv[G];
    const int32_t* src[G];
    float m[G], l[G], acc[G][DPL];
#pragma unroll
    for (int b = 0; b < G; ++b) {
#pragma unroll
        for (int i = 0; i < DPL; ++i) {
            q[b][i] = qs[b][DPL * ln + i];
            acc[b][i] = 0.f;
        }
        kv[b] = a.kvalid ? a.kvalid + (n0 + b) * a.kv_rs : nullptr;
        src[b] = a.src ? a.src + (n0 + b) * a.src_rs : nullptr;
        m[b] = -INFINITY;
        l[b] = 0.f;
    }
    const int8_t* kb = a.kc + h * a.kc_hs + DPL * ln;
    const int8_t* vb = a.vc + h * a.vc_hs + DPL * ln;
    const float* ksb = a.ks + h * a.ks_hs;
    const float* vsb = a.vs + h * a.vs_hs;
    const int8_t* kl = kb + n0 * a.kc_rs;                 // the leader's row
    const int8_t* vl = vb + n0 * a.vc_rs;
    const float* ksl = ksb + n0 * a.ks_rs;
    const float* vsl = vsb + n0 * a.vs_rs;
    const float slope = a.slopes ? a.slopes[h] : 0.f;
    // the iterations that lie wholly below shared_len come first in the range, [j0, jsh) (shared_len <= pos < j1 and kps is a multiple of
    // KEYS_PER_ITER: every key of them is live).  Each takes the shared loader for both of its keys at once, one load for the G queries.
    // They go in stages of STAGE iterations, and the loads of the next stage are issued before this one's arithmetic: a workgroup here
    // has a third or less of the waves of the ungrouped kernel's grid to hide the latency with (measured: DESIGN.md 4.20).
    const int jsh = j0 + max(min(shared_len, j1) - j0, 0) / KEYS_PER_ITER * KEYS_PER_ITER;
    // (a stage: STAGE iterations' keys; the last stage of a range may hold fewer iterations -- the same for the whole workgroup)
    const auto load_shared = [&](SharedKey (&sk)[STAGE][UNROLL], const int jb) {
#pragma unroll
        for (int i = 0; i < STAGE; ++i) {
            if (jb + i * KEYS_PER_ITER < jsh) {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const int j = jb + i * KEYS_PER_ITER + u * GROUPS + g;
                    sk[i][u].k = *reinterpret_cast<const Codes<DPL>*>(kl + (int64_t)j * HD);
                    sk[i][u].v = *reinterpret_cast<const Codes<DPL>*>(vl + (int64_t)j * HD);
                    sk[i][u].ks = ksl[j];
                    sk[i][u].vs = vsl[j];
                }
            }
        }
    };
    SharedKey cur[STAGE][UNROLL], nxt[STAGE][UNROLL];
    if (j0 < jsh) load_shared(cur, j0);
    int jb = j0;
    for (; jb < jsh; jb += STAGE * KEYS_PER_ITER) {
        const bool more = jb + STAGE * KEYS_PER_ITER < jsh;
        if (more) load_shared(nxt, jb + STAGE * KEYS_PER_ITER);
#pragma unroll
        for (int i = 0; i < STAGE; ++i) {
            if (jb + i * KEYS_PER_ITER < jsh) {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const int j = jb + i * KEYS_PER_ITER + u * GROUPS + g;
                    shared_i8_key_update<G, true>(&cur[i][u].k, &cur[i][u].v, &cur[i][u].ks, &cur[i][u].vs, q, j, true, slope * (float)(j - pos), kv,
                                                  m, l, acc);
                }
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < STAGE; ++i) {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) cur[i][u] = nxt[i][u];
            }
        }
    }
    jb = jsh;
    for (; jb < j1; jb += KEYS_PER_ITER) {
        // an iteration that straddles shared_len, lies above it, or ends the range: the loader is chosen key by key
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = jb + u * GROUPS + g;
            Codes<DPL> kr[G], vr[G];
            float ksc[G], vsc[G];
            if (j < j1 && j < shared_len) {               // shared: one load (j < shared_len <= pos)
                kr[0] = *reinterpret_cast<const Codes<DPL>*>(kl + (int64_t)j * HD);
                vr[0] = *reinterpret_cast<const Codes<DPL>*>(vl + (int64_t)j * HD);
                ksc[0] = ksl[j];
                vsc[0] = vsl[j];
#pragma unroll
                for (int b = 1; b < G; ++b) {
                    kr[b] = kr[0];
                    vr[b] = vr[0];
                    ksc[b] = ksc[0];
                    vsc[b] = vsc[0];
                }
            } else if (j < j1 && j < pos) {               // own: per query, through the table
#pragma unroll
                for (int b = 0; b < G; ++b) {
                    // a table entry outside [0, N) is clamped: it can make the result wrong, never an access outside the cache
                    const int64_t row = src[b] ? (int64_t)min(max(src[b][j], 0), a.N - 1) : (int64_t)(n0 + b);
                    kr[b] = *reinterpret_cast<const Codes<DPL>*>(kb + row * a.kc_rs + (int64_t)j * HD);
                    vr[b] = *reinterpret_cast<const Codes<DPL>*>(vb + row * a.vc_rs + (int64_t)j * HD);
                    ksc[b] = ksb[row * a.ks_rs + j];
                    vsc[b] = vsb[row * a.vs_rs + j];
                }
            } else if (j < j1) {                          // j == pos: the new tokens, as the cache now holds them
#pragma unroll
                for (int b = 0; b < G; ++b) {
                    kr[b] = *reinterpret_cast<const Codes<DPL>*>(&code_new[b][0][DPL * ln]);
                    vr[b] = *reinterpret_cast<const Codes<DPL>*>(&code_new[b][1][DPL * ln]);
                    ksc[b] = scale_new[b][0];
                    vsc[b] = scale_new[b][1];
                }
            } else {
#pragma unroll
                for (int b = 0; b < G; ++b) {
#pragma unroll
                    for (int i = 0; i < DPL / 4; ++i) {
                        kr[b].w[i] = 0;
                        vr[b].w[i] = 0;
                    }
                    ksc[b] = 0.f;
                    vsc[b] = 0.f;
                }
            }
            shared_i8_key_update<G, false>(kr, vr, ksc, vsc, q, j, j < j1, slope * (float)(j - pos), kv, m, l, acc);
        }
    }

    // 4. the 16 groups, in order, query after query (one set of LDS buffers: a barrier between two queries' combines)
#pragma unroll
    for (int b = 0; b < G; ++b) {
        if (b) __syncthreads();
        const int64_t nh = (int64_t)(n0 + b) * a.H + h;
        combine_groups<HD, GROUPS>(g, DPL * ln, m[b], l[b], acc[b], a.o, a.part, nh, nh * a.part_stride + split, nsplit);
    }
}

template <int G>
__global__ __launch_bounds__(NT) void decode_shared_i8_kernel(DsqArgs a) {
    decode_shared_i8_body<G>(a, blockIdx.x, a.pos, a.nsplit, a.kps, a.cs, a.sn);
}

// ---- the position in device memory (decode_split.h): grid (max_ranges, H, N / G) for the capacity ------------------------------------------
template <int G>
__global__ __launch_bounds__(NT) void decode_shared_i8_dyn_kernel(DsqArgs a, const int32_t* __restrict__ pos_dev, int S_max, int cus,
                                                                  int64_t table_rs) {
    DYN_POSITION_OR_RETURN(KEYS_PER_ITER, pos, sp, pos_dev, S_max, (int64_t)(a.N / G) * a.H, cus);
    if (pos < a.shared_len) return;                       // (the in-place invariant needs shared_len <= pos: such a counter does nothing)
    if ((int)blockIdx.x >= sp.nsplit) return;
    // row `pos` of the rotary tables, shared by every row (cs_rs = 0)
    decode_shared_i8_body<G>(a, blockIdx.x, pos, sp.nsplit, sp.kps, a.cs ? a.cs + (int64_t)pos * table_rs : nullptr,
                             a.cs ? a.sn + (int64_t)pos * table_rs : nullptr);
}

static_assert(2 * LANES * OTTER_DECODE_CACHED_SHARED_MAX_GROUP + 2 * OTTER_DECODE_CACHED_SHARED_MAX_GROUP <= NT,
              "decode_cache_shared_i8.hip: the append has a thread per store");

}  // namespace

// the checks of both entry points are decode_cache_i8.hip's, in its order (the first failing check names the error), with the two checks of the
// grouping after the capacity's; the one of shared_len follows the position's (scalar) or the grouping's (dyn)
extern "C" {

int otter_decode_attn_cached_shared_i8(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                       int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                       const float* cos_rows, const float* sin_rows, int64_t cos_row_stride, void* k_cache,
                                       int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                       int64_t v_cache_head_stride, float* k_scale, int64_t k_scale_row_stride, int64_t k_scale_head_stride,
                                       float* v_scale, int64_t v_scale_row_stride, int64_t v_scale_head_stride, const int32_t* src,
                                       int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride, const float* alibi_slopes,
                                       void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, int64_t pos, int64_t S_max,
                                       int64_t head_dim, float scale, int64_t group, int64_t shared_len, void* stream) {
    static const char name[] = "decode_attn_cached_shared_i8";
    DsqArgs a = {{{(const bf16_t*)q, q_row_stride, q_head_stride, (const bf16_t*)k_new, k_new_row_stride, k_new_head_stride, (const bf16_t*)v_new,
                   v_new_row_stride, v_new_head_stride, cos_rows, sin_rows, cos_row_stride},
                  (int8_t*)k_cache, k_cache_row_stride, k_cache_head_stride, (int8_t*)v_cache, v_cache_row_stride, v_cache_head_stride,
                  k_scale, k_scale_row_stride, k_scale_head_stride, v_scale, v_scale_row_stride, v_scale_head_stride,
                  src, src_row_stride, key_valid, key_valid_row_stride, alibi_slopes, (bf16_t*)o, (float*)workspace, (int)N, (int)H},
                 (int)shared_len, scale};
    if (int e = require_pointers(name, {q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, o, workspace})) return e;
    if (int e = require_cos_sin_pair(name, cos_rows, sin_rows, "rows")) return e;
    if (int e = require_shape(name, head_dim, HD, N, H)) return e;
    if (int e = require_capacity(name, S_max)) return e;
    if (int e = require_groups(name, N, group)) return e;
    if (int e = require_token_and_cache_aligned(name, a)) return e;
    if (int e = require_scales_aligned(name, a)) return e;
    if (int e = require_cache_layout(name, &a, a, 16, S_max, HD)) return e;
    if (int e = require_scale_head_strides(name, a, S_max)) return e;
    if (int e = require_position(name, pos, S_max)) return e;
    if (int e = require_shared_len(name, shared_len, pos)) return e;
    if (int e = require_row_strides(name, a, &cos_row_stride, pos)) return e;
    if (int e = require_workspace(name, workspace_bytes, OTTER_DECODE_CACHED_SHARED_I8_WORKSPACE_BYTES(N, H, pos + 1))) return e;

    // nsplit <= ceil((pos + 1) / 128): the workspace holds N * H * nsplit records
    return launch_scalar<HD>(name, a, pos, split_rule<KEYS_PER_ITER>(pos + 1, (N / group) * H, cu_count()), N / group, stream,
                             [group](dim3 grid, hipStream_t st, const DsqArgs& a) {
                                 for_group(group, [&](auto G) { hipLaunchKernelGGL(decode_shared_i8_kernel<decltype(G)::value>, grid, dim3(NT), 0, st, a); });
                             });
}

int otter_decode_attn_cached_shared_i8_dyn(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                           int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                           const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                           int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                           int64_t v_cache_head_stride, float* k_scale, int64_t k_scale_row_stride, int64_t k_scale_head_stride,
                                           float* v_scale, int64_t v_scale_row_stride, int64_t v_scale_head_stride, const int32_t* src,
                                           int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride,
                                           const float* alibi_slopes, void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H,
                                           const int32_t* pos_dev, int64_t S_max, int64_t head_dim, float scale, int64_t group, int64_t shared_len,
                                           void* stream) {
    static const char name[] = "decode_attn_cached_shared_i8_dyn";
    DsqArgs a = {{{(const bf16_t*)q, q_row_stride, q_head_stride, (const bf16_t*)k_new, k_new_row_stride, k_new_head_stride, (const bf16_t*)v_new,
                   v_new_row_stride, v_new_head_stride, cos_table, sin_table, 0},
                  (int8_t*)k_cache, k_cache_row_stride, k_cache_head_stride, (int8_t*)v_cache, v_cache_row_stride, v_cache_head_stride,
                  k_scale, k_scale_row_stride, k_scale_head_stride, v_scale, v_scale_row_stride, v_scale_head_stride,
                  src, src_row_stride, key_valid, key_valid_row_stride, alibi_slopes, (bf16_t*)o, (float*)workspace, (int)N, (int)H},
                 (int)shared_len, scale};
    if (int e = require_pointers(name, {q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, o, workspace, pos_dev})) return e;
    if (int e = require_cos_sin_pair(name, cos_table, sin_table, "table")) return e;
    if (int e = require_shape(name, head_dim, HD, N, H)) return e;
    if (int e = require_capacity(name, S_max)) return e;
    if (int e = require_groups(name, N, group)) return e;
    if (int e = require_shared_len_dyn(name, shared_len, S_max)) return e;
    if (int e = require_token_and_cache_aligned(name, a)) return e;
    if (int e = require_scales_aligned(name, a)) return e;
    if (int e = require_cache_layout(name, &a, a, 16, S_max, HD)) return e;
    if (int e = require_scale_head_strides(name, a, S_max)) return e;
    if (int e = require_pos_dev_aligned(name, pos_dev)) return e;
    if (int e = require_table_strides(name, a, table_row_stride, HD, "128", S_max)) return e;
    if (int e = require_workspace(name, workspace_bytes, OTTER_DECODE_CACHED_SHARED_I8_DYN_WORKSPACE_BYTES(N, H, S_max))) return e;

    const int cus = cu_count();
    const int64_t NH = (N / group) * H;
    // max_ranges <= ceil(S_max / 128): the workspace holds N * H * max_ranges records
    const DynStep d = {pos_dev, (int)S_max, cus, (int)split_max_ranges(S_max, NH, cus), table_row_stride};
    return launch_dyn(name, a, d, N / group, stream,
                      [group](dim3 grid, hipStream_t st, const DsqArgs& a, const DynStep& d) {
                          for_group(group, [&](auto G) {
                              hipLaunchKernelGGL(decode_shared_i8_dyn_kernel<decltype(G)::value>, grid, dim3(NT), 0, st, a, d.pos_dev, d.S_max, d.cus,
                                                 d.table_rs);
                          });
                      },
                      SharedDynCombine<HD, KEYS_PER_ITER>{NH});
}

}  // extern "C"
