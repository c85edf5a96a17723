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
#include "decode_split.h"

namespace {

constexpr int HD = 128, LANES = 16, GROUPS = NT / LANES, KEYS_PER_ITER = GROUPS * UNROLL;

struct DcArgs {
    const bf16_t* q; int64_t q_rs, q_hs;                  // new token: q / k / v [n, h, 128], row / head strides (elements), dim stride 1
    const bf16_t* kn; int64_t kn_rs, kn_hs;
    const bf16_t* vn; int64_t vn_rs, vn_hs;
    const float *cs, *sn; int64_t cs_rs;                  // rotary row(s) of position pos, fp32 [128]; row stride 0 = shared; null = no rotary
    bf16_t* kc; int64_t kc_rs, kc_hs;                     // cache [row, h, key, 128]: row / head strides, key stride 128
    bf16_t* vc; int64_t vc_rs, vc_hs;
    const int32_t* src; int64_t src_rs;                   // [N, >= pos] or null (= the row's own)
    const uint8_t* kvalid; int64_t kv_rs;                 // [N, >= pos + 1] or null
    const float* slopes;                                  // [H] or null
    bf16_t* o;                                            // [N, H * 128]
    float* part;                                          // [N * H * part_stride, PART] (nsplit > 1), part_stride >= nsplit
    int N, H, pos, nsplit, kps, part_stride;
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

__global__ __launch_bounds__(HD) void decode_cached_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ o, int H, int nsplit) {
    const int64_t nh = (int64_t)blockIdx.y * H + blockIdx.x;
    combine_ranges<HD>(part, o, nh, nsplit, nsplit);
}

// ---- the position in device memory (decode_split.h): grid (max_ranges, H, N) for the capacity --------------------------------------------
__global__ __launch_bounds__(NT) void decode_cached_dyn_kernel(DcArgs a, const int32_t* __restrict__ pos_dev, int S_max, int cus, int64_t table_rs) {
    DYN_POSITION_OR_RETURN(KEYS_PER_ITER, pos, sp, pos_dev, S_max, (int64_t)a.N * a.H, cus);
    if ((int)blockIdx.x >= sp.nsplit) return;
    // row `pos` of the rotary tables, shared by every row (cs_rs = 0)
    decode_cached_body(a, blockIdx.x, pos, sp.nsplit, sp.kps, a.cs ? a.cs + (int64_t)pos * table_rs : nullptr,
                       a.cs ? a.sn + (int64_t)pos * table_rs : nullptr);
}

__global__ __launch_bounds__(HD) void decode_cached_dyn_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ o,
                                                                       const int32_t* __restrict__ pos_dev, int N, int H, int S_max, int cus,
                                                                       int max_ranges) {
    DYN_POSITION_OR_RETURN(KEYS_PER_ITER, pos, sp, pos_dev, S_max, (int64_t)N * H, cus);
    const int nsplit = min(sp.nsplit, max_ranges);
    if (nsplit == 1) return;                              // the one live workgroup wrote o itself
    const int64_t nh = (int64_t)blockIdx.y * H + blockIdx.x;
    combine_ranges<HD>(part, o, nh, nsplit, max_ranges);
}

bool mult8(int64_t a, int64_t b) { return a % 8 == 0 && b % 8 == 0; }

}  // namespace

// the argument checks both entry points share (NAME: the entry point's name in messages).  Three macros where decode_cache_i8.hip has one:
// here the scalar entry point checks `pos` between the shape and the alignment checks and the dyn one checks `pos_dev` between the alignment
// and the stride checks, and the order of the checks is part of the ABI (the first failing check names the error).
#define DC_REQUIRE_SHAPE(NAME)                                                                                    \
    OTTER_REQUIRE(head_dim == HD, NAME ": head_dim %ld (128 only)", (long)head_dim);                             \
    OTTER_REQUIRE(N > 0 && H > 0 && N <= 65535 && H <= 65535, NAME ": bad shape N=%ld H=%ld", (long)N, (long)H);  \
    OTTER_REQUIRE(S_max >= 2 && S_max <= S_MAX_LIMIT, NAME ": S_max=%ld outside [2, %ld]", (long)S_max, (long)S_MAX_LIMIT)

#define DC_REQUIRE_ALIGNED(NAME)                                                                                            \
    OTTER_REQUIRE((((uintptr_t)q | (uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0, \
                  NAME ": q, k_new, v_new, k_cache, v_cache need 16-byte alignment")

#define DC_REQUIRE_STRIDES(NAME)                                                                                                                    \
    OTTER_REQUIRE(mult8(q_row_stride, q_head_stride) && mult8(k_new_row_stride, k_new_head_stride) && mult8(v_new_row_stride, v_new_head_stride) && \
                      mult8(k_cache_row_stride, k_cache_head_stride) && mult8(v_cache_row_stride, v_cache_head_stride),                            \
                  NAME ": q / k_new / v_new / cache strides must be multiples of 8 elements");                                                     \
    OTTER_REQUIRE(k_cache_head_stride >= S_max * HD && v_cache_head_stride >= S_max * HD && k_cache_row_stride >= 0 && v_cache_row_stride >= 0,     \
                  NAME ": a cache head stride below S_max * 128 would make the slots of two heads overlap")

#define DC_FILL_ARGS(a)                                                                                                       \
    a.q = (const bf16_t*)q; a.q_rs = q_row_stride; a.q_hs = q_head_stride;                                                    \
    a.kn = (const bf16_t*)k_new; a.kn_rs = k_new_row_stride; a.kn_hs = k_new_head_stride;                                     \
    a.vn = (const bf16_t*)v_new; a.vn_rs = v_new_row_stride; a.vn_hs = v_new_head_stride;                                     \
    a.kc = (bf16_t*)k_cache; a.kc_rs = k_cache_row_stride; a.kc_hs = k_cache_head_stride;                                     \
    a.vc = (bf16_t*)v_cache; a.vc_rs = v_cache_row_stride; a.vc_hs = v_cache_head_stride;                                     \
    a.src = src; a.src_rs = src_row_stride; a.kvalid = key_valid; a.kv_rs = key_valid_row_stride; a.slopes = alibi_slopes;    \
    a.o = (bf16_t*)o; a.part = (float*)workspace; a.N = (int)N; a.H = (int)H; a.scale = scale

extern "C" {

int otter_decode_attn_cached(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                             int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                             const float* cos_rows, const float* sin_rows, int64_t cos_row_stride, void* k_cache, int64_t k_cache_row_stride,
                             int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride, int64_t v_cache_head_stride,
                             const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride,
                             const float* alibi_slopes, void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, int64_t pos,
                             int64_t S_max, int64_t head_dim, float scale, void* stream) {
    OTTER_REQUIRE(q && k_new && v_new && k_cache && v_cache && o && workspace, "decode_attn_cached: null pointer");
    OTTER_REQUIRE((cos_rows == nullptr) == (sin_rows == nullptr), "decode_attn_cached: cos_rows and sin_rows must both be given or both be NULL");
    DC_REQUIRE_SHAPE("decode_attn_cached");
    OTTER_REQUIRE(pos >= 1, "decode_attn_cached: pos=%ld: a cached step continues a cache (pos >= 1)", (long)pos);
    OTTER_REQUIRE(pos < S_max, "decode_attn_cached: pos=%ld is beyond the cache capacity S_max=%ld", (long)pos, (long)S_max);
    DC_REQUIRE_ALIGNED("decode_attn_cached");
    DC_REQUIRE_STRIDES("decode_attn_cached");
    OTTER_REQUIRE(cos_row_stride >= 0 && (!src || src_row_stride >= pos) && (!key_valid || key_valid_row_stride >= pos + 1),
                  "decode_attn_cached: src needs a row stride >= pos, key_valid one >= pos + 1, cos / sin a non-negative one");
    const int64_t Sk = pos + 1;
    const int64_t need = OTTER_DECODE_CACHED_WORKSPACE_BYTES(N, H, Sk);
    OTTER_REQUIRE(workspace_bytes >= need, "decode_attn_cached: workspace of %ld bytes, %ld needed", (long)workspace_bytes, (long)need);

    const Split sp = split_rule<KEYS_PER_ITER>(Sk, N * H, cu_count());
    const int64_t nsplit = sp.nsplit;

    DcArgs a;
    DC_FILL_ARGS(a);
    a.cs = cos_rows; a.sn = sin_rows; a.cs_rs = cos_row_stride;
    a.pos = (int)pos; a.nsplit = (int)nsplit; a.kps = sp.kps; a.part_stride = (int)nsplit;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(decode_cached_kernel, dim3((unsigned)nsplit, (unsigned)H, (unsigned)N), dim3(NT), 0, st, a);
    OTTER_CHECK_LAUNCH("decode_attn_cached");
    if (nsplit > 1) {
        hipLaunchKernelGGL(decode_cached_combine_kernel, dim3((unsigned)H, (unsigned)N), dim3(HD), 0, st, (const float*)workspace, (bf16_t*)o, (int)H,
                           (int)nsplit);
        OTTER_CHECK_LAUNCH("decode_attn_cached (combine)");
    }
    return OTTER_OK;
}

int otter_decode_attn_cached_dyn(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                 int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                 const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                 int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                 int64_t v_cache_head_stride, const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid,
                                 int64_t key_valid_row_stride, const float* alibi_slopes, void* o, void* workspace, int64_t workspace_bytes,
                                 int64_t N, int64_t H, const int32_t* pos_dev, int64_t S_max, int64_t head_dim, float scale, void* stream) {
    OTTER_REQUIRE(q && k_new && v_new && k_cache && v_cache && o && workspace && pos_dev, "decode_attn_cached_dyn: null pointer");
    OTTER_REQUIRE((cos_table == nullptr) == (sin_table == nullptr),
                  "decode_attn_cached_dyn: cos_table and sin_table must both be given or both be NULL");
    DC_REQUIRE_SHAPE("decode_attn_cached_dyn");
    DC_REQUIRE_ALIGNED("decode_attn_cached_dyn");
    OTTER_REQUIRE(((uintptr_t)pos_dev & 3) == 0, "decode_attn_cached_dyn: pos_dev needs 4-byte alignment");
    DC_REQUIRE_STRIDES("decode_attn_cached_dyn");
    // any position below S_max may be read from pos_dev: the tables, the beam table and the mask must hold the capacity
    OTTER_REQUIRE((!cos_table || table_row_stride >= HD) && (!src || src_row_stride >= S_max - 1) && (!key_valid || key_valid_row_stride >= S_max),
                  "decode_attn_cached_dyn: cos / sin tables need a row stride >= 128, src one >= S_max - 1, key_valid one >= S_max");
    const int64_t need = OTTER_DECODE_CACHED_DYN_WORKSPACE_BYTES(N, H, S_max);
    OTTER_REQUIRE(workspace_bytes >= need, "decode_attn_cached_dyn: workspace of %ld bytes, %ld needed", (long)workspace_bytes, (long)need);

    const int cus = cu_count();
    const int64_t max_ranges = split_max_ranges(S_max, N * H, cus);

    DcArgs a;
    DC_FILL_ARGS(a);
    a.cs = cos_table; a.sn = sin_table; a.cs_rs = 0;
    a.pos = 0; a.nsplit = 0; a.kps = 0; a.part_stride = (int)max_ranges;   // (pos, nsplit, kps: read and derived on the device)
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(decode_cached_dyn_kernel, dim3((unsigned)max_ranges, (unsigned)H, (unsigned)N), dim3(NT), 0, st, a, pos_dev, (int)S_max, cus,
                       table_row_stride);
    OTTER_CHECK_LAUNCH("decode_attn_cached_dyn");
    if (max_ranges > 1) {
        hipLaunchKernelGGL(decode_cached_dyn_combine_kernel, dim3((unsigned)H, (unsigned)N), dim3(HD), 0, st, (const float*)workspace, (bf16_t*)o,
                           pos_dev, (int)N, (int)H, (int)S_max, cus, (int)max_ranges);
        OTTER_CHECK_LAUNCH("decode_attn_cached_dyn (combine)");
    }
    return OTTER_OK;
}

}  // extern "C"

#undef DC_REQUIRE_SHAPE
#undef DC_REQUIRE_ALIGNED
#undef DC_REQUIRE_STRIDES
#undef DC_FILL_ARGS
