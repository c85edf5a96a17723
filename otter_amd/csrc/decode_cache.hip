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
// Shape (csrc/persimmon_decode.hip, measured in this repository): grid (key range, head, row), 256 threads.  A 16-lane group owns one key at a
// time (lane l16: dims 8 l16 .. 8 l16 + 7, one 16-byte load each of K and V), two keys per group in flight: score by a 16-lane butterfly,
// online softmax per group (running max m, sum l, o[8]) -- no score buffer, no LDS limit on the key count.  The 16 groups are combined through
// LDS in a fixed order; with more than one range each workgroup writes (m, l, o[128]) to the workspace and a second kernel combines the
// ranges in range order: two calls on the same inputs give the same bits.  Masked keys add nothing; a fully masked row gives o = 0.
//
// Two entry points share every line of arithmetic.  otter_decode_attn_cached takes `pos` as a scalar and sizes its grid from it.
// otter_decode_attn_cached_dyn reads `pos` from device memory and launches a grid sized for the cache's CAPACITY: nothing in its launch
// depends on the position, so a captured graph of it can be replayed step after step.  Both derive the key ranges of a position from
// dc_split (host and device); a workgroup of the dyn grid whose range index is not live at the current position returns before it touches
// memory, and the combine kernel merges exactly the live ranges -- so at every position the two entry points give the same bits.
#include "common.h"

namespace {

constexpr int HD = 128, NT = 256, LANES = 16, GROUPS = NT / LANES, UNROLL = 2, KEYS_PER_ITER = GROUPS * UNROLL;
constexpr int MIN_KEYS_PER_SPLIT = 128, PART = 2 + HD;   // workspace record per (row, head, range): m, l, o[128]
constexpr int64_t S_MAX_LIMIT = 65536;

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

// THE SPLIT RULE (both entry points, host and device): about two workgroups per CU over all (row, head, range), at least MIN_KEYS_PER_SPLIT
// keys per range, a multiple of KEYS_PER_ITER keys each.  nsplit <= min(want, ceil(Sk / MIN_KEYS_PER_SPLIT)) with want = ceil(2 cus / (N H)):
// kps >= Sk / want bounds it by want, kps >= MIN_KEYS_PER_SPLIT by the other.  The range count is NOT monotone in Sk (rounding kps up to 32
// can drop a range: want 16, 4096 keys -> 16 ranges, 4100 keys -> 15), so a grid that must serve every position up to a capacity is sized by
// dc_max_ranges, that bound, not by the count at the capacity itself.
struct DcSplit { int kps, nsplit; };

__host__ __device__ inline int64_t dc_want(int64_t NH, int cus) {
    const int64_t want = (2 * (int64_t)cus + NH - 1) / NH;
    return want > 0 ? want : 1;
}

__host__ __device__ inline DcSplit dc_split(int64_t Sk, int64_t NH, int cus) {
    const int64_t want = dc_want(NH, cus);
    int64_t kps = (Sk + want - 1) / want;
    if (kps < MIN_KEYS_PER_SPLIT) kps = MIN_KEYS_PER_SPLIT;
    kps = (kps + KEYS_PER_ITER - 1) / KEYS_PER_ITER * KEYS_PER_ITER;
    DcSplit s;
    s.kps = (int)kps;
    s.nsplit = (int)((Sk + kps - 1) / kps);
    return s;
}

__host__ __device__ inline int64_t dc_max_ranges(int64_t S_max, int64_t NH, int cus) {
    const int64_t want = dc_want(NH, cus), by_keys = (S_max + MIN_KEYS_PER_SPLIT - 1) / MIN_KEYS_PER_SPLIT;
    return want < by_keys ? want : by_keys;
}

__device__ __forceinline__ float group16_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
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

// double -> bf16, round-to-nearest-even in ONE rounding: (float)y is RNE already; it misleads the second rounding only when it lands exactly
// on a bf16 midpoint that y itself was not on -- then the float is moved one step towards y first.
__device__ __forceinline__ bf16_t d2bf(double y) {
    float f = (float)y;
    const uint32_t u = __float_as_uint(f);
    if ((u & 0xffffu) == 0x8000u) {
        const double r = y - (double)f;
        if (r != 0.0) f = __uint_as_float((r > 0.0) == (f > 0.f) ? u + 1 : u - 1);
    }
    return f2bf(f);
}

// element d of the (optionally rotated) vector x[0..127]: x[d] c[d] + rotate_half(x)[d] s[d], rotate_half(x) = (-x[64..127], x[0..63])
__device__ __forceinline__ double rotated(const bf16_t* x, const float* cs, const float* sn, int d) {
    const double xd = (double)bf2f(x[d]);
    if (!cs) return xd;
    const double xp = (double)bf2f(x[d ^ 64]);
    return xd * (double)cs[d] + (d < 64 ? -xp : xp) * (double)sn[d];
}

// one workgroup's share of a step: range `split` of row blockIdx.z, head blockIdx.y
__device__ __forceinline__ void decode_cached_body(const DcArgs& a, const int split, const int pos, const int nsplit, const int kps,
                                                   const float* cs_tab, const float* sn_tab) {
    __shared__ float qs[HD];                                        // scale * q'
    __shared__ __attribute__((aligned(16))) bf16_t kv_new[2][HD];   // bf16(k') and v of the new token
    __shared__ float red_m[GROUPS], red_l[GROUPS], red_o[GROUPS][HD];
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
            s = group16_sum(s);                           // (all lanes: the shuffles stay convergent)
            s += slope * (float)(j - pos);
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

    // 4. the 16 groups, in order
    if (l16 == 0) { red_m[g] = m; red_l[g] = l; }
#pragma unroll
    for (int i = 0; i < 8; ++i) red_o[g][8 * l16 + i] = acc[i];
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
            float* pr = a.part + (nh * a.part_stride + split) * PART;
            if (tid < 2) pr[tid] = tid == 0 ? M : L;
            pr[2 + tid] = O;
        }
    }
}

__global__ __launch_bounds__(NT) void decode_cached_kernel(DcArgs a) {
    decode_cached_body(a, blockIdx.x, a.pos, a.nsplit, a.kps, a.cs, a.sn);
}

// nsplit > 1: one workgroup of 128 lanes per (head, row) combines the ranges in range order; p = the (row, head)'s first record
__device__ __forceinline__ void decode_cached_combine_body(const float* __restrict__ p, bf16_t* __restrict__ o, int64_t nh, int nsplit) {
    const int d = threadIdx.x;
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
    o[nh * HD + d] = f2bf(L > 0.f ? O / L : 0.f);
}

__global__ __launch_bounds__(HD) void decode_cached_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ o, int H, int nsplit) {
    const int64_t nh = (int64_t)blockIdx.y * H + blockIdx.x;
    decode_cached_combine_body(part + nh * nsplit * PART, o, nh, nsplit);
}

// ---- the position in device memory: a launch that does not depend on it ---------------------------------------------------------------
// The grid is (max_ranges, H, N) for the cache's capacity.  Every workgroup reads the position, derives the ranges of that position by the
// rule the host uses for the scalar entry point, and leaves at once when its range is not live (or the position is outside [1, S_max): a
// corrupt counter does nothing, it never indexes the cache).  The whole workgroup takes the same branch, before any barrier.
__global__ __launch_bounds__(NT) void decode_cached_dyn_kernel(DcArgs a, const int32_t* __restrict__ pos_dev, int S_max, int cus, int64_t table_rs) {
    const int pos = *pos_dev;
    if (pos < 1 || pos >= S_max) return;
    const DcSplit sp = dc_split((int64_t)pos + 1, (int64_t)a.N * a.H, cus);
    if ((int)blockIdx.x >= sp.nsplit) return;
    // row `pos` of the rotary tables, shared by every row (cs_rs = 0)
    decode_cached_body(a, blockIdx.x, pos, sp.nsplit, sp.kps, a.cs ? a.cs + (int64_t)pos * table_rs : nullptr,
                       a.cs ? a.sn + (int64_t)pos * table_rs : nullptr);
}

__global__ __launch_bounds__(HD) void decode_cached_dyn_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ o,
                                                                       const int32_t* __restrict__ pos_dev, int N, int H, int S_max, int cus,
                                                                       int max_ranges) {
    const int pos = *pos_dev;
    if (pos < 1 || pos >= S_max) return;
    const int nsplit = min(dc_split((int64_t)pos + 1, (int64_t)N * H, cus).nsplit, max_ranges);
    if (nsplit == 1) return;                              // the one live workgroup wrote o itself
    const int64_t nh = (int64_t)blockIdx.y * H + blockIdx.x;
    decode_cached_combine_body(part + nh * max_ranges * PART, o, nh, nsplit);
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

bool mult8(int64_t a, int64_t b) { return a % 8 == 0 && b % 8 == 0; }

}  // namespace

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
    OTTER_REQUIRE(head_dim == HD, "decode_attn_cached: head_dim %ld (128 only)", (long)head_dim);
    OTTER_REQUIRE(N > 0 && H > 0 && N <= 65535 && H <= 65535, "decode_attn_cached: bad shape N=%ld H=%ld", (long)N, (long)H);
    OTTER_REQUIRE(S_max >= 2 && S_max <= S_MAX_LIMIT, "decode_attn_cached: S_max=%ld outside [2, %ld]", (long)S_max, (long)S_MAX_LIMIT);
    OTTER_REQUIRE(pos >= 1, "decode_attn_cached: pos=%ld: a cached step continues a cache (pos >= 1)", (long)pos);
    OTTER_REQUIRE(pos < S_max, "decode_attn_cached: pos=%ld is beyond the cache capacity S_max=%ld", (long)pos, (long)S_max);
    OTTER_REQUIRE((((uintptr_t)q | (uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0,
                  "decode_attn_cached: q, k_new, v_new, k_cache, v_cache need 16-byte alignment");
    OTTER_REQUIRE(mult8(q_row_stride, q_head_stride) && mult8(k_new_row_stride, k_new_head_stride) && mult8(v_new_row_stride, v_new_head_stride) &&
                      mult8(k_cache_row_stride, k_cache_head_stride) && mult8(v_cache_row_stride, v_cache_head_stride),
                  "decode_attn_cached: q / k_new / v_new / cache strides must be multiples of 8 elements");
    OTTER_REQUIRE(k_cache_head_stride >= S_max * HD && v_cache_head_stride >= S_max * HD && k_cache_row_stride >= 0 && v_cache_row_stride >= 0,
                  "decode_attn_cached: a cache head stride below S_max * 128 would make the slots of two heads overlap");
    OTTER_REQUIRE(cos_row_stride >= 0 && (!src || src_row_stride >= pos) && (!key_valid || key_valid_row_stride >= pos + 1),
                  "decode_attn_cached: src needs a row stride >= pos, key_valid one >= pos + 1, cos / sin a non-negative one");
    const int64_t Sk = pos + 1;
    const int64_t need = OTTER_DECODE_CACHED_WORKSPACE_BYTES(N, H, Sk);
    OTTER_REQUIRE(workspace_bytes >= need, "decode_attn_cached: workspace of %ld bytes, %ld needed", (long)workspace_bytes, (long)need);

    const DcSplit sp = dc_split(Sk, N * H, cu_count());
    const int64_t nsplit = sp.nsplit, kps = sp.kps;

    DcArgs a;
    a.q = (const bf16_t*)q; a.q_rs = q_row_stride; a.q_hs = q_head_stride;
    a.kn = (const bf16_t*)k_new; a.kn_rs = k_new_row_stride; a.kn_hs = k_new_head_stride;
    a.vn = (const bf16_t*)v_new; a.vn_rs = v_new_row_stride; a.vn_hs = v_new_head_stride;
    a.cs = cos_rows; a.sn = sin_rows; a.cs_rs = cos_row_stride;
    a.kc = (bf16_t*)k_cache; a.kc_rs = k_cache_row_stride; a.kc_hs = k_cache_head_stride;
    a.vc = (bf16_t*)v_cache; a.vc_rs = v_cache_row_stride; a.vc_hs = v_cache_head_stride;
    a.src = src; a.src_rs = src_row_stride; a.kvalid = key_valid; a.kv_rs = key_valid_row_stride; a.slopes = alibi_slopes;
    a.o = (bf16_t*)o; a.part = (float*)workspace;
    a.N = (int)N; a.H = (int)H; a.pos = (int)pos; a.nsplit = (int)nsplit; a.kps = (int)kps; a.part_stride = (int)nsplit; a.scale = scale;
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
    OTTER_REQUIRE(head_dim == HD, "decode_attn_cached_dyn: head_dim %ld (128 only)", (long)head_dim);
    OTTER_REQUIRE(N > 0 && H > 0 && N <= 65535 && H <= 65535, "decode_attn_cached_dyn: bad shape N=%ld H=%ld", (long)N, (long)H);
    OTTER_REQUIRE(S_max >= 2 && S_max <= S_MAX_LIMIT, "decode_attn_cached_dyn: S_max=%ld outside [2, %ld]", (long)S_max, (long)S_MAX_LIMIT);
    OTTER_REQUIRE((((uintptr_t)q | (uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0,
                  "decode_attn_cached_dyn: q, k_new, v_new, k_cache, v_cache need 16-byte alignment");
    OTTER_REQUIRE(((uintptr_t)pos_dev & 3) == 0, "decode_attn_cached_dyn: pos_dev needs 4-byte alignment");
    OTTER_REQUIRE(mult8(q_row_stride, q_head_stride) && mult8(k_new_row_stride, k_new_head_stride) && mult8(v_new_row_stride, v_new_head_stride) &&
                      mult8(k_cache_row_stride, k_cache_head_stride) && mult8(v_cache_row_stride, v_cache_head_stride),
                  "decode_attn_cached_dyn: q / k_new / v_new / cache strides must be multiples of 8 elements");
    OTTER_REQUIRE(k_cache_head_stride >= S_max * HD && v_cache_head_stride >= S_max * HD && k_cache_row_stride >= 0 && v_cache_row_stride >= 0,
                  "decode_attn_cached_dyn: a cache head stride below S_max * 128 would make the slots of two heads overlap");
    // any position below S_max may be read from pos_dev: the tables, the beam table and the mask must hold the capacity
    OTTER_REQUIRE((!cos_table || table_row_stride >= HD) && (!src || src_row_stride >= S_max - 1) && (!key_valid || key_valid_row_stride >= S_max),
                  "decode_attn_cached_dyn: cos / sin tables need a row stride >= 128, src one >= S_max - 1, key_valid one >= S_max");
    const int64_t need = OTTER_DECODE_CACHED_DYN_WORKSPACE_BYTES(N, H, S_max);
    OTTER_REQUIRE(workspace_bytes >= need, "decode_attn_cached_dyn: workspace of %ld bytes, %ld needed", (long)workspace_bytes, (long)need);

    // the CU count is looked up once per device (a step that is to be captured has run eagerly before: no device query under capture)
    const int cus = cu_count();
    const int64_t max_ranges = dc_max_ranges(S_max, N * H, cus);

    DcArgs a;
    a.q = (const bf16_t*)q; a.q_rs = q_row_stride; a.q_hs = q_head_stride;
    a.kn = (const bf16_t*)k_new; a.kn_rs = k_new_row_stride; a.kn_hs = k_new_head_stride;
    a.vn = (const bf16_t*)v_new; a.vn_rs = v_new_row_stride; a.vn_hs = v_new_head_stride;
    a.cs = cos_table; a.sn = sin_table; a.cs_rs = 0;
    a.kc = (bf16_t*)k_cache; a.kc_rs = k_cache_row_stride; a.kc_hs = k_cache_head_stride;
    a.vc = (bf16_t*)v_cache; a.vc_rs = v_cache_row_stride; a.vc_hs = v_cache_head_stride;
    a.src = src; a.src_rs = src_row_stride; a.kvalid = key_valid; a.kv_rs = key_valid_row_stride; a.slopes = alibi_slopes;
    a.o = (bf16_t*)o; a.part = (float*)workspace;
    a.N = (int)N; a.H = (int)H; a.pos = 0; a.nsplit = 0; a.kps = 0; a.part_stride = (int)max_ranges; a.scale = scale;   // (pos, nsplit, kps: read and derived on the device)
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
