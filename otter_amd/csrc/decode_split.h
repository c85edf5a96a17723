// decode_split.h -- the one statement of the DEVICE half of the split-key (flash-decoding) decode kernels: persimmon_decode.hip,
// persimmon_decode_cache.hip, decode_cache.hip, decode_cache_i8.hip, decode_cache_shared.hip, decode_cache_shared_i8.hip.  Each of them keeps
// its Args struct, its key loop (the loaders and the score terms differ: strided past + copy-out, cache through the `src` table, codes +
// scales, a shared prompt over either cache; ALiBi or none, key scale or none) and its attention kernels.  The HOST half of the five cached
// files (argument checks, shared Args fields, combine kernels, launch sequence) is decode_cached_entry.h, which includes this header; the
// rest is here, the int8 cache's format (Codes, unpack_codes, kv_i8_scale, kv_i8_code) included:
//
//   grid (key range, head, row), NT = 256 threads.  A group of LANES lanes owns one key at a time, UNROLL keys per group in flight: score by
//   a LANES-wide butterfly (group_sum), online softmax per group (softmax_update: running max m, sum l, o[W]) -- no score buffer, no LDS
//   limit on the key count.  The groups are combined through LDS in a fixed order (combine_groups); with more than one range each workgroup
//   writes (m, l, o[HD]) to the workspace and a second kernel combines the ranges in range order (combine_ranges): two calls on the same
//   inputs give the same bits.  Masked keys add nothing; a fully masked row gives o = 0.
//
// Every kernel of these files compiles to the instructions it had when each file carried its own copy (tools/isa_equal.py); the forms of
// softmax_update, combine_groups and DYN_POSITION_OR_RETURN below are the ones that keep it so, and the comments there say what does not.
//
// The includers are anonymous-namespace translation units and this header puts its contents into that namespace too: everything here has
// internal linkage, the library exports nothing from it.  An includer defines HD, LANES, GROUPS = NT / LANES and KEYS_PER_ITER = GROUPS * UNROLL.
#pragma once
#include "common.h"

namespace {

constexpr int NT = 256, UNROLL = 2, MIN_KEYS_PER_SPLIT = 128;
constexpr int64_t S_MAX_LIMIT = 65536;                    // keys per (row, head)
template <int HD>
constexpr int PART = 2 + HD;                              // workspace record per (row, head, range): m, l, o[HD]

// THE SPLIT RULE (every entry point, host and device): about two workgroups per CU over all (row, head, range), at least MIN_KEYS_PER_SPLIT
// keys per range, a multiple of KEYS_PER_ITER keys each.  nsplit <= min(want, ceil(Sk / MIN_KEYS_PER_SPLIT)) with want = ceil(2 cus / (N H)):
// kps >= Sk / want bounds it by want, kps >= MIN_KEYS_PER_SPLIT by the other.  The range count is NOT monotone in Sk (rounding kps up to 32
// can drop a range: want 16, 4096 keys -> 16 ranges, 4100 keys -> 15), so a grid that must serve every position up to a capacity is sized by
// split_max_ranges, that bound, not by the count at the capacity itself.
struct Split { int kps, nsplit; };

__host__ __device__ constexpr int64_t split_want(int64_t NH, int cus) {
    const int64_t want = (2 * (int64_t)cus + NH - 1) / NH;
    return want > 0 ? want : 1;
}

template <int KEYS_PER_ITER>
__host__ __device__ constexpr Split split_rule(int64_t Sk, int64_t NH, int cus) {
    const int64_t want = split_want(NH, cus);
    int64_t kps = (Sk + want - 1) / want;
    if (kps < MIN_KEYS_PER_SPLIT) kps = MIN_KEYS_PER_SPLIT;
    kps = (kps + KEYS_PER_ITER - 1) / KEYS_PER_ITER * KEYS_PER_ITER;
    return Split{(int)kps, (int)((Sk + kps - 1) / kps)};
}

__host__ __device__ constexpr int64_t split_max_ranges(int64_t S_max, int64_t NH, int cus) {
    const int64_t want = split_want(NH, cus), by_keys = (S_max + MIN_KEYS_PER_SPLIT - 1) / MIN_KEYS_PER_SPLIT;
    return want < by_keys ? want : by_keys;
}

// what the dyn grids rest on: no position below a capacity has more ranges than the grid that was sized for the capacity
template <int KEYS_PER_ITER>
constexpr bool split_bound_holds(int64_t S_max, int64_t NH, int cus) {
    for (int64_t Sk = 1; Sk <= S_max; ++Sk)
        if (split_rule<KEYS_PER_ITER>(Sk, NH, cus).nsplit > split_max_ranges(S_max, NH, cus)) return false;
    return true;
}

static_assert(split_want(32, 256) == 16 && split_want(4096, 256) == 1, "split rule: want");
static_assert(split_rule<32>(4096, 32, 256).kps == 256 && split_rule<32>(4096, 32, 256).nsplit == 16, "split rule: 4096 keys");
static_assert(split_rule<32>(4100, 32, 256).kps == 288 && split_rule<32>(4100, 32, 256).nsplit == 15, "split rule: 4100 keys drop a range");
static_assert(split_rule<64>(4100, 32, 256).kps == 320 && split_rule<64>(4100, 32, 256).nsplit == 13, "split rule: 64 keys per iteration");
static_assert(split_rule<32>(100, 32, 256).kps == 128 && split_rule<32>(100, 32, 256).nsplit == 1, "split rule: MIN_KEYS_PER_SPLIT");
static_assert(split_max_ranges(4100, 32, 256) == 16 && split_max_ranges(1024, 32, 256) == 8, "split rule: range bound");
static_assert(split_bound_holds<32>(4100, 32, 256) && split_bound_holds<64>(4100, 32, 256) && split_bound_holds<32>(2048, 1, 256) &&
                  split_bound_holds<64>(2048, 640, 256),
              "split rule: a position with more ranges than split_max_ranges");

// per device, looked up once (a step that is to be captured has run eagerly before: no device query under capture)
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

// sum over the aligned group of LANES lanes, in every lane.  The butterfly is written out: as a loop over the distance it changes the
// register assignment of the kernels around it.
template <int LANES>
__device__ __forceinline__ float group_sum(float v) {
    static_assert(LANES == 8 || LANES == 16, "group_sum: 8 or 16 lanes");
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    if constexpr (LANES == 16) v += __shfl_xor(v, 8, 64);
    return v;
}

// 8 bf16 -> 8 floats
__device__ __forceinline__ void unpack8(const uint4& r, float (&v)[8]) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(w[i] << 16);
        v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}

// ---- the int8 cache (decode_cache_i8.hip, decode_cache_shared_i8.hip) -------------------------------------------------------------------
// a lane's DPL codes of one cached vector: one load of DPL bytes (8 or 16)
template <int DPL>
struct __attribute__((aligned(DPL))) Codes { uint32_t w[DPL / 4]; };

// DPL int8 codes -> DPL floats (exact)
template <int DPL>
__device__ __forceinline__ void unpack_codes(const Codes<DPL>& r, float (&v)[DPL]) {
#pragma unroll
    for (int i = 0; i < DPL / 4; ++i) {
#pragma unroll
        for (int b = 0; b < 4; ++b) v[4 * i + b] = (float)(int)(int8_t)(r.w[i] >> (8 * b));
    }
}

// THE FORMAT (otter_amd/kv_cache.py states it once for the project; quantize_kv_int8 there must agree with these two bit for bit): for the
// vector x[128] the bf16 cache would hold (k after rotary, rounded once to bf16; v as given), read as fp32:
//   amax = max |x[i]|;  scale = amax / 127 (1 when amax == 0);  code = clamp(rint(x[i] / scale), -127, 127);  value = code * scale.
// Plain `/` and rintf (round-half-even): IEEE-exact ops, the same codes and scales as torch computes.  No reciprocal.
__device__ __forceinline__ float kv_i8_scale(const float amax) { return amax == 0.f ? 1.f : amax / 127.f; }
__device__ __forceinline__ float kv_i8_code(const float x, const float sc) { return fminf(fmaxf(rintf(x / sc), -127.f), 127.f); }

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

// one key into a group's online softmax: score s (the same in every lane of the group; -inf for a masked key or a slot past the range, which
// then adds nothing), this lane's W dims of the value.  While nothing has been added m stays -inf and l, acc stay 0.  m and l go in and come
// back BY VALUE (m = r.m; l = r.l; at the call): passed by reference they are promoted to registers only after inlining, which reorders the
// key loop's phis and with them the register assignment.  The fields are in the order (l, m), against the
// parameters' (m, l), on purpose: it is the order of the two merge phis after the `if`, and with (m, l) the two moves that end a key's
// update come out swapped.  Name the fields at every use; `{l, m}` below is the only positional initialiser.
struct Softmax { float l, m; };
template <int W>
__device__ __forceinline__ Softmax softmax_update(const float m, const float l, float (&acc)[W], const float s, const float (&v)[W]) {
    Softmax r = {l, m};
    const float mn = fmaxf(m, s);
    if (mn != -INFINITY) {
        const float alpha = __expf(m - mn), p = __expf(s - mn);   // exp(-inf) = 0 for an empty history / a masked key
        r.l = fmaf(l, alpha, p);
#pragma unroll
        for (int i = 0; i < W; ++i) acc[i] = fmaf(acc[i], alpha, p * v[i]);
        r.m = mn;
    }
    return r;
}

// the same over the int8 cache: v are the key's value CODES, v_scale its value scale -- acc += (p * v_scale) * code.  m and l BY REFERENCE:
// the caller, decode_cache_shared_i8.hip's shared_i8_key_update, is itself an inlined function over m[G], l[G], and the by-value form above
// changes 10 of its 12 kernels.  decode_cache_i8.hip (16 codes per lane) keeps these statements WRITTEN OUT in its key loop, a second copy to
// keep in step by hand: neither form of this function left its two attention kernels as they were (1327 -> 1338 instruction lines).
template <int W>
__device__ __forceinline__ void softmax_update_scaled(float& m, float& l, float (&acc)[W], const float s, const float (&v)[W], const float v_scale) {
    const float mn = fmaxf(m, s);
    if (mn != -INFINITY) {
        const float alpha = __expf(m - mn), p = __expf(s - mn);   // exp(-inf) = 0 for an empty history / a masked key
        const float pv = p * v_scale;
        l = fmaf(l, alpha, p);
#pragma unroll
        for (int i = 0; i < W; ++i) acc[i] = fmaf(acc[i], alpha, pv * v[i]);
        m = mn;
    }
}

// the GROUPS groups of a workgroup, in group order.  Thread of group g whose acc[W] are dims d0 .. d0 + W - 1 (g, d0 from the caller, whose
// key loop has them: recomputed here they are merged with the caller's later and the addressing comes out differently).  Then lane
// tid < HD owns dim tid: with one range it writes o[nh * HD + tid], otherwise (M, L, O[HD]) to record `rec` of the workspace.
// (decode_cache_i8.hip keeps these statements written out: through this function its 32-group reduction is scheduled differently.)
template <int HD, int GROUPS, int W>
__device__ __forceinline__ void combine_groups(const int g, const int d0, const float m, const float l, const float (&acc)[W], bf16_t* o, float* part,
                                               const int64_t nh, const int64_t rec, const int nsplit) {
    static_assert(W * NT == HD * GROUPS, "combine_groups: a group's lanes cover the head");
    __shared__ float red_m[GROUPS], red_l[GROUPS], red_o[GROUPS][HD];
    const int tid = threadIdx.x;
    if (d0 == 0) { red_m[g] = m; red_l[g] = l; }
#pragma unroll
    for (int i = 0; i < W; ++i) red_o[g][d0 + i] = acc[i];
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
            o[nh * HD + tid] = f2bf(L > 0.f ? O / L : 0.f);
        } else {
            float* pr = part + rec * PART<HD>;
            if (tid < 2) pr[tid] = tid == 0 ? M : L;
            pr[2 + tid] = O;
        }
    }
}

// nsplit > 1: one workgroup of HD lanes per (head, row) combines the ranges in range order; the (row, head) has `stride` >= nsplit records
template <int HD>
__device__ __forceinline__ void combine_ranges(const float* part, bf16_t* o, int64_t nh, int nsplit, int stride) {
    const int d = threadIdx.x;
    const float* p = part + nh * stride * PART<HD>;
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
    o[nh * HD + d] = f2bf(L > 0.f ? O / L : 0.f);
}

// ---- the position in device memory: a launch that does not depend on it ---------------------------------------------------------------
// The grid is (max_ranges, H, N) for the cache's capacity, max_ranges = split_max_ranges >= the range count of every position (asserted
// above).  Every workgroup of a *_dyn_kernel and of a *_dyn_combine_kernel begins with this statement: it reads the position into
// `const int POS`, returns from the kernel when that is outside [1, S_max) -- a corrupt counter does nothing, it never indexes the cache --
// and derives `const Split SP`, the ranges of the position, by the rule the host uses for the scalar entry point.  The attention kernel then
// returns when blockIdx.x >= SP.nsplit (its range is not live), the combine kernel when one range is live (that workgroup wrote o itself).
// A whole workgroup takes the same branch, before any barrier.  (A macro: as a
// function, returning a flag or a struct or taking the rest of the kernel as a functor, it compiled the dyn kernels to other branches or
// another schedule than the statements written out.)
#define DYN_POSITION_OR_RETURN(KEYS_PER_ITER, POS, SP, pos_dev, S_max, NH, cus) \
    const int POS = *(pos_dev);                                                 \
    if (POS < 1 || POS >= (S_max)) return;                                      \
    const Split SP = split_rule<KEYS_PER_ITER>((int64_t)POS + 1, (NH), (cus))

// ---- the new token of a Persimmon step (head_dim 64; both Persimmon kernels, which is why the static cache returns the default cache's
// tokens): wave w < 3 owns vector w of qkv[nh] = q | k | v [3][64] of (row, head) nh, one element per lane.  fp32 LayerNorm of q and k by wave
// sums, fp32 rotate-half on the first `rot` dims with cs / sn = the rotary row of the position, ONE rounding to bf16.
// qs = scale * bf16(q'), kv_new = bf16(k') and v.  The caller's barrier follows.
__device__ __forceinline__ void persimmon_new_token(const bf16_t* qkv, int64_t nh, const float* gq, const float* bq, const float* gk, const float* bk,
                                                    const float* cs, const float* sn, int rot, float eps, float scale, float (&qs)[64],
                                                    bf16_t (&kv_new)[2][64]) {
    constexpr int HD = 64;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (w < 3) {
        float v = bf2f(qkv[(nh * 3 + w) * HD + lane]);   // (indexed as written: the address arithmetic is part of the kernels' pinned assembly)
        if (w < 2) {
            const float mean = wave_sum(v) * (1.0f / HD);
            const float dv = v - mean;
            const float rstd = rsqrtf(wave_sum(dv * dv) * (1.0f / HD) + eps);
            v = dv * rstd * (w ? gk : gq)[lane] + (w ? bk : bq)[lane];
            // rotate-half on the first `rot` dims: y1 = x1 c - x2 s, y2 = x2 c + x1 s
            const int half = rot >> 1;
            const bool in_rot = lane < rot, first = lane < half;
            const float vp = __shfl(v, in_rot ? (first ? lane + half : lane - half) : lane, 64);
            if (in_rot) v = v * cs[lane] + (first ? -vp : vp) * sn[lane];
        }
        const bf16_t vb = f2bf(v);
        if (w == 0) qs[lane] = bf2f(vb) * scale;
        else kv_new[w - 1][lane] = vb;
    }
}

}  // namespace
