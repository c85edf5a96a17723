// decode_cached_entry.h -- the HOST half of the five cached-decode files (decode_cache.hip, decode_cache_i8.hip, decode_cache_shared.hip,
// decode_cache_shared_i8.hip, persimmon_decode_cache.hip), stated once: the argument checks of their ten entry points, the Args fields they
// share, the three range-combine kernels, the switch over the group size and the launch sequence.  The device arithmetic is decode_split.h's.
// A header of its own, not a second section of decode_split.h: that one is also included by persimmon_decode.hip, which has no cache, no
// `src` table and none of these checks.
//
// THE ORDER OF THE CHECKS IS PART OF THE ABI: the first failing check names the error (tests/test_decode_cached_check_order.py holds the
// order of every entry point).  Every require_* below is one place in that order, or a run of adjacent places; it sets the message and
// returns OTTER_ERR_ARG, or returns OTTER_OK, and an entry point is the list of its checks, each as `if (int e = require_...) return e;`.
// Scalar and dyn entry points differ in one place of the order: the scalar ones check `pos` before the alignment checks (after the int8
// files' stride checks), the dyn ones check `pos_dev` between the alignment and the stride checks.  The grouped entry points add the
// grouping's checks after the capacity's and the one of shared_len: after the position's (scalar) or the grouping's (dyn).  The orders of
// the bf16 and the int8 pairs differ and stay as they are: each is what its callers have seen since the file exists.
//
// Like decode_split.h this header puts its contents into the includer's anonymous namespace: internal linkage, nothing exported.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "decode_split.h"

namespace {

// ---- the Args fields the files share ------------------------------------------------------------------------------------------------------
// Base structs of the kernels' Args, so that the kernel argument layout stays what it was: every base is a whole number of 8-byte words
// without tail padding, and the members of the derived struct follow it as they followed these fields.

// the new token of a head_dim 128 step (every file but persimmon_decode_cache.hip)
struct NewTokenArgs {
    const bf16_t* q; int64_t q_rs, q_hs;                  // new token: q / k / v [n, h, 128], row / head strides (elements), dim stride 1
    const bf16_t* kn; int64_t kn_rs, kn_hs;
    const bf16_t* vn; int64_t vn_rs, vn_hs;
    const float *cs, *sn; int64_t cs_rs;                  // rotary row(s) of position pos, fp32 [128]; row stride 0 = shared; null = no rotary
};

// a head_dim 128 step over the bf16 cache (decode_cache.hip: + scale; decode_cache_shared.hip: + shared_len, scale)
struct Bf16StepArgs : NewTokenArgs {
    bf16_t* kc; int64_t kc_rs, kc_hs;                     // cache [row, h, key, 128]: row / head strides, key stride 128
    bf16_t* vc; int64_t vc_rs, vc_hs;
    const int32_t* src; int64_t src_rs;                   // [N, >= pos] or null (= the row's own)
    const uint8_t* kvalid; int64_t kv_rs;                 // [N, >= pos + 1] or null
    const float* slopes;                                  // [H] or null
    bf16_t* o;                                            // [N, H * 128]
    float* part;                                          // [N * H * part_stride, PART] (nsplit > 1), part_stride >= nsplit
    int N, H, pos, nsplit, kps, part_stride;
};

// a head_dim 128 step over the int8 cache (decode_cache_i8.hip: + scale; decode_cache_shared_i8.hip: + shared_len, scale)
struct I8StepArgs : NewTokenArgs {
    int8_t* kc; int64_t kc_rs, kc_hs;                     // codes [row, h, key, 128]: row / head strides, key stride 128
    int8_t* vc; int64_t vc_rs, vc_hs;
    float* ks; int64_t ks_rs, ks_hs;                      // scales [row, h, key]: row / head strides, key stride 1
    float* vs; int64_t vs_rs, vs_hs;
    const int32_t* src; int64_t src_rs;                   // [N, >= pos] or null (= the row's own)
    const uint8_t* kvalid; int64_t kv_rs;                 // [N, >= pos + 1] or null
    const float* slopes;                                  // [H] or null
    bf16_t* o;                                            // [N, H * 128]
    float* part;                                          // [N * H * part_stride, PART] (nsplit > 1), part_stride >= nsplit
    int N, H, pos, nsplit, kps, part_stride;
};
static_assert(sizeof(NewTokenArgs) == 96 && sizeof(Bf16StepArgs) == 96 + 128 && sizeof(I8StepArgs) == 96 + 176,
              "decode Args: a base struct with padding moves the kernel arguments");

// ---- the combine kernels: grid (H, N), one workgroup of HD lanes per (head, row) ----------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(HD) void combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ o, int H, int nsplit) {
    const int64_t nh = (int64_t)blockIdx.y * H + blockIdx.x;
    combine_ranges<HD>(part, o, nh, nsplit, nsplit);
}

// the position in device memory (decode_split.h).  (The two grouped files have the kernel below: NH is not N * H there and a position
// below shared_len returns; through this template with those as arguments the three kernels here would not keep their instructions.)
template <int HD, int KEYS_PER_ITER>
__global__ __launch_bounds__(HD) void dyn_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ o, const int32_t* __restrict__ pos_dev,
                                                         int N, int H, int S_max, int cus, int max_ranges) {
    DYN_POSITION_OR_RETURN(KEYS_PER_ITER, pos, sp, pos_dev, S_max, (int64_t)N * H, cus);
    const int nsplit = min(sp.nsplit, max_ranges);
    if (nsplit == 1) return;                              // the one live workgroup wrote o itself
    const int64_t nh = (int64_t)blockIdx.y * H + blockIdx.x;
    combine_ranges<HD>(part, o, nh, nsplit, max_ranges);
}

// the same for a grouped step (decode_cache_shared.hip, decode_cache_shared_i8.hip): NH = (N / group) * H sizes the ranges, and a position
// below shared_len does nothing, as in the attention kernels
template <int HD, int KEYS_PER_ITER>
__global__ __launch_bounds__(HD) void shared_dyn_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ o,
                                                                const int32_t* __restrict__ pos_dev, int NH, int H, int S_max, int cus,
                                                                int max_ranges, int shared_len) {
    DYN_POSITION_OR_RETURN(KEYS_PER_ITER, pos, sp, pos_dev, S_max, (int64_t)NH, cus);
    if (pos < shared_len) return;
    const int nsplit = min(sp.nsplit, max_ranges);
    if (nsplit == 1) return;                              // the one live workgroup wrote o itself
    const int64_t nh = (int64_t)blockIdx.y * H + blockIdx.x;
    combine_ranges<HD>(part, o, nh, nsplit, max_ranges);
}

// ---- the checks (name: the entry point's, the prefix of every message; a: the entry point's Args, filled from its arguments) -------------
bool mult(int64_t m, std::initializer_list<int64_t> strides) {
    for (const int64_t s : strides)
        if (s % m != 0) return false;
    return true;
}

int require_pointers(const char* name, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs) OTTER_REQUIRE(p, "%s: null pointer", name);
    return OTTER_OK;
}

// what: "rows" (scalar entry points) or "table" (dyn)
int require_cos_sin_pair(const char* name, const float* cos, const float* sin, const char* what) {
    OTTER_REQUIRE((cos == nullptr) == (sin == nullptr), "%s: cos_%s and sin_%s must both be given or both be NULL", name, what, what);
    return OTTER_OK;
}

int require_shape(const char* name, int64_t head_dim, int HD, int64_t N, int64_t H) {
    OTTER_REQUIRE(head_dim == HD, "%s: head_dim %ld (%d only)", name, (long)head_dim, HD);
    OTTER_REQUIRE(N > 0 && H > 0 && N <= 65535 && H <= 65535, "%s: bad shape N=%ld H=%ld", name, (long)N, (long)H);
    return OTTER_OK;
}

int require_capacity(const char* name, int64_t S_max) {
    OTTER_REQUIRE(S_max >= 2 && S_max <= S_MAX_LIMIT, "%s: S_max=%ld outside [2, %ld]", name, (long)S_max, (long)S_MAX_LIMIT);
    return OTTER_OK;
}

int require_position(const char* name, int64_t pos, int64_t S_max) {
    OTTER_REQUIRE(pos >= 1, "%s: pos=%ld: a cached step continues a cache (pos >= 1)", name, (long)pos);
    OTTER_REQUIRE(pos < S_max, "%s: pos=%ld is beyond the cache capacity S_max=%ld", name, (long)pos, (long)S_max);
    return OTTER_OK;
}

// the two checks of a grouped step's grouping
int require_groups(const char* name, int64_t N, int64_t group) {
    OTTER_REQUIRE(group >= 2 && group <= OTTER_DECODE_CACHED_SHARED_MAX_GROUP, "%s: group=%ld: the kernel is built for groups of 2 to %d rows", name,
                  (long)group, OTTER_DECODE_CACHED_SHARED_MAX_GROUP);
    OTTER_REQUIRE(N % group == 0, "%s: N=%ld rows are not whole groups of %ld", name, (long)N, (long)group);
    return OTTER_OK;
}

// the shared prompt ends at or below the position (the in-place invariant of the grouped files): scalar entry points, after the position's
int require_shared_len(const char* name, int64_t shared_len, int64_t pos) {
    OTTER_REQUIRE(shared_len >= 1 && shared_len <= pos, "%s: shared_len=%ld outside [1, pos] with pos=%ld", name, (long)shared_len, (long)pos);
    return OTTER_OK;
}

// dyn entry points: below the capacity (the kernels return when the position they read is below shared_len)
int require_shared_len_dyn(const char* name, int64_t shared_len, int64_t S_max) {
    OTTER_REQUIRE(shared_len >= 1 && shared_len < S_max, "%s: shared_len=%ld outside [1, S_max) with S_max=%ld", name, (long)shared_len,
                  (long)S_max);
    return OTTER_OK;
}

// list: the pointers' names as the message gives them
int require_aligned16(const char* name, std::initializer_list<const void*> ptrs, const char* list) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    OTTER_REQUIRE((bits & 15) == 0, "%s: %s need 16-byte alignment", name, list);
    return OTTER_OK;
}

// the alignment group of the head_dim 128 files
template <typename Args>
int require_token_and_cache_aligned(const char* name, const Args& a) {
    return require_aligned16(name, {a.q, a.kn, a.vn, a.kc, a.vc}, "q, k_new, v_new, k_cache, v_cache");
}

// the two checks of the int8 files' scales: their alignment follows the codes', their head strides the codes'
template <typename Args>
int require_scales_aligned(const char* name, const Args& a) {
    OTTER_REQUIRE((((uintptr_t)a.ks | (uintptr_t)a.vs) & 3) == 0, "%s: k_scale, v_scale need 4-byte alignment", name);
    return OTTER_OK;
}

template <typename Args>
int require_scale_head_strides(const char* name, const Args& a, int64_t S_max) {
    OTTER_REQUIRE(a.ks_hs >= S_max && a.vs_hs >= S_max && a.ks_rs >= 0 && a.vs_rs >= 0,
                  "%s: a scale head stride below S_max would make the scales of two heads overlap", name);
    return OTTER_OK;
}

int require_pos_dev_aligned(const char* name, const int32_t* pos_dev) {
    OTTER_REQUIRE(((uintptr_t)pos_dev & 3) == 0, "%s: pos_dev needs 4-byte alignment", name);
    return OTTER_OK;
}

// the strides of the new token (t; null: Persimmon's packed token has none) are multiples of 8 elements, the cache's of cache_mult (8, or the
// 16 codes a lane of the int8 file loads): ONE check where the two multiples are the same, two otherwise.  Then the heads' slots are apart
template <typename Args>
int require_cache_layout(const char* name, const NewTokenArgs* t, const Args& a, int cache_mult, int64_t S_max, int HD) {
    const bool token = !t || mult(8, {t->q_rs, t->q_hs, t->kn_rs, t->kn_hs, t->vn_rs, t->vn_hs});
    const bool cache = mult(cache_mult, {a.kc_rs, a.kc_hs, a.vc_rs, a.vc_hs});
    if (!t) {
        OTTER_REQUIRE(cache, "%s: cache strides must be multiples of %d elements", name, cache_mult);
    } else if (cache_mult == 8) {
        OTTER_REQUIRE(token && cache, "%s: q / k_new / v_new / cache strides must be multiples of 8 elements", name);
    } else {
        OTTER_REQUIRE(token, "%s: q / k_new / v_new strides must be multiples of 8 elements", name);
        OTTER_REQUIRE(cache, "%s: code cache strides must be multiples of %d elements", name, cache_mult);
    }
    OTTER_REQUIRE(a.kc_hs >= S_max * HD && a.vc_hs >= S_max * HD && a.kc_rs >= 0 && a.vc_rs >= 0,
                  "%s: a cache head stride below S_max * %d would make the slots of two heads overlap", name, HD);
    return OTTER_OK;
}

// scalar entry points: the beam table and the mask hold the position.  cos_rs: the row stride of the rotary rows, null where the entry
// point has none (Persimmon: one row)
template <typename Args>
int require_row_strides(const char* name, const Args& a, const int64_t* cos_rs, int64_t pos) {
    OTTER_REQUIRE((!cos_rs || *cos_rs >= 0) && (!a.src || a.src_rs >= pos) && (!a.kvalid || a.kv_rs >= pos + 1),
                  "%s: src needs a row stride >= pos, key_valid one >= pos + 1%s", name, cos_rs ? ", cos / sin a non-negative one" : "");
    return OTTER_OK;
}

// dyn entry points: any position below S_max may be read from pos_dev, so the rotary tables (a.cs: null = none), the beam table and the
// mask must hold the capacity.  A table row is `width` floats wide, `width_text` in the message: 128, or Persimmon's rot
template <typename Args>
int require_table_strides(const char* name, const Args& a, int64_t table_rs, int64_t width, const char* width_text, int64_t S_max) {
    OTTER_REQUIRE((!a.cs || table_rs >= width) && (!a.src || a.src_rs >= S_max - 1) && (!a.kvalid || a.kv_rs >= S_max),
                  "%s: cos / sin tables need a row stride >= %s, src one >= S_max - 1, key_valid one >= S_max", name, width_text);
    return OTTER_OK;
}

int require_workspace(const char* name, int64_t workspace_bytes, int64_t need) {
    OTTER_REQUIRE(workspace_bytes >= need, "%s: workspace of %ld bytes, %ld needed", name, (long)workspace_bytes, (long)need);
    return OTTER_OK;
}

// ---- the launch sequence: the attention kernel over (ranges, H, Z), then, with more than one range, the combine kernel over (H, N) ---------
// `a` is a file's Args with everything but the position's fields set; `attention` launches the file's kernel (a callable: the grouped files
// switch over their group size, for_group below); Z is the grid's z extent (N, or the grouped files' N / group); name labels a failed launch.
int check_launch(const char* name, const char* stage) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) OTTER_FAIL(OTTER_ERR_LAUNCH, "%s%s: %s", name, stage, hipGetErrorString(e));
    return OTTER_OK;
}

template <typename Args, typename Attention, typename Combine>
int launch_ranges(const char* name, const Args& a, int ranges, int64_t Z, Attention&& attention, Combine&& combine) {
    attention(dim3((unsigned)ranges, (unsigned)a.H, (unsigned)Z));
    if (int e = check_launch(name, "")) return e;
    if (ranges > 1) {
        combine(dim3((unsigned)a.H, (unsigned)a.N));
        if (int e = check_launch(name, " (combine)")) return e;
    }
    return OTTER_OK;
}

// the position as a scalar: the grid has the sp.nsplit ranges of the position
template <int HD, typename Args, typename Attention>
int launch_scalar(const char* name, Args& a, int64_t pos, const Split sp, int64_t Z, void* stream, Attention&& attention) {
    a.pos = (int)pos; a.nsplit = sp.nsplit; a.kps = sp.kps; a.part_stride = sp.nsplit;
    hipStream_t st = (hipStream_t)stream;
    return launch_ranges(name, a, sp.nsplit, Z, [&](dim3 grid) { attention(grid, st, a); }, [&](dim3 grid) {
        hipLaunchKernelGGL(combine_kernel<HD>, grid, dim3(HD), 0, st, (const float*)a.part, a.o, a.H, sp.nsplit);
    });
}

// the position in device memory: the grid has the max_ranges ranges of the capacity, whatever pos_dev holds.  `combine` launches the file's
// dyn combine kernel (DynCombine or SharedDynCombine below)
struct DynStep { const int32_t* pos_dev; int S_max, cus, max_ranges; int64_t table_rs; };

template <typename Args, typename Attention, typename Combine>
int launch_dyn(const char* name, Args& a, const DynStep& d, int64_t Z, void* stream, Attention&& attention, Combine&& combine) {
    a.pos = 0; a.nsplit = 0; a.kps = 0; a.part_stride = d.max_ranges;   // (pos, nsplit, kps: read and derived on the device)
    hipStream_t st = (hipStream_t)stream;
    return launch_ranges(name, a, d.max_ranges, Z, [&](dim3 grid) { attention(grid, st, a, d); }, [&](dim3 grid) { combine(grid, st, a, d); });
}

// the combine of every file but the two grouped ones
template <int HD, int KEYS_PER_ITER>
struct DynCombine {
    template <typename Args>
    void operator()(dim3 grid, hipStream_t st, const Args& a, const DynStep& d) const {
        hipLaunchKernelGGL((dyn_combine_kernel<HD, KEYS_PER_ITER>), grid, dim3(HD), 0, st, (const float*)a.part, a.o, d.pos_dev, a.N, a.H, d.S_max,
                           d.cus, d.max_ranges);
    }
};

// the combine of the two grouped files: NH = (N / group) * H
template <int HD, int KEYS_PER_ITER>
struct SharedDynCombine {
    int64_t NH;
    template <typename Args>
    void operator()(dim3 grid, hipStream_t st, const Args& a, const DynStep& d) const {
        hipLaunchKernelGGL((shared_dyn_combine_kernel<HD, KEYS_PER_ITER>), grid, dim3(HD), 0, st, (const float*)a.part, a.o, d.pos_dev, (int)NH, a.H,
                           d.S_max, d.cus, d.max_ranges, a.shared_len);
    }
};

// the instances of a grouped attention kernel: one per group size (OTTER_DECODE_CACHED_SHARED_MAX_GROUP of include/otter_hip.h).  f(G)
// with G an integral constant; require_groups has passed
template <typename F>
void for_group(int64_t group, F&& f) {
    switch (group) {
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        default: f(std::integral_constant<int, 6>()); break;
    }
}

static_assert(OTTER_DECODE_CACHED_SHARED_MAX_GROUP == 6, "for_group: one instance per group size up to the header's limit");

}  // namespace
