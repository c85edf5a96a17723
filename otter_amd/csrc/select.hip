// select.hip -- the token selection of generate() (otter_amd/generation.py: generate_tokens, num_beams == 1) on the device, ONE launch per step:
// from the processed fp32 scores [N, V] the step's token of every row -- the row maximum (greedy) or a draw under temperature / top-k / top-p
// (sample) -- is written into column L of the preallocated history ids_buf [N, max_len], with the unfinished / eos bookkeeping of the host loop.
// The scores are never written.  include/otter_hip.h states the rule; in short, for one row in sample mode:
//     s'_j  = fp32(s_j * inv_temperature)                              (rounded before anything else uses it; -0 counts as +0)
//     top-k   keep s'_j >= v_k, the k-th largest s' (all ties at v_k stay)
//     top-p   over those, keep a value v iff  sum of w_j over s'_j <= v  >  floor((1 - top_p) * Z),   w_j = floor(expf(s'_j - m) * 2^40), Z = sum w
//     draw    the kept j that maximises expf(s'_j - m) / q_j (IEEE fp32), the smaller j among equal ratios
// Both thresholds are found WITHOUT sorting the row by a most-significant-digit-first radix select over the order-preserving 32-bit key of s'
// (11 + 11 + 10 bits): three histogram passes for the count (top-k), three for the mass (top-p), each followed by a workgroup-wide prefix scan
// over the 2048 bins that finds the bin the threshold lies in.  The histograms are INTEGER: counts, and the softmax numerators as 64-bit fixed
// point (at most 2^18 terms of at most 2^40), so neither arrival order nor summation order can move a threshold -- the same inputs give the same
// token on every call.  The race needs no normalisation (the arg max does not depend on Z) and no ordered scan.
//
// Shape: one workgroup of 1024 threads (16 waves) per row; nothing crosses workgroups but the one integer atomic on n_unfinished.  The row is
// read once (greedy) or 2 + 3 [top-k] + 3 [top-p] times (sample) with 16-byte loads, eight in flight per thread, once the row pointer is
// 16-byte aligned (scalar head and tail: the row stride is free).  With top-k on, the first digit of v_k bounds the candidates: when at most
// 2048 columns lie in its bin or above (the count is in the histogram, so the decision is the same on every call) one sweep compacts them
// into LDS, and every later pass -- the other two digits, top-p and the race -- reads that list: the row is read 4 times in all.  The list's
// order depends on arrival, its consumers (maxima with an index tie-break, integer sums) do not.  LDS: the 16 KiB histogram, the 16 KiB list
// and a few reduction slots.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int NT = 1024;
constexpr int NW = NT / OTTER_WAVE;
constexpr int UNROLL = 8;                         // 16-byte loads a thread keeps in flight: one workgroup reads a whole row, latency is the cost
constexpr int LIST_CAP = 2048;                    // candidates of top-k kept in LDS after the first digit (16 KiB)
constexpr int BINS = 2048;                        // 11-bit digits; the last digit has 10 bits and uses the lower half
constexpr int64_t V_MAX = 262144;
constexpr int64_t LEN_MAX = (int64_t)1 << 30;
constexpr float FX_ONE = 1099511627776.0f;        // 2^40: the fixed-point unit of a softmax numerator

struct SelArgs {
    const float* scores; int64_t s_rs;            // [N, V], row stride in elements
    const float* q; int64_t q_rs;                 // [N, V] exponential draws (sample mode)
    int64_t* ids; int64_t i_rs; int64_t L;        // [N, max_len], row stride in elements; column L is written
    uint8_t* unfinished; int32_t* n_unfinished;
    const int32_t* eos; int n_eos;
    int64_t pad;
    int V, k;                                     // k: 0 = top-k off, else min(max(top_k, 1), V)
    float inv_t;
    double omp;                                   // 1 - top_p, <= 0: top-p off
};

// a is a better maximum than b: torch.argmax's order -- NaN above everything, the first index among equals (-0 == +0)
__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || ai < bi);
    return av > bv || (av == bv && ai < bi);
}

// ascending order-preserving key of a non-NaN float
__device__ __forceinline__ uint32_t fkey(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// s' = fp32(s * inv_t): __fmul_rn is never contracted into the subtraction of the maximum; -0 becomes +0 so that keys order as values compare
__device__ __forceinline__ float scaled(float s, float inv_t) {
    const float x = __fmul_rn(s, inv_t);
    return x == 0.f ? 0.f : x;
}

// f(value, column) for every column of the row, each exactly once; the visiting order is free (every consumer is order-independent)
template <typename F>
__device__ __forceinline__ void for_row(const float* s, int V, int tid, F f) {
    int head = (int)(((16u - (unsigned)((uintptr_t)s & 15u)) & 15u) >> 2);
    if (head > V) head = V;
    if (tid < head) f(s[tid], tid);
    const int nvec = (V - head) >> 2;
    const float4* v4 = reinterpret_cast<const float4*>(s + head);
    int i = tid;
    for (; i + (UNROLL - 1) * NT < nvec; i += UNROLL * NT) {        // UNROLL independent 16-byte loads in flight per thread, then their use
        float4 x[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) x[u] = v4[i + u * NT];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int j = head + 4 * (i + u * NT);
            f(x[u].x, j); f(x[u].y, j + 1); f(x[u].z, j + 2); f(x[u].w, j + 3);
        }
    }
    for (; i < nvec; i += NT) {
        const float4 x = v4[i];
        const int j = head + 4 * i;
        f(x.x, j); f(x.y, j + 1); f(x.z, j + 2); f(x.w, j + 3);
    }
    const int done = head + 4 * nvec;
    if (tid < V - done) f(s[done + tid], done + tid);
}

struct Red {                                      // the reduction slots of the workgroup
    float v[NW]; int i[NW];
    unsigned long long t[NW];
    unsigned long long found[2];
};

// (value, index) of the best element over the workgroup, in every thread
__device__ __forceinline__ void block_best(float& v, int& i, Red& r, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    __syncthreads();                              // (the slots' previous readers are done)
    if ((tid & 63) == 0) { r.v[tid >> 6] = v; r.i[tid >> 6] = i; }
    __syncthreads();
    v = r.v[0]; i = r.i[0];
#pragma unroll
    for (int w = 1; w < NW; ++w)
        if (better(r.v[w], r.i[w], v, i)) { v = r.v[w]; i = r.i[w]; }
}

__device__ __forceinline__ unsigned long long block_sum(unsigned long long x, Red& r, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) r.t[tid >> 6] = x;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += r.t[w];
    return s;
}

// The first bin, in scan order (descending bins if `reverse`), whose inclusive prefix sum exceeds `target`; `excl` = the sum of the bins before
// it.  The caller guarantees target < the sum of all bins and a barrier between the last histogram update and this call.  Ends with a barrier
// after every read of h, so the caller may clear it at once.
template <typename T>
__device__ __forceinline__ int block_find(const T* h, unsigned long long target, bool reverse, unsigned long long& excl, Red& r, int tid) {
    const int p0 = 2 * tid, p1 = p0 + 1;                             // BINS == 2 * NT positions in scan order
    const unsigned long long a = h[reverse ? BINS - 1 - p0 : p0], b = h[reverse ? BINS - 1 - p1 : p1];
    unsigned long long inc = a + b;
    const int lane = tid & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) r.t[tid >> 6] = inc;
    __syncthreads();
    unsigned long long before = inc - (a + b);
    for (int w = 0; w < (tid >> 6); ++w) before += r.t[w];
    if (before <= target && target < before + a) { r.found[0] = (unsigned long long)p0; r.found[1] = before; }
    else if (before + a <= target && target < before + a + b) { r.found[0] = (unsigned long long)p1; r.found[1] = before + a; }
    __syncthreads();
    const int p = (int)r.found[0];
    excl = r.found[1];
    return reverse ? BINS - 1 - p : p;
}

template <bool SAMPLE>
__global__ __launch_bounds__(NT) void select_step_kernel(SelArgs a) {
    __shared__ unsigned long long hist[SAMPLE ? BINS : 1];
    __shared__ float list_v[SAMPLE ? LIST_CAP : 1];                  // the compacted candidates: s' ...
    __shared__ int list_j[SAMPLE ? LIST_CAP : 1];                    // ... and column
    __shared__ int list_n;
    __shared__ Red red;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const float* s = a.scores + row * a.s_rs;
    const int V = a.V;
    const float inv_t = a.inv_t;

    // ---- the row maximum and its first index (of s in greedy mode, of s' in sample mode; a NaN is the maximum) ----
    // A thread meets its columns in ascending order, so "strictly greater, or the first NaN" keeps the first index; a thread that met nothing
    // above -inf keeps INT_MAX, and a row of -inf alone ends at column 0 below.
    float m = -INFINITY;
    int am = INT_MAX;
    for_row(s, V, tid, [&](float x, int j) {
        if (SAMPLE) x = scaled(x, inv_t);
        if (!(x <= m) && m == m) { m = x; am = j; }
    });
    block_best(m, am, red, tid);
    if (am == INT_MAX) am = 0;
    int sel = am;

    if (SAMPLE && m == m && fabsf(m) != INFINITY) {                   // (a row with a NaN or without a finite score keeps the arg max: any token)
        uint32_t* h32 = reinterpret_cast<uint32_t*>(hist);
        unsigned long long excl;
        uint32_t thr = 0;                                            // the kept set is key(s') >= thr
        int n_list = -1;                                             // >= 0: the passes below read the compacted list, not the row
        // f(s', column) over the row, or over the candidates once they are compacted (in no particular order: every consumer is a maximum
        // or an integer sum)
        auto each = [&](auto f) {
            if (n_list >= 0) {
                for (int i = tid; i < n_list; i += NT) f(list_v[i], list_j[i]);
            } else {
                for_row(s, V, tid, [&](float x, int j) { f(scaled(x, inv_t), j); });
            }
        };
        if (a.k > 0 && a.k < V) {
            // ---- v_k: the k-th largest key, digit by digit ----
            unsigned long long k_rem = (unsigned long long)a.k;
            for (int pass = 0; pass < 3; ++pass) {
                const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
                const int up = pass == 0 ? 32 : pass == 1 ? 21 : 10;         // the digits above `up` are decided
                const uint32_t mask = (1u << (up - shift)) - 1u;
                for (int w = tid; w < BINS; w += NT) hist[w] = 0ull;
                if (pass == 0 && tid == 0) list_n = 0;               // (the compaction's cursor: written in pass 0 only, never read back)
                __syncthreads();
                const uint32_t pre = thr;
                each([&](float sp, int) {
                    const uint32_t key = fkey(sp);
                    if (pass == 0 || (key >> up) == pre) atomicAdd(&h32[(key >> shift) & mask], 1u);
                });
                __syncthreads();
                const int bin = block_find(h32, k_rem - 1, true, excl, red, tid);
                if (pass == 0) {
                    // everything top-k can keep lies in this bin or above it: when that is at most LIST_CAP columns (the usual case: top_k is
                    // tens, a bin spans a quarter of a binade), one more sweep compacts them into LDS and the row is not read again
                    const unsigned long long n_cand = excl + h32[bin];
                    __syncthreads();                                 // (h32[bin] is read before the next pass clears it)
                    if (n_cand <= (unsigned long long)LIST_CAP) {
                        const uint32_t lo = (uint32_t)bin << 21;
                        for_row(s, V, tid, [&](float x, int j) {
                            const float sp = scaled(x, inv_t);
                            if (fkey(sp) < lo) return;
                            const int at = atomicAdd(&list_n, 1);    // at < n_cand <= LIST_CAP: the histogram counted these very columns
                            list_v[at] = sp;
                            list_j[at] = j;
                        });
                        __syncthreads();
                        n_list = (int)n_cand;                        // (uniform, from the histogram: the shared cursor is not read back)
                    }
                }
                k_rem -= excl;
                thr = (thr << (up - shift)) | (uint32_t)bin;
            }
        }
        if (a.omp > 0.0) {
            // ---- the smallest kept value of top-p: the first key, ascending over the top-k survivors, whose inclusive mass exceeds R ----
            const uint32_t kth = thr;
            unsigned long long R = 0;
            uint32_t pre = 0;
            for (int pass = 0; pass < 3; ++pass) {
                const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
                const int up = pass == 0 ? 32 : pass == 1 ? 21 : 10;
                const uint32_t mask = (1u << (up - shift)) - 1u;
                for (int w = tid; w < BINS; w += NT) hist[w] = 0ull;
                __syncthreads();
                unsigned long long z = 0;
                const uint32_t pr = pre;
                each([&](float sp, int) {
                    const uint32_t key = fkey(sp);
                    if (key < kth || !(pass == 0 || (key >> up) == pr)) return;
                    const unsigned long long w = (unsigned long long)(expf(sp - m) * FX_ONE);
                    if (w == 0ull) return;
                    z += w;
                    atomicAdd(&hist[(key >> shift) & mask], w);
                });
                if (pass == 0) {
                    const unsigned long long Z = block_sum(z, red, tid);     // >= 2^40: the maximum's own numerator
                    R = (unsigned long long)(a.omp * (double)Z);             // floor((1 - top_p) * Z) ...
                    if (R > Z - 1) R = Z - 1;                                // ... below Z: the maximum is always kept
                }
                __syncthreads();
                const int bin = block_find(hist, R, false, excl, red, tid);
                R -= excl;
                pre = (pre << (up - shift)) | (uint32_t)bin;
            }
            thr = pre;
        }
        // ---- the exponential race over the kept set ----
        const float* q = a.q + row * a.q_rs;
        float bv = -1.f;
        int bi = am;                                                 // (the maximum is always kept and its ratio is > 0: it replaces this)
        each([&](float sp, int j) {
            if (fkey(sp) < thr) return;
            const float ratio = expf(sp - m) / q[j];
            if (ratio > bv || (ratio == bv && j < bi)) { bv = ratio; bi = j; }
        });
        block_best(bv, bi, red, tid);
        sel = bi;
    }

    // ---- bookkeeping: the host loop's where / isin / any ----
    if (tid == 0) {
        const bool live = a.unfinished[row] != 0;
        a.ids[row * a.i_rs + a.L] = live ? (int64_t)sel : a.pad;
        if (live) {
            bool is_eos = false;
            for (int e = 0; e < a.n_eos; ++e) is_eos |= a.eos[e] == sel;
            if (is_eos) {
                a.unfinished[row] = 0;
                atomicSub(a.n_unfinished, 1);
            }
        }
    }
}

}  // namespace

extern "C" {

int otter_select_step(const float* scores, int64_t scores_stride, int64_t N, int64_t V, int64_t* ids_buf, int64_t ids_stride, int64_t L,
                      int64_t max_len, int mode, float inv_temperature, int64_t top_k, double top_p, const float* q, int64_t q_stride,
                      uint8_t* unfinished, int32_t* n_unfinished, const int32_t* eos, int64_t n_eos, int64_t pad_token_id, void* stream) {
    OTTER_REQUIRE(scores && ids_buf && unfinished && n_unfinished, "select_step: null pointer (scores / ids_buf / unfinished / n_unfinished)");
    OTTER_REQUIRE(mode == OTTER_SELECT_GREEDY || mode == OTTER_SELECT_SAMPLE, "select_step: mode=%d is neither greedy (0) nor sample (1)", mode);
    OTTER_REQUIRE(N >= 1 && N <= INT32_MAX, "select_step: N=%ld outside 1..2^31-1", (long)N);
    OTTER_REQUIRE(V >= 1 && V <= V_MAX, "select_step: V=%ld outside 1..%ld", (long)V, (long)V_MAX);
    OTTER_REQUIRE(max_len >= 1 && max_len <= LEN_MAX, "select_step: max_len=%ld outside 1..%ld", (long)max_len, (long)LEN_MAX);
    OTTER_REQUIRE(L >= 0 && L < max_len, "select_step: L=%ld outside 0..max_len-1 (max_len=%ld)", (long)L, (long)max_len);
    OTTER_REQUIRE(scores_stride >= V && ids_stride >= max_len,
                  "select_step: a row stride below the row length (scores %ld < V=%ld or ids_buf %ld < max_len=%ld)", (long)scores_stride, (long)V,
                  (long)ids_stride, (long)max_len);
    if (mode == OTTER_SELECT_SAMPLE) {
        OTTER_REQUIRE(top_k >= 0, "select_step: top_k=%ld must be >= 0 (0 = off)", (long)top_k);
        OTTER_REQUIRE(top_p > 0.0 && top_p <= 1.0, "select_step: top_p=%g outside (0, 1] (1 = off)", top_p);
        OTTER_REQUIRE(isfinite(inv_temperature) && inv_temperature > 0.f, "select_step: inv_temperature=%g must be finite and > 0",
                      (double)inv_temperature);
        OTTER_REQUIRE(q != nullptr, "select_step: null pointer: sample mode needs q, the exponential draws");
        OTTER_REQUIRE(q_stride >= V, "select_step: a row stride below the row length (q %ld < V=%ld)", (long)q_stride, (long)V);
    }
    OTTER_REQUIRE(n_eos >= 0 && n_eos <= INT32_MAX, "select_step: eos list length out of range (n_eos=%ld)", (long)n_eos);
    OTTER_REQUIRE(eos || n_eos == 0, "select_step: null pointer for a non-empty eos list");
    OTTER_REQUIRE(((uintptr_t)scores & 3) == 0 && ((uintptr_t)q & 3) == 0 && ((uintptr_t)ids_buf & 7) == 0 && ((uintptr_t)n_unfinished & 3) == 0 &&
                      ((uintptr_t)eos & 3) == 0,
                  "select_step: alignment (scores, q, n_unfinished and eos 4 bytes, ids_buf 8 bytes)");

    SelArgs a;
    a.scores = scores; a.s_rs = scores_stride;
    a.q = q; a.q_rs = q_stride;
    a.ids = ids_buf; a.i_rs = ids_stride; a.L = L;
    a.unfinished = unfinished; a.n_unfinished = n_unfinished;
    a.eos = eos; a.n_eos = (int)n_eos;
    a.pad = pad_token_id;
    a.V = (int)V;
    a.k = top_k > 0 ? (int)(top_k < V ? top_k : V) : 0;
    a.inv_t = inv_temperature;
    a.omp = 1.0 - top_p;
    if (mode == OTTER_SELECT_SAMPLE)
        hipLaunchKernelGGL(select_step_kernel<true>, dim3((unsigned)N), dim3(NT), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(select_step_kernel<false>, dim3((unsigned)N), dim3(NT), 0, (hipStream_t)stream, a);
    OTTER_CHECK_LAUNCH("select_step");
    return OTTER_OK;
}

}  // extern "C"
