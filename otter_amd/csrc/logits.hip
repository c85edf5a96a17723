// logits.hip -- the tensor-valued logits processors of generate() (otter_amd/generation.py: _Processors) on the device, ONE launch per step:
// the [N, V] fp32 score matrix is edited in place from the token history ids [N, L] that generate_tokens already keeps on the device.  No host
// round trip, no Python loop over positions.  In this order, exactly the host loop's semantics:
//     1. repetition penalty p != 1   every DISTINCT token t of the row: s = scores[r, t];  scores[r, t] = s < 0 ? s * p : s * (1 / p)
//     2. no-repeat n-gram, L + 1 >= n   n == 1: ban every token of the row;  n > 1: ban ids[r, i + n - 1] wherever ids[r, i : i + n - 1] equals the
//                                       row's last n - 1 tokens, 0 <= i <= L - n
//     3. the always-banned tokens (one-token bad words)
//     4. multi-token bad words       word w of m >= 2 tokens: ban w[m - 1] if m - 1 <= L and the row ends in w[0 : m - 1]
//     5. the eos list, when the host says "suppress this step" (min_length / min_new_tokens)
// A ban writes -inf and wins over the penalty.  A token outside [0, V) penalises nothing, bans nothing and is never an index; as a VALUE it still
// takes part in the n-gram and word comparisons.
//
// "s / p" is "s * (1 / p)": torch's device kernel for `tensor / Python scalar` multiplies by the reciprocal it computed on the host in fp32
// (kv_cache.py's note), and the yardstick is that path on the same device, bit for bit.  1 / p is computed once in otter_logits_process.
//
// Shape: one workgroup of 256 threads per row -- O(L) compares and a handful of stores, nothing crosses workgroups.  A token that occurs k times
// must be penalised ONCE (the host gathers, then scatters): a V-bit ownership bitmap in LDS (32 KiB at the cap V = 262144), filled with LDS
// atomics; the thread that sets a token's bit applies its penalty.  A workgroup barrier orders the penalty phase before the bans, so that a
// banned token ends as -inf whichever thread penalised it.  Several threads may ban one token: they store the same value.
#include "common.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int64_t V_MAX = 262144;                 // the bitmap: V_MAX / 32 words of LDS
constexpr int64_t L_MAX = (int64_t)1 << 30;

struct LpArgs {
    float* scores; int64_t s_rs;                  // [N, V], row stride in elements
    const int64_t* ids; int64_t i_rs;             // [N, L], row stride in elements
    int V, L, n;
    float p, inv_p;                               // p == 1: no penalty phase
    const int32_t *ban, *eos;                     // eos: NULL / n_eos == 0 unless this step suppresses it
    int n_ban, n_eos;
    const int32_t *w_tok, *w_off;                 // words: tokens [w_off[n_words]], offsets [n_words + 1]
    int n_words;
};

__global__ __launch_bounds__(NT) void logits_process_kernel(LpArgs a) {
    __shared__ uint32_t seen[V_MAX / 32];
    const int tid = threadIdx.x;
    float* s = a.scores + (int64_t)blockIdx.x * a.s_rs;
    const int64_t* ids = a.ids + (int64_t)blockIdx.x * a.i_rs;
    const int64_t V = a.V;
    const int L = a.L;

    if (a.p != 1.0f) {                            // (uniform over the workgroup: both barriers are reached by all threads or by none)
        const int words = (a.V + 31) >> 5;
        for (int w = tid; w < words; w += NT) seen[w] = 0u;
        __syncthreads();
        for (int i = tid; i < L; i += NT) {
            const int64_t t = ids[i];
            if (t < 0 || t >= V) continue;
            const uint32_t bit = 1u << ((int)t & 31);
            if (atomicOr(&seen[(int)t >> 5], bit) & bit) continue;   // another position of the row owns this token
            const float v = s[t];
            s[t] = v < 0.f ? v * a.p : v * a.inv_p;
        }
        __syncthreads();                          // penalties are written before any ban of the same element
    }

    const float ninf = -INFINITY;
    const int n = a.n;
    if (n == 1) {
        for (int i = tid; i < L; i += NT) {
            const int64_t t = ids[i];
            if (t >= 0 && t < V) s[t] = ninf;
        }
    } else if (n > 1 && L + 1 >= n) {
        const int64_t* prefix = ids + (L - n + 1);                   // the row's last n - 1 tokens
        for (int i = tid; i <= L - n; i += NT) {
            int j = 0;
            while (j < n - 1 && ids[i + j] == prefix[j]) ++j;
            if (j < n - 1) continue;
            const int64_t t = ids[i + n - 1];
            if (t >= 0 && t < V) s[t] = ninf;
        }
    }
    for (int i = tid; i < a.n_ban; i += NT) {
        const int t = a.ban[i];
        if (t >= 0 && t < V) s[t] = ninf;
    }
    for (int w = tid; w < a.n_words; w += NT) {
        const int o = a.w_off[w], k = a.w_off[w + 1] - o - 1;       // k tokens to match, then the banned one
        if (k < 1 || k > L) continue;
        const int64_t* tail = ids + (L - k);
        int j = 0;
        while (j < k && tail[j] == (int64_t)a.w_tok[o + j]) ++j;
        if (j < k) continue;
        const int t = a.w_tok[o + k];
        if (t >= 0 && t < V) s[t] = ninf;
    }
    for (int i = tid; i < a.n_eos; i += NT) {
        const int t = a.eos[i];
        if (t >= 0 && t < V) s[t] = ninf;
    }
}

}  // namespace

extern "C" {

int otter_logits_process(float* scores, int64_t scores_stride, const int64_t* ids, int64_t ids_stride, int64_t N, int64_t V, int64_t L,
                         float repetition_penalty, int no_repeat_ngram, const int32_t* ban, int64_t n_ban, const int32_t* eos, int64_t n_eos,
                         int suppress_eos, const int32_t* word_tokens, const int32_t* word_offsets, int64_t n_words, void* stream) {
    OTTER_REQUIRE(scores && ids, "logits_process: null pointer (scores / ids)");
    OTTER_REQUIRE(n_ban >= 0 && n_eos >= 0 && n_words >= 0 && n_ban <= INT32_MAX && n_eos <= INT32_MAX && n_words < INT32_MAX,
                  "logits_process: list lengths out of range (n_ban=%ld n_eos=%ld n_words=%ld)", (long)n_ban, (long)n_eos, (long)n_words);
    OTTER_REQUIRE((ban || n_ban == 0) && (eos || n_eos == 0), "logits_process: null pointer for a non-empty list (ban / eos)");
    OTTER_REQUIRE(n_words == 0 || (word_tokens && word_offsets), "logits_process: null pointer: n_words=%ld needs word_tokens and word_offsets",
                  (long)n_words);
    OTTER_REQUIRE(N >= 1 && N <= INT32_MAX, "logits_process: N=%ld outside 1..2^31-1", (long)N);
    OTTER_REQUIRE(V >= 1 && V <= V_MAX, "logits_process: V=%ld outside 1..%ld (the ownership bitmap)", (long)V, (long)V_MAX);
    OTTER_REQUIRE(L >= 1 && L <= L_MAX, "logits_process: L=%ld outside 1..%ld", (long)L, (long)L_MAX);
    OTTER_REQUIRE(scores_stride >= V && ids_stride >= L, "logits_process: a row stride below the row length (scores %ld < V=%ld or ids %ld < L=%ld)",
                  (long)scores_stride, (long)V, (long)ids_stride, (long)L);
    OTTER_REQUIRE(isfinite(repetition_penalty) && repetition_penalty > 0.f, "logits_process: repetition_penalty=%g must be finite and > 0",
                  (double)repetition_penalty);
    OTTER_REQUIRE(no_repeat_ngram >= 0, "logits_process: no_repeat_ngram=%d must be >= 0", no_repeat_ngram);
    OTTER_REQUIRE(((uintptr_t)scores & 3) == 0 && ((uintptr_t)ids & 7) == 0 &&
                      (((uintptr_t)ban | (uintptr_t)eos | (uintptr_t)word_tokens | (uintptr_t)word_offsets) & 3) == 0,
                  "logits_process: alignment (scores and the int32 lists 4 bytes, ids 8 bytes)");

    LpArgs a;
    a.scores = scores; a.s_rs = scores_stride;
    a.ids = ids; a.i_rs = ids_stride;
    a.V = (int)V; a.L = (int)L; a.n = no_repeat_ngram;
    a.p = repetition_penalty; a.inv_p = 1.0f / repetition_penalty;
    a.ban = ban; a.n_ban = (int)n_ban;
    a.eos = eos; a.n_eos = suppress_eos ? (int)n_eos : 0;
    a.w_tok = word_tokens; a.w_off = word_offsets; a.n_words = (int)n_words;
    hipLaunchKernelGGL(logits_process_kernel, dim3((unsigned)N), dim3(NT), 0, (hipStream_t)stream, a);
    OTTER_CHECK_LAUNCH("logits_process");
    return OTTER_OK;
}

}  // extern "C"
