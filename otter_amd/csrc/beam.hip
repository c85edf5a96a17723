// beam.hip -- one beam-search step of generate() (otter_amd/generation.py: the plain beam-search branch of generate_tokens) on the device, TWO
// launches per step: candidate selection over the [B, nb * V] sums, BeamSearchScorer.process with its hypothesis lists, and the reorder of the
// token history.  No host round trip, no allocation; every piece of state lives in caller-owned buffers at fixed addresses.
//
// Selection.  For sentence b the candidates are s(j, t) = logp[b * nb + j, t] + beam_scores[b * nb + j] (ONE fp32 add, the add torch does), and
// the step keeps the n_cand largest in descending order.  Order: the larger sum first; among equal sums (-0 equals +0, -inf is an ordinary
// value) the smaller flat index j * V + t first.  Both go into one 64-bit key -- high word: the sum's bits made monotone, low word: ~flat --
// so that "better" is "larger key", keys are distinct, and the n_cand best are found by repeated maxima below the previous maximum.  Key 0 is
// no candidate (the low word of a real key has its top bit set: flat < 2^31): it pads the list of a chunk that holds fewer than n_cand values.
//     beam_select_kernel   one workgroup per (row b * nb + j, chunk of CHUNK columns): the chunk's 16 values per thread stay in registers as
//                          keys; n_cand rounds of (thread maximum below the last one, wave64 butterfly, 4 words of LDS) write the chunk's own
//                          top n_cand to the workspace.  A chunk keeps n_cand entries, not one: all winners can sit in one chunk.
//     beam_score_kernel    one workgroup per sentence: the same n_cand rounds over the sentence's partial lists give the sorted candidates;
//                          thread 0 then runs the scorer serially (at most n_cand iterations of scalar work), and the whole workgroup copies
//                          the rows it decided on: new hypotheses into their slots, and row r of the next ids = ids[beam_idx[r], :L] + token.
//
// Scorer.  _BeamHyps.add / is_done and the loop body, literally.  Hypothesis arithmetic is fp64 as Python's is: score = (double)sum /
// len_pow[generated_len] with the table the host filled from the Python expression, so no pow runs here and the quotients are the host's bits.
// The lists keep insertion order in hyp_score / hyp_len / hyp_slot; the token rows do not move: hyp_slot[b, i] names the physical row of list
// entry i in hyp_tokens[b].  While a list is short an entry takes slot = its position; the overflow delete (lowest (score, list index) of the
// nb + 1 entries, `worst` := the second lowest score) frees the slot the new entry takes.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int EPT = 16;                           // values per thread of the selection pass, in registers
constexpr int CHUNK = NT * EPT;                   // 4096 columns per workgroup
constexpr int MAX_CAND = OTTER_BEAM_STEP_MAX_CANDIDATES;

struct BeamArgs {
    const float* logp; int64_t lp_rs;             // [B * nb, V], row stride in elements
    float* beam_scores;                           // [B * nb], in and out
    const int64_t* ids; int64_t i_rs;             // [B * nb, L]
    int64_t* ids_next; int64_t n_rs;              // [B * nb, L + 1]
    int64_t* beam_idx;                            // [B * nb]
    const int32_t* eos; int n_eos;
    int64_t pad;
    int B, nb, V, n_cand, L, L0, max_len, early, lp_positive, chunks;
    const double* len_pow;                        // [max_len - L0 + 1]
    int32_t* done;                                // [B]
    double* hyp_score; int64_t* hyp_tokens; int32_t *hyp_len, *hyp_slot, *hyp_count; double* hyp_worst;
    int32_t* all_done;                            // [2]: the flag, the number of finished sentences
    unsigned long long* ws;                       // [B * nb, chunks, n_cand] keys
};

// the bits of a non-NaN float as an unsigned number that grows with the value; -0 and +0 give the same word
__device__ __forceinline__ uint32_t order_bits(float s) {
    const uint32_t u = __float_as_uint(s == 0.f ? 0.f : s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long make_key(float s, uint32_t flat) {
    return ((unsigned long long)order_bits(s) << 32) | (unsigned long long)(uint32_t)~flat;
}

// maximum over the workgroup, returned to every thread; red: 4 words of LDS
__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long r = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) r = red[i] > r ? red[i] : r;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(NT) void beam_select_kernel(BeamArgs a) {
    __shared__ unsigned long long red[NT / 64];
    const int tid = threadIdx.x;
    const int row = blockIdx.y, c = blockIdx.x;
    if (a.done[row / a.nb]) return;                // (uniform) a finished sentence selects nothing
    const float* lp = a.logp + (int64_t)row * a.lp_rs;
    const float bs = a.beam_scores[row];
    const uint32_t flat0 = (uint32_t)(row % a.nb) * (uint32_t)a.V;
    unsigned long long key[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int t = c * CHUNK + k * NT + tid;
        key[k] = t < a.V ? make_key(lp[t] + bs, flat0 + (uint32_t)t) : 0ull;
    }
    unsigned long long* out = a.ws + ((int64_t)row * a.chunks + c) * a.n_cand;
    unsigned long long last = ~0ull;
    for (int r = 0; r < a.n_cand; ++r) {
        unsigned long long m = 0ull;
#pragma unroll
        for (int k = 0; k < EPT; ++k) m = (key[k] < last && key[k] > m) ? key[k] : m;
        m = block_max(m, red);
        if (tid == 0) out[r] = m;
        last = m;
    }
}

__global__ __launch_bounds__(NT) void beam_score_kernel(BeamArgs a) {
    __shared__ unsigned long long red[NT / 64];
    __shared__ unsigned long long top[MAX_CAND];
    __shared__ float old_bs[MAX_CAND], n_score[MAX_CAND], c_score[MAX_CAND];
    __shared__ int c_eos[MAX_CAND];
    __shared__ int64_t n_tok[MAX_CAND];
    __shared__ int n_idx[MAX_CAND], task_row[MAX_CAND], task_slot[MAX_CAND], n_task;
    const int tid = threadIdx.x;
    const int b = blockIdx.x, nb = a.nb, L = a.L;
    const bool was_done = a.done[b] != 0;

    if (!was_done) {
        if (tid < nb) old_bs[tid] = a.beam_scores[b * nb + tid];
        const int64_t P = (int64_t)nb * a.chunks * a.n_cand;
        const unsigned long long* part = a.ws + (int64_t)b * P;
        unsigned long long last = ~0ull;
        for (int r = 0; r < a.n_cand; ++r) {
            unsigned long long m = 0ull;
            for (int64_t i = tid; i < P; i += NT) {
                const unsigned long long k = part[i];
                m = (k < last && k > m) ? k : m;
            }
            m = block_max(m, red);
            if (tid == 0) top[r] = m;
            last = m;
        }
        __syncthreads();
        if (tid < a.n_cand && top[tid] != 0ull) {  // every candidate's sum (its own bits: the key folds -0 into +0) and eos flag, side by side
            const uint32_t flat = ~(uint32_t)top[tid];
            const int j = (int)(flat / (uint32_t)a.V), tok = (int)(flat % (uint32_t)a.V);
            c_score[tid] = a.logp[((int64_t)b * nb + j) * a.lp_rs + tok] + old_bs[j];
            int e = 0;
            while (e < a.n_eos && a.eos[e] != tok) ++e;
            c_eos[tid] = e < a.n_eos;
        }
    }
    __syncthreads();

    if (tid == 0) {
        int tasks = 0;
        if (was_done) {                            // padded beams of a finished sentence
            for (int k = 0; k < nb; ++k) { n_score[k] = 0.f; n_tok[k] = a.pad; n_idx[k] = b * nb; }
        } else {
            const int g = L + 1 - a.L0;            // generated_len of a hypothesis added at this step; cur_len - prompt_len of is_done
            double* hs = a.hyp_score + (int64_t)b * nb;
            int32_t* hl = a.hyp_len + (int64_t)b * nb;
            int32_t* hslot = a.hyp_slot + (int64_t)b * nb;
            int count = a.hyp_count[b];
            double worst = a.hyp_worst[b];
            for (int k = 0; k < nb; ++k) { n_score[k] = 0.f; n_tok[k] = a.pad; n_idx[k] = 0; }
            int k = 0;
            float best = 0.f;
            for (int rank = 0; rank < a.n_cand && k < nb; ++rank) {
                const unsigned long long key = top[rank];
                if (key == 0ull) break;            // (n_cand <= nb * V: never, short of NaN scores)
                const uint32_t flat = ~(uint32_t)key;
                const int j = (int)(flat / (uint32_t)a.V), tok = (int)(flat % (uint32_t)a.V);
                const int row = b * nb + j;
                const float sc = c_score[rank];
                if (rank == 0) best = sc;
                if (!c_eos[rank]) {
                    n_score[k] = sc; n_tok[k] = tok; n_idx[k] = row;
                    ++k;
                    continue;
                }
                if (rank >= nb) continue;
                // _BeamHyps.add(ids[row], sc, g)
                const double score = (double)sc / a.len_pow[g];
                if (!(count < nb || score > worst)) continue;
                int slot;
                if (count < nb) {
                    slot = count;
                    hs[count] = score; hl[count] = L; hslot[count] = slot;
                    ++count;
                    worst = worst < score ? worst : score;          // min(score, worst)
                } else {
                    // the list with the new entry appended has nb + 1 entries (the new one at index nb): delete the lowest (score, index),
                    // `worst` becomes the second lowest score
                    int d = nb;
                    double ds = score;
                    for (int i = 0; i < nb; ++i)
                        if (hs[i] < ds || (hs[i] == ds && i < d)) { ds = hs[i]; d = i; }
                    int d2 = -1;
                    double ds2 = 0.0;
                    for (int i = 0; i <= nb; ++i) {
                        if (i == d) continue;
                        const double si = i < nb ? hs[i] : score;
                        if (d2 < 0 || si < ds2) { ds2 = si; d2 = i; }
                    }
                    worst = ds2;
                    if (d == nb) continue;                          // the new entry itself was the lowest: nothing is stored
                    slot = hslot[d];
                    for (int i = d; i + 1 < nb; ++i) { hs[i] = hs[i + 1]; hl[i] = hl[i + 1]; hslot[i] = hslot[i + 1]; }
                    hs[nb - 1] = score; hl[nb - 1] = L; hslot[nb - 1] = slot;
                }
                task_row[tasks] = row; task_slot[tasks] = slot;
                ++tasks;
            }
            a.hyp_count[b] = count;
            a.hyp_worst[b] = worst;
            // _BeamHyps.is_done(best, cur_len, prompt_len, max_length)
            bool fin = false;
            if (count >= nb) {
                if (a.early == 1) fin = true;
                else if (a.early == 2 && a.lp_positive) fin = worst >= (double)best / a.len_pow[a.max_len - a.L0];
                else fin = worst >= (double)best / a.len_pow[g];
            }
            if (fin) {
                a.done[b] = 1;
                if (atomicAdd(&a.all_done[1], 1) + 1 == a.B) a.all_done[0] = 1;
            }
        }
        n_task = tasks;
    }
    __syncthreads();

    // new hypotheses: ids[row, :L] into their slots; a slot written twice in one step keeps the later entry
    const int tasks = n_task;
    for (int t = 0; t < tasks; ++t) {
        bool later = false;
        for (int u = t + 1; u < tasks; ++u) later = later || task_slot[u] == task_slot[t];
        if (later) continue;
        const int64_t* src = a.ids + (int64_t)task_row[t] * a.i_rs;
        int64_t* dst = a.hyp_tokens + ((int64_t)b * nb + task_slot[t]) * a.max_len;
        for (int i = tid; i < L; i += NT) dst[i] = src[i];
    }
    // the next ids, the new beam scores and the reorder index
    for (int k = 0; k < nb; ++k) {
        const int64_t* src = a.ids + (int64_t)n_idx[k] * a.i_rs;
        int64_t* dst = a.ids_next + ((int64_t)b * nb + k) * a.n_rs;
        for (int i = tid; i < L; i += NT) dst[i] = src[i];
        if (tid == 0) {
            dst[L] = n_tok[k];
            a.beam_scores[b * nb + k] = n_score[k];
            a.beam_idx[b * nb + k] = n_idx[k];
        }
    }
}

int64_t chunks_of(int64_t V) { return (V + CHUNK - 1) / CHUNK; }

}  // namespace

extern "C" {

int64_t otter_beam_step_workspace_bytes(int64_t B, int64_t nb, int64_t V, int64_t n_cand) {
    if (B < 1 || nb < 1 || V < 1 || n_cand < 1 || n_cand > MAX_CAND || B > INT32_MAX || nb > MAX_CAND || V > INT32_MAX) return -1;
    return B * nb * chunks_of(V) * n_cand * 8;
}

int otter_beam_step(const float* logp, int64_t logp_stride, float* beam_scores, const int64_t* ids, int64_t ids_stride, int64_t* ids_next,
                    int64_t ids_next_stride, int64_t* beam_idx, const int32_t* eos, int64_t n_eos, int64_t pad_token_id, int64_t B, int64_t nb,
                    int64_t V, int64_t n_cand, int64_t L, int64_t L0, int64_t max_len, int early_stopping, int length_penalty_positive,
                    const double* len_pow, int32_t* done, double* hyp_score, int64_t* hyp_tokens, int32_t* hyp_len, int32_t* hyp_slot,
                    int32_t* hyp_count, double* hyp_worst, int32_t* all_done, void* workspace, int64_t workspace_bytes, void* stream) {
    OTTER_REQUIRE(logp && beam_scores && ids && ids_next && beam_idx, "beam_step: null pointer (logp / beam_scores / ids / ids_next / beam_idx)");
    OTTER_REQUIRE(len_pow && done && hyp_score && hyp_tokens && hyp_len && hyp_slot && hyp_count && hyp_worst && all_done,
                  "beam_step: null pointer (len_pow / done / hyp_score / hyp_tokens / hyp_len / hyp_slot / hyp_count / hyp_worst / all_done)");
    OTTER_REQUIRE(n_eos >= 0 && n_eos <= INT32_MAX, "beam_step: list length out of range (n_eos=%ld)", (long)n_eos);
    OTTER_REQUIRE(eos || n_eos == 0, "beam_step: null pointer for a non-empty list (eos)");
    OTTER_REQUIRE(workspace, "beam_step: null pointer (workspace)");
    OTTER_REQUIRE(((uintptr_t)logp & 3) == 0 && ((uintptr_t)beam_scores & 3) == 0 && ((uintptr_t)eos & 3) == 0 &&
                      (((uintptr_t)done | (uintptr_t)hyp_len | (uintptr_t)hyp_slot | (uintptr_t)hyp_count | (uintptr_t)all_done) & 3) == 0 &&
                      (((uintptr_t)ids | (uintptr_t)ids_next | (uintptr_t)beam_idx | (uintptr_t)len_pow | (uintptr_t)hyp_score |
                        (uintptr_t)hyp_tokens | (uintptr_t)hyp_worst | (uintptr_t)workspace) & 7) == 0,
                  "beam_step: alignment (fp32 and int32 buffers 4 bytes; int64 and fp64 buffers and the workspace 8 bytes)");
    OTTER_REQUIRE(B >= 1 && B <= INT32_MAX, "beam_step: B=%ld outside 1..2^31-1", (long)B);
    OTTER_REQUIRE(V >= 1 && V <= INT32_MAX, "beam_step: V=%ld outside 1..2^31-1", (long)V);
    OTTER_REQUIRE(nb >= 1 && n_cand >= nb && n_cand <= nb * V, "beam_step: nb=%ld must be >= 1 and n_cand=%ld within nb..nb * V=%ld", (long)nb,
                  (long)n_cand, (long)(nb * V));
    OTTER_REQUIRE(n_cand <= MAX_CAND, "beam_step: n_cand=%ld above the cap of %d candidates", (long)n_cand, MAX_CAND);
    OTTER_REQUIRE(nb * V <= INT32_MAX && B * nb <= 65535, "beam_step: nb * V=%ld above 2^31-1 (the flat index) or B * nb=%ld above 65535 (the grid)",
                  (long)(nb * V), (long)(B * nb));
    OTTER_REQUIRE(max_len <= INT32_MAX && L >= 1 && L < max_len, "beam_step: L=%ld outside 1..max_len-1 (max_len=%ld)", (long)L, (long)max_len);
    OTTER_REQUIRE(L0 >= 1 && L0 <= L, "beam_step: L0=%ld outside 1..L=%ld", (long)L0, (long)L);
    OTTER_REQUIRE(logp_stride >= V && ids_stride >= L && ids_next_stride >= L + 1,
                  "beam_step: a row stride below the row length (logp %ld < V=%ld, ids %ld < L=%ld or ids_next %ld < L+1)", (long)logp_stride, (long)V,
                  (long)ids_stride, (long)L, (long)ids_next_stride);
    {
        const int64_t n_in = (B * nb - 1) * ids_stride + L, n_out = (B * nb - 1) * ids_next_stride + L + 1;
        OTTER_REQUIRE(ids_next + n_out <= ids || ids + n_in <= ids_next, "beam_step: ids and ids_next overlap (the step reads one and writes the other)");
    }
    OTTER_REQUIRE(early_stopping >= 0 && early_stopping <= 2, "beam_step: early_stopping=%d must be 0 (False), 1 (True) or 2 (\"never\")", early_stopping);
    const int64_t need = otter_beam_step_workspace_bytes(B, nb, V, n_cand);
    OTTER_REQUIRE(need > 0 && workspace_bytes >= need, "beam_step: workspace of %ld bytes, %ld needed", (long)workspace_bytes, (long)need);

    BeamArgs a;
    a.logp = logp; a.lp_rs = logp_stride;
    a.beam_scores = beam_scores;
    a.ids = ids; a.i_rs = ids_stride;
    a.ids_next = ids_next; a.n_rs = ids_next_stride;
    a.beam_idx = beam_idx;
    a.eos = eos; a.n_eos = (int)n_eos;
    a.pad = pad_token_id;
    a.B = (int)B; a.nb = (int)nb; a.V = (int)V; a.n_cand = (int)n_cand; a.L = (int)L; a.L0 = (int)L0; a.max_len = (int)max_len;
    a.early = early_stopping; a.lp_positive = length_penalty_positive != 0;
    a.chunks = (int)chunks_of(V);
    a.len_pow = len_pow;
    a.done = done;
    a.hyp_score = hyp_score; a.hyp_tokens = hyp_tokens; a.hyp_len = hyp_len; a.hyp_slot = hyp_slot; a.hyp_count = hyp_count; a.hyp_worst = hyp_worst;
    a.all_done = all_done;
    a.ws = (unsigned long long*)workspace;
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)a.chunks, (unsigned)(B * nb)), dim3(NT), 0, (hipStream_t)stream, a);
    OTTER_CHECK_LAUNCH("beam_step (select)");
    hipLaunchKernelGGL(beam_score_kernel, dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream, a);
    OTTER_CHECK_LAUNCH("beam_step (score)");
    return OTTER_OK;
}

}  // extern "C"
