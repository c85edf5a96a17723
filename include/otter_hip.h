/*
 * otter_hip.h -- C ABI of libotter_hip.so: the MI355X (gfx950) kernels of the Otter vision->language fusion hot path.
 *
 * The reference (Luodian/Otter) is 100% Python and has NO FFI / operator registry for this path:
 * every entry point below replaces a run of ATen calls inside one of the reference's nn.Module.forward bodies
 * (and their autograd backward).  The file:line each one replaces is given per function, relative to
 * /root/reference/src/otter_ai/models/.  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C: device pointers + sizes; no torch / hip types in the signatures (streams travel as void*).
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates persistent memory;
 *     scratch is passed in (`*_workspace_bytes` tells how much).
 *   - asynchronous on the given stream (hipStream_t cast to void*; NULL = default stream); thread-safe for
 *     distinct streams; no host synchronisation inside.
 *   - return 0 on success, a negative otter_status on failure (never throws); otter_last_error() gives a
 *     thread-local message.
 *   - matrices are row-major; `ld*` / `*_stride` are ROW strides in ELEMENTS.
 *   - dtypes: OTTER_F32 / OTTER_BF16 (bf16 = upper 16 bits of an IEEE float, round-to-nearest-even on store).
 *     All reductions / accumulations are fp32 whatever the storage type.
 */
#ifndef OTTER_HIP_H
#define OTTER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTTER_ABI_VERSION 3   /* bump on ANY change of an exported signature or struct layout (otter_amd/_capi.py reads this line) */

typedef enum { OTTER_F32 = 0, OTTER_BF16 = 1 } otter_dtype;

typedef enum {
    OTTER_OK = 0,
    OTTER_ERR_ARG = -1,      /* bad shape / dtype / null pointer */
    OTTER_ERR_UNSUPPORTED = -2,
    OTTER_ERR_LAUNCH = -3,   /* hipGetLastError() after the launch */
    OTTER_ERR_WORKSPACE = -4
} otter_status;

int otter_abi_version(void);
const char* otter_last_error(void);
/* number of CUs etc. are not needed by callers; this just proves the library sees a gfx950 device. */
int otter_device_check(void);

/* ---------------------------------------------------------------------------------------------------------
 * LayerNorm / RMSNorm.  Replaces nn.LayerNorm at otter/modeling_otter.py:136-137,144,211,253,365 (perceiver +
 * gated cross-attention), LPLayerNorm at mpt/norm.py:16-45 (beta == NULL: MPT-7B has no_bias) and LlamaRMSNorm at
 * /root/reference/xformers_model/llama.py:95-112.
 *
 * Row map: output row of input row r is  (r / grp_rows) * grp_stride + row_off + (r % grp_rows)  when
 * grp_rows > 0, else r.  It lets the perceiver write norm_media(x) and norm_latents(latents) straight into
 * the [x ; latents] buffer that `to_kv` consumes (modeling_otter.py:166) without a torch.cat copy.
 * y2 (optional, may be NULL) receives the same rows again, un-mapped (dense [rows, D]).
 * ------------------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t grp_rows;   /* 0 = identity map */
    int64_t grp_stride; /* rows */
    int64_t row_off;    /* rows */
} otter_rowmap;

int otter_layernorm_fwd(const void* x, int x_dtype, const void* gamma, const void* beta, int w_dtype, void* y,
                        int y_dtype, otter_rowmap y_map, void* y2, float* mean, float* rstd, int64_t rows, int64_t D,
                        float eps, void* stream);

/* Fused residual add + LayerNorm: xsum = x + delta (stored with x's dtype), y = LN(xsum).  Replaces the
 * `x = x + resid_attn_dropout(b); m = norm_2(x)` pair of MPTBlock.forward (mpt/blocks.py:83-84): one pass over the
 * residual stream instead of two.  Backward = otter_layernorm_bwd with dres = d(xsum). */
int otter_add_layernorm_fwd(const void* x, int x_dtype, const void* delta, int delta_dtype, void* xsum, const void* gamma,
                            const void* beta, int w_dtype, void* y, int y_dtype, float* mean, float* rstd, int64_t rows,
                            int64_t D, float eps, void* stream);

/* dx = LN'(dy) (+ dres if given, same dtype as dx).  dy is read through dy_map (same convention as the forward's
 * y_map).  dx_bf16 (optional) receives a bf16 copy of dx in the same pass (the gradient of the bf16 branch output that was
 * added to the fp32 residual stream).  dgamma/dbeta (fp32, [D]) are OVERWRITTEN (or accumulated when accumulate != 0).
 * ws: see otter_layernorm_bwd_workspace_bytes.  gamma may be NULL (treated as ones); dbeta may be NULL. */
int64_t otter_layernorm_bwd_workspace_bytes(int64_t rows, int64_t D);
int otter_layernorm_bwd(const void* dy, int dy_dtype, otter_rowmap dy_map, const void* x, int x_dtype,
                        const void* gamma, int w_dtype, const float* mean, const float* rstd, const void* dres,
                        void* dx, int dx_dtype, void* dx_bf16, float* dgamma, float* dbeta, int accumulate, void* ws,
                        int64_t rows, int64_t D, void* stream);

/* out[c] (+)= sum_r src[map(r)][c]  (fp32 [D]).  Gradient of a broadcast embedding row: frame_embs /
 * media_time_embs (modeling_otter.py:224-229).  ws: otter_layernorm_bwd_workspace_bytes(rows, D). */
int otter_colsum(const void* src, int src_dtype, otter_rowmap src_map, float* out, int accumulate, void* ws, int64_t rows,
                 int64_t D, void* stream);

/* y = w * cast_to_xdtype(x * rsqrt(mean(x^2) + eps))   (HF LlamaRMSNorm rounding order) */
int otter_rmsnorm_fwd(const void* x, int x_dtype, const void* w, int w_dtype, void* y, float* rstd, int64_t rows,
                      int64_t D, float eps, void* stream);
int otter_rmsnorm_bwd(const void* dy, const void* x, int x_dtype, const void* w, int w_dtype, const float* rstd,
                      void* dx, float* dw, int accumulate, void* ws, int64_t rows, int64_t D, void* stream);

/* LLaMA host (config C4) forms of the two above.  otter_add_rmsnorm_fwd: optional fused residual add (xsum = x + delta, both
 * NULL for a plain norm) and an output dtype of its own (y = bf16 of the fp32 result: what autocast feeds the next Linear,
 * rounded once).  Replaces `hidden = residual + hidden; hidden = post_attention_layernorm(hidden)` of the decoder layer
 * (/root/reference/xformers_model/llama.py:311-318) in one pass over the residual stream.  otter_rmsnorm_bwd_ex: dy in its
 * own dtype, optional dres added to dx, optional bf16 copy of dx, dw optional (NULL for the frozen decoder). */
int otter_add_rmsnorm_fwd(const void* x, int x_dtype, const void* delta, int delta_dtype, void* xsum, const void* w, int w_dtype,
                          void* y, int y_dtype, float* rstd, int64_t rows, int64_t D, float eps, void* stream);
int otter_rmsnorm_bwd_ex(const void* dy, int dy_dtype, const void* x, int x_dtype, const void* w, int w_dtype, const float* rstd,
                         const void* dres, void* dx, int dx_dtype, void* dx_bf16, float* dw, int accumulate, void* ws, int64_t rows,
                         int64_t D, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * GEMM  C[M,N] = epilogue( A[M,K] . B[N,K]^T )  -- both operands K-contiguous ("NT": exactly nn.Linear).
 * Replaces every bias-free nn.Linear on the path (modeling_otter.py:139-141,145,147,255-257,366,368) with the
 * element-wise tail that follows it fused into the epilogue:
 *   OTTER_EPI_STORE     C = s * acc                      (s = tanh(*gate) if gate else 1; accumulate: C += ...)
 *                       with an fp32 C and partial != NULL also partial[block] = sum over the tile of C^2 (the values as stored): the
 *                       clip_grad_norm_ reduction of a weight gradient (pipeline/train/instruction_following.py:246-247) taken in the
 *                       producing launch instead of by a second sweep over the tensor; summed by otter_clip_coef like any other partial.
 *   OTTER_EPI_GELU      C = gelu_erf(acc); C2 = acc       (Linear -> nn.GELU, :366-367 / :145-146; C2 optional)
 *                       with aux_is_gelu_input == 3 (round 6c): C2 = gelu_erf'(acc) -- the DERIVATIVE is stashed for a backward that needs
 *                       nothing else of the pre-activation (a frozen MLP: mpt/blocks.py:9-20), see OTTER_EPI_GATE_BWD
 *   OTTER_EPI_SCALE_RES C = acc * s + R                  (x = attn(...) * attn_gate.tanh() + x, :380-393;
 *                                                          gate == NULL gives the perceiver's plain residual :180,184)
 *   OTTER_EPI_GATE_BWD  C = s * acc * f'(aux);  partial[block] = sum(acc * f(aux))
 *                       f = identity (aux_is_gelu_input == 0), gelu_erf (1) or the squared ReLU relu(a)^2 of the Persimmon MLP
 *                       (2; /root/reference/src/otter_ai/models/fuyu/modeling_persimmon.py:180-194); 3: aux already holds f'(a)
 *                       (stashed by the forward launch): C = s * acc * aux, partial must be NULL.
 *                       This is the dgrad GEMM of a gated branch: it yields d(branch input) and, through the
 *                       deterministic two-stage reduction otter_reduce_partials, the gradient of the scalar gate.
 * A/B are both ab_dtype.  bf16 operands run on MFMA (v_mfma_f32_32x32x16_bf16, fp32 accumulate); f32 operands
 * run on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32) -- the parity mode.
 * ------------------------------------------------------------------------------------------------------- */
typedef enum { OTTER_EPI_STORE = 0, OTTER_EPI_GELU = 1, OTTER_EPI_SCALE_RES = 2, OTTER_EPI_GATE_BWD = 3 } otter_epilogue;

typedef struct {
    int kind;            /* otter_epilogue */
    int accumulate;      /* STORE only, C must be f32 */
    const float* gate;   /* device scalar (pre-tanh) or NULL */
    const void* R;       /* SCALE_RES residual [M,N] */
    int64_t ldr;
    int r_dtype;
    void* C2;            /* GELU: pre-activation copy (same dtype as C) or NULL */
    int64_t ldc2;
    const void* aux;     /* GATE_BWD */
    int64_t ldaux;
    int aux_dtype;
    int aux_is_gelu_input; /* 0 identity, 1 erf GELU, 2 squared ReLU, 3 stashed derivative (GELU launch: C2 = GELU'; GATE_BWD launch: aux = f') */
    float* partial;      /* GATE_BWD, STORE with an f32 C: [otter_gemm_num_partials(M,N)] floats, or NULL */
    int grid_mode;       /* otter_grid_mode of THIS launch (ABI 2): how the large-grid kernel maps tiles to workgroups */
} otter_epilogue_args;

/* Per-call grid shape of the large-grid GEMM.  A persistent grid (one workgroup per CU walking its tile list) assumes the launch owns
 * the chip; while a collective's kernels hold CUs (a DP reducer is live) one workgroup per tile degrades in proportion to the CUs
 * taken instead of doubling the launch.  The caller that knows -- otter_amd.train.TrainStep -- says so per
 * launch; OTTER_GRID_DEFAULT defers to the process-wide otter_gemm_set_persistent switch (tools / A-B runs only). */
typedef enum { OTTER_GRID_DEFAULT = 0, OTTER_GRID_PERSISTENT = 1, OTTER_GRID_PER_TILE = 2 } otter_grid_mode;

int64_t otter_gemm_num_partials(int64_t M, int64_t N, int ab_dtype);
int otter_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N,
                  int64_t K, int ab_dtype, int c_dtype, const otter_epilogue_args* epi, void* stream);
/* C[M,N] = epilogue(op(A) . op(B)^T) with K-MAJOR operands (round 3): with a_kmajor != 0, A is handed over as [K rows][M columns]
 * row-major (row stride lda), i.e. the reduction index is the ROW index; likewise B as [K][N] with b_kmajor.  These are the
 * layouts the backward products of an nn.Linear have their operands in -- dW[out,in] = dy^T x (both K-major: K = token rows;
 * autograd's `grad_output.t().mm(input)`, the backward of every nn.Linear at otter/modeling_otter.py:140-147,254-256,366-368) and
 * dx = dy W with W as stored [out,in] (B K-major) -- so no operand is transposed in HBM first.  Same epilogues, dtypes and stream
 * semantics as otter_gemm_nt (which is this call with both flags 0).  Only shapes for which otter_gemm_kmajor_supported returns 1
 * are accepted (bf16, K % 128 == 0 -- any K >= 128 when BOTH operands are K-major --, >= 192 output tiles of 256 x 256, M / N / leading
 * dimensions multiples of 8, operands < 4 GB);
 * the host transposes (otter_transpose) and calls otter_gemm_nt otherwise. */
int otter_gemm(const void* A, int64_t lda, int a_kmajor, const void* B, int64_t ldb, int b_kmajor, void* C, int64_t ldc, int64_t M,
               int64_t N, int64_t K, int ab_dtype, int c_dtype, const otter_epilogue_args* epi, void* stream);
int otter_gemm_kmajor_supported(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int a_kmajor, int b_kmajor, int ab_dtype);
/* Threading: every compute entry point of this header is asynchronous on the stream it is given and may be called concurrently from
 * different host threads on DISTINCT streams (autograd's backward thread and the training thread do).  The otter_*_set_* switches below
 * (variant, debug, CU budget, grid shape) and the otter_prof_* hooks are process-wide settings for tools, benchmarks and the training
 * step's set-up phase: change them from one thread, between steps, never while another thread is launching.  The one-time
 * hipFuncSetAttribute calls behind the first launch of each kernel are idempotent (a benign race). */
/* selects the bf16 kernel schedule: 0 = auto, 1 = 128x128 register-staged, 2 = 256x256 register-staged,
 * 3 = 256x256 direct-to-LDS (global_load_lds).  Process-wide; for A/B measurements. */
int otter_gemm_set_variant(int variant);
/* 1 if `variant` is compiled into this library: 0-3, 13, 25, 26, 30 (the kernels pick_cfg can choose).  The numbers of the earlier
 * kernel generations (4-12, 14-23, 27-29) are retired: otter_gemm_set_variant refuses them with OTTER_ERR_UNSUPPORTED
 * (DESIGN_HISTORY.md names the last commit that holds their source). */
int otter_gemm_variant_available(int variant);
/* Caps the persistent GEMM grids at `cus` workgroups (0 = every CU of the device, the default; values below 8 are raised to 8).
 * Returns the grid size now in effect.  Used by the data-parallel step: with `cus` a little below the device's CU count, RCCL's
 * all-reduce kernels get CUs of their own and run concurrently with the backward GEMMs (nothing to match in the reference:
 * torch DDP relies on the GPU scheduler).  Process-wide, like the other otter_gemm_set_* switches: set it from the thread that
 * launches the GEMMs, between steps. */
int otter_gemm_set_cu_budget(int cus);
/* on = 0: the large-grid kernel (variant 26) is launched with ONE workgroup per output tile instead of one persistent workgroup per CU.
 * A persistent grid assumes it owns every CU: when a concurrent kernel (RCCL's all-reduce in the data-parallel step) holds a few CUs, the
 * workgroups that could not start run their whole tile list AFTER the others finish and the launch takes twice as long; with one
 * workgroup per tile the loss is proportional to the CUs taken (measured).  Costs ~8 us of fixed time per launch
 * when nothing else runs.  Default 1.  Process-wide, set between steps. */
int otter_gemm_set_persistent(int on);
/* Diagnostics and A/B switches of the GEMM kernels, one word.  Never set by the product path.
 *   bits 0-1  roofline ablations (results are WRONG): bit0 = no global loads inside the K loop, bit1 = no MFMAs
 *   bit 4     timing ablation (results are WRONG: C is not written): every tile takes the masked (edge-tile) tail, which then skips its
 *             global loads and stores;  bit 6: tile-phase timeline stamps (otter_gemm_read_timeline);  bit 8: 4-wide fused tail
 *   bits 9-13 tile order of the large-grid kernel (super-tile shape, walk direction; bit 13 = one workgroup per tile)
 *   bits 14-15 (round 6) cross-tile ring of the large-grid kernel: 0 = default (on), 1 = off, 2 = on
 *   bits 16-22 + bit 23 (round 6): with bit 23 set, bits 16-22 replace the K-tile order of a tile (default 3 = rotated by the tile's N panel;
 *             0 = plain: the order the bit-for-bit comparisons against other kernels use) */
int otter_gemm_set_debug(int flags);

/* out[0] (op) = scale(gate) * sum(partial[0..n))   with scale = (1 - tanh(*gate)^2) when gate != NULL.
 * accumulate != 0 adds into out[0].  Deterministic (single block, fixed order). */
int otter_reduce_partials(const float* partial, int64_t n, const float* gate, float* out, int accumulate, void* stream);

/* dst[c][r] = src[r][c]  (+ optional same-layout cast copy dst_same[r][c]).  Used for the weight shadows
 * (fp32 master -> bf16 W and bf16 W^T) and for the activation transposes the wgrad GEMMs need. */
int otter_transpose(const void* src, int64_t ld_src, int src_dtype, void* dst_t, int64_t ld_dst_t, void* dst_same,
                    int64_t ld_dst_same, int dst_dtype, int64_t rows, int64_t cols, void* stream);
int otter_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * text_time: cumulative count of <image> tokens per text position, plus the attend_previous=False rewrite.
 * Replaces modeling_otter.py:298-311.  media_locations: uint8/bool [B,T]; text_time: int32 [B,T].
 * ------------------------------------------------------------------------------------------------------- */
int otter_text_time(const uint8_t* media_locations, int32_t* text_time, int64_t B, int64_t T, int attend_previous,
                    void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Attention core (head_dim = 64 only -- the reference hard-codes dim_head=64 for both users):
 *   perceiver latent cross-attention  modeling_otter.py:168-179   (mask_mode NONE, Tq = 64 latents, M = n1+64)
 *   masked cross-attention            modeling_otter.py:290-333   (mask_mode EQ / GE with text_time)
 * q [B,Tq,H*64] (row stride q_stride), k/v [B,M,H*64] (row stride kv_stride; k and v usually point into one
 * to_kv output buffer), o like q.  sim = scale * q.k ; masked entries := -FLT_MAX ; softmax ; rows with
 * text_time == 0 are zeroed when mask_mode == EQ (only_attend_immediate_media) ; rows whose every key is masked
 * come out uniform (1/M) exactly as the reference's masked_fill(-finfo.max) + amax does.
 * media index of key j is j / n_per_media.  lse [B,H,Tq] fp32 is saved for the backward.
 * ------------------------------------------------------------------------------------------------------- */
typedef enum { OTTER_MASK_NONE = 0, OTTER_MASK_EQ = 1, OTTER_MASK_GE = 2 } otter_mask_mode;

int otter_attn_fwd(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride, void* o,
                   int64_t o_stride, float* lse, const int32_t* text_time, int64_t B, int64_t H, int64_t Tq, int64_t M,
                   int64_t n_per_media, int mask_mode, float scale, int dtype, void* stream);

/* tuning / A-B hook: 0 = MFMA kernels for bf16 inputs (attn_mfma.hip), 1 = fp32 VALU kernels for every dtype */
int otter_attn_set_variant(int variant);

int64_t otter_attn_bwd_workspace_bytes(int64_t B, int64_t H, int64_t Tq, int64_t M);
/* dq like q; dk/dv like k/v (stride dkv_stride).  ws from otter_attn_bwd_workspace_bytes. */
int otter_attn_bwd(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride, const void* o,
                   const void* d_o, int64_t o_stride, const float* lse, const int32_t* text_time, void* dq,
                   int64_t dq_stride, void* dk, void* dv, int64_t dkv_stride, void* ws, int64_t B, int64_t H,
                   int64_t Tq, int64_t M, int64_t n_per_media, int mask_mode, float scale, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Flash attention of the frozen decoder host, head_dim 128 -- and, round 3, head_dim 64 (Persimmon / Fuyu-8B,
 * /root/reference/src/otter_ai/models/fuyu/modeling_persimmon.py:310 flash_attn_func(causal=True)) --, bf16, MFMA:
 *   scaled_multihead_dot_product_attention   /root/reference/src/otter_ai/models/mpt/attention.py:22-84
 *   ALiBi bias (key-position form)           .../mpt/attention.py:447-464      bias[h,j] = slope[h] * (j - (Sk-1))
 *   key-padding mask                         .../mpt/modeling_mpt.py:135-144
 *   causal mask                              .../mpt/attention.py:64-72        key j visible to query i iff j <= i + Sk - Sq
 * out = softmax(scale * q k^T + bias + masks) v without materialising the scores; the bias is evaluated in fp32 in
 * the kernel.  q/k/v/o (and the gradients) are [B, S, H, 128] views given by element strides, so the three slices
 * of a fused Wqkv output and of its gradient buffer are addressed in place (no chunk/cat copies).
 * lse [B,H,Sq] fp32 (natural log) is written by the forward and read by the backward; delta is backward workspace of
 * 2*B*H*Sq floats (row dot products, then a log2-domain copy of lse).  A query row with no visible key yields o = 0, lse = -inf and zero gradients (exactly: tests/test_gpu_flash_exact.py); the
 * reference's masked_fill(finfo.min) would yield the uniform average there.  Such rows exist for left-padded prompts (the padded
 * positions themselves) and for Sq > Sk under the causal mask (rows i < Sq - Sk); nobody consumes them.  Inference passes over
 * left-padded prompts take this kernel (mpt.py, llama.py, fuyu.py); only a left-padded batch that needs gradients goes to the
 * host's SDPA path.  Sq != Sk is supported by every kernel, forward and backward.
 * head_dim 64: one workgroup takes two adjacent heads (H must be even); the second head of a pair lies head_stride elements after
 * the first inside the same token row (64 <= head_stride <= seq_stride - 64), so compact [B,S,H,64] tensors and the v slots of
 * Persimmon's per-head interleaved [B,S,H,3,64] projection buffer (head_stride 192) are both read / written in place.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct otter_flash_view {
    int64_t batch_stride, seq_stride, head_stride; /* in elements; multiples of 8 */
} otter_flash_view;

typedef struct otter_flash_desc {
    const void* q; const void* k; const void* v; otter_flash_view qv, kv, vv;
    void* o; otter_flash_view ov;
    float* lse;
    const float* alibi_slopes;   /* [H] fp32 or NULL */
    const uint8_t* key_valid;    /* [B, Sk] (0 = padded key) or NULL */
    int B, H, Sq, Sk, head_dim, causal;
    float scale;
    /* backward only */
    const void* dout; otter_flash_view dov;
    float* delta;
    void* dq; void* dk; void* dv; otter_flash_view dqv, dkv, dvv;
} otter_flash_desc;

int otter_flash_attn_fwd(const otter_flash_desc* d, void* stream);
/* the same forward with O UNROUNDED: o32 fp32 [B, Sq, H, 128] contiguous, 16-byte aligned, takes what d->o would take before its rounding to
 * bf16; d->o is not written (it must still be a valid aligned pointer: o32 itself will do) and lse is written as always.  head_dim 128 on
 * the default LDS-DMA forward only (flash variant not 1 or 6).  The probabilities enter the second product as a bf16 hi + lo pair (two MFMAs per
 * V fragment), so o32 is within a few 1e-6 of fp64 where the bf16-probability forward is within a few 1e-3: a consumer that goes on computing
 * with O -- otter_branch_attn_merge -- then rounds once, at its own output, and has the error of a one-kernel attention */
int otter_flash_attn_fwd_f32(const otter_flash_desc* d, float* o32, void* stream);
/* tuning / A-B hook: 0 = default (LDS-DMA tiles, longest-first block order under the causal mask, delta inside the dQ kernel, one persistent
 * dK/dV workgroup per (batch, head) when those fill the chip evenly), 1 = register-staged tiles (v1), 2 = LDS-DMA tiles on the plain 3-D grid,
 * 3 / 5 = 2 / 0 with dK+dV at two workgroups per CU, 4 = 0 with the separate delta launch, 6 = 0 with forward version 3 (16 queries per
 * wave), 7 = 0 with one dK/dV workgroup per key block, 8 = 0 with the persistent dK/dV form on every launch that can take it
 * (head_dim 64: 1 is refused, 3 / 5 = 2 / 0) */
int otter_flash_set_variant(int variant);
int otter_flash_attn_bwd(const otter_flash_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * RoPE, half-split (non-interleaved) layout, optional partial rotary.  Replaces
 * /root/reference/xformers_model/llama.py:158-166 (config C4) and flash_attn apply_rotary_emb at
 * fuyu/modeling_persimmon.py:303-304 (config C5).  x [B,S,H,d]; cos/sin fp32 [S, rot_dim]; in place allowed.
 * inverse != 0 applies the transpose rotation (= the backward).
 * ------------------------------------------------------------------------------------------------------- */
int otter_rope(const void* x, void* y, const float* cos_t, const float* sin_t, int64_t B, int64_t S, int64_t H,
               int64_t d, int64_t rot_dim, int inverse, int dtype, void* stream);

/* Same rotation, bf16, full rotary, 16-byte vectors, on STRIDED tokens: `tokens` = B*S tokens whose H rotated heads are
 * contiguous (head stride d) and which are x_token_stride / y_token_stride elements apart -- q and k inside the fused
 * [B,S,3,H,d] projection buffer are H' = 2H heads with token stride 3*H*d.  In place allowed (y == x, equal strides). */
int otter_rope_strided(const void* x, void* y, const float* cos_t, const float* sin_t, int64_t tokens, int64_t S, int64_t H,
                       int64_t d, int inverse, int64_t x_token_stride, int64_t y_token_stride, void* stream);

/* quick-GELU of the frozen CLIP tower's MLP (/root/reference/xformers_model/clip.py:84-95: x * sigmoid(1.702 x)); bf16 or
 * f32, n elements (multiple of 8), in place allowed. */
int otter_quick_gelu(const void* x, void* y, int64_t n, int dtype, void* stream);

/* Exact-erf GELU of the frozen MPT decoder's MLP (/root/reference/src/otter_ai/models/mpt/blocks.py:37-49: act = nn.GELU(approximate=
 * 'none')) and its backward dx = dy * (Phi(x) + x phi(x)); bf16 or f32, n elements (multiple of 8), y == x / dx == dy allowed. */
int otter_gelu_fwd(const void* x, void* y, int64_t n, int dtype, void* stream);
int otter_gelu_bwd(const void* x, const void* dy, void* dx, int64_t n, int dtype, void* stream);

/* SwiGLU of the LLaMA MLP (/root/reference/xformers_model/llama.py:216-223: down(act(gate(x)) * up(x)), act = SiLU) on the
 * [rows, 2*I] bf16 output of the concatenated gate|up projection: h[rows, I] = silu(g) * u;  backward writes
 * dgate_up[rows, 2*I] = (dh * u * silu'(g) | dh * silu(g)). */
int otter_swiglu_fwd(const void* gate_up, void* h, int64_t rows, int64_t I, void* stream);
int otter_swiglu_bwd(const void* gate_up, const void* dh, void* dgate_up, int64_t rows, int64_t I, void* stream);

/* x[i] += y[i] for a broadcast row block:  x [groups, rows, D] += emb [rows_e .. broadcast]; used for
 * frame_embs (modeling_otter.py:224-226).  x viewed as [outer, F, inner, D]; emb [F, D] fp32 master. */
int otter_add_frame_embs(void* x, int x_dtype, const float* emb, int64_t outer, int64_t F, int64_t inner, int64_t D,
                         void* stream);

/* dst[r] += src[map(r)] for r in [0, rows): the perceiver backward sums the two gradient paths of
 * norm_latents(latents) -- through to_q and through the latent rows of the [x ; latents] to_kv input
 * (modeling_otter.py:165-167) -- without materialising a gathered copy. */
int otter_add_rows(void* dst, const void* src, otter_rowmap src_map, int64_t rows, int64_t D, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Single-query attention over a KV cache: the cached decode step of generate() (/root/reference/src/otter_ai/models/otter/
 * modeling_otter.py:999-1042 -> mpt/attention.py:22-84 with past_key_value + ALiBi :447-464; LLaMA llama.py:169-213).
 * q, o [B, H, 128] (bf16); K and V are addressed by explicit batch / head / key / dim strides (elements), so the reference's
 * MPT cache layout k [B,H,d,S], v [B,H,S,d] and the [B,H,S,d] layout of the LLaMA host are both read in place.
 * alibi_slopes [H] fp32 or NULL (bias slope * (j - (Sk-1))); key_valid [B, Sk] (0 = padded key) or NULL.  Sk <= 16384.
 * ------------------------------------------------------------------------------------------------------- */
int otter_decode_attn(const void* q, int64_t q_batch_stride, int64_t q_head_stride, const void* k, int64_t k_batch_stride,
                      int64_t k_head_stride, int64_t k_key_stride, int64_t k_dim_stride, const void* v, int64_t v_batch_stride,
                      int64_t v_head_stride, int64_t v_key_stride, int64_t v_dim_stride, void* o, int64_t o_batch_stride,
                      int64_t o_head_stride, const float* alibi_slopes, const uint8_t* key_valid, int64_t B, int64_t H, int64_t Sk,
                      int64_t head_dim, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_persimmon_decode_attn -- one cached decode step of the OtterHD / Fuyu-8B (Persimmon) attention
 * (fuyu/modeling_persimmon.py:262-312 with a past_key_value and one new token): q / k LayerNorm over the 64-wide head and the
 * partial rotary embedding on their first `rot` dims at position S_past (the arithmetic of otter_qk_norm_rope_fwd), the new key and
 * value appended to the cache, and the single query's softmax(q k^T * scale) v over all S_past + 1 keys -- one pass.
 *   qkv      [B, H, 3, 64] bf16 contiguous: q | k | v of the new token per head (the projection output, read in place)
 *   gamma_q / beta_q / gamma_k / beta_k  fp32 [64]; cos_row / sin_row fp32 [rot]: the rotary table row of position S_past
 *   k_past / v_past  bf16, indexed [b, h, key, dim] (key < S_past) through explicit batch / head / key strides in elements, dim
 *            stride 1 and every stride a multiple of 8 (contiguous caches, the strided views the flash prefill returns and
 *            index_select results all qualify).  Read only: never written.
 *   key_valid  uint8 [B, S_past + 1] (0 = padded key) or NULL.  A row with every key masked gives o = 0.
 *   k_new / v_new  bf16 [B, H, S_past + 1, 64] contiguous, caller-allocated, not overlapping the past: rows 0..S_past-1 = the past
 *            (bit copies), row S_past = the normalised + rotated k (bf16) and the raw v.
 *   o        [B, H * 64] bf16 contiguous (the input of `dense`).
 *   workspace  fp32 scratch of at least OTTER_PERSIMMON_DECODE_WORKSPACE_BYTES(B, H, S_past + 1) bytes (split partials).
 * head_dim 64 only; rot a multiple of 16 in (0, 64]; S_past >= 1 and S_past + 1 <= 65536 keys.  The keys of each (batch, head)
 * are split across workgroups when B * H is small next to the CU count; the ranges are combined in a fixed order (deterministic).
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_PERSIMMON_DECODE_WORKSPACE_BYTES(B, H, Sk) ((int64_t)(B) * (int64_t)(H) * (((int64_t)(Sk) + 127) / 128) * 66 * 4)
int otter_persimmon_decode_attn(const void* qkv, const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k,
                                const float* cos_row, const float* sin_row, const void* k_past, int64_t k_batch_stride, int64_t k_head_stride,
                                int64_t k_key_stride, int64_t k_dim_stride, const void* v_past, int64_t v_batch_stride, int64_t v_head_stride,
                                int64_t v_key_stride, int64_t v_dim_stride, const uint8_t* key_valid, void* k_new, void* v_new, void* o,
                                void* workspace, int64_t workspace_bytes, int64_t B, int64_t H, int64_t S_past, int64_t head_dim, int64_t rot,
                                float eps, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_persimmon_decode_attn_cached / otter_persimmon_decode_attn_cached_dyn -- otter_persimmon_decode_attn over a STATIC key / value
 * cache (otter_amd/kv_cache.py), head_dim 64: the new key / value of each of the N rows (batch x beams, all at position `pos`) are written
 * in place into slot [n, h, pos] of a preallocated cache, and the row's single query attends over keys 0..pos -- keys before `pos` read
 * through a beam indirection table.  Nothing of the past is copied.
 *   qkv      [N, H, 3, 64] bf16 contiguous, 16-byte aligned: q | k | v of the new token per head (the projection output, read in place)
 *   gamma_q / beta_q / gamma_k / beta_k  fp32 [64]
 *   cos_row / sin_row  (scalar entry) fp32 [rot]: the rotary table row of position pos.
 *   cos_table / sin_table  (dyn entry) fp32 [>= S_max, rot] with a row stride >= rot (elements): the kernel takes row pos itself.
 *   k_cache / v_cache  bf16, indexed [row, h, key, 64]: row and head strides in elements (multiples of 8, head stride >= S_max * 64),
 *            key stride 64, 16-byte aligned, capacity S_max keys.  Only slot [n, :, pos, :] of each row n is written: the normalised +
 *            rotated k rounded to bf16 once, and the raw v.
 *   src      int32 [N, >= pos] (dyn: [N, >= S_max - 1]) with a row stride, or NULL: src[n, t] = the cache row holding sequence n's
 *            key / value at position t < pos (NULL: the row's own).  Entries outside [0, N) are clamped into it.
 *   key_valid  uint8 [N, >= pos + 1] (dyn: [N, >= S_max]) with a row stride (0 = padded key), or NULL.  A row with every key masked gives
 *            o = 0.
 *   o        bf16 [N, H * 64] contiguous (the input of `dense`).
 *   workspace  fp32 scratch of at least OTTER_PERSIMMON_DECODE_CACHED_WORKSPACE_BYTES(N, H, pos + 1) bytes (dyn:
 *            OTTER_PERSIMMON_DECODE_CACHED_DYN_WORKSPACE_BYTES(N, H, S_max)).
 *   pos_dev  (dyn entry) const int32 [1] in device memory, 4-byte aligned: read by the kernel.  A value outside [1, S_max) makes the
 *            call a no-op (o and the cache are left untouched): a corrupt counter never indexes the cache.
 * head_dim 64 only; rot a multiple of 16 in (0, 64]; 1 <= pos < S_max <= 65536.  The arithmetic, the key ranges and the order of every
 * reduction are those of otter_persimmon_decode_attn: on the same inputs (the past being the gathered cache, B = N, S_past = pos) o and
 * the written key slot are bit-identical to its o and k_new[:, :, S_past].  No workgroup reads a slot this call writes (reads: keys
 * < pos; writes: slot pos of the own row; key pos is taken from the new token itself), which is what makes the in-place update safe.
 * The dyn entry's launch (grid, workspace size, scalar arguments) does not depend on the position, so one captured launch can be replayed
 * at every position of a generate() call: its grid covers the most key ranges any position below S_max can have, a workgroup whose range
 * is not live returns before it touches memory, and the live ranges are combined in range order -- at every pos its o and cache slot are
 * bit-identical to the scalar entry's.  It validates before it launches, allocates nothing, does not synchronise, and queries the
 * device only for its CU count, once per device (call it once outside a stream capture).
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_PERSIMMON_DECODE_CACHED_WORKSPACE_BYTES(N, H, Sk) ((int64_t)(N) * (int64_t)(H) * (((int64_t)(Sk) + 127) / 128) * 66 * 4)
int otter_persimmon_decode_attn_cached(const void* qkv, const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k,
                                       const float* cos_row, const float* sin_row, void* k_cache, int64_t k_cache_row_stride,
                                       int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride, int64_t v_cache_head_stride,
                                       const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride, void* o,
                                       void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, int64_t pos, int64_t S_max, int64_t head_dim,
                                       int64_t rot, float eps, float scale, void* stream);
#define OTTER_PERSIMMON_DECODE_CACHED_DYN_WORKSPACE_BYTES(N, H, S_max) ((int64_t)(N) * (int64_t)(H) * (((int64_t)(S_max) + 127) / 128) * 66 * 4)
int otter_persimmon_decode_attn_cached_dyn(const void* qkv, const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k,
                                           const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                           int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                           int64_t v_cache_head_stride, const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid,
                                           int64_t key_valid_row_stride, void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H,
                                           const int32_t* pos_dev, int64_t S_max, int64_t head_dim, int64_t rot, float eps, float scale,
                                           void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_decode_attn_cached -- one cached decode step over a STATIC key / value cache (otter_amd/kv_cache.py), head_dim 128: the new
 * key / value of each of the N rows (batch x beams, all at position `pos`) are written in place into slot [n, h, pos] of a
 * preallocated cache, and the row's single query attends over keys 0..pos -- keys before `pos` read through a beam indirection table.
 *   q / k_new / v_new  bf16, indexed [n, h, 128] through their own row and head strides (elements), unit dim stride, 16-byte aligned,
 *            strides multiples of 8: three slices of one fused projection row (MPT) or three projection outputs (LLaMA), read in place.
 *   cos_rows / sin_rows  fp32 rows of 128 (the rotary table at position pos, cat(freqs, freqs) layout) with a row stride in elements
 *            (0 = one row shared by every n), or both NULL.  When given, q and k_new are rotated, x c + rotate_half(x) s with
 *            rotate_half(x) = (-x[64:], x[:64]); the rotation is evaluated exactly enough that k is rounded to bf16 ONCE, and that
 *            rounded k is both stored and used for this step's own score of key pos.
 *   k_cache / v_cache  bf16, indexed [row, h, key, 128]: row and head strides in elements (multiples of 8, head stride >= S_max * 128),
 *            key stride 128, capacity S_max keys.  Only slot [n, :, pos, :] of each row n is written.
 *   src      int32 [N, >= pos] with a row stride, or NULL: src[n, t] = the cache row holding sequence n's key / value at position
 *            t < pos (NULL: the row's own).  Entries outside [0, N) are clamped into it.
 *   key_valid  uint8 [N, >= pos + 1] with a row stride (0 = padded key), or NULL.  A row with every key masked gives o = 0.
 *   alibi_slopes  fp32 [H] or NULL: bias slope * (j - pos) on key j.
 *   o        bf16 [N, H * 128] contiguous.
 *   workspace  fp32 scratch of at least OTTER_DECODE_CACHED_WORKSPACE_BYTES(N, H, pos + 1) bytes (split partials).
 * 1 <= pos < S_max <= 65536.  No workgroup reads a slot this call writes (reads: keys < pos; writes: slot pos of the own row; key pos is
 * taken from the new token itself), which is what makes the in-place update safe.  Key ranges are combined in a fixed order: two calls
 * on the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_DECODE_CACHED_WORKSPACE_BYTES(N, H, Sk) ((int64_t)(N) * (int64_t)(H) * (((int64_t)(Sk) + 127) / 128) * 130 * 4)
int otter_decode_attn_cached(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                             int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                             const float* cos_rows, const float* sin_rows, int64_t cos_row_stride, void* k_cache, int64_t k_cache_row_stride,
                             int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride, int64_t v_cache_head_stride,
                             const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride,
                             const float* alibi_slopes, void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, int64_t pos,
                             int64_t S_max, int64_t head_dim, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_decode_attn_cached_dyn -- otter_decode_attn_cached with the position in DEVICE memory: nothing in the launch (grid, workspace
 * size, scalar arguments) depends on it, so one captured launch can be replayed at every position of a generate() call.
 *   pos_dev  const int32 [1] in device memory, 4-byte aligned: read by the kernel.  A value outside [1, S_max) makes the call a no-op
 *            (o and the cache are left untouched): a corrupt counter never indexes the cache.
 *   cos_table / sin_table  fp32 [>= S_max, 128] with a row stride >= 128 (elements), or both NULL: the kernel takes row pos itself,
 *            shared by every n.
 *   src      int32 [N, >= S_max - 1], key_valid uint8 [N, >= S_max] with row strides: columns < pos (src) and <= pos (key_valid) are
 *            read, as in the scalar entry point, but any position below S_max may come up.
 *   workspace  at least OTTER_DECODE_CACHED_DYN_WORKSPACE_BYTES(N, H, S_max) bytes.
 * Everything else is as in otter_decode_attn_cached.  The grid covers the most key ranges any position below S_max can have; the
 * ranges of the current position come from the same rule as the scalar entry point's, a workgroup whose range is not live returns
 * before it touches memory, and the live ranges are combined in range order: at every pos, o and the written cache slot are
 * bit-identical to otter_decode_attn_cached called with that pos.  The entry point validates before it launches, allocates nothing,
 * does not synchronise, and queries the device only for its CU count, once per device (call it once outside a stream capture).
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_DECODE_CACHED_DYN_WORKSPACE_BYTES(N, H, S_max) ((int64_t)(N) * (int64_t)(H) * (((int64_t)(S_max) + 127) / 128) * 130 * 4)
int otter_decode_attn_cached_dyn(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                 int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                 const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                 int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                 int64_t v_cache_head_stride, const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid,
                                 int64_t key_valid_row_stride, const float* alibi_slopes, void* o, void* workspace, int64_t workspace_bytes,
                                 int64_t N, int64_t H, const int32_t* pos_dev, int64_t S_max, int64_t head_dim, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_decode_attn_cached_i8 / otter_decode_attn_cached_i8_dyn -- otter_decode_attn_cached / _dyn over an INT8 static cache
 * (otter_amd/kv_cache.py, kv_dtype="int8"): a cached vector is 128 int8 codes and one fp32 scale.
 *   k_cache / v_cache  int8 codes, indexed [row, h, key, 128]: row and head strides in elements (multiples of 16, head stride
 *            >= S_max * 128), key stride 128, 16-byte aligned.
 *   k_scale / v_scale  fp32, indexed [row, h, key]: row and head strides in elements (head stride >= S_max), key stride 1, 4-byte aligned.
 * For x = the vector the bf16 cache would store (k after rotary, rounded once to bf16; v as given), read as fp32:
 *   amax = max |x[i]|;  scale = amax / 127 (1 when amax == 0);  code = clamp(rint(x[i] / scale), -127, 127) (half to even);
 *   what attention sees is (float)code * scale.
 * The step quantises the new token, writes its 128 + 128 codes and two scales into slot [n, h, pos] of row n, and attends over keys
 * 0..pos with key pos in its dequantised form: it returns what "append, then attend over the cache" returns.  Every other argument,
 * the in-place invariant (no workgroup reads a slot or a scale this call writes), the fixed-order reductions, and the relation of the
 * pair (at every pos in [1, S_max) the _dyn entry gives the bits of the scalar entry; outside it, it is a no-op) are as documented for
 * otter_decode_attn_cached and otter_decode_attn_cached_dyn.
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_DECODE_CACHED_I8_WORKSPACE_BYTES(N, H, Sk) ((int64_t)(N) * (int64_t)(H) * (((int64_t)(Sk) + 127) / 128) * 130 * 4)
int otter_decode_attn_cached_i8(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                const float* cos_rows, const float* sin_rows, int64_t cos_row_stride, void* k_cache, int64_t k_cache_row_stride,
                                int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride, int64_t v_cache_head_stride,
                                float* k_scale, int64_t k_scale_row_stride, int64_t k_scale_head_stride, float* v_scale,
                                int64_t v_scale_row_stride, int64_t v_scale_head_stride, const int32_t* src, int64_t src_row_stride,
                                const uint8_t* key_valid, int64_t key_valid_row_stride, const float* alibi_slopes, void* o, void* workspace,
                                int64_t workspace_bytes, int64_t N, int64_t H, int64_t pos, int64_t S_max, int64_t head_dim, float scale,
                                void* stream);
#define OTTER_DECODE_CACHED_I8_DYN_WORKSPACE_BYTES(N, H, S_max) ((int64_t)(N) * (int64_t)(H) * (((int64_t)(S_max) + 127) / 128) * 130 * 4)
int otter_decode_attn_cached_i8_dyn(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                    int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                    const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                    int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                    int64_t v_cache_head_stride, float* k_scale, int64_t k_scale_row_stride, int64_t k_scale_head_stride,
                                    float* v_scale, int64_t v_scale_row_stride, int64_t v_scale_head_stride, const int32_t* src,
                                    int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride, const float* alibi_slopes,
                                    void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, const int32_t* pos_dev,
                                    int64_t S_max, int64_t head_dim, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_decode_attn_cached_shared / otter_decode_attn_cached_shared_dyn -- otter_decode_attn_cached / _dyn for beam search over a
 * SHARED PROMPT (otter_amd/kv_cache.py, StaticKVCache.share_prompt): the N rows are N / group sentences x `group` beams, the beams of a
 * sentence contiguous, and keys [0, shared_len) of every beam are those of the sentence's first row (the leader, row (n / group) * group).
 *   group    rows per sentence: 2 .. OTTER_DECODE_CACHED_SHARED_MAX_GROUP (one compiled instance each); N must be a multiple of it.
 *   shared_len  a host scalar, 1 <= shared_len <= pos (dyn: 1 <= shared_len < S_max; a position below shared_len read from pos_dev makes
 *            the call a no-op, like one outside [1, S_max)).  Constant over a generate() call, so it may sit in a captured launch.
 *   src      as in otter_decode_attn_cached, but columns < shared_len are NOT read (they count as (n / group) * group).
 *   workspace  at least OTTER_DECODE_CACHED_SHARED_WORKSPACE_BYTES(N, H, pos + 1) bytes (dyn: ..._SHARED_DYN_...(N, H, S_max)).
 * The result is what otter_decode_attn_cached returns for a table whose columns [0, shared_len) hold (n / group) * group (the same
 * arithmetic per key; the key ranges are split for N / group * H workgroups per range, so the fixed-order sums may group differently),
 * and the written slot [n, h, pos] of every row n is bit-equal to that entry point's.  One workgroup serves a (key range, head, sentence):
 * a key below shared_len is loaded once, from the leader's row, for all `group` queries.  No workgroup reads a slot this call writes:
 * writes are slot pos of every row, reads through src are of keys < pos, shared reads of keys < shared_len <= pos.  Every other argument,
 * the fixed-order reductions (two calls on the same inputs give the same bits) and the relation of the pair (at every pos in
 * [shared_len, S_max) the _dyn entry gives the bits of the scalar entry) are as documented for otter_decode_attn_cached / _dyn.
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_DECODE_CACHED_SHARED_MAX_GROUP 6
#define OTTER_DECODE_CACHED_SHARED_WORKSPACE_BYTES(N, H, Sk) ((int64_t)(N) * (int64_t)(H) * (((int64_t)(Sk) + 127) / 128) * 130 * 4)
int otter_decode_attn_cached_shared(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                    int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                    const float* cos_rows, const float* sin_rows, int64_t cos_row_stride, void* k_cache,
                                    int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                    int64_t v_cache_head_stride, const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid,
                                    int64_t key_valid_row_stride, const float* alibi_slopes, void* o, void* workspace, int64_t workspace_bytes,
                                    int64_t N, int64_t H, int64_t pos, int64_t S_max, int64_t head_dim, float scale, int64_t group,
                                    int64_t shared_len, void* stream);
#define OTTER_DECODE_CACHED_SHARED_DYN_WORKSPACE_BYTES(N, H, S_max) ((int64_t)(N) * (int64_t)(H) * (((int64_t)(S_max) + 127) / 128) * 130 * 4)
int otter_decode_attn_cached_shared_dyn(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                        int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                        const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                        int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                        int64_t v_cache_head_stride, const int32_t* src, int64_t src_row_stride, const uint8_t* key_valid,
                                        int64_t key_valid_row_stride, const float* alibi_slopes, void* o, void* workspace,
                                        int64_t workspace_bytes, int64_t N, int64_t H, const int32_t* pos_dev, int64_t S_max, int64_t head_dim,
                                        float scale, int64_t group, int64_t shared_len, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_decode_attn_cached_shared_i8 / otter_decode_attn_cached_shared_i8_dyn -- otter_decode_attn_cached_i8 / _i8_dyn for beam search
 * over a SHARED PROMPT: the grouping of otter_decode_attn_cached_shared over the INT8 static cache.  The arguments are those of
 * otter_decode_attn_cached_i8 / _i8_dyn followed by `group, shared_len` (as documented for otter_decode_attn_cached_shared / _dyn:
 * group 2 .. OTTER_DECODE_CACHED_SHARED_MAX_GROUP, N a multiple of it; 1 <= shared_len <= pos, dyn: 1 <= shared_len < S_max and a
 * position below shared_len read from pos_dev makes the call a no-op).
 *   src      columns < shared_len are NOT read (they count as (n / group) * group).
 *   k_cache / v_cache / k_scale / v_scale  slots [0, shared_len) of the rows that are not leaders are NOT read.
 *   workspace  at least OTTER_DECODE_CACHED_SHARED_I8_WORKSPACE_BYTES(N, H, pos + 1) bytes (dyn: ..._SHARED_I8_DYN_...(N, H, S_max)).
 * The result is what otter_decode_attn_cached_i8 returns for a table whose columns [0, shared_len) hold (n / group) * group (the same
 * arithmetic per key; the key ranges are split for N / group * H workgroups per range and a key belongs to 16 lanes, so the fixed-order
 * sums may group differently), and the written slot [n, h, pos] of every row n -- 128 + 128 codes and two scales -- is bit-equal to that
 * entry point's.  One workgroup serves a (key range, head, sentence): a key below shared_len is loaded and dequantised once, from the
 * leader's row, for all `group` queries.  No workgroup reads a slot or a scale this call writes: writes are slot pos of every row, reads
 * through src are of keys < pos, shared reads of keys < shared_len <= pos.  The fixed-order reductions (two calls on the same inputs
 * give the same bits) and the relation of the pair (at every pos in [shared_len, S_max) the _dyn entry gives the bits of the scalar
 * entry) are as documented for otter_decode_attn_cached / _dyn.
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_DECODE_CACHED_SHARED_I8_WORKSPACE_BYTES(N, H, Sk) ((int64_t)(N) * (int64_t)(H) * (((int64_t)(Sk) + 127) / 128) * 130 * 4)
int otter_decode_attn_cached_shared_i8(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                       int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                       const float* cos_rows, const float* sin_rows, int64_t cos_row_stride, void* k_cache,
                                       int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                       int64_t v_cache_head_stride, float* k_scale, int64_t k_scale_row_stride, int64_t k_scale_head_stride,
                                       float* v_scale, int64_t v_scale_row_stride, int64_t v_scale_head_stride, const int32_t* src,
                                       int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride, const float* alibi_slopes,
                                       void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, int64_t pos, int64_t S_max,
                                       int64_t head_dim, float scale, int64_t group, int64_t shared_len, void* stream);
#define OTTER_DECODE_CACHED_SHARED_I8_DYN_WORKSPACE_BYTES(N, H, S_max) ((int64_t)(N) * (int64_t)(H) * (((int64_t)(S_max) + 127) / 128) * 130 * 4)
int otter_decode_attn_cached_shared_i8_dyn(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                                           int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                                           const float* cos_table, const float* sin_table, int64_t table_row_stride, void* k_cache,
                                           int64_t k_cache_row_stride, int64_t k_cache_head_stride, void* v_cache, int64_t v_cache_row_stride,
                                           int64_t v_cache_head_stride, float* k_scale, int64_t k_scale_row_stride, int64_t k_scale_head_stride,
                                           float* v_scale, int64_t v_scale_row_stride, int64_t v_scale_head_stride, const int32_t* src,
                                           int64_t src_row_stride, const uint8_t* key_valid, int64_t key_valid_row_stride,
                                           const float* alibi_slopes, void* o, void* workspace, int64_t workspace_bytes, int64_t N, int64_t H,
                                           const int32_t* pos_dev, int64_t S_max, int64_t head_dim, float scale, int64_t group, int64_t shared_len,
                                           void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_branch_attn_merge -- the self-attention of candidate rows over a cached prompt (csrc/branch_attn.hip;
 * StaticKVCache.attend_branches), head_dim 128, as many key heads as query heads.  N = B * C * T one-token rows, row
 * n = (b C + c) T + t: position t (0 <= t < T <= OTTER_BRANCH_ATTN_MAX_T) of candidate c of sentence b.  Row (b, c, t) attends over
 * the prompt of sentence b -- that part is given: o1, lse1 -- and over the keys (b, c, 0..t) of its own candidate.
 *   q / k_new / v_new  bf16 [N, H, 128] given by row and head strides (elements, multiples of 8, not negative; dim stride 1),
 *                      16-byte aligned: the three slices of the projection output, read in place (LLaMA: q, k rotated already).
 *   o1     fp32 [N, H, 128] contiguous: the attention output of each row over the prompt's keys alone, unrounded (otter_flash_attn_fwd_f32).
 *   lse1   fp32 [N / rows_per_sentence, H, rows_per_sentence] (natural log): the log-sum-exp of those scores, with the ALiBi origin
 *          at the prompt's LAST key -- exactly what otter_flash_attn_fwd_f32 (causal = 0) writes for q viewed as
 *          [B, rows_per_sentence, H, 128] against the prompt's keys.  -inf: no visible prompt key; o1 of that (row, head) is not read.
 *   rows_per_sentence  C * T: a multiple of T that divides N.
 *   alibi_slopes  fp32 [H] or NULL.      o  bf16 [N, H, 128] contiguous.
 * With a = slopes ? slopes[h] : 0:  L1 = lse1 - a (t + 1);  e_u = scale q . k_new[(b,c,u)] + a (u - t), u = 0..t;
 * M = max(L1, max_u e_u);  o = (exp(L1 - M) o1 + sum_u exp(e_u - M) v_new[(b,c,u)]) / (exp(L1 - M) + sum_u exp(e_u - M)), in fp32,
 * rounded once.  Nothing but o is written; no workspace, no atomics; two calls on the same inputs give the same bits.  A bad
 * argument (null pointer, head_dim != 128, T outside [1, 64], N not a multiple of T, rows_per_sentence, alignment, strides)
 * launches nothing: OTTER_ERR_ARG and otter_last_error().
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_BRANCH_ATTN_MAX_T 64
int otter_branch_attn_merge(const void* q, int64_t q_row_stride, int64_t q_head_stride, const void* k_new, int64_t k_new_row_stride,
                            int64_t k_new_head_stride, const void* v_new, int64_t v_new_row_stride, int64_t v_new_head_stride,
                            const float* o1, const float* lse1, const float* alibi_slopes, void* o, int64_t N, int64_t H, int64_t T,
                            int64_t rows_per_sentence, int64_t head_dim, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_xattn_decode --the masked cross-attention core of one cached decode step over a media cache (otter_amd/media_cache.py),
 * head_dim 64: N rows (batch x beams) of ONE query each attend over the projected media of their sentence.
 *   q        bf16 [N, H * 64] with a row stride (elements, a multiple of 8, >= H * 64), 16-byte aligned.
 *   k / v    bf16 views [sentences, M, H * 64] of one buffer with a shared row stride (a multiple of 8, >= H * 64; the sentence stride
 *            is M * kv_stride), 16-byte aligned.  M = T_img * n_per_media <= 65536; the media index of key j is j / n_per_media.
 *   the media of row r are sentence r / rows_per_media (rows_per_media = the beams of a sentence; N a multiple of it).
 *   text_time  int32 [N].  mask_mode EQ or GE (OTTER_MASK_NONE is rejected: a decode step always has a text_time).
 *   o        bf16 [N, H * 64] contiguous.
 * Semantics are those of otter_attn_fwd for a Tq = 1 row: masked scores take -FLT_MAX, a row whose every key is masked comes out
 * uniform (1/M over all keys), a row with text_time == 0 is zeroed in EQ mode only.  In EQ mode with 1 <= text_time <= T_img only
 * the n_per_media keys of that media are read.  No workspace, no atomics; two calls on the same inputs give the same bits.
 * ------------------------------------------------------------------------------------------------------- */
int otter_xattn_decode(const void* q, int64_t q_stride, const void* k, const void* v, int64_t kv_stride, const int32_t* text_time, void* o,
                       int64_t N, int64_t H, int64_t T_img, int64_t n_per_media, int64_t rows_per_media, int mask_mode, float scale,
                       void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Int8 weight-only products of the frozen decoder during generation (the reference's serving worker offers load_in_8bit for the
 * same model: pipeline/serve/model_worker.py:92-94).  Format: qweight int8 [N, K] row-major with row stride ldw, scale fp32 [N]:
 * scale[n] = max_k |W[n,k]| / 127 (1 for an all-zero row), q[n,k] = clamp(round_half_even(W[n,k] / scale[n]), -127, 127).
 *   otter_gemv_w8   y[M, N] = (x[M, K] . q[N, K]^T) * scale[N] (+ bias[N]), then the activation `act`, 1 <= M <= 16: the linears of a
 *       cached decode step.  act: 0 none, 1 the exact-erf GELU (MPT), 3 the squared ReLU relu(v)^2 of the Persimmon MLP, evaluated in
 *       fp32 on the fp32 value v and rounded once to y's dtype; every other code (2 included) is an argument error.  x bf16 (row stride ldx), y bf16 or fp32 (row stride ldy; only the M x N block is
 *       written), bias bf16 / fp32 or NULL.  x is not quantised; q is converted to bf16 (exact) and accumulated in fp32, the scale
 *       multiplies the finished fp32 sum, then bias, then activation.  N >= 1, K % 16 == 0, ldw % 16 == 0, ldx % 8 == 0; x, qweight,
 *       y 16-byte aligned.  workspace: at least OTTER_GEMV_W8_WORKSPACE_BYTES(M, N, K) bytes (fp32 split-K partials, combined in
 *       a fixed order: two calls on the same inputs give the same bits).
 *   otter_gemm_w8_rows   the same product, arguments, `act` codes and rules for 1 <= M <= 64: the linears of a one-token step of 17 to 64 rows
 *       (batch x beams).  The weight is still streamed once; x is shared by a workgroup through LDS.  workspace: at least
 *       OTTER_GEMM_W8_ROWS_WORKSPACE_BYTES(M, N, K) bytes.  The K split and with it the summation order of every output element
 *       depend on (N, K) only: two calls give the same bits, and row m of y has the same bits whatever M is and whatever the other
 *       rows of x hold.  For M <= 16 the result equals otter_gemv_w8's to rounding, NOT bit for bit (the two sum K in different
 *       groupings).
 *   otter_gemm_w8_panel   the same product, arguments, `act` codes and rules for 1 <= M <= 256: the linears of a one-token step of 65 to 256
 *       rows.  The weight is still streamed once; a wave owns 32 output columns (128 per workgroup) and reuses every x fragment it reads
 *       from LDS over both of its 16-row weight tiles.  workspace: at least OTTER_GEMM_W8_PANEL_WORKSPACE_BYTES(M, N, K) bytes.
 *       Row independence: the K split (at most 8 ranges, never more workgroups than one per CU of a 256-CU part, never less than 256 K
 *       elements per range) and every K range are functions of (N, K) alone, never of M; every output element is one accumulation chain
 *       per range in ascending K and the ranges are added in range order.  So two calls give the same bits, and row m of y has the same
 *       bits whatever M is, whatever the other rows of x (and R) hold -- NaN included -- and wherever the row sits in the batch.  The
 *       split rule is this entry's own: its results equal otter_gemm_w8_rows's to rounding, NOT bit for bit.
 *   otter_gemv_w8_gated (1 <= M <= 16), otter_gemm_w8_rows_gated (1 <= M <= 64), otter_gemm_w8_panel_gated (1 <= M <= 256)   the same
 *       products with the gated-residual tail of the gated cross-attention block's second FFN product (the OTTER_EPI_SCALE_RES tail of otter_gemm):
 *           y[m, n] = v * s + R[m, n],   v = (x[m, :] . q[n, :]) * scale[n] (+ bias[n]),   s = gate ? tanhf(*gate) : 1,
 *       evaluated in fp32 on the fp32 sum and rounded once to y's dtype.  Arguments: those of otter_gemv_w8 without `act`, then
 *       gate (device pointer to ONE fp32, may be NULL), R (bf16 or fp32 [M, N] with row stride ldr >= N, aligned to its element, never
 *       NULL).  y and R may NOT alias: blocks that share a byte (the same tensor included) are refused.  Workspace macro, split rule,
 *       fixed-order combination of the K ranges and -- for the rows and panel entries -- the independence of row m from M and from the
 *       other rows are those of the plain entries.  Host checks, in this order, each an OTTER_ERR_ARG with a message that names the entry:
 *         1. x, qweight, scale, y, workspace, R not NULL          5. alignment: x, qweight, y 16-byte; ldw % 16 == 0; ldx % 8 == 0
 *         2. 1 <= M <= 16 (rows: 64, panel: 256)                  6. ldw >= K, ldx >= K, ldy >= N, ldr >= N
 *         3. 1 <= N <= 2^30                                       7. y / bias / R dtype is OTTER_F32 or OTTER_BF16
 *         4. K a positive multiple of 16, at most 2^30            8. y and R do not overlap       9. workspace_bytes
 *       (the plain entries run checks 1-7 without R, then `act`, then the workspace).
 *   otter_dequant_w8   out[n, k] = bf16(float(q[n, k]) * scale[n]), out bf16 [N, K] with row stride ldo (ldo % 8 == 0, 16-byte
 *       aligned): the pass in front of the library GEMM for prompt passes of more than 16 rows (and one-token steps of more than 64, or
 *       with the panel route switched on more than 256).
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_GEMV_W8_WORKSPACE_BYTES(M, N, K) ((int64_t)8 * (int64_t)(M) * (int64_t)(N) * 4)   /* at most 8 K ranges, whatever K */
int otter_gemv_w8(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias, int bias_dtype, void* y,
                  int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, int act, void* workspace, int64_t workspace_bytes, void* stream);
#define OTTER_GEMM_W8_ROWS_WORKSPACE_BYTES(M, N, K) ((int64_t)8 * (int64_t)(M) * (int64_t)(N) * 4)   /* at most 8 K ranges, whatever K */
int otter_gemm_w8_rows(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias, int bias_dtype,
                       void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, int act, void* workspace, int64_t workspace_bytes,
                       void* stream);
int otter_gemv_w8_gated(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias, int bias_dtype,
                        void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, const float* gate, const void* R, int64_t ldr,
                        int r_dtype, void* workspace, int64_t workspace_bytes, void* stream);
int otter_gemm_w8_rows_gated(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias,
                             int bias_dtype, void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, const float* gate,
                             const void* R, int64_t ldr, int r_dtype, void* workspace, int64_t workspace_bytes, void* stream);
/* the panel entries split K into at most min(8, 256 / ceil(N / 128)) ranges (at least 1), whatever K and M */
#define OTTER_GEMM_W8_PANEL_MAX_SPLIT(N) \
    (256 / (((int64_t)(N) + 127) / 128) >= 8 ? (int64_t)8 : 256 / (((int64_t)(N) + 127) / 128) >= 1 ? 256 / (((int64_t)(N) + 127) / 128) : (int64_t)1)
#define OTTER_GEMM_W8_PANEL_WORKSPACE_BYTES(M, N, K) (OTTER_GEMM_W8_PANEL_MAX_SPLIT(N) * (int64_t)(M) * (int64_t)(N) * 4)
int otter_gemm_w8_panel(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias, int bias_dtype,
                        void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, int act, void* workspace, int64_t workspace_bytes,
                        void* stream);
int otter_gemm_w8_panel_gated(const void* x, int64_t ldx, const void* qweight, int64_t ldw, const float* scale, const void* bias,
                              int bias_dtype, void* y, int64_t ldy, int y_dtype, int64_t M, int64_t N, int64_t K, const float* gate,
                              const void* R, int64_t ldr, int r_dtype, void* workspace, int64_t workspace_bytes, void* stream);
int otter_dequant_w8(const void* qweight, int64_t ldw, const float* scale, void* out, int64_t ldo, int64_t N, int64_t K, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_logits_process -- the tensor-valued logits processors of generate() (otter_amd/generation.py: _Processors) in one launch per
 * step, in place on the score matrix, from the token history on the device.  One workgroup per row; no allocation, no synchronise.
 *   scores   fp32 [N, V] with a row stride (elements, >= V), 4-byte aligned.  1 <= V <= 262144 (a V-bit bitmap in LDS).
 *   ids      int64 [N, L] with a row stride (elements, >= L), 8-byte aligned.  1 <= L <= 2^30.
 * Applied in this order:
 *   1. repetition_penalty p (finite, > 0; 1 = off): for every DISTINCT token t of ids[r, 0:L], s = scores[r, t] becomes s * p if s < 0,
 *      else s * (1.0f / p) -- the reciprocal form is what torch's device kernel computes for `tensor / Python scalar`.  A token that
 *      occurs k times is penalised once.
 *   2. no_repeat_ngram n (>= 0; 0 = off), only when L + 1 >= n.  n == 1: every token of the row is banned.  n > 1: ids[r, i + n - 1] is
 *      banned for every 0 <= i <= L - n with ids[r, i : i + n - 1] == ids[r, L - n + 1 : L].
 *   3. ban: int32 [n_ban], banned in every row.
 *   4. words: word w is word_tokens[word_offsets[w] : word_offsets[w + 1]] (int32; word_offsets int32 [n_words + 1], non-decreasing,
 *      inside word_tokens).  A word of m >= 2 tokens bans its last token in row r if m - 1 <= L and the row ends in its first m - 1
 *      tokens; shorter words are ignored.
 *   5. eos: int32 [n_eos], banned in every row when suppress_eos != 0 (the host decides it from L, min_length and min_new_tokens).
 * A ban stores -inf and wins over the penalty.  A token outside [0, V), in ids or in a list, penalises nothing, bans nothing and is
 * never used as an index; as a value it still takes part in the n-gram and word comparisons.  List pointers may be NULL when their
 * count is 0; they are 4-byte aligned.
 * ------------------------------------------------------------------------------------------------------- */
int otter_logits_process(float* scores, int64_t scores_stride, const int64_t* ids, int64_t ids_stride, int64_t N, int64_t V, int64_t L,
                         float repetition_penalty, int no_repeat_ngram, const int32_t* ban, int64_t n_ban, const int32_t* eos, int64_t n_eos,
                         int suppress_eos, const int32_t* word_tokens, const int32_t* word_offsets, int64_t n_words, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_beam_step -- one beam-search step of generate() (otter_amd/generation.py: generate_tokens, num_beams > 1 without sampling or
 * groups) in two launches: the n_cand best continuations of every sentence, BeamSearchScorer.process with its hypothesis lists, and the
 * reordered token history.  No allocation, no synchronise, no device query; all state is the caller's, at fixed addresses.
 *   logp         fp32 [B * nb, V], row stride (elements, >= V): the processed log-probabilities.  Read only.
 *   beam_scores  fp32 [B * nb], in and out.
 *   ids          int64 [B * nb, L], row stride (>= L): the history.  ids_next int64 [B * nb, L + 1], row stride (>= L + 1), not overlapping
 *                ids: row r becomes ids[beam_idx[r], 0:L] followed by the new token.  beam_idx int64 [B * nb], out.
 *   eos          int32 [n_eos], NULL when n_eos == 0.  pad_token_id fills the beams of a finished sentence.
 *   n_cand       the host's max(2, 1 + n_eos) * nb; nb <= n_cand <= min(nb * V, OTTER_BEAM_STEP_MAX_CANDIDATES).
 *   L0, max_len  the prompt length and the length generation stops at; 1 <= L0 <= L < max_len.
 *   early_stopping  0 = False, 1 = True, 2 = "never"; length_penalty_positive: whether length_penalty > 0 (read by "never" only).
 *   len_pow      fp64 [max_len - L0 + 1]: len_pow[g] = float(g) ** length_penalty as the host computed it (entry 0 is never read).
 * Selection: for sentence b the n_cand largest of logp[b * nb + j, t] + beam_scores[b * nb + j] (one fp32 add), in descending order.
 * TIE RULE: the larger sum first; among equal sums the smaller flat index j * V + t first.  -inf is an ordinary value, -0 equals +0;
 * NaN sums are outside the contract.
 * Scorer, candidate by candidate in that order until nb beams are filled: an eos candidate at rank >= nb is skipped; at rank < nb it
 * adds ids[b * nb + j, 0:L] as a hypothesis of generated length L + 1 - L0; any other candidate becomes the next beam (sum, token,
 * source row).  Beams left unfilled get (0, pad_token_id, row 0); a finished sentence gets (0, pad_token_id, row b * nb) in every beam.
 * Then done[b] |= is_done(best sum of the step).  Hypothesis arithmetic is fp64: score = (double)sum / len_pow[generated length].
 * State (zero before the first step unless noted), nb entries per sentence:
 *   hyp_score fp64 [B, nb], hyp_len int32 [B, nb], hyp_slot int32 [B, nb]: the list of sentence b IN INSERTION ORDER, hyp_count[b]
 *       entries long; entry i's tokens are hyp_tokens[b, hyp_slot[b, i], 0:hyp_len[b, i]] (hyp_tokens int64 [B, nb, max_len]).  An entry
 *       is added when the list is short or its score exceeds hyp_worst[b]; a full list then drops its lowest (score, list index) and
 *       hyp_worst[b] becomes the second lowest score, otherwise hyp_worst[b] = min(score, hyp_worst[b]).  hyp_worst fp64 [B] starts at 1e9.
 *   done int32 [B]; all_done int32 [2]: all_done[0] = every sentence is done, all_done[1] = how many are.
 *   workspace    at least otter_beam_step_workspace_bytes(B, nb, V, n_cand) bytes (-1: arguments out of range), 8-byte aligned.
 * Limits: nb * V <= 2^31 - 1, B * nb <= 65535.
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_BEAM_STEP_MAX_CANDIDATES 64
int64_t otter_beam_step_workspace_bytes(int64_t B, int64_t nb, int64_t V, int64_t n_cand);
int otter_beam_step(const float* logp, int64_t logp_stride, float* beam_scores, const int64_t* ids, int64_t ids_stride, int64_t* ids_next,
                    int64_t ids_next_stride, int64_t* beam_idx, const int32_t* eos, int64_t n_eos, int64_t pad_token_id, int64_t B, int64_t nb,
                    int64_t V, int64_t n_cand, int64_t L, int64_t L0, int64_t max_len, int early_stopping, int length_penalty_positive,
                    const double* len_pow, int32_t* done, double* hyp_score, int64_t* hyp_tokens, int32_t* hyp_len, int32_t* hyp_slot,
                    int32_t* hyp_count, double* hyp_worst, int32_t* all_done, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * otter_select_step -- the token selection of generate() (otter_amd/generation.py: generate_tokens, num_beams == 1) in ONE launch per
 * step: the step's token of every row from the processed scores, written into the preallocated history, with the host loop's
 * unfinished / eos bookkeeping.  One workgroup per row; no allocation, no synchronise, no sort; the scores are never written.
 *   scores   fp32 [N, V], row stride (elements, >= V), 4-byte aligned.  1 <= V <= OTTER_SELECT_STEP_MAX_VOCAB.  Read only.
 *   ids_buf  int64 [N, max_len], row stride (>= max_len), 8-byte aligned; ONLY column L is written.  0 <= L < max_len <= 2^30.
 *   mode     OTTER_SELECT_GREEDY or OTTER_SELECT_SAMPLE.  inv_temperature, top_k, top_p, q are read in sample mode only.
 * GREEDY: the index of the row maximum.  TIE RULE: among equal maxima the first index wins (-0 equals +0); a NaN counts as the maximum
 * and the first NaN wins -- torch.argmax's rule.
 * SAMPLE: inv_temperature fp32 (finite, > 0: the host's fp32 1 / T), top_k >= 0 (0 = off), top_p in (0, 1] (1 = off), q fp32 [N, V]
 * with row stride q_stride (>= V): the exponential draws, `torch.empty_like(p).exponential_(1)` -- torch.multinomial(p, 1) is
 * argmax(p / q) over exactly these draws.  Per row:
 *   s'_j = fp32(s_j * inv_temperature), rounded before anything else uses it (never contracted into the subtraction below); m = max s'.
 *   top-k: k = min(max(top_k, 1), V), v_k = the k-th largest s'; keep s'_j >= v_k.  ALL ties at v_k stay: the host's `scores < kth`
 *       rule, so the kept set is the host's bit for bit.
 *   top-p, over the top-k survivors: w_j = floor(expf(s'_j - m) * 2^40) (a 64-bit integer; expf in fp32), Z = sum w_j,
 *       R = min(floor((1 - top_p) * (double)Z), Z - 1) with 1 - top_p in fp64; a value v is kept iff  sum of w_j over s'_j <= v  >  R.
 *       The maximum is always kept.  This is the host rule (ascending, `cumsum(softmax) <= 1 - top_p` is removed) with the mass in
 *       integers, so that no summation order can move the threshold, and with ONE DIFFERENCE: equal values are kept or removed
 *       TOGETHER, where the host's unstable sort splits a tie group that straddles the boundary arbitrarily.  Apart from rounding at
 *       the boundary this is the only place where the kept set can differ from the host's.
 *   draw: the kept j that maximises expf(s'_j - m) / q_j, an IEEE fp32 division (q_j = 0 gives inf, as on the host; a NaN ratio never
 *       wins).  TIE RULE: the smaller j among equal ratios.
 *   A row with a NaN score, or whose maximum s' is not finite, returns SOME token in [0, V) (the host path raises there).
 * Bookkeeping, both modes, with `sel` the selected token: ids_buf[r, L] = unfinished[r] ? sel : pad_token_id; if unfinished[r] and sel
 * is in eos (int32 [n_eos], NULL when n_eos == 0), unfinished[r] becomes 0 and *n_unfinished (int32) is decremented by an integer
 * atomic.  unfinished is uint8 [N] (1 = still generating; only ever cleared), n_unfinished starts at the number of ones in it.
 * Deterministic: every histogram is integer, so the same inputs give the same tokens on every call.
 * ------------------------------------------------------------------------------------------------------- */
#define OTTER_SELECT_STEP_MAX_VOCAB 262144
#define OTTER_SELECT_GREEDY 0
#define OTTER_SELECT_SAMPLE 1
int otter_select_step(const float* scores, int64_t scores_stride, int64_t N, int64_t V, int64_t* ids_buf, int64_t ids_stride, int64_t L,
                      int64_t max_len, int mode, float inv_temperature, int64_t top_k, double top_p, const float* q, int64_t q_stride,
                      uint8_t* unfinished, int32_t* n_unfinished, const int32_t* eos, int64_t n_eos, int64_t pad_token_id, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * OtterHD / Fuyu-8B path (config C5): row-wise kernels of the Persimmon decoder and the patch scatter.
 *   otter_qk_norm_rope_fwd  /root/reference/src/otter_ai/models/fuyu/modeling_persimmon.py:262-304: the per-head interleaved
 *       projection output qkv [tokens, H, 3, 64] (bf16) is read in place; q and k get LayerNorm over the 64-wide head
 *       (gamma / beta fp32 [64]) and the partial rotary embedding on their first `rot` dims (cos / sin fp32 [S, rot], position
 *       = token % S); q', k' (and v unless v_out is NULL: the head_dim-64 attention kernels read v in place from qkv) are written
 *       as bf16 [tokens, H, out_width]: out_width 64 = compact heads, 128 = columns 64..127 zero (head-dim padding for the
 *       128-wide flash kernels, round 2's layout).  stats [tokens, H, 2, 2] fp32 = (mean, rstd) of q and k, for the backward.
 *   otter_qk_norm_rope_bwd  dq / dk / dv [tokens, H, in_width] (columns 0..63 used) -> dqkv [tokens, H, 3, 64]; dv NULL: the v slots
 *       of dqkv are left alone (the attention backward wrote them in place); partial
 *       [otter_qk_norm_rope_bwd_blocks(tokens, H), 4, 64] fp32 = per-block sums of (dgamma_q, dbeta_q, dgamma_k, dbeta_k),
 *       to be summed over the first axis by the caller (deterministic).
 *   otter_sqrelu_fwd/_bwd   relu(x)^2 (:180-194), bf16, n % 8 == 0.
 *   otter_scatter_rows      fuyu/modeling_fuyu.py:44-77: out[b,s,:] = idx[b,s] < 0 ? word[b,s,:] : patch[b, idx[b,s], :].
 * ------------------------------------------------------------------------------------------------------- */
int otter_qk_norm_rope_fwd(const void* qkv, const float* gamma_q, const float* beta_q, const float* gamma_k, const float* beta_k,
                           const float* cos_t, const float* sin_t, void* q_out, void* k_out, void* v_out, float* stats, int64_t tokens,
                           int64_t S, int64_t H, int64_t rot, float eps, int64_t out_width, void* stream);
int64_t otter_qk_norm_rope_bwd_blocks(int64_t tokens, int64_t H);
int otter_qk_norm_rope_bwd(const void* dq, const void* dk, const void* dv, const void* qkv, const float* stats, const float* gamma_q,
                           const float* gamma_k, const float* cos_t, const float* sin_t, void* dqkv, float* partial, int64_t tokens,
                           int64_t S, int64_t H, int64_t rot, int64_t in_width, void* stream);
int otter_sqrelu_fwd(const void* x, void* y, int64_t n, void* stream);
int otter_sqrelu_bwd(const void* x, const void* dy, void* dx, int64_t n, void* stream);
int otter_scatter_rows(const void* word, int word_dtype, const void* patch, int patch_dtype, const int64_t* idx, void* out, int64_t B,
                       int64_t S, int64_t P, int64_t D, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Token cross-entropy of the decoder host on bf16 logits: F.cross_entropy(logits.view(-1, V), labels) with
 * ignore_index = -100 and mean reduction     /root/reference/src/otter_ai/models/mpt/modeling_mpt.py:428-435
 * (the caller rolls the labels).  fwd: lse[r], nll[r] (0 for ignored rows) from one read of the logits; the mean
 * is sum(nll) / max(n_valid, 1).  bwd: dlogits (bf16) = (softmax - onehot) * (*dloss) / max(*n_valid, 1), zero rows for
 * ignored labels; dloss and n_valid are device scalars (no host synchronisation).  Row strides: multiples of 4 elements (16-byte
 * accesses when they are multiples of 8 and the bases 16-byte aligned, 8-byte accesses otherwise -- LLaMA's 32004-wide vocabulary).
 * ------------------------------------------------------------------------------------------------------- */
int otter_cross_entropy_fwd(const void* logits, int64_t ld, const int64_t* labels, float* lse, float* nll, int64_t rows, int64_t V,
                            void* stream);
int otter_cross_entropy_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* lse, const float* dloss,
                            const float* n_valid, void* dlogits, int64_t ldd, int64_t rows, int64_t V, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Optimizer step of the recipe: torch.nn.utils.clip_grad_norm_(params, max_norm) followed by
 * torch.optim.AdamW.step()          /root/reference/pipeline/train/instruction_following.py:246-251
 * as two sweeps: otter_grad_sumsq (+ otter_clip_coef -> {norm, coefficient} on the device) and otter_adamw_step, which
 * multiplies the gradients by *grad_scale on the fly (the scaled gradients are NOT written back), follows torch's
 * fused AdamW arithmetic (decoupled weight decay, lerp first moment, bias corrections passed in) and optionally
 * refreshes a bf16 copy of each parameter.  torch.optim.AdamW keeps one `step` per parameter and one lr per param
 * group: a table row may carry its own lr / bias corrections (bias_correction1 != 0), which then override the
 * launch-wide arguments for that tensor.  `tensors` is a DEVICE array; block i of the launch owns elements
 * [blk_chunk[i] * otter_adamw_chunk(), ...) of tensors[blk_tensor[i]].
 * ------------------------------------------------------------------------------------------------------- */
typedef struct otter_adamw_tensor {
    float* p; const float* g; float* m; float* v;
    uint16_t* shadow;      /* bf16 copy of p, or NULL */
    int64_t numel;
    float weight_decay;
    float lr;                      /* used when bias_correction1 != 0 (per-group learning rate) */
    float bias_correction1;        /* 1 - beta1^step of THIS tensor; 0 = use the launch-wide lr / bias corrections */
    float bias_correction2_sqrt;   /* sqrt(1 - beta2^step) of this tensor */
} otter_adamw_tensor;              /* 64 bytes */

int otter_adamw_chunk(void);
int otter_grad_sumsq(const otter_adamw_tensor* tensors, const int32_t* blk_tensor, const int32_t* blk_chunk, int64_t nblocks,
                     float* partials, void* stream);
int otter_clip_coef(const float* partials, int64_t n, float max_norm, float* out2, void* stream);
int otter_adamw_step(const otter_adamw_tensor* tensors, const int32_t* blk_tensor, const int32_t* blk_chunk, int64_t nblocks, float lr,
                     float beta1, float beta2, float eps, float bias_correction1, float bias_correction2, const float* grad_scale,
                     void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Profiling hook used by bench.py for the `roofline` object: when enabled, every launch of the bf16 GEMM whose
 * (M,N,K) equals the armed shape is bracketed by hipEvents on the launch stream; otter_prof_collect waits for
 * them and returns count and total milliseconds.
 * ------------------------------------------------------------------------------------------------------- */
int otter_prof_arm_gemm(int64_t M, int64_t N, int64_t K, int max_events);
/* Diagnostics: with otter_gemm_set_debug bit 64 set, the one-wave-per-SIMD bf16 kernels (variants 18-20) record shader-clock
 * timestamps at their tile-phase boundaries for two blocks; this copies the first n of the 512 uint64 slots
 * ([block 2][wave 4][tile 8][mark 8]: 0 tile start, 1 prologue done, 2 K loop done, 3 tail done, 4 tile end; the large-grid kernel also
 * stamps the 100 MHz wall clock at tile start / end in marks 5 / 6: the shader clock of that very launch, and the launch's shape and operand
 * layout in mark 7: M << 42 | N << 21 | K, bits 63 / 62 = A / B K-major) to the host. */
int otter_gemm_read_timeline(unsigned long long* out, int n);
int otter_prof_disarm(void);
int otter_prof_collect(int* count, double* total_ms);
/* same, with the launches that had a K-major operand (otter_gemm) counted separately as well (they are included in count / total_ms) */
int otter_prof_collect_split(int* count, double* total_ms, int* count_kmajor, double* kmajor_ms);
/* Diagnostics (bench.py OTTER_BENCH_OCCUPY_CUS): n workgroups that each pin one CU's whole LDS and sleep until *flag
 * (device memory) becomes non-zero or max_ticks of the 100 MHz wall clock pass -- stands in for a communication kernel's hold on CUs. */
int otter_debug_occupy_cus(int n_workgroups, int* flag, unsigned long long max_ticks, void* stream);

/* Machine calibration for bench.py's `roofline` object (round 5; nothing in the reference to replace -- SURVEY.md 8d asks the builder to
 * "confirm with a microbenchmark and report measured peaks"): n_workgroups x 4 waves issue `iters` x 64 back-to-back
 * v_mfma_f32_16x16x32_bf16 (the product GEMM's instruction; 1 048 576 FLOP per wave and iteration) on the caller's operand bits
 * (`operands`: 1 MiB, read once).  out: uint64[2 * n_workgroups (+ slack: allocate 2 * n_workgroups + 256 * n_workgroups)]:
 * [2b] = shader-clock cycles (s_memtime), [2b + 1] = 100 MHz wall-clock ticks (s_memrealtime) of workgroup b's loop. */
int otter_probe_mfma(const void* operands, void* out, int iters, int n_workgroups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OTTER_HIP_H */
