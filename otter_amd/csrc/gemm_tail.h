// gemm_tail.h -- the device code every GEMM kernel shares: typed 4- / 8-wide loads and stores, the epilogues (epilogue4 / epilogue8 /
// epilogue_stripe), accumulators parked in LDS, the fused full-tile tails (tail_* / xtail_*), per-block partials and the tile order.
#pragma once
#include "gemm_args.h"
#include <type_traits>

// Measuring instruments of the fused tails, compile-time, tools only (-DOTTER_DIAG=mask; `python -m otter_amd.build --diag N`, which rebuilds
// every GEMM file): 4 = the tail without its global loads / stores, 128 = plain
// (cacheable, write-back) stores instead of non-temporal ones.  Compile-time on purpose: a run-time flag inside the K-loop lambdas cost the product
// kernels 3-4x.
#ifndef OTTER_DIAG
#define OTTER_DIAG 0
#endif
namespace {

__device__ __forceinline__ void load4(const void* p, int64_t idx, int dt, float (&v)[4]) {
    if (dt == OTTER_BF16) {
        const uint2 r = *reinterpret_cast<const uint2*>((const bf16_t*)p + idx);
        v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
        v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
    } else {
        const float4 r = *reinterpret_cast<const float4*>((const float*)p + idx);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    }
}
// Outputs are written once and not re-read by this kernel: non-temporal stores keep them from displacing the operand
// panels in the XCD's L2 (and from being written back in the middle of the next tile's K loop).
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
// diag bit 128: plain (cacheable, write-back) stores in the fused tail instead of non-temporal ones (timing experiment)
template <typename V>
__device__ __forceinline__ void out_store(V v, V* p) {
    if constexpr ((OTTER_DIAG & 128) != 0) *p = v;
    else __builtin_nontemporal_store(v, p);
}
__device__ __forceinline__ void store4(void* p, int64_t idx, int dt, const float (&v)[4]) {
    if (dt == OTTER_BF16) {
        u32x2_t r;
        r.x = pack2bf(v[0], v[1]);
        r.y = pack2bf(v[2], v[3]);
        out_store(r, reinterpret_cast<u32x2_t*>((bf16_t*)p + idx));
    } else {
        f32x4_t r = {v[0], v[1], v[2], v[3]};
        out_store(r, reinterpret_cast<f32x4_t*>((float*)p + idx));
    }
}

// GELU of NE accumulator values / the GELU-backward of the gate-backward tail (o = s v GELU'(a), returns sum v GELU(a)).  bf16 results take
// the packed polynomial Phi of common.h (gelu_cdf_fast2: |error| <= 1.5e-5, far inside bf16 rounding), fp32 results the A&S 7.1.26 form
// (1.5e-7): every kernel and every tail flavour of this file goes through these two, so one launch shape gives one result.
template <int NE>
__device__ __forceinline__ void gelu_apply(bool fast, const float (&v)[NE], float (&o)[NE]) {
    if (fast) {
        gelu_fast<NE>(v, o);
    } else {
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            float cdf, pdf;
            gelu_cdf_pdf(v[i], cdf, pdf);
            o[i] = v[i] * cdf;
        }
    }
}
// GELU forward whose second output is the DERIVATIVE (otter_epilogue_args::aux_is_gelu_input == 3 on an OTTER_EPI_GELU launch)
template <int NE>
__device__ __forceinline__ void gelu_apply_stash(bool fast, const float (&v)[NE], float (&o)[NE], float (&gp)[NE]) {
    if (fast) {
        gelu_and_grad_fast<NE>(v, o, gp);
    } else {
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            float cdf, pdf;
            gelu_cdf_pdf(v[i], cdf, pdf);
            o[i] = v[i] * cdf;
            gp[i] = cdf + v[i] * pdf;
        }
    }
}
template <int NE>
__device__ __forceinline__ float gelu_bwd_apply(bool fast, float s, const float (&v)[NE], const float (&a)[NE], float (&o)[NE]) {
    float part = 0.f;
    if (fast) {
        part = gelu_bwd_fast<NE>(s, v, a, o);
    } else {
#pragma unroll
        for (int i = 0; i < NE; ++i) {   // gelu and gelu' share the erf: one transcendental chain instead of two
            float cdf, pdf;
            gelu_cdf_pdf(a[i], cdf, pdf);
            part += v[i] * (a[i] * cdf);
            o[i] = s * v[i] * (cdf + a[i] * pdf);
        }
    }
    return part;
}

// Plain-store launches with an fp32 C (weight gradients) can also hand back sum(C^2) per tile -- the clip_grad_norm_ reduction of that tensor,
// taken while the values are in registers instead of by a second 4-byte-per-element sweep over it (otter_epilogue_args::partial, round 6b).
template <int NE>
__device__ __forceinline__ float sumsq_of(const float (&o)[NE]) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NE; ++i) t = fmaf(o[i], o[i], t);
    return t;
}

// epilogue on 4 consecutive output columns of row m; returns this thread's contribution to the gate partial (plain store, fp32 C: to sum(C^2))
template <int EPI>
__device__ __forceinline__ float epilogue4(const GemmArgs& g, float s, int64_t m, int64_t n, float (&v)[4]) {
    float part = 0.f;
    float o[4];
    switch (EPI) {
        case OTTER_EPI_STORE: {
            if (g.accumulate) {
                float c[4];
                load4(g.C, m * g.ldc + n, g.cdt, c);
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = c[i] + s * v[i];
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = s * v[i];
            }
            store4(g.C, m * g.ldc + n, g.cdt, o);
            if (g.cdt == OTTER_F32) part = sumsq_of<4>(o);   // (written out only when the launch asked for partials: block_partial)
            break;
        }
        case OTTER_EPI_GELU: {
            if (g.C2 && g.aux_gelu == 3) {   // derivative stash: C2 = GELU'(acc)
                float gp[4];
                gelu_apply_stash<4>(g.cdt == OTTER_BF16, v, o, gp);
                store4(g.C2, m * g.ldc2 + n, g.cdt, gp);
            } else {
                if (g.C2) store4(g.C2, m * g.ldc2 + n, g.cdt, v);
                gelu_apply<4>(g.cdt == OTTER_BF16, v, o);   // bf16 results: the packed polynomial, as in the full-tile tails (tail_apply)
            }
            store4(g.C, m * g.ldc + n, g.cdt, o);
            break;
        }
        case OTTER_EPI_SCALE_RES: {
            float r[4];
            load4(g.R, m * g.ldr + n, g.rdt, r);
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = v[i] * s + r[i];
            store4(g.C, m * g.ldc + n, g.cdt, o);
            break;
        }
        default: {  // OTTER_EPI_GATE_BWD
            float a[4];
            load4(g.aux, m * g.ldaux + n, g.auxdt, a);
            if (g.aux_gelu == 3) {   // aux IS the stashed derivative f'(a): no activation arithmetic, no gate partial
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = s * v[i] * a[i];
            } else if (g.aux_gelu == 2) {   // squared ReLU (Persimmon MLP): f(a) = relu(a)^2, f'(a) = 2 relu(a)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float r = fmaxf(a[i], 0.f);
                    part += v[i] * (r * r);
                    o[i] = s * v[i] * (2.0f * r);
                }
            } else if (g.aux_gelu) {   // tested outside the element loop (a per-element scalar branch serialises the chains)
                part += gelu_bwd_apply<4>(g.cdt == OTTER_BF16, s, v, a, o);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    part += v[i] * a[i];
                    o[i] = s * v[i];
                }
            }
            store4(g.C, m * g.ldc + n, g.cdt, o);
            break;
        }
    }
    return part;
}

// ---- 8 consecutive output columns per lane: 16-byte bf16 (2 x 16-byte f32) accesses, half as many store instructions ----
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
__device__ __forceinline__ void load8w(const void* p, int64_t idx, int dt, float (&v)[8]) {
    if (dt == OTTER_BF16) {
        const uint4 r = *reinterpret_cast<const uint4*>((const bf16_t*)p + idx);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
    } else {
        const float4 a = *reinterpret_cast<const float4*>((const float*)p + idx), b = *reinterpret_cast<const float4*>((const float*)p + idx + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
}
__device__ __forceinline__ void store8w(void* p, int64_t idx, int dt, const float (&v)[8]) {
    if (dt == OTTER_BF16) {
        u32x4_t r;
        r.x = pack2bf(v[0], v[1]); r.y = pack2bf(v[2], v[3]); r.z = pack2bf(v[4], v[5]); r.w = pack2bf(v[6], v[7]);
        out_store(r, reinterpret_cast<u32x4_t*>((bf16_t*)p + idx));
    } else {
        f32x4_t a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
        out_store(a, reinterpret_cast<f32x4_t*>((float*)p + idx));
        out_store(b, reinterpret_cast<f32x4_t*>((float*)p + idx + 4));
    }
}
template <int EPI>
__device__ __forceinline__ float epilogue8(const GemmArgs& g, float s, int64_t m, int64_t n, float (&v)[8]) {
    float part = 0.f;
    float o[8];
    switch (EPI) {
        case OTTER_EPI_STORE: {
            if (g.accumulate) {
                float c[8];
                load8w(g.C, m * g.ldc + n, g.cdt, c);
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = c[i] + s * v[i];
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = s * v[i];
            }
            if (g.cdt == OTTER_F32) part = sumsq_of<8>(o);
            break;
        }
        case OTTER_EPI_GELU: {
            if (g.C2 && g.aux_gelu == 3) {
                float gp[8];
                gelu_apply_stash<8>(g.cdt == OTTER_BF16, v, o, gp);
                store8w(g.C2, m * g.ldc2 + n, g.cdt, gp);
            } else {
                if (g.C2) store8w(g.C2, m * g.ldc2 + n, g.cdt, v);
                gelu_apply<8>(g.cdt == OTTER_BF16, v, o);   // bf16 results: the packed polynomial, as in the full-tile tails (tail_apply)
            }
            break;
        }
        case OTTER_EPI_SCALE_RES: {
            float r[8];
            load8w(g.R, m * g.ldr + n, g.rdt, r);
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = v[i] * s + r[i];
            break;
        }
        default: {  // OTTER_EPI_GATE_BWD
            float a[8];
            load8w(g.aux, m * g.ldaux + n, g.auxdt, a);
            if (g.aux_gelu == 3) {
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = s * v[i] * a[i];
            } else if (g.aux_gelu == 2) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float r = fmaxf(a[i], 0.f);
                    part += v[i] * (r * r);
                    o[i] = s * v[i] * (2.0f * r);
                }
            } else if (g.aux_gelu) {
                part += gelu_bwd_apply<8>(g.cdt == OTTER_BF16, s, v, a, o);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    part += v[i] * a[i];
                    o[i] = s * v[i];
                }
            }
            break;
        }
    }
    store8w(g.C, m * g.ldc + n, g.cdt, o);
    return part;
}

// Epilogue: a wave parks one 32-row stripe of its sub-tile (two 32x32 accumulator blocks side by side = 32 rows x 64
// columns) in wave-private LDS as fp32, then reads it back row-major: lane l handles row (l>>4) + 4*it, columns
// 4*(l&15)..+3, so 16 lanes cover one full 128-B (bf16) / 256-B (f32) run of an output row and every global access of
// the fused tail (C, C2, residual, aux) is a whole cache line.  The epilogue kind is a template parameter (one copy of
// the tail per kernel) and the row loop is a run-time loop, so the (mi) loop that indexes the accumulator registers
// statically stays small enough to be fully unrolled -- a single runtime-switched body made the unroller give up and
// demoted the accumulators to scratch; an out-of-line body took its arguments through flat (generic) pointers.
constexpr int EPI_LD = 68;  // floats per parked row (64 + 4 pad; rows stay 16-B aligned)

template <int EPI>
__device__ __forceinline__ float epilogue_stripe(const GemmArgs& g, float s, const float* __restrict__ blk, int64_t m_base,
                                                 int64_t n_base, int lane) {
    float part = 0.f;
    if (g.wide && !((OTTER_DIAG & 4) || (g.dbg & 16))) {
        // lane l: row (l>>3) + 8*it, columns 8*(l&7)..+7 -- 8 lanes cover the 128-B (bf16) run of an output row with one
        // 16-byte access each: half the store / load instructions and loop trips of the 4-wide form below
#pragma unroll 1
        for (int it = 0; it < 4; ++it) {
            const int r = (lane >> 3) + 8 * it;
            const int c = (lane & 7) * 8;
            const int64_t m = m_base + r, n = n_base + c;
            if (m < g.M && n < g.N) {
                const float4 t0 = *reinterpret_cast<const float4*>(blk + r * EPI_LD + c);
                const float4 t1 = *reinterpret_cast<const float4*>(blk + r * EPI_LD + c + 4);
                float v[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
                part += epilogue8<EPI>(g, s, m, n, v);
            }
        }
        return part;
    }
#pragma unroll 1
    for (int it = 0; it < 8; ++it) {
        const int r = (lane >> 4) + 4 * it;
        const int c = (lane & 15) * 4;
        const int64_t m = m_base + r, n = n_base + c;
        if (m < g.M && n < g.N) {
            const float4 t = *reinterpret_cast<const float4*>(blk + r * EPI_LD + c);
            float v[4] = {t.x, t.y, t.z, t.w};
            if ((OTTER_DIAG & 4) || (g.dbg & 16)) {  // diagnostics: everything but the global traffic of the tail
                part += v[0] + v[1] + v[2] + v[3];
            } else {
                part += epilogue4<EPI>(g, s, m, n, v);
            }
        }
    }
    return part;
}

// park one accumulator block at column offset col0 of the stripe: lane holds row m = lane&31, columns
// col0 + 8*grp + 4*(lane>>5) + 0..3
__device__ __forceinline__ void park_block(float* __restrict__ blk, const f32x16_t& a, int lane, int col0) {
    float* row = blk + (lane & 31) * EPI_LD + col0 + 4 * (lane >> 5);
#pragma unroll
    for (int grp = 0; grp < 4; ++grp)
        *reinterpret_cast<float4*>(row + 8 * grp) = make_float4(a[4 * grp + 0], a[4 * grp + 1], a[4 * grp + 2], a[4 * grp + 3]);
}

// deterministic block reduction of the per-thread partial into partial[blockIdx.x]
template <int NWAVES, int EPI>
__device__ __forceinline__ void block_partial(const GemmArgs& g, float part, float* red /* LDS, >= NWAVES floats */, int slot) {
    if ((EPI != OTTER_EPI_GATE_BWD && EPI != OTTER_EPI_STORE) || g.partial == nullptr) return;
    part = wave_sum(part);
    __syncthreads();  // everyone is done with the LDS that `red` aliases
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) t += red[w];
        g.partial[slot] = t;
    }
}

// ---- fast tail of the one-wave-per-SIMD kernels (variants 25, 26, 30; written for the retired 17-20), FULL tiles only ----
// With 8 waves per CU the stripe loop above hides its own latencies (another wave always has something to issue); with one
// wave per SIMD every ds_write -> ds_read -> global access chain is exposed, and the run-time switches of the generic tail
// (output dtype, bounds, wide/narrow) sit inside its loops: the K sweep of tools/gemm_ksweep.py priced the fixed part of a
// variant-18 launch at 84 us against 46 us for the 8-wave kernel and 36 us for hipBLASLt.  Here the tile is known to be
// in bounds, the output dtype is a template parameter, the per-stripe loop is fully unrolled (all LDS reads of a stripe are
// issued before the first one is consumed) and consecutive stripes alternate between TWO parking buffers, so the next
// stripe is parked while the current one's global accesses are in flight.  Same arithmetic, same access shapes (whole
// cache lines per row run) as epilogue_stripe.
// The fused tail in two phases, so that the global INPUT of a stripe (residual R, gate-backward aux, the C being accumulated
// into) can be requested one stripe ahead of the arithmetic that consumes it: with one wave per SIMD an un-prefetched
// load -> use chain exposes a full memory latency eight times per tile (gate-backward: 626 us per launch in situ against
// 553 for the 8-wave kernel, whose two waves per SIMD cover each other).  NE = elements per lane per access (8 / 4).
template <int EPI>
__device__ __forceinline__ bool tail_input(const GemmArgs& g, const void*& p, int64_t& ld, int& dt) {
    if constexpr (EPI == OTTER_EPI_STORE) { p = g.C; ld = g.ldc; dt = g.cdt; return g.accumulate != 0; }
    else if constexpr (EPI == OTTER_EPI_SCALE_RES) { p = g.R; ld = g.ldr; dt = g.rdt; return true; }
    else if constexpr (EPI == OTTER_EPI_GATE_BWD) { p = g.aux; ld = g.ldaux; dt = g.auxdt; return true; }
    else { p = nullptr; ld = 0; dt = OTTER_F32; return false; }
}
// raw (unconverted) input of NE elements: the conversion to f32 stays with the consumer so that no use sits next to the load
// INBF16: the input dtype as a TEMPLATE parameter -- as a run-time test inside each load it made the compiler emit a branch and
// an `s_waitcnt vmcnt(0)` between consecutive loads (the "prefetch" ran one memory latency per access)
template <int NE, bool INBF16>
__device__ __forceinline__ void load_raw(const void* p, int64_t idx, uint4 (&raw)[2]) {
    if constexpr (INBF16) {
        if constexpr (NE == 8) raw[0] = *reinterpret_cast<const uint4*>((const bf16_t*)p + idx);
        else { const uint2 t = *reinterpret_cast<const uint2*>((const bf16_t*)p + idx); raw[0].x = t.x; raw[0].y = t.y; }
    } else {
        raw[0] = *reinterpret_cast<const uint4*>((const float*)p + idx);
        if constexpr (NE == 8) raw[1] = *reinterpret_cast<const uint4*>((const float*)p + idx + 4);
    }
}
template <int NE, bool INBF16>
__device__ __forceinline__ void cvt_raw(const uint4 (&raw)[2], float (&a)[NE]) {
    if constexpr (INBF16) {
        const uint32_t w[4] = {raw[0].x, raw[0].y, raw[0].z, raw[0].w};
#pragma unroll
        for (int i = 0; i < NE / 2; ++i) { a[2 * i] = __uint_as_float(w[i] << 16); a[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
    } else {
        a[0] = __uint_as_float(raw[0].x); a[1] = __uint_as_float(raw[0].y); a[2] = __uint_as_float(raw[0].z); a[3] = __uint_as_float(raw[0].w);
        if constexpr (NE == 8) {
            a[4] = __uint_as_float(raw[1].x); a[5] = __uint_as_float(raw[1].y); a[6] = __uint_as_float(raw[1].z); a[7] = __uint_as_float(raw[1].w);
        }
    }
}
// arithmetic + stores of NE consecutive output columns given the accumulator values v and the (already loaded) input a:
// exactly epilogue4 / epilogue8 with their load taken out
template <int EPI, int NE>
__device__ __forceinline__ float tail_apply(const GemmArgs& g, float s, int64_t m, int64_t n, const float (&v)[NE], const float (&a)[NE], bool has_in) {
    float part = 0.f;
    float o[NE];
    if constexpr (EPI == OTTER_EPI_STORE) {
        if (has_in) {
#pragma unroll
            for (int i = 0; i < NE; ++i) o[i] = a[i] + s * v[i];
        } else {
#pragma unroll
            for (int i = 0; i < NE; ++i) o[i] = s * v[i];
        }
        if (g.cdt == OTTER_F32) part = sumsq_of<NE>(o);   // (g.cdt is a compile-time constant in the full-tile tails: bf16 stores carry nothing extra)
    } else if constexpr (EPI == OTTER_EPI_GELU) {
        if (g.C2 && g.aux_gelu == 3) {   // derivative stash (round 6c): C2 = GELU'(acc) instead of acc
            float gp[NE];
            gelu_apply_stash<NE>(g.cdt == OTTER_BF16, v, o, gp);
            if constexpr (NE == 8) store8w(g.C2, m * g.ldc2 + n, g.cdt, gp);
            else store4(g.C2, m * g.ldc2 + n, g.cdt, gp);
        } else {
            if (g.C2) {
                if constexpr (NE == 8) store8w(g.C2, m * g.ldc2 + n, g.cdt, v);
                else store4(g.C2, m * g.ldc2 + n, g.cdt, v);
            }
            gelu_apply<NE>(g.cdt == OTTER_BF16, v, o);   // (the dtype is a compile-time constant in the full-tile tails)
        }
    } else if constexpr (EPI == OTTER_EPI_SCALE_RES) {
#pragma unroll
        for (int i = 0; i < NE; ++i) o[i] = v[i] * s + a[i];
    } else {
        // the aux kind is tested ONCE, outside the element loop: inside it the compiler kept a scalar branch between
        // elements, which serialised eight independent rcp / exp / fma chains (gate-backward tail: 88 k cycles per tile)
        if (g.aux_gelu == 3) {   // aux is the stashed derivative (round 6c)
#pragma unroll
            for (int i = 0; i < NE; ++i) o[i] = s * v[i] * a[i];
        } else if (g.aux_gelu == 2) {   // squared ReLU: f'(a) = 2 relu(a)
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const float r = fmaxf(a[i], 0.f);
                part += v[i] * (r * r);
                o[i] = s * v[i] * (2.0f * r);
            }
        } else if (g.aux_gelu) {
            part += gelu_bwd_apply<NE>(g.cdt == OTTER_BF16, s, v, a, o);
        } else {
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                part += v[i] * a[i];
                o[i] = s * v[i];
            }
        }
    }
    if constexpr (NE == 8) store8w(g.C, m * g.ldc + n, g.cdt, o);
    else store4(g.C, m * g.ldc + n, g.cdt, o);
    return part;
}

template <bool CBF16>
struct TailShape {  // bf16 output: 4 accesses of 8 columns per lane and stripe; f32 output: 8 accesses of 4 columns
    static constexpr int NE = CBF16 ? 8 : 4, NIT = CBF16 ? 4 : 8;
    static __device__ __forceinline__ int row(int lane, int it) { return CBF16 ? (lane >> 3) + 8 * it : (lane >> 4) + 4 * it; }
    static __device__ __forceinline__ int col(int lane) { return CBF16 ? (lane & 7) * 8 : (lane & 15) * 4; }
};

template <int EPI, bool CBF16, bool INBF16>
__device__ __forceinline__ void tail_stripe_load(const void* p, int64_t ld, int64_t m_base, int64_t n_base, int lane,
                                                 uint4 (&raw)[TailShape<CBF16>::NIT][2]) {
    using T = TailShape<CBF16>;
#pragma unroll
    for (int it = 0; it < T::NIT; ++it) load_raw<T::NE, INBF16>(p, (m_base + T::row(lane, it)) * ld + n_base + T::col(lane), raw[it]);
}

template <int EPI, bool CBF16, bool INBF16>
__device__ __forceinline__ float tail_stripe_full(GemmArgs g, float s, const float* __restrict__ blk, int64_t m_base, int64_t n_base, int lane,
                                                  const uint4 (&raw)[TailShape<CBF16>::NIT][2], bool has_in) {
    using T = TailShape<CBF16>;
    float part = 0.f;
    g.cdt = CBF16 ? OTTER_BF16 : OTTER_F32;  // compile-time constant from here on: the dtype switches of the stores fold away
    float v[T::NIT][T::NE];
#pragma unroll
    for (int it = 0; it < T::NIT; ++it) {
        const float* src = blk + T::row(lane, it) * EPI_LD + T::col(lane);
        const float4 t0 = *reinterpret_cast<const float4*>(src);
        v[it][0] = t0.x; v[it][1] = t0.y; v[it][2] = t0.z; v[it][3] = t0.w;
        if constexpr (CBF16) {
            const float4 t1 = *reinterpret_cast<const float4*>(src + 4);
            v[it][4] = t1.x; v[it][5] = t1.y; v[it][6] = t1.z; v[it][7] = t1.w;
        }
    }
#pragma unroll
    for (int it = 0; it < T::NIT; ++it) {
        float a[T::NE];
        if (has_in) cvt_raw<T::NE, INBF16>(raw[it], a);
        else {
#pragma unroll
            for (int i = 0; i < T::NE; ++i) a[i] = 0.f;
        }
        part += tail_apply<EPI, T::NE>(g, s, m_base + T::row(lane, it), n_base + T::col(lane), v[it], a, has_in);
    }
    return part;
}

// whole 128x128 wave tile = 8 stripes of 32 rows x 64 columns, FOUR parking buffers per wave: half of the wave tile is parked
// in one go (32 ds_write_b128 with static accumulator indices -- a dynamically indexed accumulator array is demoted to
// scratch, and so is one selected by a switch inside a loop: tried, 512 B of scratch per lane with accesses in the K loop),
// then a RUN-TIME loop walks the four parked stripes with ONE copy of the stripe arithmetic (unrolling it eight times made
// the GELU / gate-backward instantiations 22k-39k lines with 956 scratch accesses: 1150 us per launch in situ).  The
// buffers are wave-private and a wave's LDS operations execute in order, so no barrier is needed between the phases.
constexpr int TAIL_STRIPES = 4;
constexpr int TAIL_LDS_BYTES = 4 * TAIL_STRIPES * 32 * EPI_LD * 4;  // 4 waves: 139264 B

// stripe st (0..7) of a 128x128 wave tile = rows 32*(st>>1).., columns 64*(st&1)..; the two accumulator layouts park it differently
__device__ __forceinline__ void park_stripe(float* __restrict__ blk, const f32x16_t (&acc)[4][4], int st, int lane) {
    park_block(blk, acc[st >> 1][2 * (st & 1)], lane, 0);
    park_block(blk, acc[st >> 1][2 * (st & 1) + 1], lane, 32);
}
// 16x16 blocks (v_mfma_f32_16x16x32 with the operands swapped): lane holds row m = lane&15 of the block, columns 4*(lane>>4) + 0..3
__device__ __forceinline__ void park_stripe(float* __restrict__ blk, const f32x4_t (&acc)[8][8], int st, int lane) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const f32x4_t& v = acc[2 * (st >> 1) + a][4 * (st & 1) + b];
            *reinterpret_cast<float4*>(blk + (16 * a + (lane & 15)) * EPI_LD + 16 * b + 4 * (lane >> 4)) = make_float4(v[0], v[1], v[2], v[3]);
        }
}

// Accumulators held in EXPLICIT AGPRs (K-major instantiations of variant 26: block (mi, ni) = a[4 (8 mi + ni) .. + 3], written by asm MFMAs):
// parked straight out of the AGPR half with ds_write_b128 (DS instructions take AGPR data on gfx90a+), same LDS image as the overload
// above -- the values never become C++ values, so hipcc has nothing to copy, split or spill.  The caller has waited out the MFMA -> read
// hazard.  LDS operations of a wave complete in order: the tail's compiler-visible reads of `blk` that follow see these writes.
struct AgprAcc {};
#define PARK_AGPR_BLOCK(A_, B_, MI_, NI_)                                                                                             \
    asm volatile("ds_write_b128 %0, a[%c1:%c2] offset:%c3" : : "v"(addr), "n"(((MI_) * 8 + (NI_)) * 4), "n"(((MI_) * 8 + (NI_)) * 4 + 3), \
                 "n"(((A_) * 16 * EPI_LD + (B_) * 16) * 4) : "memory")
#define PARK_AGPR_STRIPE(ST_)                                                                                                          \
    do {                                                                                                                              \
        PARK_AGPR_BLOCK(0, 0, 2 * ((ST_) >> 1), 4 * ((ST_) & 1)); PARK_AGPR_BLOCK(0, 1, 2 * ((ST_) >> 1), 4 * ((ST_) & 1) + 1);         \
        PARK_AGPR_BLOCK(0, 2, 2 * ((ST_) >> 1), 4 * ((ST_) & 1) + 2); PARK_AGPR_BLOCK(0, 3, 2 * ((ST_) >> 1), 4 * ((ST_) & 1) + 3);     \
        PARK_AGPR_BLOCK(1, 0, 2 * ((ST_) >> 1) + 1, 4 * ((ST_) & 1)); PARK_AGPR_BLOCK(1, 1, 2 * ((ST_) >> 1) + 1, 4 * ((ST_) & 1) + 1); \
        PARK_AGPR_BLOCK(1, 2, 2 * ((ST_) >> 1) + 1, 4 * ((ST_) & 1) + 2); PARK_AGPR_BLOCK(1, 3, 2 * ((ST_) >> 1) + 1, 4 * ((ST_) & 1) + 3); \
    } while (0)
__device__ __forceinline__ void park_stripe(float* __restrict__ blk, const AgprAcc&, int st, int lane) {
    const unsigned addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)(blk + (lane & 15) * EPI_LD + 4 * (lane >> 4));
    switch (st) {   // st is a constant after unrolling: one case survives
        case 0: PARK_AGPR_STRIPE(0); break;
        case 1: PARK_AGPR_STRIPE(1); break;
        case 2: PARK_AGPR_STRIPE(2); break;
        case 3: PARK_AGPR_STRIPE(3); break;
        case 4: PARK_AGPR_STRIPE(4); break;
        case 5: PARK_AGPR_STRIPE(5); break;
        case 6: PARK_AGPR_STRIPE(6); break;
        default: PARK_AGPR_STRIPE(7); break;
    }
}
#undef PARK_AGPR_STRIPE
#undef PARK_AGPR_BLOCK

// HASIN (round 5): whether the tail reads a global input (accumulate / residual / aux) is a TEMPLATE parameter.  As a run-time flag the
// compiler had to keep the waits of the input prefetch on every path: `s_waitcnt vmcnt(7)` in front of each store of a tail that had
// issued no load at all -- and on gfx9 vmcnt counts stores, so a plain-store tail never had more than 7 stores per wave in flight
// (7 KB per ~1.5 us of write latency = the "9.3 bytes per cycle and CU" that bounded the bf16 store tail).
template <int EPI, bool CBF16, bool INBF16, int NS, bool HASIN, typename ACC>
__device__ __forceinline__ float tail_wave_full_t(const GemmArgs& g, float s, const ACC& acc, float* __restrict__ blk4 /* NS stripes */,
                                                  int64_t m_wave, int64_t n_wave, int lane, const void* ip, int64_t ild) {
    using T = TailShape<CBF16>;
    constexpr bool has_in = HASIN;
    static_assert(NS % 2 == 0, "the stripe loop handles two stripes per iteration (ping-pong input buffers)");
    float part = 0.f;
    // Two input buffers used alternately, NO register copies between them (round 5): the former `cur = nxt` hand-over at the end of every
    // stripe made the compiler wait for the just-issued loads -- s_waitcnt vmcnt(0) / vmcnt(1) once per stripe, i.e. a full drain of every
    // outstanding load AND store (vmcnt counts stores on gfx9): the residual / gate-backward tails paid one store round trip per stripe
    // (34-60 k cycles per tile).  Now a buffer is requested TWO stripes before it is consumed -- also on the loop's
    // entry edge, which is what the compiler's wait-count merge at the loop header takes -- so the first wait of an iteration leaves 15
    // younger operations in flight instead of draining the previous stripe's stores.
    uint4 bufA[T::NIT][2], bufB[T::NIT][2];
    if (has_in) {   // stripes 0 and 1 are requested up front: a buffer is always TWO stripes ahead of its use (see the wait counts above)
        tail_stripe_load<EPI, CBF16, INBF16>(ip, ild, m_wave, n_wave, lane, bufA);
        tail_stripe_load<EPI, CBF16, INBF16>(ip, ild, m_wave, n_wave + 64, lane, bufB);
    }
#pragma unroll
    for (int half = 0; half < 8 / NS; ++half) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const int st = half * NS + q;
            park_stripe(blk4 + q * (32 * EPI_LD), acc, st, lane);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int q = 0; q < NS; q += 2) {
            const int st = half * NS + q;
            part += tail_stripe_full<EPI, CBF16, INBF16>(g, s, blk4 + q * (32 * EPI_LD), m_wave + (st >> 1) * 32, n_wave + (st & 1) * 64, lane, bufA,
                                                         has_in);
            if (has_in && st + 2 < 8)
                tail_stripe_load<EPI, CBF16, INBF16>(ip, ild, m_wave + ((st + 2) >> 1) * 32, n_wave + ((st + 2) & 1) * 64, lane, bufA);
            part += tail_stripe_full<EPI, CBF16, INBF16>(g, s, blk4 + (q + 1) * (32 * EPI_LD), m_wave + ((st + 1) >> 1) * 32, n_wave + ((st + 1) & 1) * 64,
                                                         lane, bufB, has_in);
            if (has_in && st + 3 < 8)
                tail_stripe_load<EPI, CBF16, INBF16>(ip, ild, m_wave + ((st + 3) >> 1) * 32, n_wave + ((st + 3) & 1) * 64, lane, bufB);
        }
        __builtin_amdgcn_wave_barrier();
    }
    return part;
}

template <int EPI, bool CBF16, int NS = TAIL_STRIPES, typename ACC>
__device__ __forceinline__ float tail_wave_full(const GemmArgs& g, float s, const ACC& acc, float* __restrict__ blk4, int64_t m_wave,
                                                int64_t n_wave, int lane) {
    const void* ip; int64_t ild; int idt;
    const bool has_in = tail_input<EPI>(g, ip, ild, idt);
    if constexpr (EPI == OTTER_EPI_GELU) {       // no global input at all: one instantiation
        return tail_wave_full_t<EPI, CBF16, true, NS, false>(g, s, acc, blk4, m_wave, n_wave, lane, ip, ild);
    } else if constexpr (EPI == OTTER_EPI_STORE) {   // input only when accumulating into C
        if (!has_in) return tail_wave_full_t<EPI, CBF16, true, NS, false>(g, s, acc, blk4, m_wave, n_wave, lane, ip, ild);
        if (idt == OTTER_BF16) return tail_wave_full_t<EPI, CBF16, true, NS, true>(g, s, acc, blk4, m_wave, n_wave, lane, ip, ild);
        return tail_wave_full_t<EPI, CBF16, false, NS, true>(g, s, acc, blk4, m_wave, n_wave, lane, ip, ild);
    } else {                                       // residual / aux kinds always read their input
        if (idt == OTTER_BF16) return tail_wave_full_t<EPI, CBF16, true, NS, true>(g, s, acc, blk4, m_wave, n_wave, lane, ip, ild);
        return tail_wave_full_t<EPI, CBF16, false, NS, true>(g, s, acc, blk4, m_wave, n_wave, lane, ip, ild);
    }
}

// ---- tail of the cross-tile form (round 6): ONE 8 KB parking stripe per wave, above the ring ----
// The ring (2 x 64 KB) is busy during this tail -- the next tile's first two K-tiles are landing in it -- so a wave parks in the 32 KB of LDS
// above it: one stripe of 32 rows x 64 fp32 = 8192 B per wave, unpadded (256-byte rows = one full sweep of the 64 banks), 16-byte chunk c
// of row r stored at chunk c ^ (r & 15): the eight lanes of a ds_write_b128 group (8 rows, one chunk) and the sixteen of a ds_read_b128 group hit
// distinct bank quads.  Single-buffered: stripe s + 1 is parked right behind the read-back of stripe s (a wave's LDS operations execute in order,
// so the reads see the old stripe) and lands under the arithmetic and the global accesses of stripe s.
constexpr int XPARK_BYTES = 32 * 256;   // per wave
__device__ __forceinline__ void xpark_stripe(unsigned base /* LDS byte address of the wave's stripe */, int st, int lane) {
    const unsigned r = (unsigned)lane & 15u, gq = (unsigned)lane >> 4;
    const unsigned row = base + r * 256u;
    const unsigned a0 = row + (((0u + gq) ^ r) << 4), a1 = row + (((4u + gq) ^ r) << 4), a2 = row + (((8u + gq) ^ r) << 4), a3 = row + (((12u + gq) ^ r) << 4);
#define XPARK_BLOCK(ADDR_, A_, MI_, NI_)                                                                                               \
    asm volatile("ds_write_b128 %0, a[%c1:%c2] offset:%c3" : : "v"(ADDR_), "n"(((MI_) * 8 + (NI_)) * 4), "n"(((MI_) * 8 + (NI_)) * 4 + 3), \
                 "n"((A_) * 4096) : "memory")
#define XPARK_STRIPE(ST_)                                                                                                              \
    do {                                                                                                                              \
        XPARK_BLOCK(a0, 0, 2 * ((ST_) >> 1), 4 * ((ST_) & 1)); XPARK_BLOCK(a1, 0, 2 * ((ST_) >> 1), 4 * ((ST_) & 1) + 1);                \
        XPARK_BLOCK(a2, 0, 2 * ((ST_) >> 1), 4 * ((ST_) & 1) + 2); XPARK_BLOCK(a3, 0, 2 * ((ST_) >> 1), 4 * ((ST_) & 1) + 3);            \
        XPARK_BLOCK(a0, 1, 2 * ((ST_) >> 1) + 1, 4 * ((ST_) & 1)); XPARK_BLOCK(a1, 1, 2 * ((ST_) >> 1) + 1, 4 * ((ST_) & 1) + 1);        \
        XPARK_BLOCK(a2, 1, 2 * ((ST_) >> 1) + 1, 4 * ((ST_) & 1) + 2); XPARK_BLOCK(a3, 1, 2 * ((ST_) >> 1) + 1, 4 * ((ST_) & 1) + 3);    \
    } while (0)
    switch (st) {   // run-time stripe index (a scalar branch tree): the AGPR block numbers are immediates
        case 0: XPARK_STRIPE(0); break;
        case 1: XPARK_STRIPE(1); break;
        case 2: XPARK_STRIPE(2); break;
        case 3: XPARK_STRIPE(3); break;
        case 4: XPARK_STRIPE(4); break;
        case 5: XPARK_STRIPE(5); break;
        case 6: XPARK_STRIPE(6); break;
        default: XPARK_STRIPE(7); break;
    }
#undef XPARK_STRIPE
#undef XPARK_BLOCK
}
// read the parked stripe back row-major (the lane -> (row, columns) map of TailShape), through the chunk swizzle
template <bool CBF16>
__device__ __forceinline__ void xpark_read(const char* __restrict__ stripe, int lane, float (&v)[TailShape<CBF16>::NIT][TailShape<CBF16>::NE]) {
    using T = TailShape<CBF16>;
#pragma unroll
    for (int it = 0; it < T::NIT; ++it) {
        const int row = T::row(lane, it), c0 = T::col(lane) >> 2;
        const char* src = stripe + row * 256 + ((c0 ^ (row & 15)) << 4);
        const float4 t0 = *reinterpret_cast<const float4*>(src);
        v[it][0] = t0.x; v[it][1] = t0.y; v[it][2] = t0.z; v[it][3] = t0.w;
        if constexpr (CBF16) {   // c0 is even: chunk c0 + 1 lies at the address with bit 4 flipped
            const float4 t1 = *reinterpret_cast<const float4*>(stripe + row * 256 + (((c0 ^ (row & 15)) << 4) ^ 16));
            v[it][4] = t1.x; v[it][5] = t1.y; v[it][6] = t1.z; v[it][7] = t1.w;
        }
    }
}
template <int EPI, bool CBF16, bool INBF16>
__device__ __forceinline__ float xtail_stripe_apply(GemmArgs g, float s, const float (&v)[TailShape<CBF16>::NIT][TailShape<CBF16>::NE], int64_t m_base,
                                                    int64_t n_base, int lane, const uint4 (&raw)[TailShape<CBF16>::NIT][2], bool has_in) {
    using T = TailShape<CBF16>;
    float part = 0.f;
    g.cdt = CBF16 ? OTTER_BF16 : OTTER_F32;
#pragma unroll
    for (int it = 0; it < T::NIT; ++it) {
        float a[T::NE];
        if (has_in) cvt_raw<T::NE, INBF16>(raw[it], a);
        else {
#pragma unroll
            for (int i = 0; i < T::NE; ++i) a[i] = 0.f;
        }
        part += tail_apply<EPI, T::NE>(g, s, m_base + T::row(lane, it), n_base + T::col(lane), v[it], a, has_in);
    }
    return part;
}
template <int EPI, bool CBF16, bool INBF16, bool HASIN>
__device__ __forceinline__ float xtail_wave_full_t(const GemmArgs& g, float s, char* __restrict__ stripe, int64_t m_wave, int64_t n_wave, int lane,
                                                   const void* ip, int64_t ild) {
    using T = TailShape<CBF16>;
    const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)stripe;
    float part = 0.f;
    uint4 bufA[T::NIT][2], bufB[T::NIT][2];   // input stripes, requested two stripes ahead of their use (see tail_wave_full_t)
    if (HASIN) {
        tail_stripe_load<EPI, CBF16, INBF16>(ip, ild, m_wave, n_wave, lane, bufA);
        tail_stripe_load<EPI, CBF16, INBF16>(ip, ild, m_wave, n_wave + 64, lane, bufB);
    }
    xpark_stripe(base, 0, lane);
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {   // stripes 2 q (bufA) and 2 q + 1 (bufB)
        float v[T::NIT][T::NE];
        __builtin_amdgcn_wave_barrier();
        xpark_read<CBF16>(stripe, lane, v);
        xpark_stripe(base, 2 * q + 1, lane);
        part += xtail_stripe_apply<EPI, CBF16, INBF16>(g, s, v, m_wave + q * 32, n_wave, lane, bufA, HASIN);
        if (HASIN && q < 3) tail_stripe_load<EPI, CBF16, INBF16>(ip, ild, m_wave + (q + 1) * 32, n_wave, lane, bufA);
        __builtin_amdgcn_wave_barrier();
        xpark_read<CBF16>(stripe, lane, v);
        if (q < 3) xpark_stripe(base, 2 * q + 2, lane);
        part += xtail_stripe_apply<EPI, CBF16, INBF16>(g, s, v, m_wave + q * 32, n_wave + 64, lane, bufB, HASIN);
        if (HASIN && q < 3) tail_stripe_load<EPI, CBF16, INBF16>(ip, ild, m_wave + (q + 1) * 32, n_wave + 64, lane, bufB);
    }
    return part;
}
template <int EPI, bool CBF16>
__device__ __forceinline__ float xtail_wave_full(const GemmArgs& g, float s, char* __restrict__ stripe, int64_t m_wave, int64_t n_wave, int lane) {
    const void* ip; int64_t ild; int idt;
    const bool has_in = tail_input<EPI>(g, ip, ild, idt);
    if constexpr (EPI == OTTER_EPI_GELU) {
        return xtail_wave_full_t<EPI, CBF16, true, false>(g, s, stripe, m_wave, n_wave, lane, ip, ild);
    } else if constexpr (EPI == OTTER_EPI_STORE) {
        if (!has_in) return xtail_wave_full_t<EPI, CBF16, true, false>(g, s, stripe, m_wave, n_wave, lane, ip, ild);
        if (idt == OTTER_BF16) return xtail_wave_full_t<EPI, CBF16, true, true>(g, s, stripe, m_wave, n_wave, lane, ip, ild);
        return xtail_wave_full_t<EPI, CBF16, false, true>(g, s, stripe, m_wave, n_wave, lane, ip, ild);
    } else {
        if (idt == OTTER_BF16) return xtail_wave_full_t<EPI, CBF16, true, true>(g, s, stripe, m_wave, n_wave, lane, ip, ild);
        return xtail_wave_full_t<EPI, CBF16, false, true>(g, s, stripe, m_wave, n_wave, lane, ip, ild);
    }
}

__device__ __forceinline__ void tile_of_block(const GemmArgs& g, int bid, int& tile_m, int& tile_n) {
    // bijective XCD-chunked order (blocks are dispatched round-robin over the 8 XCDs: block b -> XCD b % 8)
    const int nwg = g.gm * g.gn;
    const int xcd = bid & 7, idx = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    const int swz = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    // super-tile shape: 2^lm (M) x 2^(5-lm) (N) tiles, default 8 x 4; g.order (otter_gemm_set_debug bits 9-12, diagnostics) overrides
    // it: bits 0-2 = lm + 1 (0 = default), bit 3 = walk the super-tiles N-major instead of M-major
    const int lm = (g.order & 7) ? (g.order & 7) - 1 : 3;
    const int smt = 1 << lm, snt = 32 >> lm;
    if ((g.gm & (smt - 1)) == 0 && (g.gn & (snt - 1)) == 0) {
        // super-tiles of 8 (M) x 4 (N) tiles: the ~32 blocks an XCD has resident at any time form a compact patch, so its
        // L2 holds 8 A-slabs + 4 B-slabs per K-step (384 KB) instead of 16 + 2 (576 KB) for the plain M-sweep
        const int st = swz >> 5, w = swz & 31, gms = g.gm >> lm, gns = g.gn / snt;
        if (g.order & 8) {
            tile_n = (st % gns) * snt + (w >> lm);
            tile_m = (st / gns) * smt + (w & (smt - 1));
        } else {
            tile_m = (st % gms) * smt + (w & (smt - 1));
            tile_n = (st / gms) * snt + (w >> lm);
        }
    } else {
        tile_m = swz % g.gm;
        tile_n = swz / g.gm;
    }
}

}  // namespace
