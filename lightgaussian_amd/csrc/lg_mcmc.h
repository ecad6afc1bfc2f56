// lg_mcmc.h -- 3DGS-MCMC on the device (Kheradmand et al., NeurIPS 2024): the per-iteration position noise and
// the row movement behind relocation (in place) and growth (new tensors).
// Replaces (published statement): build_scaling_rotation, L @ L^T, randn_like * sigmoid-gate, bmm, add_ -- about fifteen launches and
// three [N,3,3] temporaries per iteration -- and, for relocation, the float32 powf evaluation of the alternating binomial sum.
//
//   lg_mcmc_noise_kernel   one lane per row, in place on xyz: the opacity alone decides whether the row is read at all (gate == 0:
//                          the row keeps its bits), then xyz += R (s^2 o (R^T (noise * gate)))  (lg_math.h: lg_mcmc_gate / lg_mcmc_noise_xyz).
//                          Rows of 12 and 16 bytes read per lane: a wave's loads cover one contiguous span of each tensor.
//   lg_mcmc_count_kernel   cnt[src[j]] += 1 over the n draws: integer atomics, order-independent.
//   lg_mcmc_plan_kernel    one lane per row: a row drawn cnt > 0 times gets its new opacity and scaling (lg_math.h: lg_mcmc_relocate,
//                          double) into scratch {opacity', scaling'[3]}.  Reads the model only.
//   lg_mcmc_move           grid.y = tensor, one 32-bit word per thread.  Growth (separate tensors): words [0, N * row) carry the old
//                          rows over -- a drawn row takes its planned opacity / scaling and zero moments -- and words behind them are
//                          the n copies, row dst[j] from row src[j] after that update.  In place: only the n copies are walked; each
//                          also writes the planned opacity / scaling and the zero moments of its source row (duplicate writers of a
//                          source write identical bits).  No thread reads a word another thread of the launch writes: copied words
//                          come from source rows, which are never destinations; rewritten words come from scratch.
// Guards: a source outside [0, N), a destination outside its range ([0, N) and not itself drawn in place, [N, N_out) in growth) is
// skipped, neither read through nor written.
// wave64, plain vector stores, no float atomics, no LDS, no scratch memory; word offsets are 64-bit.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include "../../include/lightgaussian_mcmc.h"
#include "lg_host.h"
#include "lg_densify.h"

static_assert(LG_MCMC_MAX_COPIES == LG_MCMC_BINOM_MAX, "lg_mcmc_relocate clamps at the header's LG_MCMC_MAX_COPIES");
static_assert(LG_MCMC_COPY == LG_DENSIFY_COPY && LG_MCMC_MOMENT == LG_DENSIFY_MOMENT, "the two roles lg_densify_tensor shares");

__global__ void __launch_bounds__(256)
lg_mcmc_noise_kernel(int N, float* xyz, const float* __restrict__ scaling, const float* __restrict__ rotation,
                     const float* __restrict__ opacity, const float* __restrict__ noise, float c, float k, float x0)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= N) return;
    const float gate = lg_mcmc_gate(opacity[i], c, k, x0);
    if (gate == 0.0f) return;                                       // the row keeps its value; nothing else of it is read
    const float* sr = scaling + 3 * (size_t)i;
    const float* qr = rotation + 4 * (size_t)i;
    const float* zr = noise + 3 * (size_t)i;
    float* xr = xyz + 3 * (size_t)i;
    const float q[4] = { qr[0], qr[1], qr[2], qr[3] }, s[3] = { expf(sr[0]), expf(sr[1]), expf(sr[2]) };
    const float z[3] = { zr[0], zr[1], zr[2] }, x[3] = { xr[0], xr[1], xr[2] };
    float o[3];
    lg_mcmc_noise_xyz(q, s, z, gate, x, o);
    xr[0] = o[0]; xr[1] = o[1]; xr[2] = o[2];
}

__global__ void __launch_bounds__(256)
lg_mcmc_count_kernel(int N, int n, const int32_t* __restrict__ src, int32_t* __restrict__ cnt)
{
    const int j = blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= n) return;
    const int32_t s = src[j];
    if ((uint32_t)s < (uint32_t)N) atomicAdd(&cnt[s], 1);
}

__global__ void __launch_bounds__(256)
lg_mcmc_plan_kernel(int N, const int32_t* __restrict__ cnt, const float* __restrict__ opacity, const float* __restrict__ scaling,
                    float min_opacity, float4* __restrict__ planned)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= N) return;
    const int32_t c = cnt[i];
    if (c <= 0) return;
    const float* sr = scaling + 3 * (size_t)i;
    const float s[3] = { sr[0], sr[1], sr[2] };
    float op, ns[3];
    lg_mcmc_relocate(opacity[i], s, c, min_opacity, op, ns);
    planned[i] = make_float4(op, ns[0], ns[1], ns[2]);
}

// what a drawn row holds after the update, for the roles that do not copy
__device__ __forceinline__ uint32_t lg_mcmc_planned_word(uint32_t role, uint32_t col, const float4 p)
{
    if (role == LG_MCMC_OPACITY) return lg_f2bits(p.x);
    if (role == LG_MCMC_SCALING) return lg_f2bits(col == 0 ? p.y : (col == 1 ? p.z : p.w));
    return 0u;                                                      // LG_MCMC_MOMENT
}

__global__ void __launch_bounds__(256)
lg_mcmc_move(int N, int64_t N_out, int n, const int32_t* __restrict__ dst_rows, const int32_t* __restrict__ src_rows,
             const int32_t* __restrict__ cnt, const float4* __restrict__ planned, const LgDensifyArgs a, int inplace)
{
    const uint32_t t = blockIdx.y;
    const uint32_t wpr = a.words[t], role = a.role[t];
    const uint32_t* src = a.src[t];                                 // (in place src == dst: no __restrict__)
    uint32_t* dst = a.dst[t];
    const size_t base = inplace ? 0 : (size_t)N * wpr;              // growth: the old rows first
    const size_t total = base + (size_t)n * wpr;
    const bool narrow = total <= 0xFFFFFFFFull;                     // (uniform) 32-bit division where it suffices
    for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < total; w += (size_t)gridDim.x * 256) {
        if (w < base) {
            const size_t row = narrow ? (size_t)((uint32_t)w / wpr) : w / wpr;
            uint32_t v = src[w];
            if (role != LG_MCMC_COPY && cnt[row] > 0) v = lg_mcmc_planned_word(role, (uint32_t)(w - row * wpr), planned[row]);
            dst[w] = v;
            continue;
        }
        const size_t u = w - base;
        const size_t j = narrow ? (size_t)((uint32_t)u / wpr) : u / wpr;
        const uint32_t col = (uint32_t)(u - j * wpr);
        const int32_t s = src_rows[j], d = dst_rows[j];
        if ((uint32_t)s >= (uint32_t)N) continue;
        if (inplace ? ((uint32_t)d >= (uint32_t)N || cnt[d] > 0) : ((int64_t)d < (int64_t)N || (int64_t)d >= N_out)) continue;
        if (role == LG_MCMC_COPY) {
            dst[(size_t)d * wpr + col] = src[(size_t)s * wpr + col];
        } else {
            const uint32_t v = lg_mcmc_planned_word(role, col, planned[s]);
            dst[(size_t)d * wpr + col] = v;
            if (inplace) dst[(size_t)s * wpr + col] = v;
        }
    }
}
