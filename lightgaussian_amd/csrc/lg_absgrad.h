// lg_absgrad.h -- absolute screen-space mean gradients per Gaussian: lg_absgrad_rows (LG_FLAG_ABSGRAD, lg_backward_abs).
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers; this one after lg_camera.h).
//
// K7's ABS instantiations (lg_blend_bwd<EXACT, true>, lg_blend.h) leave sum_pixels |t (2 ha dx + nb dy)| and its y twin in floats 9 and 10
// of every instance's 48-byte gradient row.  This kernel sums them per Gaussian and finishes them with the record's opacity
// (lg_abs_rows_to_grad, lg_math.h): out [N][3] in the NDC units and layout of dL_dmeans2D, z = 0.  One lane per Gaussian; only the THIRD
// float4 of every row is read (16 of its 48 bytes).  K9 is not involved and not changed: an opt-in kernel of its own between K7 and K9.
//
// Summation order (fixed: bit-identical run to run, no atomics): a Gaussian of up to LG_COOP_ROWS instances is summed by its lane, rows in
// slot order, LG_ABS_GATHER loads in flight; a larger one by the whole wave as lg_k9_gather_coop does (lane l adds rows l, l + 64, ...,
// then the DPP wave sum).
// Exact zeros for Gaussians with radii <= 0 and for a view that left no rows (aborted forward, another segment length: K9's own test).
#pragma once

#include "lg_host.h"
#include "lg_wave.h"
#include "lg_preprocess.h"

#define LG_ABS_THREADS 256
#define LG_ABS_GATHER 4    // rows a lane requests per round trip (as LG_K9_GATHER)

__global__ void __launch_bounds__(LG_ABS_THREADS)
lg_absgrad_rows(int N, int W, int H, uint32_t rows_cap, const int32_t* __restrict__ radii, const float4* __restrict__ rec,
                const uint32_t* __restrict__ counters, const uint32_t* __restrict__ meta, uint32_t S, const uint32_t* __restrict__ touched,
                const uint32_t* __restrict__ offsets, const float4* __restrict__ part, float* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & (LG_PP - 1);
    const int i = (int)blockIdx.x * LG_ABS_THREADS + (int)threadIdx.x;
    // (as lg_camera_bwd: R is the device's own count, capped by the rows the caller's scratch holds; a row range outside [0, R) -- it
    // cannot happen after a forward that was not abandoned -- contributes nothing, so every load stays inside the buffer)
    const bool view_ok = lg_k9_view_has_rows(counters, meta, S, false);
    const uint32_t R = min(counters[3], rows_cap);
    bool vis = view_ok && (i < N) && radii[i] > 0;
    uint32_t my_t = 0u, my_u0 = 0u;
    if (vis) {
        const uint32_t t = touched[i], off = offsets[i];
        if (off < t || off > R) vis = false;
        else { my_t = t; my_u0 = off - t; }
    }
    float sx = 0.0f, sy = 0.0f;
    // whole wave, one big Gaussian at a time (every lane of the wave takes part: `big` is wave-uniform)
    uint64_t big = __ballot(my_t > LG_COOP_ROWS);
    while (big) {
        const int src = (int)__builtin_ctzll(big);
        big &= big - 1;
        const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)my_t, src);
        const uint32_t u0 = (uint32_t)__builtin_amdgcn_readlane((int)my_u0, src);
        float ax = 0.0f, ay = 0.0f;
        for (uint32_t u = u0 + lane; u < u0 + t; u += LG_PP) {
            const float4 v2 = part[3 * (size_t)u + 2];
            ax += v2.y; ay += v2.z;
        }
        const float tx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_sum_to_lane63(ax)), 63));
        const float ty = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_sum_to_lane63(ay)), 63));
        if ((int)lane == src) { sx = tx; sy = ty; }
    }
    if (vis && my_t <= LG_COOP_ROWS) {
        const uint32_t ue = my_u0 + my_t;
        for (uint32_t u = my_u0; u < ue; u += LG_ABS_GATHER) {
            float4 a[LG_ABS_GATHER];
#pragma unroll
            for (int j = 0; j < LG_ABS_GATHER; j++) a[j] = part[3 * (size_t)min(u + (uint32_t)j, ue - 1u) + 2];   // (past the last row: re-read, not added)
#pragma unroll
            for (int j = 0; j < LG_ABS_GATHER; j++)
                if (u + (uint32_t)j < ue) { sx += a[j].y; sy += a[j].z; }
        }
    }
    if (i < N) {
        float o[3] = {0.0f, 0.0f, 0.0f};
        if (vis) lg_abs_rows_to_grad(sx, sy, rec[LG_REC_F4 * (size_t)i + 1].y, W, H, o);
        out[3 * (size_t)i] = o[0]; out[3 * (size_t)i + 1] = o[1]; out[3 * (size_t)i + 2] = o[2];
    }
}
