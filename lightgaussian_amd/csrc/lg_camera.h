// lg_camera.h -- camera pose gradients: lg_camera_bwd<RAW> (per Gaussian, K9's read side) and lg_camera_reduce (one workgroup).
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers; this one after all others).
//
// dL/dviewmatrix, dL/dprojmatrix, dL/dcampos of one view: 27 sums over its visible Gaussians of the per-Gaussian camera terms
// (lg_backward_camera_terms, lg_math.h).  A kernel of its own that gathers the moment rows a blend backward left AGAIN, on purpose: it is
// opt-in (lg_backward_camera is called only by renders with option camera_grad) and K9 stays exactly as it was.
//
// Summation order (fixed: the result is bit-identical run to run, no atomics, no look-back):
//   per Gaussian     float32 terms, as every per-Gaussian gradient of K9
//   wave             each term widened to float64, xor butterfly over the 64 lanes (partners 1, 2, 4, 8, 16, 32: a + b == b + a, so every
//                    lane holds the same bits)
//   workgroup        waves 0..3 added in that order by one thread per term; ONE plain store of 27 doubles to partials[workgroup]
//   lg_camera_reduce thread t adds partials[t], [t + 256], [t + 512] ... sequentially, then a halving tree over the 256 threads in LDS,
//                    one rounding to float32, 16 + 16 + 3 floats stored (the columns the forward never reads: exact zeros)
// float64 from the lane upward: the sums cancel (a pose gradient is the small difference of large per-splat pulls) over up to millions of
// terms, and the contract is against a float64 twin.
#pragma once

#include "lg_host.h"
#include "lg_wave.h"
#include "lg_preprocess.h"

#define LG_CAM_THREADS 256
#define LG_CAM_WAVES (LG_CAM_THREADS / LG_PP)

__device__ __forceinline__ double lg_wave_sum_f64(double v)
{
#pragma unroll
    for (int m = 1; m < LG_PP; m <<= 1) v += __shfl_xor(v, m, LG_PP);
    return v;
}

template <bool RAW>
__global__ void __launch_bounds__(LG_CAM_THREADS)
lg_camera_bwd(int N, int M, int D, int W, int H, float tanfovx, float tanfovy, float mod, uint32_t rows_cap,
              const float* __restrict__ viewmatrix, const float* __restrict__ projmatrix, const float* __restrict__ campos,
              const float* __restrict__ means3D, const float* __restrict__ shs, const float* __restrict__ scales,
              const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp, const int32_t* __restrict__ radii,
              const float4* __restrict__ rec, const uint32_t* __restrict__ counters, const uint32_t* __restrict__ meta, uint32_t S,
              const uint32_t* __restrict__ touched, const uint32_t* __restrict__ offsets, const float4* __restrict__ part,
              const float* __restrict__ shjac, double* __restrict__ partials)
{
    __shared__ double wsum[LG_CAM_WAVES][LG_CAM_TERMS];
    const uint32_t lane = threadIdx.x & (LG_PP - 1), wave = threadIdx.x / LG_PP;
    const int i = (int)blockIdx.x * LG_CAM_THREADS + (int)threadIdx.x;
    float vm[16], pm[16], cp[3];
#pragma unroll
    for (int k = 0; k < 16; k++) { vm[k] = viewmatrix[k]; pm[k] = projmatrix[k]; }
    cp[0] = campos[0]; cp[1] = campos[1]; cp[2] = campos[2];
    const bool use_sh = shs != nullptr;
    // the discipline of every kernel behind K2 (see lg_preprocess_bwd): an abandoned view, another segment length than the forward's or
    // a missing Jacobian marker leave no rows to read -- exact zeros.  R is the device's own count, capped by the rows the caller's
    // scratch holds; a Gaussian whose row range does not lie inside [0, R) contributes nothing (it cannot happen after a forward that
    // was not abandoned: the check keeps every load inside the buffer whatever the buffers hold)
    const bool view_ok = counters[0] == 0u && meta[2] == S && (!use_sh || counters[9] == LG_SHJAC_MAGIC);
    const uint32_t R = min(counters[3], rows_cap);
    bool vis = view_ok && (i < N) && radii[i] > 0;
    uint32_t my_t = 0u, my_u0 = 0u;
    if (vis) {
        const uint32_t t = touched[i], off = offsets[i];
        if (off < t || off > R) vis = false;
        else { my_t = t; my_u0 = off - t; }
    }
    float coop[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    {
        // K9's cooperative form: a splat with more than LG_COOP_ROWS instances is summed by its whole wave, 64 rows per step
        uint64_t big = __ballot(my_t > LG_COOP_ROWS);
        while (big) {
            const int src = (int)__builtin_ctzll(big);
            big &= big - 1;
            const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)my_t, src);
            const uint32_t u0 = (uint32_t)__builtin_amdgcn_readlane((int)my_u0, src);
            float acc9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t u = u0 + lane; u < u0 + t; u += LG_PP) {      // u0 + t <= R < 2^30: no wrap
                const float4* rp = part + 3 * (size_t)u;
                const float4 v0 = rp[0], v1 = rp[1], v2 = rp[2];
                acc9[0] += v0.x; acc9[1] += v0.y; acc9[2] += v0.z; acc9[3] += v0.w; acc9[4] += v1.x; acc9[5] += v1.y; acc9[6] += v1.z;
                acc9[7] += v1.w; acc9[8] += v2.x;
            }
#pragma unroll
            for (int k9 = 0; k9 < 9; k9++) {
                const float tot = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_sum_to_lane63(acc9[k9])), 63));
                if ((int)lane == src) coop[k9] = tot;
            }
        }
    }
    float term[LG_CAM_TERMS];
#pragma unroll
    for (int k = 0; k < LG_CAM_TERMS; k++) term[k] = 0.0f;
    if (vis) {
        float mo[9];
#pragma unroll
        for (int k9 = 0; k9 < 9; k9++) mo[k9] = coop[k9];
        if (my_t <= LG_COOP_ROWS) {
            const uint32_t ue = my_u0 + my_t;
            for (uint32_t u = my_u0; u < ue; u += LG_K9_GATHER) {
                float4 a[LG_K9_GATHER][3];
#pragma unroll
                for (int j = 0; j < LG_K9_GATHER; j++) {
                    const float4* rp = part + 3 * (size_t)min(u + (uint32_t)j, ue - 1u);
                    a[j][0] = rp[0]; a[j][1] = rp[1]; a[j][2] = rp[2];
                }
#pragma unroll
                for (int j = 0; j < LG_K9_GATHER; j++) {
                    if (u + (uint32_t)j < ue) {
                        mo[0] += a[j][0].x; mo[1] += a[j][0].y; mo[2] += a[j][0].z; mo[3] += a[j][0].w; mo[4] += a[j][1].x; mo[5] += a[j][1].y;
                        mo[6] += a[j][1].z; mo[7] += a[j][1].w; mo[8] += a[j][2].x;
                    }
                }
            }
        }
        const float4 q0 = rec[LG_REC_F4 * (size_t)i], q1 = rec[LG_REC_F4 * (size_t)i + 1], q2 = rec[LG_REC_F4 * (size_t)i + 2];
        const float px = means3D[3 * (size_t)i], py = means3D[3 * (size_t)i + 1], pz = means3D[3 * (size_t)i + 2];
        float a[9];
        lg_rows_to_grads(mo, q0.z, q0.w, q1.x, q1.y, a);
        float Sg[6];
        if (cov3D_precomp) {
#pragma unroll
            for (int k = 0; k < 6; k++) Sg[k] = cov3D_precomp[6 * (size_t)i + k];
        } else {
            float sc[3] = { scales[3 * (size_t)i], scales[3 * (size_t)i + 1], scales[3 * (size_t)i + 2] };
            const float4 q4 = *reinterpret_cast<const float4*>(rotations + 4 * (size_t)i);
            float q[4] = { q4.x, q4.y, q4.z, q4.w };
            if (RAW) {      // K9's expressions, which are K1's
                sc[0] = expf(sc[0]); sc[1] = expf(sc[1]); sc[2] = expf(sc[2]);
                const float qn = fmaxf(sqrtf((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3])), 1e-12f);
                q[0] /= qn; q[1] /= qn; q[2] /= qn; q[3] /= qn;
            }
            lg_cov3d(sc, mod, q, Sg);
        }
        float d[3] = {0.0f, 0.0f, 0.0f};
        if (use_sh) {
            const uint32_t cb = __float_as_uint(q2.w) >> LG_ID_BITS;
            const float dRGB[3] = { (cb & 1u) ? 0.0f : a[6], (cb & 2u) ? 0.0f : a[7], (cb & 4u) ? 0.0f : a[8] };
            const float* jr = shjac + 9 * (size_t)i;
            const lg_f4u j0 = reinterpret_cast<const lg_f4u*>(jr)[0], j1 = reinterpret_cast<const lg_f4u*>(jr)[1];
            const float J[9] = { j0.x, j0.y, j0.z, j0.w, j1.x, j1.y, j1.z, j1.w, jr[8] };
            lg_backward_sh_jac(D, J, px, py, pz, cp, dRGB, d, [](int, int, float) {});
        }
        lg_backward_camera_terms(vm, pm, px, py, pz, Sg, a, W, H, tanfovx, tanfovy, d, term);
    }
    (void)M;
#pragma unroll
    for (int k = 0; k < LG_CAM_TERMS; k++) {
        const double s = lg_wave_sum_f64((double)term[k]);
        if (lane == 0) wsum[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < LG_CAM_TERMS) {
        double s = wsum[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < LG_CAM_WAVES; w++) s += wsum[w][threadIdx.x];
        partials[(size_t)blockIdx.x * LG_CAM_TERMS + threadIdx.x] = s;
    }
}

// One workgroup: out = sum over n partial rows, fixed order (header comment); n == 0 (an empty model) writes zeros.
__global__ void __launch_bounds__(LG_CAM_THREADS)
lg_camera_reduce(uint32_t n, const double* __restrict__ partials, float* __restrict__ dL_dviewmatrix, float* __restrict__ dL_dprojmatrix,
                 float* __restrict__ dL_dcampos)
{
    __shared__ double red[LG_CAM_THREADS];
    __shared__ float tot[LG_CAM_TERMS];
    const uint32_t t = threadIdx.x;
    for (int k = 0; k < LG_CAM_TERMS; k++) {
        double s = 0.0;
        for (uint32_t r = t; r < n; r += LG_CAM_THREADS) s += partials[(size_t)r * LG_CAM_TERMS + k];
        red[t] = s;
        __syncthreads();
        for (uint32_t h = LG_CAM_THREADS / 2; h > 0; h >>= 1) {
            if (t < h) red[t] += red[t + h];
            __syncthreads();
        }
        if (t == 0) tot[k] = (float)red[0];
        __syncthreads();
    }
    // packed terms -> the 4 x 4 row-vector matrices: vm columns 0..2, pm columns 0, 1, 3
    if (t < 16) {
        const uint32_t r = t >> 2, c = t & 3u;
        dL_dviewmatrix[t] = (c < 3u) ? tot[3 * r + c] : 0.0f;
        dL_dprojmatrix[t] = (c == 2u) ? 0.0f : tot[12 + 3 * r + (c == 3u ? 2u : c)];
    }
    if (t < 3) dL_dcampos[t] = tot[24 + t];
}
