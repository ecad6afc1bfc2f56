// lg_camera.h -- camera pose gradients: lg_camera_bwd<RAW, AA> (per Gaussian, K9's read side) and lg_camera_reduce (one workgroup).
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers; this one after all others).
//
// dL/dviewmatrix, dL/dprojmatrix, dL/dcampos of one view: 27 sums over its visible Gaussians of the per-Gaussian camera terms
// (lg_backward_camera_terms, lg_math.h).  A second pass over the moment rows a blend backward left, through K9's own functions
// (lg_k9_*, lg_preprocess.h): the view check, both row gathers, the covariance, the clamp-masked dRGB and the Jacobian row are the
// code K9 runs, so the rows are summed in K9's order whatever its tuning.  A kernel of its own because it is opt-in
// (lg_backward_camera is called only by renders with option camera_grad).
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

// AA (LG_FLAG_ANTIALIAS): the compensation factor of the opacity depends on the camera through T2 and the view-space mean; the terms
// need the input opacity (`opacities`, the last parameter, activated as K1 did; never read when AA = false, whose instantiations are the
// kernels as they were, instruction for instruction).
template <bool RAW, bool AA>
__global__ void __launch_bounds__(LG_CAM_THREADS)
lg_camera_bwd(int N, int M, int D, int W, int H, float tanfovx, float tanfovy, float mod, uint32_t rows_cap,
              const float* __restrict__ viewmatrix, const float* __restrict__ projmatrix, const float* __restrict__ campos,
              const float* __restrict__ means3D, const float* __restrict__ shs, const float* __restrict__ scales,
              const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp, const int32_t* __restrict__ radii,
              const float4* __restrict__ rec, const uint32_t* __restrict__ counters, const uint32_t* __restrict__ meta, uint32_t S,
              const uint32_t* __restrict__ touched, const uint32_t* __restrict__ offsets, const float4* __restrict__ part,
              const float* __restrict__ shjac, double* __restrict__ partials, const float* __restrict__ opacities)
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
    const bool view_ok = lg_k9_view_has_rows(counters, meta, S, use_sh);
    const uint32_t R = min(counters[3], rows_cap);
    bool vis = view_ok && (i < N) && radii[i] > 0;
    uint32_t my_t = 0u, my_u0 = 0u;
    if (vis) {
        const uint32_t t = touched[i], off = offsets[i];
        if (off < t || off > R) vis = false;
        else { my_t = t; my_u0 = off - t; }      // my_u0 + my_t <= R < 2^30: no wrap
    }
    float coop[9];
    lg_k9_gather_coop(part, my_t, my_u0, lane, coop);
    float term[LG_CAM_TERMS];
#pragma unroll
    for (int k = 0; k < LG_CAM_TERMS; k++) term[k] = 0.0f;
    if (vis) {
        float mo[9];
        lg_k9_gather_lane(part, my_t, my_u0, coop, mo);
        const float4 q0 = rec[LG_REC_F4 * (size_t)i], q1 = rec[LG_REC_F4 * (size_t)i + 1], q2 = rec[LG_REC_F4 * (size_t)i + 2];
        const float px = means3D[3 * (size_t)i], py = means3D[3 * (size_t)i + 1], pz = means3D[3 * (size_t)i + 2];
        float a[9];
        lg_rows_to_grads(mo, q0.z, q0.w, q1.x, q1.y, a);
        float Sg[6], sc[3], q[4], qn;
        lg_k9_cov3d<RAW>(i, mod, cov3D_precomp, scales, rotations, Sg, sc, q, qn);
        float d[3] = {0.0f, 0.0f, 0.0f};
        if (use_sh) {
            float dRGB[3], J[9];
            lg_k9_drgb(q2.w, a, dRGB);
            lg_k9_jac_row(shjac, i, J);
            lg_backward_sh_jac(D, J, px, py, pz, cp, dRGB, d, [](int, int, float) {});
        }
        const float op_in = !AA ? 0.0f : RAW ? lg_sigmoid(opacities[i]) : opacities[i];
        lg_backward_camera_terms_t<AA>(vm, pm, px, py, pz, Sg, a, W, H, tanfovx, tanfovy, d, term, op_in);
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
