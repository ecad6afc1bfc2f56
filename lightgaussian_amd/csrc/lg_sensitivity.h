// lg_sensitivity.h -- the sensitivity pruning score of PUP 3D-GS: per Gaussian the 6 x 6 block, over (mean3D, activated scale), of the
// Gauss-Newton Hessian of the L2 reconstruction error, accumulated over the sorted tile lists a colour forward left behind, and its
// log-determinant: lg_sensitivity_walk, lg_sensitivity_accum, lg_sensitivity_score_kernel.  DESIGN section 10.14;
// include/lightgaussian_sensitivity.h; the arithmetic is lg_math.h's (lg_sensitivity_step, _moments_to_M, _AtMA, _logdet).
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
//
// A Hessian block needs the outer product of the per-pixel Jacobian, which no backward of a scalar loss gives.  It factors: a pixel sees
// theta_i only through the Gaussian's 2D mean and conic, so dI_c/dtheta_i = v_c G u^T B A and H_i(view) = A^T (B U B^T) A with
// U = sum_pixels |v|^2 G^2 u u^T -- twelve moments sum w dx^a dy^b, 2 <= a + b <= 4, per (tile, Gaussian) instance.
//
// Walk: lg_feat_walk_back (lg_features.h) with TWELVE values per hit entry.  The colour of an entry is its blend record's (r, g in the
// queued row 1; b is staged next to the wave queue, as lg_distortion.h stages m); the walk's own S serves the red channel, the hook's
// captures the other two.  The sink stores the 48-byte row of every visited instance, zeros included, at its pre-sort slot; the WHOLE
// list is walked, so every row the accumulate kernel reads was written by this launch.  No atomics, no memset.  A view the forward
// abandoned or a segment length other than the forward's leave no rows, and lg_sensitivity_accum (lg_k9_view_has_rows) reads none.
// Accum: a lane per Gaussian sums its contiguous rows in slot order in float64 (the addressing of lg_features_gather, the bounds of
// lg_camera_bwd), builds M from the record's conic and opacity, A from the five unit seeds through the ONE copy of the backward chain,
// and adds A^T M A into the caller's H [N][21] float64: mean and scale entries differ by orders of magnitude and the determinant is
// taken at the end.  A Gaussian without instances leaves its H untouched.
#pragma once

#include "../../include/lightgaussian_sensitivity.h"
#include "lg_features.h"
#include "lg_preprocess.h"

#define LG_SENS_THREADS 256

template <bool EXACT>
__global__ void __launch_bounds__(256)
lg_sensitivity_walk(LgFeatView v, uint32_t S, const uint32_t* __restrict__ meta, const uint4* __restrict__ tinfo, const float* __restrict__ bg,
                    const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib, float* __restrict__ rows)
{
    constexpr int NV = LG_SENS_NV;
    __shared__ LgFeatQueue queue;
    __shared__ float qb[4][LG_Q];
    LG_FEAT_MERGE_LDS(NV, mg);
    const int tile = xcd_tile(blockIdx.x);
    if (tile >= v.ntiles) return;
    const int wave = threadIdx.x >> 6;
    const LgBlock g = lg_block(v.W, v.H, tile % v.gx, tile / v.gx, wave, threadIdx.x & 63);
    const LgFeatWaveQueue q = queue.of(wave);
    LgBackWalk bw;
    if (!lg_feat_back_begin(v, tile, g, S, meta, final_T, n_contrib, bw)) return;

    // per pixel: the background term of the three channels, the green and blue of what lies behind
    float Tfb[3] = { 0.0f, 0.0f, 0.0f }, S1 = 0.0f, S2 = 0.0f;
    if (bg) { Tfb[0] = bw.T * bg[0]; Tfb[1] = bw.T * bg[1]; Tfb[2] = bw.T * bg[2]; }
    // the blue of a batch's hits, next to the wave's queue (ids in the queue are below N)
    auto stage = [&](uint32_t nhit) {
        if (nhit == 0u) return;
        if (g.lane < nhit) qb[wave][g.lane] = v.rec[LG_REC_F4 * (size_t)q.qid[g.lane] + 2].x;
        lg_wave_lds_sync();
    };
    auto hit = [&](const LgBackHit& h, float& T, float& Sb, float (&p)[NV]) {
        const float4 r1 = q.q1[h.j];
        const float c[3] = { r1.z, r1.w, qb[wave][h.j] };
        float Sc[3] = { Sb, S1, S2 };
        const bool ok = lg_sensitivity_step<EXACT>(h.live, h.power, h.G, h.alpha, h.dx, h.dy, c, Tfb, T, Sc, p);
        Sb = Sc[0]; S1 = Sc[1]; S2 = Sc[2];
        return ok;
    };
    auto sink = [&](uint32_t sl, const float (&t)[NV]) {
        float4* dst = reinterpret_cast<float4*>(rows) + 3 * (size_t)sl;
        dst[0] = make_float4(t[0], t[1], t[2], t[3]);
        dst[1] = make_float4(t[4], t[5], t[6], t[7]);
        dst[2] = make_float4(t[8], t[9], t[10], t[11]);
    };
    lg_feat_walk_back<NV, EXACT>(v, tile, g, tinfo, bw, bw.n_list, q, mg, stage, hit, sink);
}

// rows_cap: the rows the caller's scratch holds (num_rendered).  The view's checks are those of every kernel behind K2.
template <bool RAW>
__global__ void __launch_bounds__(LG_SENS_THREADS)
lg_sensitivity_accum(int N, int W, int H, float tanfovx, float tanfovy, float mod, uint32_t rows_cap, const float* __restrict__ viewmatrix,
                     const float* __restrict__ projmatrix, const float* __restrict__ means3D, const float* __restrict__ scales,
                     const float* __restrict__ rotations, const int32_t* __restrict__ radii, const float4* __restrict__ rec,
                     const uint32_t* __restrict__ counters, const uint32_t* __restrict__ meta, uint32_t S, const uint32_t* __restrict__ touched,
                     const uint32_t* __restrict__ offsets, const float4* __restrict__ rows, double* __restrict__ Hout)
{
    const int i = (int)blockIdx.x * LG_SENS_THREADS + (int)threadIdx.x;
    if (i >= N || radii[i] <= 0 || !lg_k9_view_has_rows(counters, meta, S, false)) return;
    const uint32_t R = min(counters[3], rows_cap);
    const uint32_t t = touched[i], off = offsets[i];
    if (t == 0u || off < t || off > R) return;      // no instances, or a row range outside [0, R): nothing is read
    double mo[LG_SENS_NV];
#pragma unroll
    for (int k = 0; k < LG_SENS_NV; k++) mo[k] = 0.0;
    for (uint32_t u = off - t; u < off; u++) {
        const float4* rp = rows + 3 * (size_t)u;
        const float4 a = rp[0], b = rp[1], c = rp[2];
        mo[0] += (double)a.x; mo[1] += (double)a.y; mo[2] += (double)a.z; mo[3] += (double)a.w;
        mo[4] += (double)b.x; mo[5] += (double)b.y; mo[6] += (double)b.z; mo[7] += (double)b.w;
        mo[8] += (double)c.x; mo[9] += (double)c.y; mo[10] += (double)c.z; mo[11] += (double)c.w;
    }
    float vm[16], pm[16];
#pragma unroll
    for (int k = 0; k < 16; k++) { vm[k] = viewmatrix[k]; pm[k] = projmatrix[k]; }
    const float4 q0 = rec[LG_REC_F4 * (size_t)i], q1 = rec[LG_REC_F4 * (size_t)i + 1];
    const float px = means3D[3 * (size_t)i], py = means3D[3 * (size_t)i + 1], pz = means3D[3 * (size_t)i + 2];
    float Sg[6], sc[3], q[4], qn;
    lg_k9_cov3d<RAW>(i, mod, nullptr, scales, rotations, Sg, sc, q, qn);
    double M[15];
    lg_sensitivity_moments_to_M(mo, q0.z, q0.w, q1.x, q1.y, M);
    // A: the chain of the five unit seeds d/d(mean2D x, y, conic A, B, C); acc[5..8] = 0
    float A[5][6];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        float acc[9] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
        acc[k] = 1.0f;
        LgGradOut go;
        float unused, dsc[3], drot[4];
        lg_backward_geom_t<false>(vm, pm, px, py, pz, Sg, acc, W, H, tanfovx, tanfovy, go, 0.0f, unused);
        lg_backward_cov3d(sc, mod, q, go.cov3D, dsc, drot);
        A[k][0] = go.mean3D[0]; A[k][1] = go.mean3D[1]; A[k][2] = go.mean3D[2];
        A[k][3] = dsc[0]; A[k][4] = dsc[1]; A[k][5] = dsc[2];
    }
    double Hi[LG_SENS_H];
    double* dst = Hout + (size_t)LG_SENS_H * (size_t)i;
#pragma unroll
    for (int k = 0; k < LG_SENS_H; k++) Hi[k] = dst[k];
    lg_sensitivity_AtMA(A, M, Hi);
#pragma unroll
    for (int k = 0; k < LG_SENS_H; k++) dst[k] = Hi[k];
}

__global__ void __launch_bounds__(LG_SENS_THREADS)
lg_sensitivity_score_kernel(int N, const double* __restrict__ Hin, const float* __restrict__ scales, double* __restrict__ out)
{
    const int i = (int)blockIdx.x * LG_SENS_THREADS + (int)threadIdx.x;
    if (i >= N) return;
    double Hi[LG_SENS_H];
#pragma unroll
    for (int k = 0; k < LG_SENS_H; k++) Hi[k] = Hin[(size_t)LG_SENS_H * (size_t)i + k];
    double s = lg_sensitivity_logdet(Hi);
    if (scales) {
        const float* sp = scales + 3 * (size_t)i;
        s = s + 2.0 * ((log((double)sp[0]) + log((double)sp[1])) + log((double)sp[2]));
    }
    out[i] = s;
}
