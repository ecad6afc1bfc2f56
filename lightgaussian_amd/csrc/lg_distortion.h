// lg_distortion.h -- depth distortion D = sum_{i<j} w_i w_j (m_i - m_j)^2 and the median of a per-Gaussian scalar m over the sorted tile
// lists a forward left behind (lg_blend_distortion), and their gradient with respect to the geometry and to m (lg_backward_distortion):
// lg_distortion_fwd, lg_distortion_bwd.  DESIGN section 10.12; include/lightgaussian_distortion.h.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
//
// D can be composed from lg_blend_features with columns [m, m m] as A M2 - M1^2, but that difference cancels in float32 exactly where the
// loss matters (a thin surface far from the camera); the sums here run about the pixel's first contributor (lg_distortion_step,
// lg_math.h), a per-pixel shift no per-Gaussian channel can express.  The median is not a blend at all.
//
// Forward: lg_features_fwd's loop (lg_features.h) without feature rows: the m of a batch's hits is staged next to the queue, a
// contributing hit is one lg_distortion_step.  Writes distortion [H,W], median [H,W] (optional) and the state the backward needs:
// (A, P1, P2, c) as one 16-byte store per pixel, then med_pos [H W] uint32.  An abandoned view has empty lists: zeros everywhere.
//
// Backward: lg_feat_walk_back with SEVEN values per hit entry: the six pixel-offset moments of lg_feature_bwd_step and dm
// (lg_distortion_bwd_step).  The sink adds columns 0..5 to the instance's 12-float moment row (ACCUM) or writes the whole row (!ACCUM),
// and stores dm with one plain store into dm_rows [num_rendered] at the same pre-sort slot, zeros included -- so EVERY batch of the list
// is visited (the ones no pixel reached get their zeros), also under ACCUM.  Under a segment length other than the forward's the lists
// cannot be located (the buffer's layout depends on it): the kernel zero-fills the dm rows and returns before it reads a list (K9
// refuses the view's moment rows by itself).
// lg_features_gather (C = 1) then sums every Gaussian's dm rows in slot order.  No float atomics, no memset: bit-identical run to run.
#pragma once

#include "../../include/lightgaussian_distortion.h"
#include "lg_features.h"

#define LG_DIST_NV 7

// the m of a batch's hits, next to the wave's queue (ids in the queue are below N)
__device__ __forceinline__ void lg_dist_stage_m(const float* m, int m_stride, const LgFeatWaveQueue& q, uint32_t nhit, float* qm, uint32_t lane)
{
    if (nhit == 0u) return;
    if (lane < nhit) qm[lane] = m[(size_t)q.qid[lane] * (size_t)m_stride];
    lg_wave_lds_sync();
}

template <bool EXACT>
__global__ void __launch_bounds__(256)
lg_distortion_fwd(LgFeatView v, const float* __restrict__ m, int m_stride, float* __restrict__ distortion, float* __restrict__ median,
                  float4* __restrict__ st, uint32_t* __restrict__ st_pos)
{
    __shared__ LgFeatQueue queue;
    __shared__ float qm[4][LG_Q];
    const int tile = xcd_tile(blockIdx.x);
    if (tile >= v.ntiles) return;
    const int wave = threadIdx.x >> 6;
    const LgBlock g = lg_block(v.W, v.H, tile % v.gx, tile / v.gx, wave, threadIdx.x & 63);
    const LgFeatWaveQueue q = queue.of(wave);
    uint32_t lo, hi;
    (void)lg_feat_list(v, tile, lo, hi);        // an abandoned view has empty lists: zeros

    const float pxf = (float)g.pxi, pyf = (float)g.pyi;
    float T = 1.0f;
    LgDistortion s = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u };
    bool done = !g.inside;
    for (uint32_t base = lo; base < hi; base += LG_Q) {
        if (__ballot(!done) == 0) break;        // every pixel of this wave is saturated or outside
        const uint32_t nhit = lg_feat_front(v, base + g.lane, hi, g, q);
        if (nhit == 0u) continue;
        lg_dist_stage_m(m, m_stride, q, nhit, qm[wave], g.lane);
        const uint32_t rel = base - lo + 1u;    // 1-based list position of the batch's entry 0
        for (uint32_t j = 0; j < nhit; j++) {
            const float Tin = T;
            float w;
            const int res = lg_feat_pair<EXACT>(q.q0[j], q.q1[j], done, pxf, pyf, T, w);
            done = done || res == 2;
            if (res == 1) lg_distortion_step(w, Tin, qm[wave][j], rel + q.qpos[j], s);
        }
        lg_feat_batch_end();
    }
    if (g.inside) {
        const size_t pid = (size_t)g.pyi * v.W + g.pxi;
        distortion[pid] = s.D;
        if (median) median[pid] = s.med;
        st[pid] = make_float4(s.A, s.P1, s.P2, s.c);
        st_pos[pid] = s.med_pos;
    }
}

template <bool EXACT, bool ACCUM>
__global__ void __launch_bounds__(256)
lg_distortion_bwd(LgFeatView v, uint32_t S, const uint32_t* __restrict__ meta, const uint4* __restrict__ tinfo, const float* __restrict__ m,
                  int m_stride, const float4* __restrict__ st, const uint32_t* __restrict__ st_pos, const float* __restrict__ dL_dD,
                  const float* __restrict__ dL_dmed, const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
                  float* __restrict__ rows, float* __restrict__ dm_rows)
{
    constexpr int NV = LG_DIST_NV;
    // the wave queues as four arrays, not one LgFeatQueue: as one LDS object they cost lg_distortion_bwd<false, true> two VGPRs
    __shared__ float4 q0[4][LG_Q], q1[4][LG_Q];
    __shared__ uint32_t qid[4][LG_Q], qpos[4][LG_Q];
    __shared__ float qm[4][LG_Q];
    LG_FEAT_MERGE_LDS(NV, mg);
    if (!v.live) return;                                         // no lists, no binning buffer: lg_features_gather writes the zeros
    if (meta[2] != S) {
        // another segment length than the forward's: the binning buffer is laid out by S behind meta, so the entries cannot be found.
        // K9 refuses the moment rows by itself; the dm rows get their zeros here, a share per workgroup (v.cap = num_rendered rows)
        for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < (size_t)v.cap; i += (size_t)gridDim.x * 256u) dm_rows[i] = 0.0f;
        return;
    }
    const int tile = xcd_tile(blockIdx.x);
    if (tile >= v.ntiles) return;
    const int wave = threadIdx.x >> 6;
    const LgBlock g = lg_block(v.W, v.H, tile % v.gx, tile / v.gx, wave, threadIdx.x & 63);
    const LgFeatWaveQueue q = { q0[wave], q1[wave], qid[wave], qpos[wave] };
    LgBackWalk bw;
    if (!lg_feat_back_begin(v, tile, g, S, meta, final_T, n_contrib, bw)) return;      // (an abandoned view: lg_features_gather gives zeros)

    // per pixel: the forward's final sums, the two gradients
    LgDistortion s = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u };
    float gD = 0.0f, gM = 0.0f;
    if (g.inside) {
        const size_t pid = (size_t)g.pyi * v.W + g.pxi;
        const float4 f = st[pid];
        s.A = f.x; s.P1 = f.y; s.P2 = f.z; s.c = f.w;
        s.med_pos = st_pos[pid];
        if (dL_dD) gD = dL_dD[pid];
        if (dL_dmed) gM = dL_dmed[pid];
    }
    auto stage = [&](uint32_t nhit) { lg_dist_stage_m(m, m_stride, q, nhit, qm[wave], g.lane); };
    auto hit = [&](const LgBackHit& h, float& T, float& Sb, float (&p)[NV]) {
        return lg_distortion_bwd_step<EXACT>(h.live, h.power, h.G, h.alpha, h.dx, h.dy, qm[wave][h.j], h.pos, s, gD, gM, T, Sb, p, p[6]);
    };
    auto sink = [&](uint32_t sl, const float (&t)[NV]) { lg_feat_store_moments<ACCUM>(rows, sl, t); dm_rows[sl] = t[6]; };
    // the whole list, also under ACCUM: every dm row gets its value, the ones no pixel reached their zeros
    lg_feat_walk_back<NV, EXACT>(v, tile, g, tinfo, bw, bw.n_list, q, mg, stage, hit, sink);
}
