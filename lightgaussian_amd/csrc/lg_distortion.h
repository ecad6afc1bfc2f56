// lg_distortion.h -- depth distortion D = sum_{i<j} w_i w_j (m_i - m_j)^2 and the median of a per-Gaussian scalar m over the sorted tile
// lists a forward left behind (lg_blend_distortion), and their gradient with respect to the geometry and to m (lg_backward_distortion):
// lg_distortion_fwd, lg_distortion_bwd.  DESIGN section 10.12; include/lightgaussian_distortion.h.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
//
// D can be composed from lg_blend_features with columns [m, m m] as A M2 - M1^2, but that difference cancels in float32 exactly where the
// loss matters (a thin surface far from the camera); the sums here run about the pixel's first contributor (lg_distortion_step,
// lg_math.h), a per-pixel shift no per-Gaussian channel can express.  The median is not a blend at all.
//
// Forward: lg_features_fwd's walk (lg_feat_list, _front, _pair: a workgroup per 16 x 16 tile, a wave per 8 x 8 block, batches of LG_Q
// entries, each pixel terminates on its own T) without feature rows: the m of a batch's hits is staged next to the queue.  Writes
// distortion [H,W], median [H,W] (optional) and the state the backward needs: (A, P1, P2, c) as one 16-byte store per pixel, then
// med_pos [H W] uint32.  An abandoned view has empty lists: zeros everywhere.
//
// Backward: lg_features_bwd_geom's walk, back to front, the same workgroup-uniform barriers, `live` from the img buffer's final_T /
// n_contrib.  Per hit entry SEVEN values are reduced over the wave (lg_feat_reduce<7>): the six pixel-offset moments of
// lg_feature_bwd_step and dm.  The four waves meet in LDS; thread e adds columns 0..5 to the instance's 12-float moment row (ACCUM) or
// writes the whole row (!ACCUM), and stores dm with one plain store into dm_rows [num_rendered] at the same pre-sort slot, zeros
// included -- so EVERY batch of the list is visited (the ones no pixel reached get their zeros), also under ACCUM.  Under a segment length
// other than the forward's the lists cannot be located (the buffer's layout depends on it): the kernel zero-fills the dm rows and returns
// before it reads a list (K9 refuses the view's moment rows by itself).
// lg_features_gather (C = 1) then sums every Gaussian's dm rows in slot order.  No float atomics, no memset: bit-identical run to run.
#pragma once

#include "../../include/lightgaussian_distortion.h"
#include "lg_features.h"

#define LG_DIST_NV 7

template <bool EXACT>
__global__ void __launch_bounds__(256)
lg_distortion_fwd(LgFeatView v, const float* __restrict__ m, int m_stride, float* __restrict__ distortion, float* __restrict__ median,
                  float4* __restrict__ st, uint32_t* __restrict__ st_pos)
{
    __shared__ float4 q0[4][LG_Q], q1[4][LG_Q];
    __shared__ uint32_t qid[4][LG_Q], qpos[4][LG_Q];
    __shared__ float qm[4][LG_Q];
    const int tile = xcd_tile(blockIdx.x);
    if (tile >= v.ntiles) return;
    const int wave = threadIdx.x >> 6;
    const uint32_t lane = threadIdx.x & 63;
    const LgBlock g = lg_block(v.W, v.H, tile % v.gx, tile / v.gx, wave, lane);
    const float pxf = (float)g.pxi, pyf = (float)g.pyi;
    uint32_t lo, hi;
    (void)lg_feat_list(v, tile, lo, hi);        // an abandoned view has empty lists: zeros

    float T = 1.0f;
    LgDistortion s = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u };
    bool done = !g.inside;
    for (uint32_t base = lo; base < hi; base += LG_Q) {
        if (__ballot(!done) == 0) break;        // every pixel of this wave is saturated or outside
        const uint32_t nhit = lg_feat_front(v, base + lane, hi, (float)g.wx0, (float)g.wy0, q0[wave], q1[wave], qid[wave], qpos[wave], lane);
        if (nhit == 0u) continue;
        if (lane < nhit) qm[wave][lane] = m[(size_t)qid[wave][lane] * (size_t)m_stride];     // (ids in the queue are below N)
        lg_wave_lds_sync();
        const uint32_t rel = base - lo + 1u;    // 1-based list position of the batch's entry 0
        for (uint32_t j = 0; j < nhit; j++) {
            const float4 a = q0[wave][j], b = q1[wave][j];
            const float Tin = T;
            float w;
            const int res = lg_feat_pair<EXACT>(a, b, done, pxf, pyf, T, w);
            done = done || res == 2;
            if (res == 1) lg_distortion_step(w, Tin, qm[wave][j], rel + qpos[wave][j], s);
        }
        // release + barrier without the acquire (so not lg_wave_lds_sync): the LDS accesses above must be done first; no read below depends on them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();        // (the next batch overwrites the queue)
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
    __shared__ float4 q0[4][LG_Q], q1[4][LG_Q];
    __shared__ uint32_t qid[4][LG_Q], qpos[4][LG_Q];
    __shared__ float qm[4][LG_Q];
    __shared__ __attribute__((aligned(16))) float red[4][NV * LG_RED_STRIDE];
    __shared__ float part[4][LG_Q * LG_FEAT_PART_STRIDE(NV)];
    __shared__ unsigned long long wmask[4];
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
    const uint32_t lane = threadIdx.x & 63;
    const int tx = tile % v.gx, ty = tile / v.gx;
    const LgBlock g = lg_block(v.W, v.H, tx, ty, wave, lane);
    const float pxf = (float)g.pxi, pyf = (float)g.pyi;
    uint32_t lo, hi;
    if (!lg_feat_list(v, tile, lo, hi) || lo == hi) return;      // workgroup-uniform (an abandoned view: lg_features_gather gives zeros)
    const uint32_t slot_cap = min(v.counters[3], v.cap);
    const uint32_t n_list = hi - lo;

    // per pixel: the forward's final sums, the two gradients, the replay state
    LgDistortion s = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u };
    float gD = 0.0f, gM = 0.0f, T = 0.0f, Sb = 0.0f;
    uint32_t last = 0u;
    if (g.inside) {
        const size_t pid = (size_t)g.pyi * v.W + g.pxi;
        const float4 f = st[pid];
        s.A = f.x; s.P1 = f.y; s.P2 = f.z; s.c = f.w;
        s.med_pos = st_pos[pid];
        T = final_T[pid];
        last = min(n_contrib[pid], n_list);
        if (dL_dD) gD = dL_dD[pid];
        if (dL_dmed) gM = dL_dmed[pid];
    }
    // the last list position any pixel of the wave reached
    const uint32_t wl = (uint32_t)__builtin_amdgcn_readfirstlane((int)lg_wave_all_max(last));

    for (int k = (int)((n_list - 1u) / LG_Q); k >= 0; k--) {
        const uint32_t rel0 = (uint32_t)k * LG_Q, base = lo + rel0;
        const uint32_t nbt = min((uint32_t)LG_Q, n_list - rel0);
        // thread e of the workgroup owns entry e of the batch: the pre-sort slot its rows live at
        const uint32_t sl = lg_feat_slot(v, tinfo, base + threadIdx.x, threadIdx.x < nbt, tx, ty);
        uint64_t hitmask = 0ull;                                  // entries of the batch this wave has a partial row for (scalar)
        if (wl > rel0) {
            const uint32_t nhit = lg_feat_front(v, base + lane, hi, (float)g.wx0, (float)g.wy0, q0[wave], q1[wave], qid[wave], qpos[wave], lane);
            if (nhit != 0u) {
                if (lane < nhit) qm[wave][lane] = m[(size_t)qid[wave][lane] * (size_t)m_stride];
                lg_wave_lds_sync();
            }
            for (int j = (int)nhit - 1; j >= 0; j--) {
                const float4 a = q0[wave][j], b = q1[wave][j];
                const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)qpos[wave][j]);
                float dx, dy;
                const float power = lg_rec_power(a, b, pxf, pyf, dx, dy);
                float G;
                const float alpha = lg_feat_alpha<EXACT>(b.y, power, G);
                float p[NV] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                const uint32_t pos = rel0 + e + 1u;
                const bool ok = lg_distortion_bwd_step<EXACT>(pos <= last, power, G, alpha, dx, dy, qm[wave][j], pos, s, gD, gM, T, Sb, p, p[6]);
                if (__ballot(ok) == 0) continue;                  // no pixel of the wave took the entry
                lg_feat_reduce<NV>(p, red[wave], &part[wave][e * LG_FEAT_PART_STRIDE(NV)], lane);
                hitmask |= 1ull << e;
            }
        }
        if (lane == 0u) wmask[wave] = hitmask;
        __syncthreads();
        if (threadIdx.x < nbt && sl < slot_cap) {
            const uint32_t e = threadIdx.x;
            float t[NV] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int u = 0; u < 4; u++)
                if ((wmask[u] >> e) & 1ull) {
#pragma unroll
                    for (int r = 0; r < NV; r++) t[r] += part[u][e * LG_FEAT_PART_STRIDE(NV) + r];
                }
            float4* dst = reinterpret_cast<float4*>(rows) + 3 * (size_t)sl;
            if (ACCUM) {
                const float4 r0 = dst[0];
                const float2 r1 = *reinterpret_cast<const float2*>(dst + 1);
                dst[0] = make_float4(r0.x + t[0], r0.y + t[1], r0.z + t[2], r0.w + t[3]);
                *reinterpret_cast<float2*>(dst + 1) = make_float2(r1.x + t[4], r1.y + t[5]);
            } else {
                dst[0] = make_float4(t[0], t[1], t[2], t[3]);
                dst[1] = make_float4(t[4], t[5], 0.0f, 0.0f);
                dst[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            dm_rows[sl] = t[6];
        }
        __syncthreads();                                          // (the next batch overwrites the queue, the partials and the masks)
    }
}
