// lg_features.h -- blend C per-Gaussian feature channels over the sorted tile lists a forward left behind (lg_blend_features), and the
// gradient of that blend with respect to the features (lg_blend_features_backward): lg_features_fwd, lg_features_bwd, lg_features_gather.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
//
// The blending weights w = alpha T of a view are a function of what its forward leaves in the geom / binning buffers -- the 48-byte
// records, the sorted keys, the tile ranges, tinfo -- so any number of further channels is composited without K1, the scan, the
// duplication, the radix passes and the tile sort, and the gradient with respect to the channels, dF[j][c] = sum_pixels w[p][j] g[c][p],
// needs neither K7's back-to-front replay nor K9.
//
// Walk (both kernels): K6's -- a workgroup per 16 x 16 tile, a wave per 8 x 8 block, batches of 64 list entries, lg_block_hit against the
// wave's block, hits compacted in list order into the wave's LDS queue -- but only the 32 bytes of record the pair step reads are queued,
// next to the Gaussian id.  The pair step is lg_feature_step (lg_math.h) on lg_pair_power and on lg_alpha_exact (canonical) or the
// forward's guarded hardware exp (LG_FLAG_FAST_EXP): the include / exclude decisions are the forward's.  Each pixel terminates on its own
// T (1 - alpha) < 1e-4; n_contrib is not read.  Lists of any length are walked serially (no checkpoints).  Nothing spins or waits; every
// loop is bounded by the tile's range clamped to the view's instance count (geom.counters, as every kernel behind K2), ids are
// checked against N.  A view the forward abandoned on the device has empty lists here: the image is the background, the gradient zero.
//
// Forward: the feature rows of a batch's hits are staged through LDS (coalesced row segments; the pair loop reads them as broadcast
// ds_read_b128) and CG = 4 / 16 / 32 channels are carried per walk -- one walk up to 32 channels, two up to 64.  out_c = fma(T, bg_c, F_c).
// alpha is accumulated as one more channel whose feature is 1 (sum of w): bit for bit the blend of a column of ones, equal to 1 - T
// up to rounding.
//
// Backward: K7's discipline -- no float atomics, no memset.  Per hit entry a wave reduces w g[c] over its 64 pixels through an LDS
// transpose (lg_feat_reduce: K7's wave_reduce_via_lds, lg_blend.h, for NV = 4 / 8 / 16 values; entries no lane of the wave hit are skipped), the four waves'
// partials meet in LDS and one row of NV sums per (tile, Gaussian) instance goes to the instance's pre-sort slot (lg_slot_of), written
// exactly once, zeros included.  lg_features_gather adds every Gaussian's contiguous rows in slot order: bit-identical run to run.
// Every step of the walk is one function (lg_feat_list, _front, _alpha, _pair, _stage_rows, _slot, _reduce); only the cross-wave merges
// of lg_features_bwd (a thread per (entry, value)) and lg_features_bwd_geom (a thread per entry, 12-float rows) stay with their kernels.
#pragma once

#include "lg_host.h"
#include "lg_wave.h"
#include "lg_blend.h"

// what both kernels need of a view (by value in the kernel arguments)
struct LgFeatView {
    int W, H, gx, ntiles, N;
    int live;                       // the view has Gaussians and a binning buffer with instances; otherwise every list is empty and counters is not read
    uint32_t cap;                   // instances the binning buffer was carved for
    uint32_t gid_mask;
    const uint2* ranges; const uint64_t* entries; const float4* rec; const uint32_t* counters;
};

// Entries [lo, hi) of the tile's list, clamped to the view's instance count.  False: the forward abandoned the view on the device.
__device__ __forceinline__ bool lg_feat_list(const LgFeatView& v, int tile, uint32_t& lo, uint32_t& hi)
{
    lo = hi = 0u;
    if (!v.live) return true;
    if (v.counters[0] != 0u) return false;
    const uint32_t R = min(v.counters[3], v.cap);
    const uint2 r = v.ranges[tile];
    hi = min(r.y, R); lo = min(r.x, hi);
    return true;
}

// The front of one batch: lane l takes list entry idx = base + l (when idx < hi), tests its footprint against the wave's 8 x 8 block and
// the hits are compacted in list order into the wave's queue: record rows 0 and 1, the Gaussian id, the entry's position in the batch.
// Returns the number of hits.
__device__ __forceinline__ uint32_t lg_feat_front(const LgFeatView& v, uint32_t idx, uint32_t hi, float bx0, float by0, float4* q0, float4* q1,
                                                  uint32_t* qid, uint32_t* qpos, uint32_t lane)
{
    bool hit = false;
    float4 r0, r1;
    uint32_t id = 0;
    if (idx < hi) {
        id = (uint32_t)v.entries[idx] & v.gid_mask;
        if (id < (uint32_t)v.N) {
            r0 = v.rec[LG_REC_F4 * (size_t)id]; r1 = v.rec[LG_REC_F4 * (size_t)id + 1];
            const float4 r2 = v.rec[LG_REC_F4 * (size_t)id + 2];
            hit = lg_block_hit(r0, r1, r2, lg_reach(r0, r1, r2), bx0, by0);
        }
    }
    const uint64_t mask = __ballot(hit);
    if (mask == 0) return 0u;
    if (hit) {
        const uint32_t pos = prefix_popc(mask);
        q0[pos] = r0; q1[pos] = r1; qid[pos] = id; qpos[pos] = lane;
    }
    lg_wave_lds_sync();
    return (uint32_t)__popcll(mask);
}

// alpha of a (pixel, entry) pair as the forward evaluated it, and the exponential G it is made of (the geometry backward chains through
// it): lg_alpha_exact with its exp kept (canonical), or the forward's guarded hardware exp.
template <bool EXACT>
__device__ __forceinline__ float lg_feat_alpha(float op, float power, float& G)
{
    G = EXACT ? lg_exp(fminf(power, 0.0f)) : __expf(power);
    const float alpha = fminf(LG_ALPHA_MAX, op * G);
    return EXACT ? alpha : guard_alpha(alpha, op, power);
}

// The pre-sort slot of list entry idx, where its row goes; 0xFFFFFFFF (past every slot_cap) for !live and for an id that is not below N.
__device__ __forceinline__ uint32_t lg_feat_slot(const LgFeatView& v, const uint4* tinfo, uint32_t idx, bool live, int tx, int ty)
{
    uint32_t sl = 0xFFFFFFFFu;
    if (live) {
        const uint32_t id = (uint32_t)v.entries[idx] & v.gid_mask;
        if (id < (uint32_t)v.N) sl = lg_slot_of(tinfo[id], tx, ty);
    }
    return sl;
}

// The feature rows of a batch's nhit hits into the wave's frow: channels [c0, c0 + CG) of each hit, CG consecutive floats per hit
// (zeros past channel C), read as coalesced row segments.
template <int CG>
__device__ __forceinline__ void lg_feat_stage_rows(const float* features, int C, int c0, const uint32_t* qid, uint32_t nhit, float* frow,
                                                   uint32_t lane)
{
    for (uint32_t i = lane; i < nhit * CG; i += 64u) {
        const uint32_t j = i / CG, c = i % CG;
        frow[i] = (c0 + (int)c < C) ? features[(size_t)qid[j] * C + c0 + c] : 0.0f;
    }
    lg_wave_lds_sync();
}

// One (pixel, entry) step: power and alpha as the forward's pair step evaluates them (fwd_pair_m), then lg_feature_step.  Called by all
// 64 lanes (guard_alpha ballots); w = 0 unless the entry contributes to the pixel.
template <bool EXACT>
__device__ __forceinline__ int lg_feat_pair(const float4& a, const float4& b, bool done, float pxf, float pyf, float& T, float& w)
{
    float dx, dy, G;
    const float power = lg_rec_power(a, b, pxf, pyf, dx, dy);
    const float alpha = lg_feat_alpha<EXACT>(b.y, power, G);
    w = 0.0f;
    return done ? 0 : lg_feature_step(power, alpha, T, w);
}

// ------------------------------------------------------------------------------------------------
// forward: channels [c0, c0 + CG) of out[C][H][W] (those below C), and alpha[H][W] with the first group
template <int CG, bool EXACT>
__global__ void __launch_bounds__(256)
lg_features_fwd(LgFeatView v, int C, int c0, const float* __restrict__ features, const float* __restrict__ bg, float* __restrict__ out,
                float* __restrict__ alpha_out)
{
    static_assert(CG % 4 == 0, "feature rows are read as float4");
    __shared__ float4 q0[4][LG_Q], q1[4][LG_Q];
    __shared__ uint32_t qid[4][LG_Q], qpos[4][LG_Q];
    __shared__ __attribute__((aligned(16))) float frow[4][LG_Q * CG];
    const int tile = xcd_tile(blockIdx.x);
    if (tile >= v.ntiles) return;
    const int wave = threadIdx.x >> 6;
    const uint32_t lane = threadIdx.x & 63;
    const LgBlock g = lg_block(v.W, v.H, tile % v.gx, tile / v.gx, wave, lane);
    const float pxf = (float)g.pxi, pyf = (float)g.pyi;
    uint32_t lo, hi;
    (void)lg_feat_list(v, tile, lo, hi);        // an abandoned view has empty lists: background, alpha 0

    float T = 1.0f, A = 0.0f, F[CG];
#pragma unroll
    for (int c = 0; c < CG; c++) F[c] = 0.0f;
    bool done = !g.inside;
    for (uint32_t base = lo; base < hi; base += LG_Q) {
        if (__ballot(!done) == 0) break;        // every pixel of this wave is saturated or outside
        const uint32_t nhit = lg_feat_front(v, base + lane, hi, (float)g.wx0, (float)g.wy0, q0[wave], q1[wave], qid[wave], qpos[wave], lane);
        if (nhit == 0u) continue;
        lg_feat_stage_rows<CG>(features, C, c0, qid[wave], nhit, frow[wave], lane);
        for (uint32_t j = 0; j < nhit; j++) {
            const float4 a = q0[wave][j], b = q1[wave][j];
            float w;
            const int res = lg_feat_pair<EXACT>(a, b, done, pxf, pyf, T, w);
            done = done || res == 2;
            A = fmaf(1.0f, w, A);
            const float4* fr = reinterpret_cast<const float4*>(&frow[wave][j * CG]);
#pragma unroll
            for (int k = 0; k < CG / 4; k++) {
                const float4 f = fr[k];
                F[4 * k] = fmaf(f.x, w, F[4 * k]); F[4 * k + 1] = fmaf(f.y, w, F[4 * k + 1]);
                F[4 * k + 2] = fmaf(f.z, w, F[4 * k + 2]); F[4 * k + 3] = fmaf(f.w, w, F[4 * k + 3]);
            }
        }
        // release + barrier without the acquire (so not lg_wave_lds_sync): the LDS accesses above must be done first; no read below depends on them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();        // (the next batch overwrites the queue)
    }
    if (g.inside) {
        const size_t pid = (size_t)g.pyi * v.W + g.pxi, HW = (size_t)v.H * v.W;
#pragma unroll
        for (int c = 0; c < CG; c++)
            if (c0 + c < C) out[(size_t)(c0 + c) * HW + pid] = bg ? fmaf(T, bg[c0 + c], F[c]) : F[c];
        if (alpha_out && c0 == 0) alpha_out[pid] = A;
    }
}

// ------------------------------------------------------------------------------------------------
// backward
// lg_feat_reduce: K7's LDS wave reduction (wave_reduce_via_lds, lg_blend.h) for NV <= 16 values; total r of the entry is left at dst[r].
template <int NV>
__device__ __forceinline__ void lg_feat_reduce(const float (&p)[NV], float* red, float* dst, uint32_t lane)
{
    wave_reduce_via_lds<NV>(p, red, lane, [&](uint32_t r, float s) { dst[r] = s; });
}

// Channels [c0, c0 + NV) (those below c1) of the partial rows: rows[slot][CW], column (c0 - cb) + k, for every entry of every list.
// The four waves of a tile walk the list batch by batch TOGETHER (two workgroup barriers per batch, reached by every thread: the trip
// count is the tile's); a wave whose pixels are all saturated skips the batch's arithmetic, and the rows of entries nobody hit are zeros.
#define LG_FEAT_PART_STRIDE(NV) ((NV) + 1)
template <int NV, bool EXACT>
__global__ void __launch_bounds__(256)
lg_features_bwd(LgFeatView v, int c0, int c1, int cb, int CW, const uint4* __restrict__ tinfo, const float* __restrict__ dL_dout,
                float* __restrict__ rows)
{
    __shared__ float4 q0[4][LG_Q], q1[4][LG_Q];
    __shared__ uint32_t qid[4][LG_Q], qpos[4][LG_Q];
    __shared__ __attribute__((aligned(16))) float red[4][NV * LG_RED_STRIDE];
    __shared__ float part[4][LG_Q * LG_FEAT_PART_STRIDE(NV)];
    __shared__ uint32_t slot[LG_Q];
    __shared__ unsigned long long wmask[4];
    const int tile = xcd_tile(blockIdx.x);
    if (tile >= v.ntiles) return;
    const int wave = threadIdx.x >> 6;
    const uint32_t lane = threadIdx.x & 63;
    const int tx = tile % v.gx, ty = tile / v.gx;
    const LgBlock g = lg_block(v.W, v.H, tx, ty, wave, lane);
    const float pxf = (float)g.pxi, pyf = (float)g.pyi;
    uint32_t lo, hi;
    if (!lg_feat_list(v, tile, lo, hi) || lo == hi) return;      // workgroup-uniform
    const uint32_t slot_cap = min(v.counters[3], v.cap);         // (lo < hi: the view is live)

    float gv[NV];
    {
        const size_t pid = (size_t)g.pyi * v.W + g.pxi, HW = (size_t)v.H * v.W;
#pragma unroll
        for (int k = 0; k < NV; k++) gv[k] = (g.inside && c0 + k < c1) ? dL_dout[(size_t)(c0 + k) * HW + pid] : 0.0f;
    }
    float T = 1.0f;
    bool done = !g.inside;
    for (uint32_t base = lo; base < hi; base += LG_Q) {
        const uint32_t nbt = min((uint32_t)LG_Q, hi - base);
        if (wave == 0) slot[lane] = lg_feat_slot(v, tinfo, base + lane, lane < nbt, tx, ty);      // where the batch's rows go
        uint64_t hitmask = 0ull;                                  // entries of the batch this wave has a partial row for (scalar)
        if (__ballot(!done) != 0) {
            const uint32_t nhit = lg_feat_front(v, base + lane, hi, (float)g.wx0, (float)g.wy0, q0[wave], q1[wave], qid[wave], qpos[wave], lane);
            for (uint32_t j = 0; j < nhit; j++) {
                const float4 a = q0[wave][j], b = q1[wave][j];
                float w;
                const int res = lg_feat_pair<EXACT>(a, b, done, pxf, pyf, T, w);
                done = done || res == 2;
                if (__ballot(res == 1) == 0) continue;            // no pixel of the wave took the entry
                float p[NV];
#pragma unroll
                for (int k = 0; k < NV; k++) p[k] = w * gv[k];
                const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)qpos[wave][j]);
                lg_feat_reduce<NV>(p, red[wave], &part[wave][e * LG_FEAT_PART_STRIDE(NV)], lane);
                hitmask |= 1ull << e;
            }
        }
        if (lane == 0u) wmask[wave] = hitmask;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nbt * NV; i += 256u) {
            const uint32_t e = i / NV, k = i % NV;
            float s = 0.0f;
#pragma unroll
            for (int u = 0; u < 4; u++)
                if ((wmask[u] >> e) & 1ull) s += part[u][e * LG_FEAT_PART_STRIDE(NV) + k];
            const uint32_t sl = slot[e];
            if (sl < slot_cap && c0 + (int)k < c1) rows[(size_t)sl * CW + (c0 - cb) + k] = s;
        }
        __syncthreads();                                          // (the next batch overwrites the queue, the partials and the slots)
    }
}

// dF[i][cb .. cb + cw) = the sum of Gaussian i's rows (consecutive pre-sort slots offsets - touched .. offsets) in slot order; zeros
// for a Gaussian without instances and for a view that was abandoned.  A thread per (Gaussian, channel of the chunk).
__global__ void __launch_bounds__(256)
lg_features_gather(int N, int C, int cb, int cw, int live, uint32_t cap, const uint32_t* __restrict__ touched, const uint32_t* __restrict__ offsets,
                   const uint32_t* __restrict__ counters, const float* __restrict__ rows, float* __restrict__ dF)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)N * cw) return;
    const uint32_t i = (uint32_t)(t / (size_t)cw), k = (uint32_t)(t % (size_t)cw);
    uint32_t n = 0, base = 0;
    if (live && counters[0] == 0u) {
        const uint32_t R = min(counters[3], cap);
        n = touched[i]; base = offsets[i] - n;
        if (base >= R || n > R - base) n = 0;
    }
    float s = 0.0f;
    for (uint32_t j = 0; j < n; j++) s += rows[(size_t)(base + j) * cw + k];
    dF[(size_t)i * C + cb + k] = s;
}

// ------------------------------------------------------------------------------------------------
// backward with respect to the GEOMETRY: the six pixel-offset moments of a loss on out / alpha, added to (ACCUM) or written as (!ACCUM)
// the per-instance moment rows [R][12] that K7 (lg_blend_bwd) writes and K9 (lg_preprocess_bwd) sums and chains to every input.
// The moments are linear in the per-pixel loss gradient, so a colour loss (K7), CG channels of dL_dout per walk and dL_dalpha (with the
// walk of channel 0) meet in the same rows and K9 runs once.
//
// Walk: lg_features_bwd's -- a workgroup per tile, a wave per 8 x 8 block, the four waves take a batch of 64 entries together, hits
// through lg_feat_front -- but BACK TO FRONT: batches from the tile's last one down to its first, the hits of a batch from the last
// to the first.  Per pixel T starts at the colour forward's final_T and an entry counts when its list position is <= the pixel's
// n_contrib (img buffer), then lg_feature_bwd_step (lg_math.h) on the forward's own power / alpha.  Lists of any length are walked
// serially, no checkpoints are read; every loop is bounded by the tile's range clamped to counters[3], ids are checked against N,
// nothing spins or waits (two workgroup barriers per batch, reached by every thread: the trip count is the tile's).  A view the
// forward abandoned and a segment length other than the forward's (meta[2]) return at once: K9 refuses those too, the gradients are
// zero.  A wave none of whose pixels reached a batch skips its arithmetic; with ACCUM the batches behind the last one any pixel of the
// tile reached are not visited at all, without it they get their zero rows (K9 reads every row).
//
// Channels [c0, c0 + CG) (those below C): g_c in registers, the feature rows of a batch's hits staged through LDS as in lg_features_fwd,
// q = sum_c f_c g_c (+ dL_dalpha when c0 == 0).  Reduction: K7's discipline -- per hit entry lg_feat_reduce<6> over the wave's 64
// pixels, the four waves' partials meet in LDS, thread e of the workgroup owns entry e of the batch and updates columns 0..5 of its
// row at the pre-sort slot (lg_slot_of).  !ACCUM writes all 12 floats.  Walks are stream-ordered and a slot has one writer per walk:
// no float atomics, no memset, bit-identical run to run.
#define LG_FEAT_GEOM_NV 6
template <int CG, bool EXACT, bool ACCUM>
__global__ void __launch_bounds__(256)
lg_features_bwd_geom(LgFeatView v, uint32_t S, const uint32_t* __restrict__ meta, int C, int c0, const uint4* __restrict__ tinfo,
                     const float* __restrict__ features, const float* __restrict__ bg, const float* __restrict__ dL_dout,
                     const float* __restrict__ dL_dalpha, const float* __restrict__ final_T, const uint32_t* __restrict__ n_contrib,
                     float* __restrict__ rows)
{
    static_assert(CG % 4 == 0, "feature rows are read as float4");
    constexpr int NV = LG_FEAT_GEOM_NV;
    __shared__ float4 q0[4][LG_Q], q1[4][LG_Q];
    __shared__ uint32_t qid[4][LG_Q], qpos[4][LG_Q];
    __shared__ __attribute__((aligned(16))) float frow[4][LG_Q * CG];
    __shared__ __attribute__((aligned(16))) float red[4][NV * LG_RED_STRIDE];
    __shared__ float part[4][LG_Q * LG_FEAT_PART_STRIDE(NV)];
    __shared__ unsigned long long wmask[4];
    __shared__ uint32_t wlast[4];
    const int tile = xcd_tile(blockIdx.x);
    if (tile >= v.ntiles) return;
    const int wave = threadIdx.x >> 6;
    const uint32_t lane = threadIdx.x & 63;
    const int tx = tile % v.gx, ty = tile / v.gx;
    const LgBlock g = lg_block(v.W, v.H, tx, ty, wave, lane);
    const float pxf = (float)g.pxi, pyf = (float)g.pyi;
    uint32_t lo, hi;
    if (!lg_feat_list(v, tile, lo, hi) || lo == hi) return;      // workgroup-uniform
    if (meta[2] != S) return;                                    // (lo < hi: the view is live, the binning buffer is there)
    const uint32_t slot_cap = min(v.counters[3], v.cap);
    const uint32_t n_list = hi - lo;

    // per pixel: the gradient of this group of channels, the background term, the replay state
    float gv[CG];
    float gA = 0.0f, T = 0.0f, Tfb = 0.0f, Sb = 0.0f;
    uint32_t last = 0u;
    const bool have = dL_dout != nullptr;
    {
        const size_t pid = (size_t)g.pyi * v.W + g.pxi, HW = (size_t)v.H * v.W;
        float bgdot = 0.0f;
#pragma unroll
        for (int k = 0; k < CG; k++) {
            gv[k] = (have && g.inside && c0 + k < C) ? dL_dout[(size_t)(c0 + k) * HW + pid] : 0.0f;
            if (bg && c0 + k < C) bgdot = fmaf(bg[c0 + k], gv[k], bgdot);
        }
        if (g.inside) {
            T = final_T[pid];
            last = min(n_contrib[pid], n_list);
            if (dL_dalpha && c0 == 0) gA = dL_dalpha[pid];
        }
        Tfb = T * bgdot;
    }
    // the last list position any pixel of the wave / of the tile reached
    const uint32_t wl = (uint32_t)__builtin_amdgcn_readfirstlane((int)lg_wave_all_max(last));
    if (lane == 0u) wlast[wave] = wl;
    __syncthreads();
    const uint32_t tl = max(max(wlast[0], wlast[1]), max(wlast[2], wlast[3]));
    const uint32_t n_walk = ACCUM ? tl : n_list;                 // entries this walk visits
    if (n_walk == 0u) return;                                    // workgroup-uniform

    for (int k = (int)((n_walk - 1u) / LG_Q); k >= 0; k--) {
        const uint32_t rel0 = (uint32_t)k * LG_Q, base = lo + rel0;
        const uint32_t nbt = min((uint32_t)LG_Q, n_list - rel0);
        // thread e of the workgroup owns entry e of the batch: the pre-sort slot its row lives at
        const uint32_t sl = lg_feat_slot(v, tinfo, base + threadIdx.x, threadIdx.x < nbt, tx, ty);
        uint64_t hitmask = 0ull;                                  // entries of the batch this wave has a partial row for (scalar)
        if (wl > rel0) {
            const uint32_t nhit = lg_feat_front(v, base + lane, hi, (float)g.wx0, (float)g.wy0, q0[wave], q1[wave], qid[wave], qpos[wave], lane);
            if (have) lg_feat_stage_rows<CG>(features, C, c0, qid[wave], nhit, frow[wave], lane);
            for (int j = (int)nhit - 1; j >= 0; j--) {
                const float4 a = q0[wave][j], b = q1[wave][j];
                const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)qpos[wave][j]);
                float dx, dy;
                const float power = lg_rec_power(a, b, pxf, pyf, dx, dy);
                float G;
                const float alpha = lg_feat_alpha<EXACT>(b.y, power, G);
                float q = gA;
                if (have) {
                    const float4* fr = reinterpret_cast<const float4*>(&frow[wave][j * CG]);
#pragma unroll
                    for (int u = 0; u < CG / 4; u++) {
                        const float4 f = fr[u];
                        q = fmaf(f.x, gv[4 * u], q); q = fmaf(f.y, gv[4 * u + 1], q);
                        q = fmaf(f.z, gv[4 * u + 2], q); q = fmaf(f.w, gv[4 * u + 3], q);
                    }
                }
                float p[NV] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                float w;
                const bool ok = lg_feature_bwd_step<EXACT>(rel0 + e + 1u <= last, power, G, alpha, dx, dy, q, Tfb, T, Sb, p, w);
                if (__ballot(ok) == 0) continue;                  // no pixel of the wave took the entry
                lg_feat_reduce<NV>(p, red[wave], &part[wave][e * LG_FEAT_PART_STRIDE(NV)], lane);
                hitmask |= 1ull << e;
            }
        }
        if (lane == 0u) wmask[wave] = hitmask;
        __syncthreads();
        if (threadIdx.x < nbt && sl < slot_cap) {
            const uint32_t e = threadIdx.x;
            float s[NV] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int u = 0; u < 4; u++)
                if ((wmask[u] >> e) & 1ull) {
#pragma unroll
                    for (int r = 0; r < NV; r++) s[r] += part[u][e * LG_FEAT_PART_STRIDE(NV) + r];
                }
            float4* dst = reinterpret_cast<float4*>(rows) + 3 * (size_t)sl;
            if (ACCUM) {
                const float4 r0 = dst[0];
                const float2 r1 = *reinterpret_cast<const float2*>(dst + 1);
                dst[0] = make_float4(r0.x + s[0], r0.y + s[1], r0.z + s[2], r0.w + s[3]);
                *reinterpret_cast<float2*>(dst + 1) = make_float2(r1.x + s[4], r1.y + s[5]);
            } else {
                dst[0] = make_float4(s[0], s[1], s[2], s[3]);
                dst[1] = make_float4(s[4], s[5], 0.0f, 0.0f);
                dst[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        __syncthreads();                                          // (the next batch overwrites the queue, the partials and the masks)
    }
}

// Channels per chunk of the backward: the partial rows of a chunk, [num_rendered][cw] floats, stay within LG_FEAT_SCRATCH_BUDGET bytes
// where 16 channels do (the caller's scratch: lg_features_scratch_bytes).
#define LG_FEAT_SCRATCH_BUDGET ((size_t)1 << 30)
static inline int lg_features_chunk(int64_t R, int C)
{
    const size_t per = (size_t)(R > 0 ? R : 1) * sizeof(float);
    const size_t fit = LG_FEAT_SCRATCH_BUDGET / per / 16 * 16;
    return (int)std::min<size_t>((size_t)C, std::max<size_t>(16, fit));
}
