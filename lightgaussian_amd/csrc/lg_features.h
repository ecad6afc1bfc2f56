// lg_features.h -- blend C per-Gaussian feature channels over the sorted tile lists a forward left behind (lg_blend_features), and the
// gradient of that blend with respect to the features (lg_blend_features_backward): lg_features_fwd, lg_features_bwd, lg_features_gather.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
//
// The blending weights w = alpha T of a view are a function of what its forward leaves in the geom / binning buffers -- the 48-byte
// records, the sorted keys, the tile ranges, tinfo -- so any number of further channels is composited without K1, the scan, the
// duplication, the radix passes and the tile sort, and the gradient with respect to the channels, dF[j][c] = sum_pixels w[p][j] g[c][p],
// needs neither K7's back-to-front replay nor K9.
//
// Every kernel here and in lg_distortion.h walks the lists as K6 does -- a workgroup per 16 x 16 tile, a wave per 8 x 8 block, batches of
// LG_Q list entries, lg_block_hit against the wave's block, hits compacted in list order into the wave's LDS queue (LgFeatQueue: only the
// 32 bytes of record the pair step reads, next to the Gaussian id) -- with power and alpha exactly as the forward evaluated them
// (lg_feat_alpha): the include / exclude decisions are the forward's.  Lists of any length are walked serially (no checkpoints).  Nothing
// spins or waits; every loop is bounded by the tile's range clamped to the view's instance count (geom.counters, as every kernel behind
// K2), ids are checked against N.  A view the forward abandoned on the device has empty lists here: the image is the background, the
// gradient zero.  The back-to-front walk with its reduction into per-instance rows exists once (lg_feat_back_begin, lg_feat_walk_back): a
// kernel hands it its staging, its per-hit arithmetic and its sink.  The three front-to-back loops (lg_features_fwd, lg_features_bwd,
// lg_distortion_fwd) are short and stay with their kernels, on the shared steps lg_feat_front, _pair and _batch_end.
//
// The gradients keep K7's discipline -- no float atomics, no memset.  Per hit entry a wave reduces its 64 pixels' values through an LDS
// transpose (lg_feat_reduce: K7's wave_reduce_via_lds, lg_blend.h; entries no lane of the wave hit are skipped), the four waves' partials
// meet in LDS (LgFeatMerge) and one row per (tile, Gaussian) instance goes to the instance's pre-sort slot (lg_slot_of), written exactly
// once per walk, zeros included.  lg_features_gather adds every Gaussian's contiguous rows in slot order: bit-identical run to run.
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

// The hits of a batch, a queue per wave (one __shared__ LgFeatQueue per kernel): record rows 0 and 1, the Gaussian id, the entry's
// position in the batch.  A wave works on its own view of it.
struct LgFeatWaveQueue { float4 *q0, *q1; uint32_t *qid, *qpos; };
struct LgFeatQueue {
    float4 q0[4][LG_Q], q1[4][LG_Q];
    uint32_t qid[4][LG_Q], qpos[4][LG_Q];
    __device__ __forceinline__ LgFeatWaveQueue of(int wave) { return { q0[wave], q1[wave], qid[wave], qpos[wave] }; }
};

// The front of one batch: lane l takes list entry idx = base + l (when idx < hi), tests its footprint against the wave's 8 x 8 block and
// the hits are compacted in list order into the wave's queue.  Returns the number of hits.
__device__ __forceinline__ uint32_t lg_feat_front(const LgFeatView& v, uint32_t idx, uint32_t hi, const LgBlock& g, const LgFeatWaveQueue& q)
{
    bool hit = false;
    float4 r0, r1;
    uint32_t id = 0;
    if (idx < hi) {
        id = (uint32_t)v.entries[idx] & v.gid_mask;
        if (id < (uint32_t)v.N) {
            r0 = v.rec[LG_REC_F4 * (size_t)id]; r1 = v.rec[LG_REC_F4 * (size_t)id + 1];
            const float4 r2 = v.rec[LG_REC_F4 * (size_t)id + 2];
            hit = lg_block_hit(r0, r1, r2, lg_reach(r0, r1, r2), (float)g.wx0, (float)g.wy0);
        }
    }
    const uint64_t mask = __ballot(hit);
    if (mask == 0) return 0u;
    if (hit) {
        const uint32_t pos = prefix_popc(mask);
        q.q0[pos] = r0; q.q1[pos] = r1; q.qid[pos] = id; q.qpos[pos] = g.lane;
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

// The end of a batch in a front-to-back walk: release + barrier without the acquire (so not lg_wave_lds_sync) -- the LDS accesses of
// the batch must be done before the next one overwrites the queue; no read below depends on them.
__device__ __forceinline__ void lg_feat_batch_end()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------
// forward: channels [c0, c0 + CG) of out[C][H][W] (those below C), and alpha[H][W] with the first group.  The feature rows of a batch's
// hits are staged through LDS (coalesced row segments; the hits read them as broadcast ds_read_b128) and CG = 4 / 16 / 32 channels are
// carried per walk -- one walk up to 32 channels, two up to 64.  out_c = fma(T, bg_c, F_c).  alpha is accumulated as one more channel
// whose feature is 1 (sum of w): bit for bit the blend of a column of ones, equal to 1 - T up to rounding.
template <int CG, bool EXACT>
__global__ void __launch_bounds__(256)
lg_features_fwd(LgFeatView v, int C, int c0, const float* __restrict__ features, const float* __restrict__ bg, float* __restrict__ out,
                float* __restrict__ alpha_out)
{
    static_assert(CG % 4 == 0, "feature rows are read as float4");
    __shared__ LgFeatQueue queue;
    __shared__ __attribute__((aligned(16))) float frow[4][LG_Q * CG];
    const int tile = xcd_tile(blockIdx.x);
    if (tile >= v.ntiles) return;
    const int wave = threadIdx.x >> 6;
    const LgBlock g = lg_block(v.W, v.H, tile % v.gx, tile / v.gx, wave, threadIdx.x & 63);
    const LgFeatWaveQueue q = queue.of(wave);
    uint32_t lo, hi;
    (void)lg_feat_list(v, tile, lo, hi);        // an abandoned view has empty lists: background, alpha 0

    const float pxf = (float)g.pxi, pyf = (float)g.pyi;
    float T = 1.0f, A = 0.0f, F[CG];
#pragma unroll
    for (int c = 0; c < CG; c++) F[c] = 0.0f;
    bool done = !g.inside;
    for (uint32_t base = lo; base < hi; base += LG_Q) {
        if (__ballot(!done) == 0) break;        // every pixel of this wave is saturated or outside
        const uint32_t nhit = lg_feat_front(v, base + g.lane, hi, g, q);
        if (nhit == 0u) continue;
        lg_feat_stage_rows<CG>(features, C, c0, q.qid, nhit, frow[wave], g.lane);
        for (uint32_t j = 0; j < nhit; j++) {
            float w;
            const int res = lg_feat_pair<EXACT>(q.q0[j], q.q1[j], done, pxf, pyf, T, w);
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
        lg_feat_batch_end();
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

// Where the four waves of a workgroup meet per batch: a wave's reduction scratch, its partial row of NV totals per entry it has one for
// (part[wave][e * LG_FEAT_PART_STRIDE(NV) + r]) and the mask of those entries.  Three LDS arrays, declared by LG_FEAT_MERGE_LDS, and not
// one struct: the compiler places separate arrays as it always did, one object costs six lg_features_bwd_geom instances two VGPRs.
#define LG_FEAT_PART_STRIDE(NV) ((NV) + 1)
template <int NV>
struct LgFeatMerge { float (*red)[NV * LG_RED_STRIDE]; float (*part)[LG_Q * LG_FEAT_PART_STRIDE(NV)]; unsigned long long* wmask; };
#define LG_FEAT_MERGE_LDS(NV, mg) \
    __shared__ __attribute__((aligned(16))) float mg##_red[4][(NV) * LG_RED_STRIDE]; \
    __shared__ float mg##_part[4][LG_Q * LG_FEAT_PART_STRIDE(NV)]; \
    __shared__ unsigned long long mg##_wmask[4]; \
    const LgFeatMerge<NV> mg = { mg##_red, mg##_part, mg##_wmask }

// Channels [c0, c0 + NV) (those below c1) of the partial rows: rows[slot][CW], column (c0 - cb) + k, for every entry of every list:
// per hit entry a wave reduces w g[c] over its pixels, NV = 4 / 8 / 16 values.  The order is the forward's, but the four waves take every
// batch TOGETHER (two workgroup barriers per batch, reached by every thread: the trip count is the tile's), a wave whose pixels are all
// saturated only skips the batch's arithmetic, and a thread per (entry, value) merges -- zeros for entries nobody hit.
template <int NV, bool EXACT>
__global__ void __launch_bounds__(256)
lg_features_bwd(LgFeatView v, int c0, int c1, int cb, int CW, const uint4* __restrict__ tinfo, const float* __restrict__ dL_dout,
                float* __restrict__ rows)
{
    __shared__ LgFeatQueue queue;
    LG_FEAT_MERGE_LDS(NV, mg);
    __shared__ uint32_t slot[LG_Q];
    const int tile = xcd_tile(blockIdx.x);
    if (tile >= v.ntiles) return;
    const int wave = threadIdx.x >> 6, tx = tile % v.gx, ty = tile / v.gx;
    const uint32_t lane = threadIdx.x & 63;
    const LgBlock g = lg_block(v.W, v.H, tx, ty, wave, lane);
    const LgFeatWaveQueue q = queue.of(wave);
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
            const uint32_t nhit = lg_feat_front(v, base + lane, hi, g, q);
            for (uint32_t j = 0; j < nhit; j++) {
                float w;
                const int res = lg_feat_pair<EXACT>(q.q0[j], q.q1[j], done, pxf, pyf, T, w);
                done = done || res == 2;
                if (__ballot(res == 1) == 0) continue;            // no pixel of the wave took the entry
                float p[NV];
#pragma unroll
                for (int k = 0; k < NV; k++) p[k] = w * gv[k];
                const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.qpos[j]);
                lg_feat_reduce<NV>(p, mg.red[wave], &mg.part[wave][e * LG_FEAT_PART_STRIDE(NV)], lane);
                hitmask |= 1ull << e;
            }
        }
        if (lane == 0u) mg.wmask[wave] = hitmask;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nbt * NV; i += 256u) {
            const uint32_t e = i / NV, k = i % NV;
            float s = 0.0f;
#pragma unroll
            for (int u = 0; u < 4; u++)
                if ((mg.wmask[u] >> e) & 1ull) s += mg.part[u][e * LG_FEAT_PART_STRIDE(NV) + k];
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
// The BACK-TO-FRONT walk of a tile: the replay behind every gradient with respect to the geometry (lg_features_bwd_geom here,
// lg_distortion_bwd in lg_distortion.h).  The four waves take a batch of LG_Q entries together, from the tile's last batch down to its
// first, the hits of a batch from the last to the first.  Per pixel T starts at the colour forward's final_T, S at 0, and an entry is
// live when its list position is <= the pixel's n_contrib (img buffer); power, G and alpha are the forward's own.  Per hit entry NV
// values are reduced over the wave, the waves' partials meet in LDS and thread e of the workgroup owns entry e of the batch: its
// four-wave total (lg_feat_merge) and the pre-sort slot of its row.  Walks are stream-ordered and a slot has one writer per walk.  Two
// workgroup barriers per batch, reached by every thread (the trip count is the tile's): every return in front of them is
// workgroup-uniform.  A wave none of whose pixels reached a batch skips its arithmetic.
struct LgBackWalk {
    uint32_t lo, hi, n_list, slot_cap;          // the tile's entries [lo, hi), n_list of them; rows live at slots below slot_cap
    uint32_t last, wl; float T;                 // the last list position the pixel / any pixel of its wave reached; the pixel's final_T
};
// what the per-hit hook gets: hit j of the wave's queue at 1-based list position pos, live or not, the pair as the forward saw it
struct LgBackHit { uint32_t j, pos; bool live; float power, G, alpha, dx, dy; };

// False (workgroup-uniform, the kernel returns): the tile's list is empty, the forward abandoned the view, or the segment length is not
// the forward's (meta[2]: the binning buffer is laid out by it) -- K9 refuses those views too, the gradients are zero.
__device__ __forceinline__ bool lg_feat_back_begin(const LgFeatView& v, int tile, const LgBlock& g, uint32_t S, const uint32_t* meta,
                                                   const float* final_T, const uint32_t* n_contrib, LgBackWalk& bw)
{
    if (!lg_feat_list(v, tile, bw.lo, bw.hi) || bw.lo == bw.hi) return false;
    if (meta[2] != S) return false;             // (lo < hi: the view is live, the binning buffer is there)
    bw.slot_cap = min(v.counters[3], v.cap); bw.n_list = bw.hi - bw.lo;
    bw.T = 0.0f; bw.last = 0u;                  // (outside the image)
    if (g.inside) {
        const size_t pid = (size_t)g.pyi * v.W + g.pxi;
        bw.T = final_T[pid]; bw.last = min(n_contrib[pid], bw.n_list);
    }
    bw.wl = (uint32_t)__builtin_amdgcn_readfirstlane((int)lg_wave_all_max(bw.last));
    return true;
}

// the four-wave total t of entry e: waves 0..3 in this order, those that have a partial row for the entry
template <int NV>
__device__ __forceinline__ void lg_feat_merge(const LgFeatMerge<NV>& mg, uint32_t e, float (&t)[NV])
{
#pragma unroll
    for (int r = 0; r < NV; r++) t[r] = 0.0f;
#pragma unroll
    for (int u = 0; u < 4; u++)
        if ((mg.wmask[u] >> e) & 1ull) {
#pragma unroll
            for (int r = 0; r < NV; r++) t[r] += mg.part[u][e * LG_FEAT_PART_STRIDE(NV) + r];
        }
}

// The batches that hold the first n_walk entries of the list (workgroup-uniform), after lg_feat_back_begin.  Per batch a wave reached:
// stage(nhit) once (also for nhit == 0), then per hit, last to first, ok = hit(h, T, S, p) fills the pixel's p[NV] (zeros on entry)
// and advances T and S when the pixel takes the entry.  Per entry of every visited batch: sink(slot, t), t the merged totals -- zeros
// for an entry nobody took.
template <int NV, bool EXACT, typename Stage, typename Hit, typename Sink>
__device__ __forceinline__ void lg_feat_walk_back(const LgFeatView& v, int tile, const LgBlock& g, const uint4* tinfo, const LgBackWalk& bw,
                                                  uint32_t n_walk, const LgFeatWaveQueue& q, const LgFeatMerge<NV>& mg, Stage& stage, Hit& hit, Sink& sink)
{
    if (n_walk == 0u) return;
    const int tx = tile % v.gx, ty = tile / v.gx, wave = g.sub;
    const float pxf = (float)g.pxi, pyf = (float)g.pyi;
    float T = bw.T, Sb = 0.0f;
    for (int k = (int)((n_walk - 1u) / LG_Q); k >= 0; k--) {
        const uint32_t rel0 = (uint32_t)k * LG_Q, base = bw.lo + rel0;
        const uint32_t nbt = min((uint32_t)LG_Q, bw.n_list - rel0);
        const uint32_t sl = lg_feat_slot(v, tinfo, base + threadIdx.x, threadIdx.x < nbt, tx, ty);
        uint64_t hitmask = 0ull;                                  // entries of the batch this wave has a partial row for (scalar)
        if (bw.wl > rel0) {
            const uint32_t nhit = lg_feat_front(v, base + g.lane, bw.hi, g, q);
            stage(nhit);
            for (int j = (int)nhit - 1; j >= 0; j--) {
                const float4 a = q.q0[j], b = q.q1[j];
                const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.qpos[j]);
                LgBackHit h;
                h.j = (uint32_t)j; h.pos = rel0 + e + 1u; h.live = h.pos <= bw.last;
                h.power = lg_rec_power(a, b, pxf, pyf, h.dx, h.dy);
                h.alpha = lg_feat_alpha<EXACT>(b.y, h.power, h.G);
                float p[NV];
#pragma unroll
                for (int r = 0; r < NV; r++) p[r] = 0.0f;
                const bool ok = hit(h, T, Sb, p);
                if (__ballot(ok) == 0) continue;                  // no pixel of the wave took the entry
                lg_feat_reduce<NV>(p, mg.red[wave], &mg.part[wave][e * LG_FEAT_PART_STRIDE(NV)], g.lane);
                hitmask |= 1ull << e;
            }
        }
        if (g.lane == 0u) mg.wmask[wave] = hitmask;
        __syncthreads();
        if (threadIdx.x < nbt && sl < bw.slot_cap) {
            float t[NV];
            lg_feat_merge<NV>(mg, threadIdx.x, t);
            sink(sl, t);
        }
        __syncthreads();                                          // (the next batch overwrites the queue, the partials and the masks)
    }
}

// Columns 0..5 of the 12-float moment row at slot sl (K7's rows, lg_blend_bwd; K9 sums them): t[0..5] added (ACCUM) or the whole row
// written, zeros behind them (!ACCUM: the first walk into the rows when K7 did not run).
template <bool ACCUM>
__device__ __forceinline__ void lg_feat_store_moments(float* rows, uint32_t sl, const float* t)
{
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
}

// ------------------------------------------------------------------------------------------------
// backward with respect to the GEOMETRY: the six pixel-offset moments of a loss on out / alpha, added to (ACCUM) or written as (!ACCUM)
// the per-instance moment rows [R][12] that K7 (lg_blend_bwd) writes and K9 (lg_preprocess_bwd) sums and chains to every input.
// The moments are linear in the per-pixel loss gradient, so a colour loss (K7), CG channels of dL_dout per walk and dL_dalpha (with the
// walk of channel 0) meet in the same rows and K9 runs once.
//
// Channels [c0, c0 + CG) (those below C): g_c in registers, the feature rows of a batch's hits staged through LDS as in lg_features_fwd,
// q = sum_c f_c g_c (+ dL_dalpha when c0 == 0), then lg_feature_bwd_step (lg_math.h).  With ACCUM the batches behind the last one any
// pixel of the tile reached are not visited at all; without it they get their zero rows (K9 reads every row).
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
    __shared__ LgFeatQueue queue;
    __shared__ __attribute__((aligned(16))) float frow[4][LG_Q * CG];
    LG_FEAT_MERGE_LDS(NV, mg);
    __shared__ uint32_t wlast[4];
    const int tile = xcd_tile(blockIdx.x);
    if (tile >= v.ntiles) return;
    const int wave = threadIdx.x >> 6;
    const LgBlock g = lg_block(v.W, v.H, tile % v.gx, tile / v.gx, wave, threadIdx.x & 63);
    const LgFeatWaveQueue q = queue.of(wave);
    LgBackWalk bw;
    if (!lg_feat_back_begin(v, tile, g, S, meta, final_T, n_contrib, bw)) return;

    // per pixel: the gradient of this group of channels, the background term
    float gv[CG], gA = 0.0f, bgdot = 0.0f;
    const bool have = dL_dout != nullptr;
    const size_t pid = (size_t)g.pyi * v.W + g.pxi, HW = (size_t)v.H * v.W;
#pragma unroll
    for (int k = 0; k < CG; k++) {
        gv[k] = (have && g.inside && c0 + k < C) ? dL_dout[(size_t)(c0 + k) * HW + pid] : 0.0f;
        if (bg && c0 + k < C) bgdot = fmaf(bg[c0 + k], gv[k], bgdot);
    }
    if (g.inside && dL_dalpha && c0 == 0) gA = dL_dalpha[pid];
    const float Tfb = bw.T * bgdot;
    // the last list position any pixel of the tile reached
    if (g.lane == 0u) wlast[wave] = bw.wl;
    __syncthreads();
    const uint32_t tl = max(max(wlast[0], wlast[1]), max(wlast[2], wlast[3]));

    auto stage = [&](uint32_t nhit) { if (have) lg_feat_stage_rows<CG>(features, C, c0, q.qid, nhit, frow[wave], g.lane); };
    auto hit = [&](const LgBackHit& h, float& T, float& Sb, float (&p)[NV]) {
        float qf = gA;
        if (have) {
            const float4* fr = reinterpret_cast<const float4*>(&frow[wave][h.j * CG]);
#pragma unroll
            for (int u = 0; u < CG / 4; u++) {
                const float4 f = fr[u];
                qf = fmaf(f.x, gv[4 * u], qf); qf = fmaf(f.y, gv[4 * u + 1], qf);
                qf = fmaf(f.z, gv[4 * u + 2], qf); qf = fmaf(f.w, gv[4 * u + 3], qf);
            }
        }
        float w;
        return lg_feature_bwd_step<EXACT>(h.live, h.power, h.G, h.alpha, h.dx, h.dy, qf, Tfb, T, Sb, p, w);
    };
    auto sink = [&](uint32_t sl, const float (&t)[NV]) { lg_feat_store_moments<ACCUM>(rows, sl, t); };
    lg_feat_walk_back<NV, EXACT>(v, tile, g, tinfo, bw, ACCUM ? tl : bw.n_list, q, mg, stage, hit, sink);
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
