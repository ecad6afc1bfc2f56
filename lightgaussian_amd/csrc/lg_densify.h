// lg_densify.h -- densification on the device: the per-iteration view statistics and the clone / split / prune
// of GaussianModel.densify_and_prune as one plan and one row-writing launch.
// Replaces (reference): add_densification_stats + the trainer's max_radii2D statement (scene/gaussian_model.py:784-788,
// train_densify_prune.py:172-177: four boolean-mask statements, each a nonzero() + host sync) and densify_and_prune (:602-761: two
// cat_tensors_to_optimizer, two prune_points, build_rotation + bmm, a repeat of every parameter -- the model rewritten three times).
//
//   lg_densify_stats_kernel   one lane per row: accum += |grad.xy|, denom += 1, max_radii2D = max(., radii) where the filter is set.
//   lg_densify_classify       one streaming pass over _scaling, _opacity, accum, denom: a flag byte per row (keep | clone | split |
//                             child kept) and four counts per 1024 rows.  exp and sigmoid in K1's LG_FLAG_RAW_PARAMS forms
//                             (expf, 1 / (1 + expf(-x))): bit-equal to torch on this GPU, so the decisions are torch's.
//   lg_densify_scan           one workgroup: exclusive scan of the four counts, the device record {N_out, n_keep, n_clone, n_s, n_child}.
//   lg_densify_map            per output row {source row, kind << 30 | rank k of the parent among ALL split-selected rows}.
//                             Output order: kept originals, kept clones, first children, second children -- each in source order.
//   lg_densify_move           grid.y = tensor: every output word of every tensor from the map.  Parameters gathered, moments
//                             gathered for kept rows and zero for new ones, bookkeeping zero, _xyz / _scaling of children computed
//                             (lg_math.h: lg_densify_child_xyz / lg_densify_child_scaling) from the parent's raw rows and the noise.
// wave64, plain vector stores, no atomics, no scratch memory; word offsets are 64-bit.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include "lg_host.h"
#include "lg_wave.h"

#define LG_DENSIFY_ROWS 1024           // rows per workgroup of the plan kernels (256 threads x 4)
// flag byte of a row
#define LG_DF_KEEP 1u                  // the original stays: not split-selected and passes the prune test
#define LG_DF_CLONE 2u                 // clone-selected and passes the prune test: one bit-for-bit copy
#define LG_DF_SPLIT 4u                 // split-selected: takes rank k and noise rows k, n_s + k whether its children stay or not
#define LG_DF_CHILD 8u                 // split-selected and its children pass the prune test (parent's opacity, max scale / 1.6)
// kind of an output row (top two bits of the map's second word)
#define LG_DK_KEEP 0u
#define LG_DK_CLONE 1u
#define LG_DK_CHILD_A 2u
#define LG_DK_CHILD_B 3u
#define LG_DENSIFY_RANK_MASK 0x3FFFFFFFu

struct LgDensifyThresholds {
    float thr_g, thr_d, thr_w, min_opacity;     // each evaluated in double on the host and rounded once
    int use_extent;                             // max_screen_size truthy: the world-space size test applies
};

__global__ void __launch_bounds__(256)
lg_densify_stats_kernel(int N, const float* __restrict__ grad, const uint8_t* __restrict__ filter, const int32_t* __restrict__ radii,
                        float* __restrict__ max_radii, float* __restrict__ accum, float* __restrict__ denom)
{
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= N || !filter[i]) return;
    const float gx = grad[3 * (size_t)i], gy = grad[3 * (size_t)i + 1];
    accum[i] = accum[i] + sqrtf(fmaf(gy, gy, gx * gx));       // one explicit fmaf: the two-term sum of squares with a single rounding
    denom[i] = denom[i] + 1.0f;
    if (radii) {
        const float r = (float)radii[i], m = max_radii[i];
        max_radii[i] = r > m ? r : m;
    }
}

__device__ __forceinline__ bool lg_densify_pruned(float sigma, float mu, const LgDensifyThresholds& th)
{
    return sigma < th.min_opacity || (th.use_extent && mu > th.thr_w);
}

__global__ void __launch_bounds__(256)
lg_densify_classify(int N, const float* __restrict__ scaling, const float* __restrict__ opacity, const float* __restrict__ accum,
                    const float* __restrict__ denom, const LgDensifyThresholds th, uint8_t* __restrict__ flags, uint4* __restrict__ blk_sum)
{
    __shared__ uint32_t ws[4][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = blockIdx.x * LG_DENSIFY_ROWS + k * 256 + (int)threadIdx.x;     // lanes on consecutive rows: coalesced
        uint32_t f = 0;
        if (i < N) {
            const float s0 = expf(scaling[3 * (size_t)i]), s1 = expf(scaling[3 * (size_t)i + 1]), s2 = expf(scaling[3 * (size_t)i + 2]);
            const float m = fmaxf(fmaxf(s0, s1), s2);
            const float op = opacity[i];
            const float sigma = 1.0f / (1.0f + expf(-op));
            float g = accum[i] / denom[i];
            if (g != g) g = 0.0f;                                   // grads[grads.isnan()] = 0
            const bool hot = g >= th.thr_g;
            const bool big = m > th.thr_d, small = m <= th.thr_d;
            const bool pass = !lg_densify_pruned(sigma, m, th);
            if (hot && big) {
                f = LG_DF_SPLIT | (lg_densify_pruned(sigma, m / LG_DENSIFY_SHRINK, th) ? 0u : LG_DF_CHILD);
            } else {
                f = (pass ? LG_DF_KEEP : 0u) | (hot && small && pass ? LG_DF_CLONE : 0u);
            }
            flags[i] = (uint8_t)f;
        }
        c0 += (uint32_t)__popcll(__ballot(f & LG_DF_KEEP));
        c1 += (uint32_t)__popcll(__ballot(f & LG_DF_CLONE));
        c2 += (uint32_t)__popcll(__ballot(f & LG_DF_SPLIT));
        c3 += (uint32_t)__popcll(__ballot(f & LG_DF_CHILD));
    }
    if (lane == 0u) { ws[wave][0] = c0; ws[wave][1] = c1; ws[wave][2] = c2; ws[wave][3] = c3; }
    __syncthreads();
    if (threadIdx.x == 0)
        blk_sum[blockIdx.x] = make_uint4(ws[0][0] + ws[1][0] + ws[2][0] + ws[3][0], ws[0][1] + ws[1][1] + ws[2][1] + ws[3][1],
                                         ws[0][2] + ws[1][2] + ws[2][2] + ws[3][2], ws[0][3] + ws[1][3] + ws[2][3] + ws[3][3]);
}

// exclusive scan of n uint4 (four independent channels) by one workgroup; the record from the four totals
__global__ void __launch_bounds__(1024)
lg_densify_scan(int n, const uint4* __restrict__ in, uint4* __restrict__ out, int32_t* __restrict__ record)
{
    __shared__ uint32_t wsum[16][4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry[4] = { 0, 0, 0, 0 };
    for (int base = 0; base < n; base += 1024) {
        const int i = base + (int)tid;
        const uint4 v4 = i < n ? in[i] : make_uint4(0, 0, 0, 0);
        const uint32_t v[4] = { v4.x, v4.y, v4.z, v4.w };
        const uint32_t x[4] = { lg_wave_scan_incl(v4.x, lane), lg_wave_scan_incl(v4.y, lane), lg_wave_scan_incl(v4.z, lane), lg_wave_scan_incl(v4.w, lane) };
        if (lane == 63u) { wsum[wave][0] = x[0]; wsum[wave][1] = x[1]; wsum[wave][2] = x[2]; wsum[wave][3] = x[3]; }
        __syncthreads();
        uint32_t r[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            uint32_t woff = 0, tot = 0;
#pragma unroll                                                      // (written out: a strided lg_block_scan_get changes the kernel's VGPR figure)
            for (int w = 0; w < 16; w++) {
                const uint32_t t = wsum[w][c];
                woff += (w < (int)wave) ? t : 0u;
                tot += t;
            }
            r[c] = carry[c] + woff + x[c] - v[c];
            carry[c] += tot;
        }
        if (i < n) out[i] = make_uint4(r[0], r[1], r[2], r[3]);
        __syncthreads();
    }
    if (tid == 0) {
        record[0] = (int32_t)(carry[0] + carry[1] + 2u * carry[3]);    // N_out  (< 2^31: N < 2^30 and a row yields at most two)
        record[1] = (int32_t)carry[0];                                  // n_keep
        record[2] = (int32_t)carry[1];                                  // n_clone
        record[3] = (int32_t)carry[2];                                  // n_s: split-selected parents, kept or not
        record[4] = (int32_t)carry[3];                                  // n_child: parents whose children stay
        record[5] = record[6] = record[7] = 0;
    }
}

__global__ void __launch_bounds__(256)
lg_densify_map(int N, const uint8_t* __restrict__ flags, const uint4* __restrict__ blk_off, const int32_t* __restrict__ record,
               uint2* __restrict__ map)
{
    __shared__ uint32_t ws[4][2];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * LG_DENSIFY_ROWS + (int)threadIdx.x * 4;
    uint32_t f4[4];
    uint32_t a = 0, b = 0;               // keep | clone << 16,  split | child << 16  (a workgroup holds at most 1024 of each)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        f4[k] = r0 + k < N ? (uint32_t)flags[r0 + k] : 0u;
        a += (f4[k] & LG_DF_KEEP ? 1u : 0u) + (f4[k] & LG_DF_CLONE ? 0x10000u : 0u);
        b += (f4[k] & LG_DF_SPLIT ? 1u : 0u) + (f4[k] & LG_DF_CHILD ? 0x10000u : 0u);
    }
    const uint32_t ia = lg_wave_scan_incl(a, lane), ib = lg_wave_scan_incl(b, lane);
    if (lane == 63u) { ws[wave][0] = ia; ws[wave][1] = ib; }
    __syncthreads();
    uint32_t ea = ia - a, eb = ib - b;
    for (uint32_t w = 0; w < wave; w++) { ea += ws[w][0]; eb += ws[w][1]; }
    const uint4 off = blk_off[blockIdx.x];
    const uint32_t n_keep = (uint32_t)record[1], n_clone = (uint32_t)record[2], n_child = (uint32_t)record[4];
    uint32_t p_keep = off.x + (ea & 0xFFFFu), p_clone = n_keep + off.y + (ea >> 16);
    uint32_t rank = off.z + (eb & 0xFFFFu), p_child = n_keep + n_clone + off.w + (eb >> 16);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t f = f4[k], row = (uint32_t)(r0 + k);
        if (f & LG_DF_KEEP) map[p_keep++] = make_uint2(row, LG_DK_KEEP << 30);
        if (f & LG_DF_CLONE) map[p_clone++] = make_uint2(row, LG_DK_CLONE << 30);
        if (f & LG_DF_CHILD) {
            map[p_child] = make_uint2(row, (LG_DK_CHILD_A << 30) | rank);
            map[(size_t)p_child + n_child] = make_uint2(row, (LG_DK_CHILD_B << 30) | rank);
            p_child++;
        }
        if (f & LG_DF_SPLIT) rank++;
    }
}

// every output word of every tensor.  Tensor t: rows of words[t] 32-bit words, contiguous; role[t] says what a new row gets.
struct LgDensifyArgs {
    const uint32_t* src[LG_DENSIFY_MAX_TENSORS];
    uint32_t* dst[LG_DENSIFY_MAX_TENSORS];
    uint32_t words[LG_DENSIFY_MAX_TENSORS];
    uint32_t role[LG_DENSIFY_MAX_TENSORS];
};
__global__ void __launch_bounds__(256)
lg_densify_move(int64_t n_out_host, const uint2* __restrict__ map, const int32_t* __restrict__ record, const LgDensifyArgs a,
                const float* __restrict__ rotation, const float* __restrict__ scaling, const float* __restrict__ noise, int64_t noise_rows)
{
    const uint32_t t = blockIdx.y;
    const uint32_t wpr = a.words[t], role = a.role[t];
    const uint32_t* __restrict__ src = a.src[t];
    uint32_t* __restrict__ dst = a.dst[t];
    const int64_t n_dev = record[0];
    const size_t n_out = (size_t)(n_out_host < n_dev ? n_out_host : n_dev);      // never beyond what the plan mapped
    const size_t n_s = (size_t)record[3];
    const size_t total = n_out * wpr;
    const bool narrow = total <= 0xFFFFFFFFull;                                  // (uniform) 32-bit division where it suffices
    for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < total; w += (size_t)gridDim.x * 256) {
        if (role == LG_DENSIFY_ZERO) { dst[w] = 0u; continue; }
        const size_t row = narrow ? (size_t)((uint32_t)w / wpr) : w / wpr;
        const uint32_t col = (uint32_t)(w - row * wpr);
        const uint2 e = map[row];
        const uint32_t kind = e.y >> 30;
        const size_t parent = e.x;
        uint32_t v = 0u;
        if (role != LG_DENSIFY_MOMENT || kind == LG_DK_KEEP) v = src[parent * wpr + col];
        if (kind >= LG_DK_CHILD_A) {
            if (role == LG_DENSIFY_SCALING) {
                v = lg_f2bits(lg_densify_child_scaling(expf(lg_bits2f(v))));
            } else if (role == LG_DENSIFY_XYZ) {
                const size_t nrow = (size_t)(e.y & LG_DENSIFY_RANK_MASK) + (kind == LG_DK_CHILD_B ? n_s : 0);
                if (nrow < (size_t)noise_rows) {                                 // (a short noise tensor is never read past its end)
                    const float* q = rotation + 4 * parent;
                    const float* sr = scaling + 3 * parent;
                    const float* z = noise + 3 * nrow;
                    const float* x = (const float*)src + 3 * parent;
                    const float qq[4] = { q[0], q[1], q[2], q[3] }, s[3] = { expf(sr[0]), expf(sr[1]), expf(sr[2]) };
                    const float zz[3] = { z[0], z[1], z[2] }, xx[3] = { x[0], x[1], x[2] };
                    float o[3];
                    lg_densify_child_xyz(qq, s, zz, xx, o);
                    v = lg_f2bits(col == 0 ? o[0] : (col == 1 ? o[1] : o[2]));
                }
            }
        }
        dst[w] = v;
    }
}
