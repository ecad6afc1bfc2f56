// lg_vq_train.h -- one training step of the VecTree quantiser's Euclidean codebook: the importance-weighted EMA k-means
// update of vectree/vq.py:262-299 (EuclideanCodebook.forward in training mode, temperature 0, no DDP, no code expiry) behind
// the nearest-code search of lg_vq.h.
//
// The reference forms F.one_hot(embed_ind, K) -- an n x K matrix with one 1 per row -- and gets the per-code weighted sums
// from a dense n x K x d GEMM against it.  Here the sums are a segmented reduction over an INVERTED INDEX (per code, the list
// of its rows in ascending row order), without float atomics and without any n x K intermediate:
//
//   lg_vq_keys        key[i] = (code[i] << 32) | i; the same pass leaves the first level of the fixed-order sum of `weight`
//                     (one partial per LG_VQ_WSUM_TILE rows)
//   lg_sort_keys      the stable radix sort of lg_sort.h on the code bits alone: keys grouped by code, rows ascending
//   lg_vq_starts      start[c] = first sorted position of code c (boundary pass over the sorted keys; start[K] = n)
//   lg_vq_chunk_scan  one workgroup: chunk_off = exclusive scan over the codes of ceil(m_c / LG_VQ_SUM_CHUNK), and the second
//                     level of the weight sum
//   lg_vq_chunk_sum   one wave per chunk of at most LG_VQ_SUM_CHUNK consecutive rows of ONE list, one lane per dimension
//                     (lane d carries the weight itself): a sequential sum in row order -> partial[chunk][0..d]
//   lg_vq_combine     per (code, dimension): the partials of the code's chunks added in chunk order; the EMA of cluster_size
//   lg_vq_size_sum    one workgroup: fixed-order sum of the updated cluster_size
//   lg_vq_epilogue    Laplace smoothing and the EMA of embed, in place
//
// Summation order: a code's rows are added in ascending row index inside chunks of LG_VQ_SUM_CHUNK rows, the
// chunk sums are then added in chunk order -- fixed by (n, K, ind) alone, whatever the grid or the hardware's scheduling.
// The arithmetic is the one written down (the library is built with -ffp-contract=off and correctly rounded division).
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include "lg_host.h"
#include "lg_sort.h"
#include "lg_vq.h"

#define LG_VQ_SUM_CHUNK 256     // rows per chunk of a code's list: a compile-time constant, so that the order of every addition is too
#define LG_VQ_WSUM_TILE 4096    // rows per first-level partial of the weight sum
#define LG_VQ_RED_THREADS 1024  // the single-workgroup kernels

struct VqEmaView {
    float* cbA;            // augmented codebook of the search (lg_vq_prepare)
    uint64_t* keys_in;     // [n] (code << 32) | row
    uint64_t* keys_out;    // [n] the same, grouped by code
    void* sort_temp; size_t sort_temp_bytes;
    uint32_t* start;       // [K + 1] first sorted position of every code's list
    uint32_t* chunk_off;   // [K + 1] first chunk of every code
    float* partial;        // [max_chunks][d + 1]
    float* esum;           // [K][d + 1] weighted row sum per code; column d = weighted row count
    float* wpart;          // [ceil(n / LG_VQ_WSUM_TILE)]
    float* scal;           // [0] sum of weight, [1] sum of the updated cluster_size
    size_t max_chunks, total;
};
static VqEmaView carve_vq_ema(void* base, size_t n, size_t K, size_t d)
{
    VqEmaView v{};
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
    if (n == 0) n = 1;
    v.cbA = (float*)take((size_t)lg_vq_kpad((int)K) * 2 * lg_vq_dk2((int)d) * sizeof(float));
    v.keys_in = (uint64_t*)take(n * 8);
    v.keys_out = (uint64_t*)take(n * 8);
    v.sort_temp_bytes = lg_sort_layout(n).total;
    v.sort_temp = take(v.sort_temp_bytes);
    v.start = (uint32_t*)take((K + 1) * 4);
    v.chunk_off = (uint32_t*)take((K + 1) * 4);
    v.max_chunks = n / LG_VQ_SUM_CHUNK + std::min(n, K);      // a code with m >= 1 rows has at most m / CHUNK + 1 chunks
    v.partial = (float*)take(v.max_chunks * (d + 1) * 4);
    v.esum = (float*)take(K * (d + 1) * 4);
    v.wpart = (float*)take((n + LG_VQ_WSUM_TILE - 1) / LG_VQ_WSUM_TILE * 4);
    v.scal = (float*)take(64);
    v.total = off;
    return v;
}

// Sum of one value per thread over a workgroup of LG_VQ_RED_THREADS: a binary tree through LDS, the same tree every time.
__device__ __forceinline__ float lg_vq_block_sum(float v, float* sh)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t s = LG_VQ_RED_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// keys + first level of the weight sum.  Workgroup b owns rows [b * TILE, (b + 1) * TILE): thread t adds its rows t, t + 256, ...
// in that order, then the 256 values go through a fixed LDS tree.  A code index outside [0, K) (the search of a row of NaNs) is
// clamped: every list stays inside the codebook.
__global__ void __launch_bounds__(256)
lg_vq_keys(uint32_t n, uint32_t K, const int32_t* __restrict__ ind, const float* __restrict__ weight, uint64_t* __restrict__ keys,
           float* __restrict__ wpart)
{
    __shared__ float sh[256];
    const uint32_t t = threadIdx.x;
    const uint32_t b0 = blockIdx.x * LG_VQ_WSUM_TILE;
    float acc = 0.0f;
    for (uint32_t k = t; k < LG_VQ_WSUM_TILE; k += 256) {
        const uint32_t i = b0 + k;
        if (i < n) {
            const uint32_t c = min((uint32_t)max(ind[i], 0), K - 1u);
            keys[i] = ((uint64_t)c << 32) | i;
            if (weight) acc = acc + weight[i];
        }
    }
    if (!weight) return;
    sh[t] = acc;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    if (t == 0) wpart[blockIdx.x] = sh[0];
}

// start[c] = number of sorted keys whose code is below c.  The thread at the first key of a code's run writes the entry of
// that code and of the empty codes in front of it; the thread at the last key writes the tail (start[K] = n).
__global__ void __launch_bounds__(256)
lg_vq_starts(uint32_t n, uint32_t K, const uint64_t* __restrict__ sorted, uint32_t* __restrict__ start)
{
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int c = (int)(sorted[q] >> 32);
    const int prev = q > 0 ? (int)(sorted[q - 1] >> 32) : -1;
    for (int e = prev + 1; e <= c; e++) start[e] = q;
    if (q == n - 1)
        for (int e = c + 1; e <= (int)K; e++) start[e] = n;
}

// One workgroup.  chunk_off[c] = sum over c' < c of ceil(m_c' / CHUNK), chunk_off[K] = number of chunks; scal[0] = sum of the
// first-level weight partials (thread t adds partials t, t + 1024, ... in order, then the fixed tree).
__global__ void __launch_bounds__(LG_VQ_RED_THREADS)
lg_vq_chunk_scan(uint32_t K, const uint32_t* __restrict__ start, uint32_t* __restrict__ chunk_off, uint32_t nwpart,
                 const float* __restrict__ wpart, float* __restrict__ scal)
{
    __shared__ uint32_t sc[LG_VQ_RED_THREADS];
    __shared__ float sh[LG_VQ_RED_THREADS];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < K; c0 += LG_VQ_RED_THREADS) {
        const uint32_t c = c0 + t;
        const uint32_t cnt = c < K ? (start[c + 1] - start[c] + LG_VQ_SUM_CHUNK - 1) / LG_VQ_SUM_CHUNK : 0u;
        sc[t] = cnt;
        __syncthreads();
        for (uint32_t s = 1; s < LG_VQ_RED_THREADS; s <<= 1) {
            const uint32_t add = t >= s ? sc[t - s] : 0u;
            __syncthreads();
            sc[t] += add;
            __syncthreads();
        }
        if (c < K) chunk_off[c] = carry + sc[t] - cnt;
        carry += sc[LG_VQ_RED_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) chunk_off[K] = carry;
    if (wpart) {
        float acc = 0.0f;
        for (uint32_t k = t; k < nwpart; k += LG_VQ_RED_THREADS) acc = acc + wpart[k];
        const float s = lg_vq_block_sum(acc, sh);
        if (t == 0) scal[0] = s;
    }
}

// One wave per chunk, lane j < d = dimension j of the rows, lane d = their weight.  Rows in sorted (= ascending row) order,
// acc = acc + fl(x * w) one row after the other; eight rows are loaded ahead of the adds that consume them.
// w = fl(fl(weight * n) / sum weight) -- vq.py:264 -- or 1 without a weight.
template <bool WEIGHTED>
__global__ void __launch_bounds__(256)
lg_vq_chunk_sum(uint32_t n, int d, uint32_t K, const float* __restrict__ x, const float* __restrict__ weight, const float* __restrict__ scal,
                const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ start, const uint32_t* __restrict__ chunk_off,
                float* __restrict__ partial)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= chunk_off[K]) return;
    uint32_t lo = 0, hi = K;                                   // chunk_off[lo] <= g < chunk_off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (chunk_off[mid] <= g) lo = mid; else hi = mid;
    }
    const uint32_t c = lo;
    const uint32_t b = start[c] + (g - chunk_off[c]) * LG_VQ_SUM_CHUNK;
    const uint32_t e = min(b + LG_VQ_SUM_CHUNK, start[c + 1]);
    const bool dim = (int)lane < d;
    const float nf = (float)n;
    const float wsum = WEIGHTED ? scal[0] : 1.0f;
    float acc = 0.0f;
    for (uint32_t q = b; q < e; q += 8) {
        float xv[8], wv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            xv[u] = 1.0f; wv[u] = 1.0f;
            if (q + u < e) {
                const uint32_t r = (uint32_t)sorted[q + u];
                if (WEIGHTED) wv[u] = weight[r];
                if (dim) xv[u] = x[(size_t)r * d + lane];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (q + u < e) {
                float term = xv[u];
                if (WEIGHTED) {
                    const float w = (wv[u] * nf) / wsum;
                    term = dim ? xv[u] * w : w;
                }
                acc = acc + term;
            }
        }
    }
    if ((int)lane <= d) partial[(size_t)g * (d + 1) + lane] = acc;
}

// Thread (c, j): esum[c][j] = the partials of code c's chunks added in chunk order (0 for a code without rows).  Column d is the
// weighted row count: cluster_size[c] <- decay * cluster_size[c] + (1 - decay) * count.  sort_err != 0 (the radix sort's
// look-back gave up; never seen, see lg_sort.h) poisons cluster_size with NaN, which the smoothing carries into every row of
// embed: a void step cannot pass for a good one.
__global__ void __launch_bounds__(256)
lg_vq_combine(uint32_t K, int d, const uint32_t* __restrict__ chunk_off, const float* __restrict__ partial, float* __restrict__ esum,
              float* __restrict__ cluster_size, float decay, float one_minus_decay, const uint32_t* __restrict__ sort_err)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t w = (uint32_t)d + 1u;
    if (idx >= (size_t)K * w) return;
    const uint32_t c = (uint32_t)(idx / w), j = (uint32_t)(idx % w);
    const uint32_t g0 = chunk_off[c], g1 = chunk_off[c + 1];
    float acc = 0.0f;
    for (uint32_t g = g0; g < g1; g++) acc = g == g0 ? partial[(size_t)g * w + j] : acc + partial[(size_t)g * w + j];
    esum[idx] = acc;
    if (j == (uint32_t)d) {
        const float cs = decay * cluster_size[c] + one_minus_decay * acc;
        cluster_size[c] = *sort_err ? __builtin_nanf("") : cs;
    }
}

// One workgroup: scal[1] = sum of cluster_size (thread t adds codes t, t + 1024, ... in order, then the fixed tree).
__global__ void __launch_bounds__(LG_VQ_RED_THREADS)
lg_vq_size_sum(uint32_t K, const float* __restrict__ cluster_size, float* __restrict__ scal)
{
    __shared__ float sh[LG_VQ_RED_THREADS];
    float acc = 0.0f;
    for (uint32_t c = threadIdx.x; c < K; c += LG_VQ_RED_THREADS) acc = acc + cluster_size[c];
    const float s = lg_vq_block_sum(acc, sh);
    if (threadIdx.x == 0) scal[1] = s;
}

// vq.py:296-298: smoothed = (cluster_size + eps) / (sum + K * eps) * sum;  embed <- decay * embed + (1 - decay) * (esum / smoothed).
__global__ void __launch_bounds__(256)
lg_vq_epilogue(uint32_t K, int d, const float* __restrict__ esum, const float* __restrict__ cluster_size, const float* __restrict__ scal,
               float* __restrict__ embed, float decay, float one_minus_decay, float eps, float k_eps)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)K * d) return;
    const uint32_t c = (uint32_t)(idx / (uint32_t)d), j = (uint32_t)(idx % (uint32_t)d);
    const float total = scal[1];
    const float smoothed = ((cluster_size[c] + eps) / (total + k_eps)) * total;
    const float mean = esum[(size_t)c * (d + 1) + j] / smoothed;
    embed[idx] = decay * embed[idx] + one_minus_decay * mean;
}
