// lg_vq_color_bwd.h -- backward of lg_vq_colors (lg_vq_color.h): dL/drgb [N,3] -> dL/d(row table) and the colour part of dL/dxyz,
// so that a VecTree-compressed model can be fine-tuned in its compressed form (lightgaussian_amd/vectree.py TrainableCompressed).
//
//   dL/drow[r][idx(M,k,c)] = sum over the Gaussians i with slot[i] = r of  [rgb_{i,c} not clamped] B_k(dir_i) g_{i,c}     k < (D+1)^2
//                          = 0                                                                      k >= (D+1)^2, rows nobody uses
//   dL/dxyz_i              = the direction term of lg_backward_sh
//
// The per-Gaussian arithmetic is lg_backward_sh (lg_math.h) on the fp16 row the forward read, the clamp re-evaluated by
// lg_sh_to_rgb: for a Gaussian with a row of its own the gradient row is, bit for bit, the one K9 writes for the dense model.
// A row table has two kinds of rows with nothing in common:
//
//   non-VQ rows (slot >= K): one Gaussian per row, no reduction.  lg_vq_colors_bwd_rows_kernel, one lane per Gaussian as in the
//       forward; it also writes dL/dxyz of ALL N Gaussians (nullable).  The 3 M floats of a lane's gradient row go through LDS
//       ([64][3 M | 1] floats, odd stride: no bank conflicts) and leave as a flat copy -- element e of the wave's 64 x 3 M block
//       by lane e mod 64 -- because vectree.py numbers the non-VQ rows in Gaussian order: the rows of a wave's non-VQ lanes are
//       neighbours in the table and the dword stores of one instruction cover whole lines.  Every lane storing its own row at a
//       192-byte stride is the pattern K9 measured at three times the cost (partial-line writes; lg_preprocess.h).
//   codebook rows (slot < K): a segmented sum over an inverted index built ONCE per model (the assignment does not change while
//       fine-tuning): lg_vq_slot_keys -> lg_sort_keys on the code bits -> lg_vq_starts -> lg_vq_chunk_scan (the last three are
//       the kernels of lg_vq_train.h, unchanged; a non-VQ Gaussian sorts under the pseudo-code K, behind every list).
//       lg_vq_colors_bwd_chunk_kernel: one wave per chunk of at most LG_VQ_SUM_CHUNK Gaussians of one code, 64 at a time: lane
//       per Gaussian runs lg_backward_sh with a store into the LDS tile, then lane j < 3 M adds column j over the tile's rows
//       in order.  lg_vq_colors_bwd_combine adds a code's chunk partials in chunk order and writes 0 for a code without Gaussians.
//
// Summation order (the one lg_vq_train.h defines): a code's Gaussians are added in ascending Gaussian index inside chunks of
// LG_VQ_SUM_CHUNK, acc = acc + term from acc = 0; the chunk partials are then added in chunk order.  No float atomics: the
// result is a function of (slot, inputs) alone, whatever the grid, the stream or the hardware's scheduling.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include "lg_vq_color.h"
#include "lg_vq_train.h"

#define LG_VQ_BWD_WAVE 64

// The persistent index of a model (lg_vq_code_index): ids [N] the Gaussians grouped by code, ascending inside a code (the
// non-VQ ones behind them); start [K + 2]; chunk_off [K + 1]; err: the radix sort's give-up word.
struct VqIndexView {
    uint32_t* ids;
    uint32_t* start;
    uint32_t* chunk_off;
    uint32_t* err;
    size_t total;
};
static VqIndexView carve_vq_index(void* base, size_t N, size_t K)
{
    VqIndexView v{};
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
    v.ids = (uint32_t*)take(std::max<size_t>(N, 1) * 4);
    v.start = (uint32_t*)take((K + 2) * 4);
    v.chunk_off = (uint32_t*)take((K + 1) * 4);
    v.err = (uint32_t*)take(64);
    v.total = off;
    return v;
}
struct VqIndexScratch {
    uint64_t* keys_in;
    uint64_t* keys_out;
    void* sort_temp; size_t sort_temp_bytes;
    size_t total;
};
static VqIndexScratch carve_vq_index_scratch(void* base, size_t N)
{
    VqIndexScratch v{};
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
    if (N == 0) N = 1;
    v.keys_in = (uint64_t*)take(N * 8);
    v.keys_out = (uint64_t*)take(N * 8);
    v.sort_temp_bytes = lg_sort_layout(N).total;
    v.sort_temp = take(v.sort_temp_bytes);
    v.total = off;
    return v;
}
// a code with m >= 1 Gaussians has at most m / CHUNK + 1 chunks
static inline size_t lg_vq_bwd_max_chunks(size_t N, size_t K) { return N / LG_VQ_SUM_CHUNK + std::min(N, K); }

// key[i] = (code << 32) | i with code = slot[i] for a VQ Gaussian and K for every other one
__global__ void __launch_bounds__(256)
lg_vq_slot_keys(uint32_t N, uint32_t K, const uint32_t* __restrict__ slot, uint64_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    keys[i] = ((uint64_t)min(slot[i], K) << 32) | i;
}

// the Gaussian ids of the sorted keys, and the sort's give-up word next to them
__global__ void __launch_bounds__(256)
lg_vq_index_ids(uint32_t N, const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ sort_err, uint32_t* __restrict__ ids,
                uint32_t* __restrict__ err)
{
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q == 0) *err = *sort_err;
    if (q < N) ids[q] = (uint32_t)sorted[q];
}

// One Gaussian's share: the fp16 row -> [M][3] floats, the clamp from lg_sh_to_rgb, lg_backward_sh (its one-pass form) with `store` writing
// tile[lg_vq_row_index(M, k, c)] (the file's column order), the direction term into dm.  The caller zeroed the tile row.
template <int M>
__device__ __forceinline__ void lg_vq_bwd_one(int D, uint32_t need, const float* __restrict__ means3D, const float* cp,
                                              const unsigned char* __restrict__ rows, uint32_t row_stride, uint32_t r, uint32_t i,
                                              const float* __restrict__ dL_drgb, float* tile_row, float dm[3])
{
    constexpr int NH = 3 * M, NQ = (NH + 7) / 8;
    const float px = means3D[3 * (size_t)i], py = means3D[3 * (size_t)i + 1], pz = means3D[3 * (size_t)i + 2];
    const lg_h8* row = reinterpret_cast<const lg_h8*>(rows + (size_t)r * row_stride);
    _Float16 h[NQ * 8];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        lg_h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (need & (1u << q)) v = row[q];
#pragma unroll
        for (int k = 0; k < 8; k++) h[8 * q + k] = v[k];
    }
    const int Ma = (D + 1) * (D + 1);
    float sh[3 * M];
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
        for (int c = 0; c < 3; c++) sh[3 * m + c] = m < Ma ? (float)h[lg_vq_row_index(M, m, c)] : 0.0f;
    float rgb[3];
    uint32_t cb;
    lg_sh_to_rgb(D, sh, px, py, pz, cp, rgb, cb);
    const float g0 = dL_drgb[3 * (size_t)i], g1 = dL_drgb[3 * (size_t)i + 1], g2 = dL_drgb[3 * (size_t)i + 2];
    const float dRGB[3] = { (cb & 1u) ? 0.0f : g0, (cb & 2u) ? 0.0f : g1, (cb & 4u) ? 0.0f : g2 };
    lg_backward_sh_one_pass(D, sh, px, py, pz, cp, dRGB, dm, [&](int k, int c, float v) { tile_row[lg_vq_row_index(M, k, c)] = v; });
}

// lane per Gaussian: dL/dxyz of every Gaussian, the gradient row of a non-VQ one (through LDS, see the head of the file)
template <int M>
__global__ void __launch_bounds__(LG_VQ_BWD_WAVE)
lg_vq_colors_bwd_rows_kernel(int N, int D, uint32_t need, uint32_t K, uint32_t n_rows, const float* __restrict__ means3D,
                             const float* __restrict__ campos, const uint32_t* __restrict__ slot, const unsigned char* __restrict__ rows,
                             uint32_t row_stride, const float* __restrict__ dL_drgb, float* __restrict__ dL_drows,
                             float* __restrict__ dL_dmeans)
{
    constexpr int NF = 3 * M, ST = NF | 1;
    __shared__ float tile[LG_VQ_BWD_WAVE * ST];
    __shared__ uint32_t dest[LG_VQ_BWD_WAVE];
    const uint32_t lane = threadIdx.x;
    const int i = blockIdx.x * LG_VQ_BWD_WAVE + (int)lane;
    const uint32_t r = i < N ? slot[i] : 0u;
    const bool own = i < N && r >= K && r < n_rows;          // a row of its own inside the table
    float* tile_row = tile + lane * ST;
#pragma unroll
    for (int j = 0; j < NF; j++) tile_row[j] = 0.0f;
    dest[lane] = own ? r : 0xFFFFFFFFu;
    if (i < N && (own || dL_dmeans)) {
        const float cp[3] = { campos[0], campos[1], campos[2] };
        float dm[3] = {0.0f, 0.0f, 0.0f};
        lg_vq_bwd_one<M>(D, need, means3D, cp, rows, row_stride, r, (uint32_t)i, dL_drgb, tile_row, dm);
        if (dL_dmeans) { dL_dmeans[3 * (size_t)i] = dm[0]; dL_dmeans[3 * (size_t)i + 1] = dm[1]; dL_dmeans[3 * (size_t)i + 2] = dm[2]; }
    }
    __syncthreads();
    for (uint32_t e = lane; e < LG_VQ_BWD_WAVE * NF; e += LG_VQ_BWD_WAVE) {
        const uint32_t t = e / NF, j = e % NF;
        const uint32_t rr = dest[t];
        if (rr != 0xFFFFFFFFu) dL_drows[(size_t)rr * NF + j] = tile[t * ST + j];
    }
}

// one wave per chunk of one code's list: partial[g][0 .. 3 M) in the file's column order
template <int M>
__global__ void __launch_bounds__(LG_VQ_BWD_WAVE)
lg_vq_colors_bwd_chunk_kernel(int D, uint32_t need, uint32_t K, const float* __restrict__ means3D, const float* __restrict__ campos,
                              const unsigned char* __restrict__ rows, uint32_t row_stride, const float* __restrict__ dL_drgb,
                              const uint32_t* __restrict__ ids, const uint32_t* __restrict__ start, const uint32_t* __restrict__ chunk_off,
                              const uint32_t* __restrict__ err, float* __restrict__ partial)
{
    constexpr int NF = 3 * M, ST = NF | 1;
    __shared__ float tile[LG_VQ_BWD_WAVE * ST];
    const uint32_t lane = threadIdx.x;
    const uint32_t g = blockIdx.x;
    if (*err || g >= chunk_off[K]) return;                     // (an index whose sort gave up is not followed: combine writes NaN)
    uint32_t lo = 0, hi = K;                                   // chunk_off[lo] <= g < chunk_off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (chunk_off[mid] <= g) lo = mid; else hi = mid;
    }
    const uint32_t c = lo;
    const uint32_t b = start[c] + (g - chunk_off[c]) * LG_VQ_SUM_CHUNK;
    const uint32_t e = min(b + LG_VQ_SUM_CHUNK, start[c + 1]);
    const float cp[3] = { campos[0], campos[1], campos[2] };
    float* tile_row = tile + lane * ST;
    float acc = 0.0f;
    for (uint32_t q0 = b; q0 < e; q0 += LG_VQ_BWD_WAVE) {
        const uint32_t cnt = min((uint32_t)LG_VQ_BWD_WAVE, e - q0);
#pragma unroll
        for (int j = 0; j < NF; j++) tile_row[j] = 0.0f;
        if (lane < cnt) {
            float dm[3] = {0.0f, 0.0f, 0.0f};
            lg_vq_bwd_one<M>(D, need, means3D, cp, rows, row_stride, c, ids[q0 + lane], dL_drgb, tile_row, dm);
        }
        __syncthreads();
        if (lane < NF)
            for (uint32_t t = 0; t < cnt; t++) acc = acc + tile[t * ST + lane];
        __syncthreads();
    }
    if (lane < NF) partial[(size_t)g * NF + lane] = acc;
}

// Thread (c, j): dL_drows[c][j] = the partials of code c's chunks added in chunk order; 0 for a code without Gaussians.  A sort
// that gave up while the index was built (never seen, see lg_sort.h) poisons every codebook row with NaN.
__global__ void __launch_bounds__(256)
lg_vq_colors_bwd_combine(uint32_t K, uint32_t NF, const uint32_t* __restrict__ chunk_off, const float* __restrict__ partial,
                         const uint32_t* __restrict__ err, float* __restrict__ dL_drows)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)K * NF) return;
    const uint32_t c = (uint32_t)(idx / NF), j = (uint32_t)(idx % NF);
    const uint32_t g0 = chunk_off[c], g1 = chunk_off[c + 1];
    float acc = 0.0f;
    for (uint32_t g = g0; g < g1; g++) acc = g == g0 ? partial[(size_t)g * NF + j] : acc + partial[(size_t)g * NF + j];
    dL_drows[idx] = *err ? __builtin_nanf("") : acc;
}
