// lg_rows.h -- the four-rows-per-lane walk over per-Gaussian tensors, used by lg_filter3d_apply(_bwd)_kernel and
// lg_normal_rows(_bwd)_kernel; the float vector type every kernel header shares; the grid size and the row limit of the walk.
//
// One lane takes FOUR consecutive rows i0 .. i0 + 3 of every tensor.  Four rows of width W floats are 4 W consecutive floats from
// p + W i0, so a lane whose four rows exist, in a launch whose pointers are all 16-byte aligned (`vec`, uniform), moves them as W dwordx4
// (LgRowsVec).  Every other lane -- a pointer off 16 bytes, or the last N % 4 rows -- moves its `live` rows (1 .. 4) one row at a time
// with dword accesses and touches nothing past row N - 1 (LgRowsDword).  A kernel hands lg_rows4_walk a generic lambda (i0, path): its
// loads, its row math under `k < lg_rows4_live(path)` and its stores are written once and compiled once per path, so the dwordx4 path
// carries no trace of the other one.  Index arithmetic is 64-bit.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float lg_f4 __attribute__((ext_vector_type(4)));

#define LG_ROWS_MAX (1 << 30)           // row counts of the per-Gaussian entry points are in [0, 2^30)
static inline unsigned lg_rows4_wgs(int32_t N, int threads) { return (unsigned)((((int64_t)N + 3) / 4 + threads - 1) / threads); }

struct LgRowsVec {};                    // all four rows live, every pointer 16-byte aligned
struct LgRowsDword { int live; };       // rows i0 .. i0 + live - 1
__device__ __forceinline__ constexpr int lg_rows4_live(LgRowsVec) { return 4; }
__device__ __forceinline__ int lg_rows4_live(LgRowsDword d) { return d.live; }

// v[k] = row i0 + k.  Element e of the lane's 4 W floats is lane e % 4 of vector e / 4 and column e % W of row e / W.
template <int W>
__device__ __forceinline__ void lg_rows4_load(LgRowsVec, const float* p, size_t i0, float (&v)[4][W])
{
    lg_f4 t[W];
#pragma unroll
    for (int j = 0; j < W; j++) t[j] = *(const lg_f4*)(p + W * i0 + 4 * j);
#pragma unroll
    for (int e = 0; e < 4 * W; e++) v[e / W][e % W] = t[e / 4][e % 4];
}
template <int W>
__device__ __forceinline__ void lg_rows4_store(LgRowsVec, float* p, size_t i0, const float (&v)[4][W])
{
#pragma unroll
    for (int j = 0; j < W; j++) {
        lg_f4 t;
#pragma unroll
        for (int c = 0; c < 4; c++) t[c] = v[(4 * j + c) / W][(4 * j + c) % W];
        *(lg_f4*)(p + W * i0 + 4 * j) = t;
    }
}
// the rows at and past d.live are neither read nor written, and their v[k] stay as they were
template <int W>
__device__ __forceinline__ void lg_rows4_load(LgRowsDword d, const float* p, size_t i0, float (&v)[4][W])
{
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k < d.live) {
#pragma unroll
            for (int c = 0; c < W; c++) v[k][c] = p[W * (i0 + k) + c];
        }
}
template <int W>
__device__ __forceinline__ void lg_rows4_store(LgRowsDword d, float* p, size_t i0, const float (&v)[4][W])
{
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k < d.live) {
#pragma unroll
            for (int c = 0; c < W; c++) p[W * (i0 + k) + c] = v[k][c];
        }
}
// A row of a [N,4] tensor is one dwordx4 of its own: a kernel may store row i the moment it has it, which spreads its stores between
// its row math (lg_normal_rows_kernel at 3 M rows: 0.028 ms against 0.031 ms with the four stores at the end)
__device__ __forceinline__ void lg_rows4_store_row(LgRowsVec, float* p, size_t i, const float (&v)[4])
{
    *(lg_f4*)(p + 4 * i) = lg_f4{ v[0], v[1], v[2], v[3] };
}
__device__ __forceinline__ void lg_rows4_store_row(LgRowsDword, float* p, size_t i, const float (&v)[4])
{
#pragma unroll
    for (int c = 0; c < 4; c++) p[4 * i + c] = v[c];
}

template <int THREADS, class F>
__device__ __forceinline__ void lg_rows4_walk(int N, int vec, F f)
{
    const size_t i0 = 4 * ((size_t)blockIdx.x * THREADS + threadIdx.x), n = (size_t)N;
    if (i0 >= n) return;
    if (vec && i0 + 4 <= n) f(i0, LgRowsVec{});
    else f(i0, LgRowsDword{ i0 + 4 <= n ? 4 : (int)(n - i0) });
}
