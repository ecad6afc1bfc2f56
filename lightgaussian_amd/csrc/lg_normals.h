// lg_normals.h -- normals of the Gaussians and of the rendered depth surface, and the fused depth-normal consistency loss
// (include/lightgaussian_normals.h).  Replaces, per training step, normalize / build_rotation / argmin / gather /
// two matmuls / where over N (about twenty launches and [N,3,3] temporaries) and 2DGS's depth_to_normal with the loss on top of it
// (about thirty launches over [3,H,W] temporaries, forward and backward).
//
//   lg_normal_rows_kernel / lg_normal_rows_bwd_kernel
//       one lane per FOUR consecutive rows, the walk of lg_rows.h: xyz and scaling rows are three dwordx4 each, rotation, the output
//       rows and their gradients four.  The view matrix is 16 uniform loads.  lg_math.h: lg_normal_row / lg_normal_row_bwd.
//   lg_normal_fwd <LOSS>
//       ONE WAVE streams a strip of LG_NRM_FWD_COLS (62) columns down LG_NRM_ROWS (32) rows, lg_loss.h's decomposition: lane l holds
//       column cx0 - 1 + l, so strips overlap by the halo of one column and the left and right depths of a pixel are its neighbour
//       lanes' registers (lane exchange, no LDS).  The three depth rows a pixel needs are a ring in registers; the row after them is in
//       flight while a row is worked on.  LOSS = false writes N_d; LOSS = true also reads N_r, alpha and weight, writes N_d only when
//       asked and leaves ONE partial sum per wave with a plain store (per-lane sums over the rows, then the lanes in DPP order).
//   lg_mean_finalize<1>       (lg_loss.h) one workgroup: the partials in a fixed order, accumulated in double, times 1 / (H W).
//   lg_normal_bwd <LOSS>
//       the gather form, lane l = column cx0 - 2 + l, LG_NRM_BWD_COLS (60) output columns per strip: every pixel q of the strip and its
//       halo recomputes its cross product once and turns dL/dN_d(q) into the four taps of its neighbours' depths (lg_depth_normal_bwd);
//       the output pixel sums the down tap of the row above, the up tap of the row below -- rows of the register ring -- and the right /
//       left taps of its neighbour lanes.  Depth rows r - 1 .. r + 1 and the taps of rows r - 2 .. r: the 13-point diamond, a halo of 2.
//       LOSS = true forms dL/dN_d from N_r, alpha, weight and the upstream scalar read from device memory, and writes dL/dN_r as well.
// Loads are unconditional with row and column clamped into the image (lg_loss.h says why); what a clamped load returns is never used:
// such a pixel is outside the image or on its border, where N_d is zero by definition.
// No atomics, no memset, no LDS, no scratch memory, no host read-back; results are bit-identical from run to run.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include "../../include/lightgaussian_normals.h"
#include "lg_host.h"
#include "lg_wave.h"
#include "lg_rows.h"
#include "lg_loss.h"          // lg_mean_finalize

#define LG_NRM_THREADS 256
#define LG_NRM_ROWS 32                      // output rows per wave
#define LG_NRM_FWD_COLS 62                  // output columns per wave of the forward: 64 lanes less a halo of 1 either side
#define LG_NRM_BWD_COLS 60                  // ... of the backward: a halo of 2
#define LG_NRM_MAX_DIM 32768                // H, W <= 2^15: H W < 2^31, grids far below the limits

static inline int lg_nrm_strips(int W, int cols) { return (W + cols - 1) / cols; }
static inline int lg_nrm_segs(int H) { return (H + LG_NRM_ROWS - 1) / LG_NRM_ROWS; }

// ---- per Gaussian ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LG_NRM_THREADS)
lg_normal_rows_kernel(int N, int vec, const float* __restrict__ xyz, const float* __restrict__ scaling, const float* __restrict__ rotation,
                      const float* __restrict__ viewmatrix, float* __restrict__ rows)
{
    lg_rows4_walk<LG_NRM_THREADS>(N, vec, [&](size_t i0, auto path) {
        float vm[16];
#pragma unroll
        for (int k = 0; k < 16; k++) vm[k] = viewmatrix[k];
        float x[4][3], s[4][3], q[4][4], o[4][4];
        lg_rows4_load(path, xyz, i0, x); lg_rows4_load(path, scaling, i0, s); lg_rows4_load(path, rotation, i0, q);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < lg_rows4_live(path)) {
                lg_normal_row(vm, x[k], s[k], q[k], o[k]);
                lg_rows4_store_row(path, rows, i0 + k, o[k]);
            }
    });
}

__global__ void __launch_bounds__(LG_NRM_THREADS)
lg_normal_rows_bwd_kernel(int N, int vec, const float* __restrict__ xyz, const float* __restrict__ scaling, const float* __restrict__ rotation,
                          const float* __restrict__ viewmatrix, const float* __restrict__ g_rows, float* __restrict__ d_xyz, float* __restrict__ d_rotation)
{
    lg_rows4_walk<LG_NRM_THREADS>(N, vec, [&](size_t i0, auto path) {
        float vm[16];
#pragma unroll
        for (int k = 0; k < 16; k++) vm[k] = viewmatrix[k];
        float x[4][3], s[4][3], q[4][4], g[4][4], dx[4][3], dq[4][4];
        lg_rows4_load(path, xyz, i0, x); lg_rows4_load(path, scaling, i0, s); lg_rows4_load(path, rotation, i0, q); lg_rows4_load(path, g_rows, i0, g);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < lg_rows4_live(path)) lg_normal_row_bwd(vm, x[k], s[k], q[k], g[k], dx[k], dq[k]);
        lg_rows4_store(path, d_xyz, i0, dx); lg_rows4_store(path, d_rotation, i0, dq);       // (at the end: per-row stores of dq measured 9 % slower here)
    });
}

// ---- per pixel ------------------------------------------------------------------------------------------------------------------
// what a lane knows about its column: the clamped index its loads use, the rays of the column and of its neighbours, whether N_d can be
// non-zero there (not the first or the last column of the image)
struct LgNrmCol { int x; uint32_t xc; float rx, rxm, rxp; bool inner; };
__device__ __forceinline__ LgNrmCol lg_nrm_col(int x, int W, float tanfovx)
{
    LgNrmCol c;
    c.x = x;
    c.xc = (uint32_t)min(max(x, 0), W - 1);
    c.rx = lg_pixel_ray(x, W, tanfovx); c.rxm = lg_pixel_ray(x - 1, W, tanfovx); c.rxp = lg_pixel_ray(x + 1, W, tanfovx);
    c.inner = x >= 1 && x <= W - 2;
    return c;
}
__device__ __forceinline__ const float* lg_nrm_row(const float* p, int y, int H, int W) { return p + (size_t)min(max(y, 0), H - 1) * W; }

// N_d of the pixel (c.x, y) from the ring (above, here, below) of this lane's column; zero on the border and outside the image
__device__ __forceinline__ void lg_nrm_pixel(const LgNrmCol& c, int y, int H, float tanfovy, float above, float here, float below, LgDepthNormal& o)
{
    const float dl = __shfl_up(here, 1, 64), dr = __shfl_down(here, 1, 64);
    const float ry = lg_pixel_ray(y, H, tanfovy), rym = lg_pixel_ray(y - 1, H, tanfovy), ryp = lg_pixel_ray(y + 1, H, tanfovy);
    lg_depth_normal(here, above, below, dl, dr, c.rx, c.rxm, c.rxp, ry, rym, ryp, o);
    if (!(c.inner && y >= 1 && y <= H - 2)) { o.ok = false; o.n[0] = o.n[1] = o.n[2] = 0.0f; }
}

// forward: grid (strips of 62 columns, segments of 32 rows), one wave per workgroup
template <bool LOSS>
__global__ void __launch_bounds__(64)
lg_normal_fwd(int H, int W, float tanfovx, float tanfovy, const float* __restrict__ depth, const float* __restrict__ nr, const float* __restrict__ alpha,
              const float* __restrict__ weight, float* __restrict__ nd, float* __restrict__ partials)
{
    const int lane = (int)threadIdx.x;
    const int y0 = (int)blockIdx.y * LG_NRM_ROWS, nout = min(LG_NRM_ROWS, H - y0);
    const LgNrmCol c = lg_nrm_col((int)blockIdx.x * LG_NRM_FWD_COLS - 1 + lane, W, tanfovx);
    const bool own = lane >= 1 && lane <= LG_NRM_FWD_COLS && c.x < W;        // this lane's column is an output column of the strip
    const size_t plane = (size_t)H * W;
    float d0 = lg_nrm_row(depth, y0 - 1, H, W)[c.xc], d1 = lg_nrm_row(depth, y0, H, W)[c.xc], d2 = lg_nrm_row(depth, y0 + 1, H, W)[c.xc];
    float sum = 0.0f;
    for (int ib = 0; ib < nout; ib += 4) {
#pragma unroll
        for (int j = 0; j < 4; j++) {           // (the last turn may run past nout: clamped loads and arithmetic nobody keeps)
            const int i = ib + j, y = y0 + i;
            const float d3 = lg_nrm_row(depth, y + 2, H, W)[c.xc];
            const size_t p = (size_t)min(y, H - 1) * W + c.xc;
            float n[3] = { 0.0f, 0.0f, 0.0f }, w = 0.0f;
            if (LOSS) {
                n[0] = nr[p]; n[1] = nr[plane + p]; n[2] = nr[2 * plane + p];
                w = alpha[p];
                if (weight) w = w * weight[p];
            }
            LgDepthNormal o;
            lg_nrm_pixel(c, y, H, tanfovy, d0, d1, d2, o);
            if (own && i < nout) {
                if (nd) { nd[p] = o.n[0]; nd[plane + p] = o.n[1]; nd[2 * plane + p] = o.n[2]; }
                if (LOSS) sum += lg_normal_term(w, n, o.n);
            }
            d0 = d1; d1 = d2; d2 = d3;
        }
    }
    if (LOSS) {
        sum = wave_sum_to_lane63(sum);
        if (lane == 63) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sum;
    }
}

// backward: grid (strips of 60 columns, segments of 32 rows), one wave per workgroup.
// LOSS: g = N_r [3,H,W], g_scalar = dL/dL on the device, d_nr written;  otherwise g = dL/dN_d [3,H,W].
template <bool LOSS>
__global__ void __launch_bounds__(64)
lg_normal_bwd(int H, int W, float tanfovx, float tanfovy, const float* __restrict__ depth, const float* __restrict__ g, const float* __restrict__ alpha,
              const float* __restrict__ weight, const float* __restrict__ g_scalar, float inv_count, float* __restrict__ d_nr, float* __restrict__ d_depth)
{
    const int lane = (int)threadIdx.x;
    const int y0 = (int)blockIdx.y * LG_NRM_ROWS, nout = min(LG_NRM_ROWS, H - y0);
    const LgNrmCol c = lg_nrm_col((int)blockIdx.x * LG_NRM_BWD_COLS - 2 + lane, W, tanfovx);
    const bool own = lane >= 2 && lane < 2 + LG_NRM_BWD_COLS && c.x < W;
    const size_t plane = (size_t)H * W;
    const float scale = LOSS ? g_scalar[0] * inv_count : 0.0f;
    // step i works on the pixels q of row r = y0 - 1 + i (i = 0 .. nout + 1) and finishes the output row r - 1
    float d0 = lg_nrm_row(depth, y0 - 2, H, W)[c.xc], d1 = lg_nrm_row(depth, y0 - 1, H, W)[c.xc], d2 = lg_nrm_row(depth, y0, H, W)[c.xc];
    float down2 = 0.0f, down1 = 0.0f, left1 = 0.0f, right1 = 0.0f;      // taps of rows r - 2 (down) and r - 1
    for (int ib = 0; ib < nout + 2; ib += 4) {
#pragma unroll
        for (int j = 0; j < 4; j++) {           // (the last turn may run past nout + 2: see lg_normal_fwd)
            const int i = ib + j, r = y0 - 1 + i;
            const float d3 = lg_nrm_row(depth, r + 2, H, W)[c.xc];
            const size_t p = (size_t)min(max(r, 0), H - 1) * W + c.xc;
            float G[3] = { g[p], g[plane + p], g[2 * plane + p] };
            float coef = 0.0f;
            if (LOSS) {
                float w = alpha[p];
                if (weight) w = w * weight[p];
                coef = -(scale * w);
#pragma unroll
                for (int k = 0; k < 3; k++) G[k] = coef * G[k];
            }
            LgDepthNormal o;
            lg_nrm_pixel(c, r, H, tanfovy, d0, d1, d2, o);
            LgNormalTaps t;
            const float ry = lg_pixel_ray(r, H, tanfovy), rym = lg_pixel_ray(r - 1, H, tanfovy), ryp = lg_pixel_ray(r + 1, H, tanfovy);
            lg_depth_normal_bwd(o, G, c.rx, c.rxm, c.rxp, ry, rym, ryp, t);
            if (LOSS && own && i >= 1 && i <= nout) { d_nr[p] = coef * o.n[0]; d_nr[plane + p] = coef * o.n[1]; d_nr[2 * plane + p] = coef * o.n[2]; }
            const float from_left = __shfl_up(right1, 1, 64), from_right = __shfl_down(left1, 1, 64);
            if (own && i >= 2 && i <= nout + 1) d_depth[(size_t)(r - 1) * W + c.xc] = lg_depth_grad(down2, t.up, from_left, from_right);
            down2 = down1; down1 = t.down; left1 = t.left; right1 = t.right;
            d0 = d1; d1 = d2; d2 = d3;
        }
    }
}
