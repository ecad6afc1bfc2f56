// lg_filter3d.h -- Mip-Splatting's 3D smoothing filter: the per-Gaussian filter size from the training cameras
// (lg_filter3d_update) and its application to scales and opacity, forward and backward, in the raw or the activated domain
// (lg_filter3d_apply / lg_filter3d_apply_bwd).  Replaces the published compute_3D_filter loop (about 15 elementwise launches over N
// per camera) and get_scaling_with_3D_filter / get_opacity_with_3D_filter with their autograd twins (about two dozen per render).
//
//   lg_filter3d_update_kernel  one lane per Gaussian: the mean is read once (12 B), then every camera is visited in registers
//                              (lg_math.h: lg_filter3d_term).  The camera table is STAGED THROUGH LDS in chunks of LG_F3D_CHUNK (64)
//                              cameras: lane k of the workgroup turns table entry k into its LgFilterCam (the divisions W / (2 tanfovx)
//                              happen once per camera and workgroup, not once per pair), every lane then reads the entries as LDS
//                              broadcasts.  Writes filter = sqrtf(0.2f) min t for a seen row and -1 for an unseen one, the seen byte,
//                              and ONE partial maximum per workgroup with a plain store.  The grid is capped at LG_F3D_MAX_WGS
//                              workgroups that stride over the rows, so there are never more than 2048 partials.
//   lg_filter3d_fill_kernel    the reduce and the fill in one launch: every workgroup takes the maximum of the partials in a fixed
//                              order (<= 8 KB from L2) and gives the unseen rows of its stride that maximum, or 0 when no row was seen.
//                              A maximum of floats is exact, so the order cannot change a bit; it is fixed all the same.
//   lg_filter3d_apply_kernel / lg_filter3d_apply_bwd_kernel <RAW>
//                              elementwise, one lane per FOUR consecutive rows, the walk of lg_rows.h: 48 bytes of scaling rows are
//                              three dwordx4, opacity, filter and the gradients one dwordx4 each, all loads issued before the arithmetic.
// No atomics, no memset, no host read-back, no scratch memory; results are bit-identical from run to run.
//
// Apply, per row (f = the row's filter; f == 0: the row is copied bit for bit by an explicit branch), float32, nothing contracted:
//   raw        e_k = expf(r_k)   u_k = e_k e_k + f f   r'_k = 0.5f logf(u_k)   w_k = e_k e_k / u_k
//              c = sqrtf((w_0 w_1) w_2)   y = sigmoid(o) c   o' = logf(y / (1 - y))          sigmoid as K1's: 1 / (1 + expf(-o))
//   activated  u_k = s_k s_k + f f        s'_k = sqrtf(u_k)      w_k as above, c as above     sigma' = sigma c
// Backward (the filter takes no gradient), with v_k = f f / u_k -- which is 1 - w_k without the cancellation -- and
// 1 - sigmoid(o) evaluated as sigmoid(-o):
//   raw        dL/dr_k = g_r'_k w_k + (g_o' / (1 - y)) v_k                    dL/do = g_o' sigmoid(-o) / (1 - y)
//   activated  dL/ds_k = g_s'_k q_k + (g_sigma' sigma) (q_i q_j) v_k / s'_k    dL/dsigma = g_sigma' c
//              q_k = s_k / s'_k (= sqrt(w_k); i, j the other two axes): dc/ds_k = c (1 - w_k) / s_k written without the division by s_k
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include "lg_host.h"
#include "lg_preprocess.h"      // lg_sigmoid
#include "lg_rows.h"

#define LG_F3D_THREADS 256
#define LG_F3D_CHUNK 64                 // cameras per LDS stage (80 bytes each: 5 KB)
#define LG_F3D_MAX_WGS 2048             // workgroups of the update and of the fill: the number of partial maxima never exceeds it
static_assert(sizeof(lg_filter_camera) == 80, "lg_filter_camera is 80 bytes");
static_assert(LG_F3D_CHUNK <= LG_F3D_THREADS, "one lane stages one camera");

// maximum over the workgroup's 256 lanes, in every lane (ws: 4 floats of LDS)
__device__ __forceinline__ float lg_f3d_wg_max(float m, float* ws)
{
    m = lg_wave_all_max(m);
    __syncthreads();                                    // ws may still be read from an earlier call
    if ((threadIdx.x & 63u) == 0u) ws[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(ws[0], ws[1]), fmaxf(ws[2], ws[3]));
}

__global__ void __launch_bounds__(LG_F3D_THREADS)
lg_filter3d_update_kernel(int N, const float* __restrict__ means3D, int V, const lg_filter_camera* __restrict__ cameras,
                          float* __restrict__ filter3d, uint8_t* __restrict__ seen, float* __restrict__ partial)
{
    __shared__ LgFilterCam cam[LG_F3D_CHUNK];
    __shared__ float ws[4];
    const int tid = (int)threadIdx.x;
    float best = -1.0f;                                 // largest filter among the seen rows of this workgroup
    int staged = -1;                                    // first camera of the chunk in LDS (uniform): V <= 64 stages once
    for (int base = (int)blockIdx.x * LG_F3D_THREADS; base < N; base += (int)gridDim.x * LG_F3D_THREADS) {
        const int i = base + tid;
        const bool live = i < N;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        if (live) { px = means3D[3 * (size_t)i]; py = means3D[3 * (size_t)i + 1]; pz = means3D[3 * (size_t)i + 2]; }
        float tmin = INFINITY;
        bool any = false;
        for (int c0 = 0; c0 < V; c0 += LG_F3D_CHUNK) {
            const int nc = min(LG_F3D_CHUNK, V - c0);
            if (staged != c0) {
                __syncthreads();                        // the readers of the previous chunk are done
                if (tid < nc) {
                    const lg_filter_camera* s = cameras + c0 + tid;
                    float vm[16];
#pragma unroll
                    for (int k = 0; k < 16; k++) vm[k] = s->viewmatrix[k];
                    lg_filter3d_camera(vm, s->tanfovx, s->tanfovy, s->width, s->height, cam[tid]);
                }
                __syncthreads();
                staged = c0;
            }
            for (int k = 0; k < nc; k++) {
                float t;
                if (lg_filter3d_term(cam[k], px, py, pz, t)) { any = true; tmin = t < tmin ? t : tmin; }
            }
        }
        if (live) {
            const float f = any ? lg_filter3d_value(tmin) : -1.0f;
            filter3d[i] = f;
            if (seen) seen[i] = any ? 1 : 0;
            best = fmaxf(best, f);
        }
    }
    best = lg_f3d_wg_max(best, ws);
    if (tid == 0) partial[blockIdx.x] = best;
}

__global__ void __launch_bounds__(LG_F3D_THREADS)
lg_filter3d_fill_kernel(int N, int num_partial, const float* __restrict__ partial, float* __restrict__ filter3d)
{
    __shared__ float ws[4];
    float m = -1.0f;
    for (int k = (int)threadIdx.x; k < num_partial; k += LG_F3D_THREADS) m = fmaxf(m, partial[k]);
    m = lg_f3d_wg_max(m, ws);
    const float fill = m < 0.0f ? 0.0f : m;             // nobody seen: every row becomes 0, the identity of the apply
    for (int i = (int)blockIdx.x * LG_F3D_THREADS + (int)threadIdx.x; i < N; i += (int)gridDim.x * LG_F3D_THREADS)
        if (filter3d[i] < 0.0f) filter3d[i] = fill;
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------
template <bool RAW>
__device__ __forceinline__ void lg_filter3d_row(const float r[3], float o, float f, float ro[3], float& oo)
{
    if (f == 0.0f) { ro[0] = r[0]; ro[1] = r[1]; ro[2] = r[2]; oo = o; return; }
    const float f2 = f * f;
    float w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float s = RAW ? expf(r[k]) : r[k];
        const float s2 = s * s, u = s2 + f2;
        ro[k] = RAW ? 0.5f * logf(u) : sqrtf(u);
        w[k] = s2 / u;
    }
    const float c = sqrtf((w[0] * w[1]) * w[2]);
    if (RAW) {
        const float y = lg_sigmoid(o) * c;
        oo = logf(y / (1.0f - y));
    } else {
        oo = o * c;
    }
}

template <bool RAW>
__device__ __forceinline__ void lg_filter3d_row_bwd(const float r[3], float o, float f, const float gr[3], float go, float dr[3], float& d_o)
{
    if (f == 0.0f) { dr[0] = gr[0]; dr[1] = gr[1]; dr[2] = gr[2]; d_o = go; return; }
    const float f2 = f * f;
    float w[3], v[3], q[3], sp[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float s = RAW ? expf(r[k]) : r[k];
        const float s2 = s * s, u = s2 + f2;
        w[k] = s2 / u;
        v[k] = f2 / u;
        if (!RAW) { sp[k] = sqrtf(u); q[k] = s / sp[k]; }
    }
    const float c = sqrtf((w[0] * w[1]) * w[2]);
    if (RAW) {
        const float y = lg_sigmoid(o) * c;
        const float h = go / (1.0f - y);
#pragma unroll
        for (int k = 0; k < 3; k++) dr[k] = gr[k] * w[k] + h * v[k];
        d_o = h * lg_sigmoid(-o);
    } else {
        const float h = go * o;
        dr[0] = gr[0] * q[0] + h * (q[1] * q[2]) * v[0] / sp[0];
        dr[1] = gr[1] * q[1] + h * (q[0] * q[2]) * v[1] / sp[1];
        dr[2] = gr[2] * q[2] + h * (q[0] * q[1]) * v[2] / sp[2];
        d_o = go * c;
    }
}

// one lane per four consecutive rows (lg_rows.h).  vec (uniform): every pointer is 16-byte aligned
template <bool RAW>
__global__ void __launch_bounds__(LG_F3D_THREADS)
lg_filter3d_apply_kernel(int N, int vec, const float* __restrict__ scaling, const float* __restrict__ opacity, const float* __restrict__ filter3d,
                         float* __restrict__ out_scaling, float* __restrict__ out_opacity)
{
    lg_rows4_walk<LG_F3D_THREADS>(N, vec, [&](size_t i0, auto path) {
        float r[4][3], o[4][1], f[4][1], ro[4][3], oo[4][1];
        lg_rows4_load(path, scaling, i0, r); lg_rows4_load(path, opacity, i0, o); lg_rows4_load(path, filter3d, i0, f);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < lg_rows4_live(path)) lg_filter3d_row<RAW>(r[k], o[k][0], f[k][0], ro[k], oo[k][0]);
        lg_rows4_store(path, out_scaling, i0, ro); lg_rows4_store(path, out_opacity, i0, oo);
    });
}

template <bool RAW>
__global__ void __launch_bounds__(LG_F3D_THREADS)
lg_filter3d_apply_bwd_kernel(int N, int vec, const float* __restrict__ scaling, const float* __restrict__ opacity,
                             const float* __restrict__ filter3d, const float* __restrict__ g_scaling, const float* __restrict__ g_opacity,
                             float* __restrict__ d_scaling, float* __restrict__ d_opacity)
{
    lg_rows4_walk<LG_F3D_THREADS>(N, vec, [&](size_t i0, auto path) {
        float r[4][3], gr[4][3], o[4][1], f[4][1], go[4][1], dr[4][3], dq[4][1];
        lg_rows4_load(path, scaling, i0, r); lg_rows4_load(path, g_scaling, i0, gr);
        lg_rows4_load(path, opacity, i0, o); lg_rows4_load(path, filter3d, i0, f); lg_rows4_load(path, g_opacity, i0, go);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < lg_rows4_live(path)) lg_filter3d_row_bwd<RAW>(r[k], o[k][0], f[k][0], gr[k], go[k][0], dr[k], dq[k][0]);
        lg_rows4_store(path, d_scaling, i0, dr); lg_rows4_store(path, d_opacity, i0, dq);
    });
}
