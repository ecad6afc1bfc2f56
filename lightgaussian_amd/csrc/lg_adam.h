// lg_adam.h -- lg_adam_step: one Adam / AdamW step over up to LG_ADAM_MAX_TENSORS tensors per launch.
// Replaces the optimizer.step() of the reference's training_setup (scene/gaussian_model.py: torch.optim.AdamW(l, lr=0.0, eps=1e-15),
// six one-tensor groups with an lr each): torch's default step is ~8 multi-tensor kernels over parameters and moments, this is ONE
// launch that reads param, grad, exp_avg, exp_avg_sq once (16 B per element) and writes param and the moments once (12 B).
//
// Layout.  The per-tensor table travels BY VALUE in the kernel arguments (no device allocation, no copy, no synchronisation).
// Every workgroup owns ONE contiguous span of LG_ADAM_SPAN elements of ONE tensor: first_wg[t] is the first workgroup of tensor t,
// the search over the table is wave-uniform, so pointers and hyper-parameters stay in SGPRs.  A full span of a tensor whose four
// pointers are 16-byte aligned goes through dwordx4 loads / stores, all of them issued before the arithmetic; a tensor with a
// misaligned pointer and the last, partial span of any tensor go one dword per lane.  param, exp_avg and exp_avg_sq of an
// element are read and written by the same lane; grad is only read.  No LDS, no atomics, no scratch.
//
// Arithmetic per element, float32, no implicit contraction, correctly rounded divide and square root (the library's flags):
//     g' = g + wd * p   (L2 form, only when wd != 0)        p = p * (1 - lr wd)   (decoupled form)
//     m  = m + (1 - beta1) * (g' - m)                       v = beta2 * v + (1 - beta2) * (g' * g')
//     p  = p - step_size * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))
// The sum that closes each of the four lines is ONE explicit fmaf (a single rounding, written out -- not left to the compiler):
// fmaf(wd, p, g), fmaf(1 - beta1, g' - m, m) as ATen's lerp, fmaf(1 - beta2, round(g' g'), round(beta2 v)) as ATen's addcmul a + alpha (b c), fmaf(-step_size, q, p).
// step_size = lr / (1 - beta1^t), sqrt(1 - beta2^t), 1 - lr wd, 1 - beta1, 1 - beta2 are evaluated in double on the host and rounded
// once to float -- what torch's default (non-capturable) step does.  Non-finite gradients propagate.
// Part of liblightgaussian_hip.so (single translation unit: lg_api.hip includes the lg_*.h kernel headers).
#pragma once

#include "lg_host.h"
#include "lg_adam_rows.h"
#include "lg_rows.h"              // lg_f4

// LG_ADAM_MAX_TENSORS (8) and LG_ADAM_SPAN (elements per workgroup: 256 lanes x LG_ADAM_SPAN / 1024 dwordx4 per stream; 4096 by
// measurement on the MI355X, EXPERIMENTS "Adam step"; -DLG_ADAM_SPAN=... for an A/B build) come from include/lightgaussian.h.
// 1: grad (read once, never written) is loaded nontemporally.  Measured on the MI355X (EXPERIMENTS, "Adam step").
#ifndef LG_ADAM_NT_GRAD
#define LG_ADAM_NT_GRAD 1
#endif
#define LG_ADAM_THREADS 256
#define LG_ADAM_VEC (LG_ADAM_SPAN / (LG_ADAM_THREADS * 4))
static_assert(LG_ADAM_SPAN % (LG_ADAM_THREADS * 4) == 0 && LG_ADAM_VEC >= 1, "a span is a whole number of dwordx4 per lane");


struct LgAdamTable {
    float* param[LG_ADAM_MAX_TENSORS];
    const float* grad[LG_ADAM_MAX_TENSORS];
    float* exp_avg[LG_ADAM_MAX_TENSORS];
    float* exp_avg_sq[LG_ADAM_MAX_TENSORS];
    int64_t numel[LG_ADAM_MAX_TENSORS];
    uint32_t first_wg[LG_ADAM_MAX_TENSORS];     // first workgroup of tensor t; 0xFFFFFFFF for the unused entries
    float step_size[LG_ADAM_MAX_TENSORS];       // lr / (1 - beta1^step)
    float bc2_sqrt[LG_ADAM_MAX_TENSORS];        // sqrt(1 - beta2^step)
    float decay[LG_ADAM_MAX_TENSORS];           // decoupled: 1 - lr wd;  L2 form: wd
    uint32_t vec_mask;                          // bit t: all four pointers of tensor t are 16-byte aligned
    float one_minus_beta1, beta2, one_minus_beta2, eps;
};

template <bool DECOUPLED>
__device__ __forceinline__ void lg_adam_element(float& p, float g, float& m, float& v, float decay, float step_size, float bc2_sqrt,
                                                float om_b1, float b2, float om_b2, float eps)
{
    if (DECOUPLED) p = p * decay;
    else if (decay != 0.0f) g = fmaf(decay, p, g);      // (uniform: torch skips the term for wd == 0, so an infinite p gives no 0 * inf)
    m = fmaf(om_b1, g - m, m);
    v = fmaf(om_b2, g * g, b2 * v);
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = fmaf(-step_size, m / denom, p);
}

// ---- lg_adam_step_rows: the same step over the rows a byte mask names ("visible rows") -----------------------
// A tensor [rows, ...] with a mask of `rows` bytes: an element of a row whose byte is non-zero takes lg_adam_element exactly as above;
// an element of a row whose byte is zero is neither loaded nor stored (param and both moments keep their bits, its gradient is never
// read).  An entry without a mask is a dense entry of the same launch.  Same work split, same table by value, same two paths.
// The mask has byte alignment and is read with byte loads, inside [mask, mask + rows) only (every element a lane looks up lies inside
// the tensor).  The row of an element: lg_adam_rows.h -- one uniform 64-bit division per workgroup, 32-bit arithmetic per lane.
// The mask bytes of a lane's dwordx4 are loaded first, from L2 (no LDS, no barrier); a dwordx4 wholly in unseen rows issues no load and
// no store, one that straddles a seen and an unseen row is computed and selected per element (the unseen elements store the bits they
// loaded), and a span without a seen row ends after its mask bytes.  With row_len >= 3 four consecutive elements lie in at most
// two rows: two byte loads per dwordx4; shorter rows load a byte per element.
struct LgAdamRowsTable {
    LgAdamTable a;
    const uint8_t* row_mask[LG_ADAM_MAX_TENSORS];   // nullptr: dense entry
    uint32_t row_len[LG_ADAM_MAX_TENSORS];          // numel / rows, <= LG_ADAM_MAX_ROW_LEN
    uint32_t row_rcp[LG_ADAM_MAX_TENSORS];          // lg_adam_row_rcp(row_len), lg_adam_row_thr(row_len): the row of an element
    uint32_t row_thr[LG_ADAM_MAX_TENSORS];          //   without a division or a branch
};

// vis[u], bit c: element c of the lane's dwordx4 u lies in a row the mask names (a full, aligned span; rem = the span's first element
// inside its first row, mask = that row's byte)
__device__ __forceinline__ void lg_adam_span_vis(const uint8_t* __restrict__ mask, uint32_t rem, uint32_t row_len, uint32_t rcp, uint32_t thr,
                                                 uint32_t (&vis)[LG_ADAM_VEC])
{
    uint32_t row[LG_ADAM_VEC][4], mb[LG_ADAM_VEC][4];
#pragma unroll
    for (int u = 0; u < LG_ADAM_VEC; u++) {
        const uint32_t x = rem + (uint32_t)(u * LG_ADAM_THREADS + (int)threadIdx.x) * 4u;
#pragma unroll
        for (int c = 0; c < 4; c++) row[u][c] = lg_adam_local_row(x + (uint32_t)c, rcp, thr);
    }
    if (row_len >= 3u) {                        // (uniform) two rows at the most: the middle elements belong to one of them
#pragma unroll
        for (int u = 0; u < LG_ADAM_VEC; u++) { mb[u][0] = mask[row[u][0]]; mb[u][3] = mask[row[u][3]]; }
#pragma unroll
        for (int u = 0; u < LG_ADAM_VEC; u++) {
            mb[u][1] = row[u][1] == row[u][0] ? mb[u][0] : mb[u][3];
            mb[u][2] = row[u][2] == row[u][0] ? mb[u][0] : mb[u][3];
        }
    } else {
#pragma unroll
        for (int u = 0; u < LG_ADAM_VEC; u++)
#pragma unroll
            for (int c = 0; c < 4; c++) mb[u][c] = mask[row[u][c]];
    }
#pragma unroll
    for (int u = 0; u < LG_ADAM_VEC; u++)
        vis[u] = (mb[u][0] ? 1u : 0u) | (mb[u][1] ? 2u : 0u) | (mb[u][2] ? 4u : 0u) | (mb[u][3] ? 8u : 0u);
}

// One workgroup's span: the ONE body behind lg_adam_kernel (ROWS = false: r is not read, and there is no mask, no vis, no zero-fill of
// the registers and no `continue` -- the dense kernel as it always was) and lg_adam_rows_kernel (ROWS = true).
template <bool DECOUPLED, bool ROWS>
__device__ __forceinline__ void lg_adam_span(const LgAdamTable& a, const LgAdamRowsTable* r)
{
    const uint32_t wg = blockIdx.x;
    uint32_t t = 0;
#pragma unroll
    for (int k = 1; k < LG_ADAM_MAX_TENSORS; k++) t += wg >= a.first_wg[k] ? 1u : 0u;   // first_wg ascends: t = the last entry <= wg
    float* __restrict__ const P = a.param[t];
    const float* __restrict__ const G = a.grad[t];
    float* __restrict__ const M = a.exp_avg[t];
    float* __restrict__ const V = a.exp_avg_sq[t];
    const float decay = a.decay[t], step_size = a.step_size[t], bc2_sqrt = a.bc2_sqrt[t];
    const float om_b1 = a.one_minus_beta1, b2 = a.beta2, om_b2 = a.one_minus_beta2, eps = a.eps;
    const int64_t base = (int64_t)(wg - a.first_wg[t]) * LG_ADAM_SPAN;
    const int64_t left = a.numel[t] - base;             // > 0 by the host's workgroup count
    [[maybe_unused]] uint32_t row_len = 0, rcp = 0, thr = 0, rem = 0;
    [[maybe_unused]] const uint8_t* __restrict__ mask = nullptr;
    if constexpr (ROWS) {
        row_len = r->row_len[t]; rcp = r->row_rcp[t]; thr = r->row_thr[t];
        mask = r->row_mask[t];
        if (mask) mask += lg_adam_first_row(base, row_len, &rem);      // uniform: the mask byte of the span's first row
    }
    if (((a.vec_mask >> t) & 1u) && left >= LG_ADAM_SPAN) {
        [[maybe_unused]] uint32_t vis[LG_ADAM_VEC];     // ROWS: bit c = element c of the lane's dwordx4 u is stepped
        if constexpr (ROWS) {
#pragma unroll
            for (int u = 0; u < LG_ADAM_VEC; u++) vis[u] = 0xFu;
            if (mask) lg_adam_span_vis(mask, rem, row_len, rcp, thr, vis);
        }
        lg_f4 p[LG_ADAM_VEC], g[LG_ADAM_VEC], m[LG_ADAM_VEC], v[LG_ADAM_VEC];
#pragma unroll
        for (int u = 0; u < LG_ADAM_VEC; u++) {
            if constexpr (ROWS) {
                p[u] = g[u] = m[u] = v[u] = lg_f4{ 0.0f, 0.0f, 0.0f, 0.0f };
                if (vis[u] == 0u) continue;
            }
            const int64_t i = base + (int64_t)(u * LG_ADAM_THREADS + (int)threadIdx.x) * 4;
#if LG_ADAM_NT_GRAD
            g[u] = __builtin_nontemporal_load((const lg_f4*)(G + i));
#else
            g[u] = *(const lg_f4*)(G + i);
#endif
            p[u] = *(const lg_f4*)(P + i);
            m[u] = *(const lg_f4*)(M + i);
            v[u] = *(const lg_f4*)(V + i);
        }
        __builtin_amdgcn_sched_barrier(0);              // every load of the span is in flight before the first dependent instruction
#pragma unroll
        for (int u = 0; u < LG_ADAM_VEC; u++) {
            if constexpr (ROWS) { if (vis[u] == 0u) continue; }
            const int64_t i = base + (int64_t)(u * LG_ADAM_THREADS + (int)threadIdx.x) * 4;
            float pe[4] = { p[u].x, p[u].y, p[u].z, p[u].w }, me[4] = { m[u].x, m[u].y, m[u].z, m[u].w };
            float ve[4] = { v[u].x, v[u].y, v[u].z, v[u].w };
            const float ge[4] = { g[u].x, g[u].y, g[u].z, g[u].w };
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if constexpr (ROWS) {
                    float pn = pe[c], mn = me[c], vn = ve[c];
                    lg_adam_element<DECOUPLED>(pn, ge[c], mn, vn, decay, step_size, bc2_sqrt, om_b1, b2, om_b2, eps);
                    const bool on = (vis[u] >> c) & 1u;     // an unseen element of a straddling dwordx4 stores the bits it loaded
                    pe[c] = on ? pn : pe[c]; me[c] = on ? mn : me[c]; ve[c] = on ? vn : ve[c];
                } else {
                    lg_adam_element<DECOUPLED>(pe[c], ge[c], me[c], ve[c], decay, step_size, bc2_sqrt, om_b1, b2, om_b2, eps);
                }
            }
            *(lg_f4*)(P + i) = lg_f4{ pe[0], pe[1], pe[2], pe[3] };
            *(lg_f4*)(M + i) = lg_f4{ me[0], me[1], me[2], me[3] };
            *(lg_f4*)(V + i) = lg_f4{ ve[0], ve[1], ve[2], ve[3] };
        }
    } else {
        const int n = (int)(left < LG_ADAM_SPAN ? left : LG_ADAM_SPAN);
        for (int k = (int)threadIdx.x; k < n; k += LG_ADAM_THREADS) {
            if constexpr (ROWS) { if (mask && mask[lg_adam_local_row(rem + (uint32_t)k, rcp, thr)] == 0) continue; }
            const int64_t i = base + k;
            float p = P[i], m = M[i], v = V[i];
            const float g = G[i];
            lg_adam_element<DECOUPLED>(p, g, m, v, decay, step_size, bc2_sqrt, om_b1, b2, om_b2, eps);
            P[i] = p; M[i] = m; V[i] = v;
        }
    }
}

template <bool DECOUPLED>
__global__ void __launch_bounds__(LG_ADAM_THREADS) lg_adam_kernel(const LgAdamTable a) { lg_adam_span<DECOUPLED, false>(a, nullptr); }

template <bool DECOUPLED>
__global__ void __launch_bounds__(LG_ADAM_THREADS) lg_adam_rows_kernel(const LgAdamRowsTable r) { lg_adam_span<DECOUPLED, true>(r.a, &r); }
