/* lightgaussian_mcmc.h -- extension of the C ABI of liblightgaussian_hip.so (include/lightgaussian.h, same LG_ABI_VERSION): 3DGS-MCMC
 * (Kheradmand et al., NeurIPS 2024) for float32 device tensors of a Gaussian model in its RAW form -- _xyz [N,3], _scaling [N,3]
 * log-scales, _rotation [N,4] as (r, x, y, z), _opacity [N,1] logits.  Error codes, lg_last_error(), LG_FLAG_PROFILE, the stream
 * argument and lg_densify_tensor are lightgaussian.h's.  DESIGN.md section 10.8 holds the contract and its reasons.
 *
 * --- position noise -----------------------------------------------------------------------------------
 * lg_mcmc_noise, ONE launch, in place on xyz, no read-back.  Per row, in float32 with every operation rounded on its own:
 *     sigma = 1 / (1 + exp(-opacity))      s = exp(scaling)      R = R(q / |q|), the rotation of lg_densify_rows' children
 *     g = 1 / (1 + exp(-k ((1 - sigma) - x0)))           (exp overflowing to +inf gives g = 0, not NaN)
 *     v = noise * (g c)                                  noise float32 [N,3], unit normal, drawn by the caller
 *     xyz += R (s^2 o (R^T v))                           = L L^T v with L = R diag(s): the published Sigma v, no 3x3 matrix stored
 * c = float(noise_lr * xyz_lr): evaluate the product in double and round once.  A row whose g c is exactly 0 keeps its bits (and is
 * not read beyond its opacity).  The published defaults are k = 100, x0 = 0.995.
 *
 * --- relocation and growth: one row movement ----------------------------------------------------------
 * n draws (dst[j], src[j]), int32 on the device: row dst[j] becomes a copy of row src[j].  Every dst[j] is distinct; every src[j]
 * lies in [0, N) and is never a destination.  cnt[i] = the number of j with src[j] == i, counted on the device.
 * lg_mcmc_plan counts and, for every row with cnt > 0, evaluates in DOUBLE from the float32 inputs, each output rounded once:
 *     M = min(cnt + 1, LG_MCMC_MAX_COPIES)      o = sigmoid(opacity)      x = 1 - (1 - o)^(1/M)
 *     D = sum_{k=0..M-1} C(M, k+1) (-1)^k x^(k+1) / sqrt(k+1)          (the published double sum, collapsed: C exact, x^k by products)
 *     opacity' = logit(clamp(x, min_opacity, 1 - 2^-23))                scaling' = scaling + log(o / D) per axis (x unclamped)
 * into scratch (lg_mcmc_scratch_bytes(N), 16-byte aligned); it reads the model and writes scratch only.  0 <= min_opacity < 1.
 * lg_mcmc_rows, one launch (grid.y = tensor), moves the rows of up to LG_DENSIFY_MAX_TENSORS tensors; call it after lg_mcmc_plan
 * with the same N, n, src and scratch.  tensors is a HOST array of lg_densify_tensor; rows of row_words 32-bit words (> 0; leave
 * empty tensors out), contiguous; role:
 *     LG_MCMC_COPY      a parameter that is only copied
 *     LG_MCMC_MOMENT    an Adam moment: zero at every source and every destination row
 *     LG_MCMC_OPACITY   _opacity, row_words 1: sources and their copies take opacity'
 *     LG_MCMC_SCALING   _scaling, row_words 3: sources and their copies take scaling'
 * N_out == N is the in-place form (relocation): src == dst for every tensor, every dst[j] in [0, N).  Afterwards every drawn row has
 * opacity' and scaling', row dst[j] of every tensor equals row src[j] after that update bit for bit, moments are zero at src U dst,
 * and every other word has the bits it had.
 * N_out > N is growth: dst tensors of N_out rows that do not overlap the src tensors of N rows, every dst[j] in [N, N_out).  The first
 * N rows are the old ones with the same update of the drawn rows (their moments zero), rows dst[j] as above; a row in [N, N_out) that
 * no dst[j] names is not written.
 * An index outside its range -- and, in place, a destination that is itself drawn -- is skipped on the device: neither read through
 * nor written.  Bit-identical from run to run (integer atomics in the count only).  N < 2^30, N_out < 2^31.
 * flags: LG_FLAG_PROFILE records "mcmc_noise", "mcmc_count", "mcmc_plan", "mcmc_rows", one entry per call that launches.
 * LG_ERR_INVALID_ARGUMENT, before any device call: a size outside its range, a null or misaligned pointer (float32 / int32: 4 bytes,
 * scratch: 16), a NaN among c, k, x0, a min_opacity outside [0, 1), an unknown role, a row_words the role does not take, src == dst
 * in growth or src != dst in place; the message names the argument. */
#ifndef LIGHTGAUSSIAN_MCMC_H
#define LIGHTGAUSSIAN_MCMC_H

#include "lightgaussian.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LG_MCMC_COPY 0
#define LG_MCMC_MOMENT 1
#define LG_MCMC_OPACITY 2
#define LG_MCMC_SCALING 3
#define LG_MCMC_MAX_COPIES 51

size_t lg_mcmc_scratch_bytes(int32_t N);
int lg_mcmc_noise(int32_t N, float* xyz, const float* scaling, const float* rotation, const float* opacity, const float* noise,
                  float c, float k, float x0, uint32_t flags, void* stream);
int lg_mcmc_plan(int32_t N, int32_t n, const int32_t* src, const float* opacity, const float* scaling, float min_opacity,
                 void* scratch, uint32_t flags, void* stream);
int lg_mcmc_rows(int32_t N, int64_t N_out, int32_t n, const int32_t* dst, const int32_t* src, const void* scratch,
                 int32_t num_tensors, const lg_densify_tensor* tensors /* host */, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTGAUSSIAN_MCMC_H */
