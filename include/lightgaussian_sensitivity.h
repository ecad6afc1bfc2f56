/* lightgaussian_sensitivity.h -- extension of the C ABI of liblightgaussian_hip.so (include/lightgaussian.h, same LG_ABI_VERSION): the
 * sensitivity pruning score of PUP 3D-GS, accumulated over the tile lists a forward left.  Error codes, lg_last_error(), the lg_view
 * flags and the stream argument are lightgaussian.h's.  DESIGN.md section 10.14 holds the contract and its reasons;
 * lightgaussian_amd/csrc/lg_math.h (lg_sensitivity_step, _moments_to_M, _AtMA, _logdet) writes every operation out in order.
 *
 * Per Gaussian i, theta_i = (mean3D, activated scale) in R^6:
 *     H_i   = sum_views sum_pixels sum_channels (dI_c/dtheta_i)(dI_c/dtheta_i)^T      the colours held constant
 *     score = log det H_i
 * dI/dtheta is what lg_backward computes for a one-hot image gradient: straight through the 0.99 clamp, pairs with power > 0 or
 * alpha < 1/255 take no part, the 1e-7 of the conic chain, no gradient through the +-1.3 tanfov clamp, the +0.3 blur.  The
 * view-direction term of SH colours and the opacity are not part of it.
 *
 * lg_sensitivity_accumulate: after a COLOUR forward of the same view (lg_forward / lg_forward_bounded without count outputs; geom,
 * binning, img and num_rendered as lg_backward takes them).  Adds the view's blocks into H [N][21] float64, the upper triangle of the
 * 6 x 6 block row-major, which the caller zeroes before the first view; a Gaussian without instances in the view keeps its H.  On the
 * stream: one back-to-front walk of the lists ("sensitivity_walk": twelve moments per (tile, Gaussian) instance, one plain store each),
 * then one lane per Gaussian ("sensitivity_accum").  scratch: lg_sensitivity_scratch_bytes(N, num_rendered), 16-byte aligned, nothing
 * of it is read before it is written.  A view the forward abandoned, or a segment_length other than the forward's, adds nothing.  No
 * atomics: bit-identical from run to run, and accumulating views one after another equals adding their separate blocks in float64.
 * LG_FLAG_FAST_EXP, LG_FLAG_RAW_PARAMS, LG_FLAG_DEBUG, LG_FLAG_PROFILE are honoured.
 * LG_ERR_INVALID_ARGUMENT, before any device call: what lg_backward refuses of a view and a model; a null H or scratch with N > 0;
 * cov3D_precomp (there are no scales to differentiate); a count forward's view (LG_FLAG_SKIP_COLOR, LG_FLAG_SCORE_MAX, a non-null count_sum: it leaves no
 * final_T / n_contrib of a colour blend); LG_FLAG_ANTIALIAS (the compensated opacity depends on the covariance: an opacity column).
 *
 * lg_sensitivity_score: out [N] float64 = 2 sum_k log L_kk of the Cholesky factor of H_i, plus 2 sum_k log scales[3 i + k] when scales
 * [N][3] (activated) is given: the block with respect to the log-scales is D H D, D = diag(1, 1, 1, s).  -inf at the first pivot that
 * is not above 2^-26 of its diagonal entry: a Gaussian that was never seen, or whose views do not span six directions. */
#ifndef LIGHTGAUSSIAN_SENSITIVITY_H
#define LIGHTGAUSSIAN_SENSITIVITY_H

#include "lightgaussian.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t lg_sensitivity_scratch_bytes(int32_t N, int64_t num_rendered);
int lg_sensitivity_accumulate(const lg_view* view, const lg_gaussians* g, const int32_t* radii, const void* geom, const void* binning,
                              const void* img, int64_t num_rendered, double* H, void* scratch, void* stream);
int lg_sensitivity_score(int32_t N, const double* H, const float* scales, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTGAUSSIAN_SENSITIVITY_H */
