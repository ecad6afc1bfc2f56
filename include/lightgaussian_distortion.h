/* lightgaussian_distortion.h -- extension of the C ABI of liblightgaussian_hip.so (include/lightgaussian.h, same LG_ABI_VERSION): the
 * depth distortion term of 2DGS / GOF / PGSR / RaDe-GS and the median depth map, over the tile lists a forward left.  Error codes,
 * lg_last_error(), the lg_view flags and the stream argument are lightgaussian.h's.  DESIGN.md section 10.12 holds the contract and its
 * reasons; lightgaussian_amd/csrc/lg_math.h (lg_distortion_step, lg_distortion_bwd_step) writes every operation out in order.
 *
 * Per pixel, with the blending weights w_i = alpha_i T_i of the view's forward and a per-Gaussian scalar m_i = m[i * m_stride]
 * (m_stride >= 1 floats: a column of a feature tensor is passed without a copy):
 *     D      = sum_{i<j} w_i w_j (m_i - m_j)^2          accumulated about the pixel's first contributor (no cancellation)
 *     median = the m of the entry whose incoming T is the last above 0.5: the entry that carries T across one half, or the last
 *              contributor when T never gets there.  0 for a pixel without contributors.
 *
 * lg_blend_distortion: after a forward of the same view (geom / binning as lg_blend_features takes them).  distortion [H,W], median
 * [H,W] or NULL, state: lg_distortion_state_bytes(W, H) bytes, 16-byte aligned, opaque, read by lg_backward_distortion.  N == 0 and a
 * view the forward abandoned give zero maps.  LG_FLAG_FAST_EXP, LG_FLAG_DEBUG, LG_FLAG_PROFILE ("distortion_fwd") are honoured.
 *
 * lg_backward_distortion: lg_backward_features with two more losses.  Every argument up to dL_dfeatures is lg_backward_features' (C = 0
 * with NULL features / dL_dout / dL_dfeatures is allowed here); then m, m_stride and state as the forward had them, dL_ddistortion
 * [H,W] or NULL, dL_dmedian [H,W] or NULL, and dL_dm [N], written for every Gaussian (zeros without instances).  On the stream, in this
 * order: K7 when dL_dcolor is given; the feature walks when dL_dout or dL_dalpha is given; the distortion walk ("distortion_bwd") into
 * the same moment rows; K9 ONCE; dL_dfeatures; the dL_dm gather.  scratch: lg_backward_distortion_scratch_bytes(N, num_rendered, C).
 * The median passes its gradient to the m of the selected entry only.  An abandoned view, or a segment_length other than the
 * forward's, gives zero gradients.  No float atomics: bit-identical from run to run and across streams.
 * LG_ERR_INVALID_ARGUMENT, before any device call: what lg_backward_features refuses; C outside [0, LG_FEATURES_MAX]; a null m with
 * N > 0; m_stride < 1; a null state or dL_dm; a null distortion map. */
#ifndef LIGHTGAUSSIAN_DISTORTION_H
#define LIGHTGAUSSIAN_DISTORTION_H

#include "lightgaussian.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t lg_distortion_state_bytes(int32_t W, int32_t H);
int lg_blend_distortion(const lg_view* view, int32_t N, const void* geom, const void* binning, int64_t num_rendered, const float* m,
                        int32_t m_stride, float* distortion, float* median, void* state, void* stream);
size_t lg_backward_distortion_scratch_bytes(int32_t N, int64_t num_rendered, int32_t C);
int lg_backward_distortion(const lg_view* view, const lg_gaussians* g, const int32_t* radii, const void* geom, const void* binning,
                           const void* img, int64_t num_rendered, const float* dL_dcolor, const float* features, int32_t C,
                           const float* bg_features, const float* dL_dout, const float* dL_dalpha, float* dL_dmeans2D,
                           float* dL_dmeans3D, float* dL_dshs, float* dL_dcolors, float* dL_dopacity, float* dL_dscales,
                           float* dL_drotations, float* dL_dcov3D, float* dL_dshs_rest, float* dL_dfeatures, const float* m,
                           int32_t m_stride, const void* state, const float* dL_ddistortion, const float* dL_dmedian, float* dL_dm,
                           void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTGAUSSIAN_DISTORTION_H */
