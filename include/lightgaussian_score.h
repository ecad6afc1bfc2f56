/* lightgaussian_score.h -- extension of the C ABI of liblightgaussian_hip.so (include/lightgaussian.h, same LG_ABI_VERSION, same entry
 * points, same structs): one more bit of lg_view.flags, read by lg_forward_count and by lg_forward_bounded with count outputs.
 * DESIGN.md section 10.10 holds the contract and its reasons.
 *
 * LG_FLAG_SCORE_MAX -- max-contribution significance.  In a count forward whose weight policy is LG_WEIGHT_ALPHA or LG_WEIGHT_ALPHA_T,
 * out_score[j] is the MAXIMUM over the view's hits of Gaussian j of the hit's fp32 weight (alpha, or alpha T: the largest share the
 * Gaussian has of any pixel of the view -- RadSplat's pruning score once the caller takes the maximum over the views) instead of their
 * Q24.40 sum.  The value is one the blend computed: nothing is quantised or rounded, and a maximum does not depend on the order it is
 * taken in, so scores are bit-identical run to run, across kernel variants and across any partition of the views.  out_score[j] is 0
 * where out_count[j] == 0; out_count itself is unchanged, and so is the image of a count forward that keeps it.  The 2^24-pixel limit
 * of the sums does not apply.
 * LG_ERR_INVALID_ARGUMENT before any device call: with LG_WEIGHT_ONE / LG_WEIGHT_OPACITY in a count forward (the maximum of equal
 * addends is the addend: there is nothing to compute) and together with LG_FLAG_FAST_EXP in a count forward.  A colour forward ignores
 * the flag, as it ignores the weight policy.  Without the flag every kernel launched is unchanged. */
#ifndef LIGHTGAUSSIAN_SCORE_H
#define LIGHTGAUSSIAN_SCORE_H

enum { LG_FLAG_SCORE_MAX = 65536 };

#endif
