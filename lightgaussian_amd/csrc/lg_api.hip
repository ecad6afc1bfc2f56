// lg_api.hip -- C ABI (include/lightgaussian.h) of the gfx950 (CDNA4, wave64) LightGaussian rasterizer.
// The single translation unit of liblightgaussian_hip.so; the kernels live in the headers it includes:
//   lg_math.h        scalar float arithmetic shared with the CPU test harness (canonical operation order); one copy each of the projection steps,
//                    the backward chain (lg_backward_chain), the SH backward steps (lg_sh_*) and the quaternion matrix (lg_quat_to_rot)
//   lg_plan.h        host-side plans of one forward, plain C++ (also compiled by the CPU tests): KeyPlan (sort-key layout), ForwardPlan (kernel variants)
//   lg_host.h        error strings, optional hipEvent profiler, scratch carving (GeomView / ImgView / BinView)
//   lg_wave.h        wave64 primitives (DPP reductions; lg_wave_scan_incl: the one wave prefix sum; lg_wave_all_max / _or; lg_block_scan_put / _get: the
//                    workgroup scan around the caller's barrier; lg_wave_lds_sync: the LDS hand-over inside a wave)
//   lg_rows.h        the four-rows-per-lane walk of the per-Gaussian row kernels (lg_rows4_walk / _load / _store: dwordx4, or dwords for a tail and
//                    for pointers off 16 bytes), its grid size and row limit; lg_f4, the float vector type of every kernel header
//   lg_preprocess.h  K1 lg_preprocess<RAW, DIRECT, AA>, K8+K9 lg_preprocess_bwd<RAW, JAC, AA> (AA: LG_FLAG_ANTIALIAS)   (per Gaussian, HBM-bound); lg_k9_*: K9's read side, shared with lg_camera.h;
//                    lg_sh_rows_flush: how dL/dSH rows leave LDS (K9 and lg_sh_grad_from_rgb_kernel)
//   lg_binning.h     K2 lg_scan_blocks, K3 lg_duplicate, lg_tile_sort / _long (second sort stage), lg_tile_ranges (one-stage cross-check only),
//                    lg_work_order (K2-K5 all hand-written; lg_sort.h = K4)
//   lg_loss.h        lg_loss_fwd / lg_loss_bwd: fused L1 + SSIM of the training step             (a wave per 64-column strip, register ring);
//                    lg_mean_finalize<Q>: the one ordered sum of per-wave partials in double (also lg_normal_loss's)
//   lg_prune.h       lg_select_pass, lg_v_imp_score_kernel, lg_prune_mask_kernel: device-resident prune epilogue (radix selects)
//   lg_knn.h         distCUDA2 (simple-knn): exact 3-nearest-neighbour mean squared distance on a multi-level uniform grid
//   lg_compact.h     lg_compact_plan / lg_compact_rows: one scan + one launch compacting all Gaussian tensors after a prune
//   lg_vq.h          lg_vq_nearest: nearest-code search of the VecTree quantiser on f32 MFMA (32x32x2), fused row argmin
//   lg_vq_train.h    lg_vq_ema_step: one EMA k-means step of the VecTree codebook (search, inverted index, ordered segmented sum, EMA)
//   lg_vq_color.h    lg_vq_colors: per-Gaussian colours of a VecTree-compressed model (fp16 row table + slot) through the same lg_sh_to_rgb as K1
//   lg_vq_color_bwd.h lg_vq_code_index / lg_vq_colors_bwd: its backward -- per-row gradients of the row table (ordered segmented sum over a
//                    per-model inverted index for the codebook rows) and the colour part of dL/dxyz
//   lg_adam.h        lg_adam_step: one Adam / AdamW step over all parameter tensors of the model in one launch (table by value, dwordx4);
//                    lg_adam_step_rows: the same step over the rows a byte mask names (row index: lg_adam_rows.h); both kernels are lg_adam_span<DECOUPLED, ROWS>
//   lg_densify.h     lg_densify_stats / lg_densify_plan / lg_densify_rows: view statistics and clone / split / prune of densify_and_prune
//   lg_mcmc.h        lg_mcmc_noise / lg_mcmc_plan / lg_mcmc_rows: 3DGS-MCMC position noise, relocation and growth (include/lightgaussian_mcmc.h)
//   lg_blend.h       K6 lg_blend_fwd<COUNT,FSCORE,EXACT,COLOR,MAX>, lg_score_kernel, K7 lg_blend_bwd<EXACT, ABS>   (per tile, VALU-bound); wave_reduce_via_lds<NV> (also lg_features.h's)
//   lg_features.h    lg_features_fwd / _bwd / _gather: C further per-Gaussian channels blended over the lists a forward left, and dL/dfeatures
//   lg_camera.h      lg_camera_bwd<RAW, AA> / lg_camera_reduce: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos from the rows a backward left, through lg_k9_* (float64 ordered sums)
//   lg_absgrad.h     lg_absgrad_rows: absolute screen-space mean gradients per Gaussian from floats 9, 10 of the rows K7<ABS> left (lg_backward_abs)
//   lg_filter3d.h    lg_filter3d_update / _apply / _apply_bwd: Mip-Splatting's 3D smoothing filter from the training cameras, and its raw -> raw
//                    (or activated) application to scales and opacity with its backward
//   lg_normals.h     lg_normal_rows / lg_depth_normals / lg_normal_loss and their backwards: view-space normals of the Gaussians, normals of a
//                    depth map, the fused depth-normal consistency loss (include/lightgaussian_normals.h; a wave per strip, register ring)
//   lg_distortion.h  lg_distortion_fwd / _bwd: depth distortion and median depth over the lists a forward left, and their gradient into K7's
//                    moment rows and a per-instance dm row (include/lightgaussian_distortion.h; lg_features.h's walks)
//   lg_sensitivity.h lg_sensitivity_walk / _accum / _score_kernel: the per-Gaussian 6 x 6 Gauss-Newton blocks over (mean, scale) from twelve moments
//                    per instance, and their log-determinants (include/lightgaussian_sensitivity.h; lg_features.h's back-to-front walk)
//   lg_tsdf.h        lg_tsdf_integrate / lg_mesh_count / lg_mesh_emit: depth maps of up to 8 views per pass into a dense TSDF volume, and marching
//                    tetrahedra over it with indexed vertices (include/lightgaussian_mesh.h; count, scan, emit: no atomics)
//   lg_blocks.h      lg_blocks_touch / _merge / _regrid / _integrate / _mesh_count / _mesh_emit: the same fusion and extraction over a block-sparse
//                    volume for unbounded scenes, blocks allocated from the depth maps and kept in sorted-key order (include/lightgaussian_blocks.h).
//                    The host side of the two volumes shares tsdf_views (one view checker), tsdf_batch (the by-value views of an integrate
//                    launch), mesh_args / mesh_counts_ptr / mesh_emit_args (the checks and the read-back of the count and emit calls) and
//                    carve_mesh (one scratch layout); each volume keeps its own volume check, tsdf_volume and block_volume
//
// Pipeline of one view:
//   K1 project + EWA + SH->RGB + exact footprint culling  ->  K2 scan of instance counts, blocking read of R
//   K3 packed keys tile|depth|id  ->  K4 stable keys-only radix passes over the TILE bits (the last one also leaves the tile ranges)
//   K5b every tile's list ordered by depth inside LDS (lg_tile_sort); the sorted keys ARE the per-tile lists (no id / slot arrays)
//   K6 front-to-back blend (4 autonomous waves per 16x16 tile, LDS queue, select-based pair step, ballot early exit)
//   K7 back-to-front replay (1 wave per tile, longest lists first, 4 px/lane, packed permlane reduction, one 48-B
//      gradient row per instance at its pre-sort slot, recomputed from the Gaussian's tile rectangle)
//   K9 per-Gaussian gather of its contiguous rows + cov2D/cov3D/projection/SH backward
// Written for wave64; no CUDA compatibility paths.
//
// Host side, what a new entry point plugs into: refuse(who, what) and check_view / sh_shape_ok for its refusals; view_state for the
// buffers a forward left; one *_kernel() selector and one launch line per templated kernel, KCHECK / KLAUNCHED behind it; GradOut /
// BackwardOpts for a backward; lg_sort_error_word (lg_sort.h) for a sort without view counters.
#include "lg_host.h"
#include "lg_wave.h"
#include "lg_rows.h"
#include "lg_preprocess.h"
#include "lg_binning.h"
#include "lg_blend.h"
#include "lg_loss.h"
#include "lg_prune.h"
#include "lg_knn.h"
#include "lg_compact.h"
#include "lg_vq.h"
#include "lg_vq_train.h"
#include "lg_vq_color.h"
#include "lg_vq_color_bwd.h"
#include "lg_adam.h"
#include "lg_densify.h"
#include "lg_mcmc.h"
#include "lg_features.h"
#include "lg_camera.h"
#include "lg_absgrad.h"
#include "lg_filter3d.h"
#include "lg_normals.h"
#include "lg_distortion.h"
#include "lg_sensitivity.h"
#include "lg_tsdf.h"
#include "lg_blocks.h"

// ------------------------------------------------------------------------------------------------
// host side
// What every entry point derives from (view, N): the tile grid, the padded grid of the per-tile kernels, the segment length and the
// Gaussian-id field of the list entries -- the backward and the lg_debug_* readers see what the forward saw.
struct ViewGeom { int W, H, gx, gy, ntiles, ntiles_pad, S, gid_bits; uint32_t gid_mask; };
static ViewGeom view_geom(const lg_view* v, int N)
{
    ViewGeom q;
    q.W = v->image_width; q.H = v->image_height;
    q.gx = (q.W + LG_TILE - 1) / LG_TILE; q.gy = (q.H + LG_TILE - 1) / LG_TILE;
    q.ntiles = (int)((int64_t)q.gx * q.gy);
    q.ntiles_pad = (int)(((int64_t)q.ntiles + LG_TILE_GRID_ALIGN - 1) / LG_TILE_GRID_ALIGN * LG_TILE_GRID_ALIGN); // grid of the per-tile kernels
    q.S = lg_segment_of(v);     // list entries per segment of a long tile (checkpoints for the backward): part of the view
    q.gid_bits = lg_gid_bits(N);
    q.gid_mask = lg_gid_mask(q.gid_bits);
    return q;
}

// The tests of the view alone that check_args and features_args both make, in this order; each caller words its own message.
enum ViewFault { VIEW_OK = 0, VIEW_BAD_SIZE, VIEW_BAD_SEGMENT, VIEW_TOO_LARGE };
static ViewFault check_view(const lg_view* v, int N)
{
    if (v->image_width <= 0 || v->image_height <= 0) return VIEW_BAD_SIZE;
    if (v->segment_length != 0 && (v->segment_length < 64 || v->segment_length % 64 != 0)) return VIEW_BAD_SEGMENT;
    const ViewGeom q = view_geom(v, N);
    return (q.gx >= 65536 || q.gy >= 65536) ? VIEW_TOO_LARGE : VIEW_OK;
}

// The state a forward left, as the entry points behind it see it: what view_geom derives and the three carved buffers.  The callers hold
// these buffers as const (they read them); this is the one place that casts.  NULL for a buffer the caller does not look at.
struct ViewState { ViewGeom q; GeomView geo; ImgView img; BinView bin; };
static ViewState view_state(const lg_view* v, int N, const void* geom_p, const void* img_p, const void* bin_p, int64_t R)
{
    ViewState s;
    s.q = view_geom(v, N);
    s.geo = carve_geom(const_cast<void*>(geom_p), N);
    s.img = carve_img(const_cast<void*>(img_p), s.q.W, s.q.H);
    s.bin = carve_bin(const_cast<void*>(bin_p), R, s.q.W, s.q.H, s.q.S);
    return s;
}

// M SH coefficients per channel evaluated up to degree D: what check_args, lg_sh_grad_from_rgb, lg_vq_colors and lg_vq_colors_bwd accept,
// each with its own message
static bool sh_shape_ok(int M, int D) { return (M == 1 || M == 4 || M == 9 || M == 16) && D >= 0 && D <= 3 && (D + 1) * (D + 1) <= M; }

static int check_args(const lg_view* v, const lg_gaussians* g)
{
    if (!v || !g) return fail(LG_ERR_INVALID_ARGUMENT, "null view/gaussians");
    const ViewFault vf = check_view(v, g->N);
    if (g->N < 0 || vf == VIEW_BAD_SIZE) return fail(LG_ERR_INVALID_ARGUMENT, "bad sizes");
    if (vf == VIEW_BAD_SEGMENT) return fail(LG_ERR_INVALID_ARGUMENT, "lg_view.segment_length must be 0 (default 512) or a multiple of 64");
    if ((v->flags & LG_FLAG_LONG_SERIAL) && (v->flags & LG_FLAG_LONG_PARALLEL))
        return fail(LG_ERR_INVALID_ARGUMENT, "LG_FLAG_LONG_SERIAL and LG_FLAG_LONG_PARALLEL exclude each other");
    if (g->N == 0) return LG_OK; // nothing to validate against: empty tensors carry no pointers
    if (g->N >= (1 << LG_ID_BITS)) return fail(LG_ERR_INVALID_ARGUMENT, "more than 2^29-1 Gaussians (the blend record packs the id in 29 bits)");
    if ((g->shs == nullptr) == (g->colors_precomp == nullptr))
        return fail(LG_ERR_INVALID_ARGUMENT, "Please provide excatly one of either SHs or precomputed colors!");
    const bool sr = g->scales != nullptr && g->rotations != nullptr;
    if ((g->scales != nullptr) != (g->rotations != nullptr) || sr == (g->cov3D_precomp != nullptr))
        return fail(LG_ERR_INVALID_ARGUMENT, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    if (g->shs_rest && !(v->flags & LG_FLAG_RAW_PARAMS)) return fail(LG_ERR_INVALID_ARGUMENT, "shs_rest needs LG_FLAG_RAW_PARAMS");
    if ((v->flags & LG_FLAG_RAW_PARAMS) && (g->cov3D_precomp || g->colors_precomp))
        return fail(LG_ERR_INVALID_ARGUMENT, "LG_FLAG_RAW_PARAMS takes raw scales/rotations/opacities and SH tensors only");
    if ((v->flags & LG_FLAG_RAW_PARAMS) && g->shs && g->M > 1 && !g->shs_rest)
        return fail(LG_ERR_INVALID_ARGUMENT, "LG_FLAG_RAW_PARAMS with M > 1 needs shs (dc) and shs_rest");
    if (g->shs) {
        if (!sh_shape_ok(g->M, 0)) return fail(LG_ERR_INVALID_ARGUMENT, "M must be 1, 4, 9 or 16");       // (degree 0 fits every M there is)
        if (!sh_shape_ok(g->M, v->sh_degree)) return fail(LG_ERR_INVALID_ARGUMENT, "sh_degree needs (D+1)^2 <= M, D <= 3");
    }
    if (!v->bg || !v->viewmatrix || !v->projmatrix || !v->campos || !g->means3D || !g->opacities)
        return fail(LG_ERR_INVALID_ARGUMENT, "missing required pointer");
    if (vf == VIEW_TOO_LARGE) return fail(LG_ERR_INVALID_ARGUMENT, "image too large");
    return LG_OK;
}


// 64-byte pinned host slots for the forward's read-back, recycled through a process-wide free list (a thread_local slot
// would be allocated -- and leaked -- by every short-lived host thread of the views-in-flight helpers).
static std::mutex g_pin_mu;
static std::vector<std::pair<uint32_t*, hipEvent_t>> g_pin_free;
struct PinnedSlot {
    uint32_t* p = nullptr;
    hipEvent_t ev = nullptr;   // marks the copy into p (validated bounded forward: the host waits for THIS, not for the stream)
    PinnedSlot()
    {
        {
            std::lock_guard<std::mutex> lk(g_pin_mu);
            if (!g_pin_free.empty()) { p = g_pin_free.back().first; ev = g_pin_free.back().second; g_pin_free.pop_back(); }
        }
        if (!p) {
            if (hipHostMalloc((void**)&p, 64, hipHostMallocDefault) != hipSuccess) { p = nullptr; return; }
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(p); p = nullptr; ev = nullptr; }
        }
    }
    ~PinnedSlot()
    {
        if (p) { std::lock_guard<std::mutex> lk(g_pin_mu); g_pin_free.emplace_back(p, ev); }
    }
    PinnedSlot(const PinnedSlot&) = delete;
    PinnedSlot& operator=(const PinnedSlot&) = delete;
};

// Behind every launch.  KLAUNCHED: the launch error alone -- the entry points without LG_FLAG_DEBUG never synchronise.
// KCHECK: the entry points that read LG_FLAG_DEBUG into a local `debug` also wait for `stream` under it and report the execution error.
#define KLAUNCHED(name)                                                                      \
    do {                                                                                     \
        hipError_t _e = hipGetLastError();                                                   \
        if (_e != hipSuccess) return fail(LG_ERR_DEVICE, name " launch", _e);                \
    } while (0)
#define KCHECK(name)                                                                         \
    do {                                                                                     \
        KLAUNCHED(name);                                                                     \
        if (debug) {                                                                         \
            hipError_t _e = hipStreamSynchronize(stream);                                    \
            if (_e != hipSuccess) return fail(LG_ERR_DEVICE, name " execution", _e);         \
        }                                                                                    \
    } while (0)

#define LG_STATUS_PENDING 0xFFFFFFFFu   // sentinel of the host-visible status word 0 (a real abort word has only its low bits set)

// ---- template selection: one place per kernel, and exactly the instantiations named here ----
static_assert(LG_W_ALPHA == LG_WEIGHT_ALPHA && LG_W_ALPHA_T == LG_WEIGHT_ALPHA_T, "ForwardPlan::fscore is the kernels' FSCORE");
using PreprocessKernel = decltype(&lg_preprocess<false, false, false>);
// (antialias: LG_FLAG_ANTIALIAS of the view -- carried beside the plans: ForwardPlan is pinned field by field)
static PreprocessKernel preprocess_kernel(bool raw, bool direct, bool antialias)
{
#define LG_K1(AA) { { lg_preprocess<false, false, AA>, lg_preprocess<false, true, AA> }, { lg_preprocess<true, false, AA>, lg_preprocess<true, true, AA> } }
    static const PreprocessKernel k[2][2][2] = { LG_K1(false), LG_K1(true) };     // [antialias][raw][direct]
#undef LG_K1
    return k[antialias][raw][direct];
}
using BlendFwdKernel = decltype(&lg_blend_fwd<false, 0, true, true>);
static BlendFwdKernel blend_fwd_kernel(const ForwardPlan& p)
{
    static const BlendFwdKernel color[2] = { lg_blend_fwd<false, 0, false, true>, lg_blend_fwd<false, 0, true, true> };    // [exact]
    static const BlendFwdKernel count_image[3][2] = { { lg_blend_fwd<true, 0, false, true>, lg_blend_fwd<true, 0, true, true> },   // [policy][exact]
                                                      { lg_blend_fwd<true, LG_W_ALPHA, false, true>, lg_blend_fwd<true, LG_W_ALPHA, true, true> },
                                                      { lg_blend_fwd<true, LG_W_ALPHA_T, false, true>, lg_blend_fwd<true, LG_W_ALPHA_T, true, true> } };
    static const BlendFwdKernel significance[3] = { lg_blend_fwd<true, 0, true, false>, lg_blend_fwd<true, LG_W_ALPHA, true, false>,
                                                    lg_blend_fwd<true, LG_W_ALPHA_T, true, false> };                           // [policy]
    // LG_FLAG_SCORE_MAX (ForwardPlan::fmax): the per-hit policies of a canonical count forward, with or without the image
    static const BlendFwdKernel score_max[2][2] = { { lg_blend_fwd<true, LG_W_ALPHA, true, false, true>, lg_blend_fwd<true, LG_W_ALPHA, true, true, true> },   // [policy][color]
                                                    { lg_blend_fwd<true, LG_W_ALPHA_T, true, false, true>, lg_blend_fwd<true, LG_W_ALPHA_T, true, true, true> } };
    const int w = p.fscore == LG_W_ALPHA ? 1 : p.fscore == LG_W_ALPHA_T ? 2 : 0;
    if (p.fmax) return score_max[w - 1][p.color];      // (exact: forward_impl refuses the flag with LG_FLAG_FAST_EXP)
    return !p.count ? color[p.exact] : p.color ? count_image[w][p.exact] : significance[w];
}
using BlendBwdKernel = decltype(&lg_blend_bwd<true, false>);
// (abs: lg_backward_abs alone -- the rows' floats 9 and 10 carry the absolute mean-gradient sums, lg_absgrad.h)
static BlendBwdKernel blend_bwd_kernel(bool exact, bool abs)
{
    static const BlendBwdKernel k[2][2] = { { lg_blend_bwd<false, false>, lg_blend_bwd<true, false> }, { lg_blend_bwd<false, true>, lg_blend_bwd<true, true> } };   // [abs][exact]
    return k[abs][exact];
}
using PreprocessBwdKernel = decltype(&lg_preprocess_bwd<false, false, false>);
static PreprocessBwdKernel preprocess_bwd_kernel(bool raw, bool jac, bool antialias)
{
#define LG_K9(AA) { { lg_preprocess_bwd<false, false, AA>, lg_preprocess_bwd<false, true, AA> }, { lg_preprocess_bwd<true, false, AA>, lg_preprocess_bwd<true, true, AA> } }
    static const PreprocessBwdKernel k[2][2][2] = { LG_K9(false), LG_K9(true) };  // [antialias][raw][jac]
#undef LG_K9
    return k[antialias][raw][jac];
}
using CameraBwdKernel = decltype(&lg_camera_bwd<false, false>);
static CameraBwdKernel camera_bwd_kernel(bool raw, bool antialias)
{
    static const CameraBwdKernel k[2][2] = { { lg_camera_bwd<false, false>, lg_camera_bwd<true, false> }, { lg_camera_bwd<false, true>, lg_camera_bwd<true, true> } };   // [antialias][raw]
    return k[antialias][raw];
}
using VqNearestKernel = decltype(&lg_vq_nearest_kernel<2>);
static VqNearestKernel vq_nearest_kernel(int dk2)      // dk2: lg_vq_dk2(d), one of these eight
{
    switch (dk2) {
        case 2: return lg_vq_nearest_kernel<2>;
        case 4: return lg_vq_nearest_kernel<4>;
        case 7: return lg_vq_nearest_kernel<7>;
        case 8: return lg_vq_nearest_kernel<8>;
        case 14: return lg_vq_nearest_kernel<14>;
        case 16: return lg_vq_nearest_kernel<16>;
        case 25: return lg_vq_nearest_kernel<25>;
        default: return lg_vq_nearest_kernel<32>;
    }
}
// the kernels with one variant per SH coefficient count M (1, 4, 9 or 16: sh_shape_ok)
#define LG_BY_M(KERNEL, M) ((M) == 1 ? KERNEL<1> : (M) == 4 ? KERNEL<4> : (M) == 9 ? KERNEL<9> : KERNEL<16>)
static decltype(&lg_vq_colors_kernel<1>) vq_colors_kernel(int M) { return LG_BY_M(lg_vq_colors_kernel, M); }
static decltype(&lg_vq_colors_bwd_rows_kernel<1>) vq_colors_bwd_rows_kernel(int M) { return LG_BY_M(lg_vq_colors_bwd_rows_kernel, M); }
static decltype(&lg_vq_colors_bwd_chunk_kernel<1>) vq_colors_bwd_chunk_kernel(int M) { return LG_BY_M(lg_vq_colors_bwd_chunk_kernel, M); }
#undef LG_BY_M
// the kernels with two variants
#define LG_BY_FLAG(KERNEL, on) ((on) ? KERNEL<true> : KERNEL<false>)
static decltype(&lg_vq_chunk_sum<false>) vq_chunk_sum_kernel(bool weighted) { return LG_BY_FLAG(lg_vq_chunk_sum, weighted); }
static decltype(&lg_adam_kernel<false>) adam_kernel(bool decoupled) { return LG_BY_FLAG(lg_adam_kernel, decoupled); }
static decltype(&lg_adam_rows_kernel<false>) adam_rows_kernel(bool decoupled) { return LG_BY_FLAG(lg_adam_rows_kernel, decoupled); }
static decltype(&lg_filter3d_apply_kernel<false>) filter3d_apply_kernel(bool raw) { return LG_BY_FLAG(lg_filter3d_apply_kernel, raw); }
static decltype(&lg_filter3d_apply_bwd_kernel<false>) filter3d_apply_bwd_kernel(bool raw) { return LG_BY_FLAG(lg_filter3d_apply_bwd_kernel, raw); }
static decltype(&lg_distortion_fwd<false>) distortion_fwd_kernel(bool exact) { return LG_BY_FLAG(lg_distortion_fwd, exact); }
static decltype(&lg_sensitivity_walk<false>) sensitivity_walk_kernel(bool exact) { return LG_BY_FLAG(lg_sensitivity_walk, exact); }
static decltype(&lg_sensitivity_accum<false>) sensitivity_accum_kernel(bool raw) { return LG_BY_FLAG(lg_sensitivity_accum, raw); }
#undef LG_BY_FLAG

// Arguments of the capacity-bounded forward (lg_forward_bounded); NULL = exact forward with its one read-back.
struct Bounded { void* binning; int64_t capacity; float max_depth; uint32_t* status; uint32_t* host_status; };

// One forward: forward_impl checks and fills the arguments, then runs the stages in order.  The stages read the two plans (lg_plan.h);
// none of them looks at v->flags to pick a kernel variant.
struct Forward {
    const lg_view* v; const lg_gaussians* g; const Bounded* bounded; lg_alloc_fn alloc; void* alloc_user; int weight_policy;
    float* out_color; int32_t* out_radii; int32_t* out_count; float* out_score; void** binning_out; int64_t* num_rendered;
    hipStream_t stream; bool debug, prof;
    int N, nblk; ViewGeom q; GeomView geo; ImgView img; BinView bin;
    KeyPlan kp; ForwardPlan plan;
    int64_t cap;            // instances the binning buffer holds: R itself (exact) or the caller's capacity (bounded)
    bool k1_cleared_sort;   // bounded forward: K1 also cleared the sort's histograms / tickets / states (the buffer and the key layout were known already)
    // validated bounded forward: K2 writes its four status words STRAIGHT into pinned host memory (system-scope release on word 0)
    // and the host waits for word 0 to leave its sentinel once everything of the view has been
    // enqueued -- no device-to-host copy node behind K2 (a 4 us blit kernel + its launch gap on the critical path of every view)
    PinnedSlot vslot;
    uint32_t* device_status() const { return bounded ? bounded->status : nullptr; }
    int front_end();    // K1, K2; the exact forward's read-back and allocation, or the bounded forward's buffer and status slot.  Leaves kp, plan, bin, cap
    int binning();      // duplicate, sort, tile ranges or tile sort
    int blend();        // K6 and its long-tile chain
    int score();
    int epilogue();     // LG_FLAG_DEBUG's look at the abort word; the validated forward's status words
};

int Forward::front_end()
{
    const bool count = out_count != nullptr;
    if (bounded) {
        if (!bounded->binning || bounded->capacity <= 0 || bounded->capacity >= (1ll << 30) || !(bounded->max_depth > 0.2f))
            return fail(LG_ERR_INVALID_ARGUMENT, "lg_forward_bounded: binning buffer, 0 < max_rendered < 2^30 and max_depth > 0.2 required");
        kp = make_key_plan(q.ntiles, N, __builtin_bit_cast(uint32_t, bounded->max_depth), v->flags);
        cap = bounded->capacity;
        bin = carve_bin(bounded->binning, cap, q.W, q.H, q.S);
        if (N == 0) {
            HIP_TRY(lg_zero_async(geo.counters, 16, stream));
            if (bounded->status) HIP_TRY(lg_zero_async(bounded->status, 16, stream));
            HIP_TRY(lg_zero_async(bin.ranges, (size_t)q.ntiles * 8, stream));
        }
    }
    // The exact forward learns its instance count from K2 and makes the plan again with it, below: until then it is the plan of a view
    // with instances.  K1 and K2 read only what does not depend on the count (k1_skip_color, k1_clears_count: tests/test_forward_plan.py).
    plan = make_forward_plan(v->flags, count, weight_policy, N, bounded ? cap : 1);
    const bool host_words = bounded && bounded->host_status;
    if (host_words) {
        if (!vslot.p) return fail(LG_ERR_ALLOC, "hipHostMalloc of the status slot failed");
        if (N > 0) { vslot.p[1] = vslot.p[2] = vslot.p[3] = 0u; __atomic_store_n(&vslot.p[0], LG_STATUS_PENDING, __ATOMIC_RELEASE); }
        else memset(vslot.p, 0, 16);
    }
    uint32_t* k1_clear = nullptr;
    uint32_t k1_nclear = 0;
    if (bounded && plan.live) {
        k1_clear = (uint32_t*)bin.sort_temp;
        k1_nclear = (uint32_t)(lg_sort_clear_bytes(lg_sort_layout((size_t)cap), (unsigned)kp.sort_passes()) / 4);
    }
    k1_cleared_sort = k1_clear != nullptr;
    if (N > 0) {
        {
            ProfScope ps(prof, "preprocess", stream);
            // SH rows are read directly by their lanes (dword-aligned dwordx4 loads); LG_K1_LDS=1 selects the LDS-staged reads
            const bool direct = !(v->flags & LG_FLAG_K1_LDS), raw = v->flags & LG_FLAG_RAW_PARAMS;
            // K1 runs faster with FEWER waves in flight where it reads SH rows: unused dynamic LDS caps it at 12 waves per CU there (the sweep,
            // K9's opposite behaviour and the significance pass's A/B: EXPERIMENTS.md, "K1 / K9")
            const size_t k1_dyn = (direct && g->shs && !g->colors_precomp && !plan.k1_skip_color) ? LG_K1_PAD_LDS : 0;
            preprocess_kernel(raw, direct, v->flags & LG_FLAG_ANTIALIAS)<<<nblk, LG_PP, k1_dyn, stream>>>(
                N, g->M, v->sh_degree, q.W, q.H, v->tanfovx, v->tanfovy, v->scale_modifier, v->prefiltered, plan.k1_skip_color ? 1 : 0, v->viewmatrix,
                v->projmatrix, v->campos, g->means3D, g->shs, g->shs_rest, g->colors_precomp, g->opacities, g->scales, g->rotations, g->cov3D_precomp, geo,
                out_radii, plan.k1_clears_count ? out_count : nullptr, out_score, k1_clear, k1_nclear, (v->flags & LG_FLAG_SAVE_SH_JACOBIAN) ? 1 : 0);
        }
        KCHECK("lg_preprocess");
        {
            // K2: one workgroup scans the per-K1-workgroup instance counts and reduces the depth maxima (replaces a
            // device-wide scan of N words + a separate reduction kernel)
            ProfScope ps(prof, "scan", stream);
            lg_scan_blocks<<<(nblk + LG_PART - 1) / LG_PART, LG_PART, 0, stream>>>(nblk, geo.blk_sum, geo.blk_dmax, geo.blk_off, geo.part_sum,
                                                                                  geo.part_dmax, geo.part_prefix, geo.counters + 8,
                                                                                  bounded ? (uint32_t)cap : 0xFFFFFFFFu,
                                                                                  bounded ? kp.depth_bits : 32, geo.counters,
                                                                                  host_words ? vslot.p : device_status());
        }
        KCHECK("lg_scan_blocks");
    }
    if (!bounded) {
        uint32_t h_counters[4] = {0, 0, 0, 0};
        if (N > 0) {
            // The exact forward has ONE blocking read-back: the instance count R (it sizes the binning buffer), with the
            // depth maximum and the prefiltered flag riding along in one 16-byte copy into pinned host memory.
            // lg_forward_bounded has none.
            PinnedSlot slot;                                      // process-wide pool: host threads come and go (views in flight)
            if (!slot.p) return fail(LG_ERR_ALLOC, "hipHostMalloc of the read-back slot failed");
            HIP_TRY(hipMemcpyAsync(slot.p, geo.counters, 16, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            for (int k = 0; k < 4; k++) h_counters[k] = slot.p[k];
            if (v->prefiltered && h_counters[1]) return fail(LG_ERR_PREFILTERED, "Point is filtered although prefiltered is set. This shouldn't happen!");
            if (h_counters[0] & 1u) return fail(LG_ERR_INVALID_ARGUMENT, "more than 2^32-1 tile instances in one view");
        }
        cap = h_counters[3];
        if (cap >= (1ll << 30)) return fail(LG_ERR_INVALID_ARGUMENT, "more than 2^30-1 tile instances in one view");
        kp = make_key_plan(q.ntiles, N, h_counters[2], v->flags);
        plan = make_forward_plan(v->flags, count, weight_policy, N, cap);
        void* bin_p = alloc(alloc_user, carve_bin(nullptr, cap, q.W, q.H, q.S).total);
        if (!bin_p) return fail(LG_ERR_ALLOC, "binning allocator returned NULL");
        if (binning_out) *binning_out = bin_p;
        bin = carve_bin(bin_p, cap, q.W, q.H, q.S);
        if (num_rendered) *num_rendered = cap;
        if (cap == 0) HIP_TRY(lg_zero_async(bin.ranges, (size_t)q.ntiles * 8, stream)); // otherwise cleared by lg_duplicate
    }
    // (bounded->status is written by lg_scan_blocks itself, or cleared above for N == 0: no copy node; validated mode: K2 wrote the
    // words into vslot.p itself and the host looks at them in epilogue())
    g_stats.num_rendered = bounded ? -1 : cap;
    g_stats.num_visible = -1; // not tracked on the device (see lg_preprocess); callers count radii > 0
    return LG_OK;
}

int Forward::binning()
{
    if (!plan.live) return LG_OK;
    const int sort_begin = kp.sort_begin(), sort_end = kp.sort_end();
    const LgSortLayout SL = lg_sort_layout((size_t)cap);
    // one clear for the digit histograms, the tile tickets and the look-back states of every radix pass (exact forward: the
    // buffer was allocated a moment ago; the bounded forward's K1 did it already)
    if (!k1_cleared_sort) HIP_TRY(lg_zero_async(bin.sort_temp, lg_sort_clear_bytes(SL, (unsigned)kp.sort_passes()), stream));
    uint32_t* hist = (uint32_t*)((char*)bin.sort_temp + SL.hist_off);
    {
        ProfScope ps(prof, "duplicate", stream);
        const int dgrid = std::max(1, std::min((nblk + 4 * LG_DUP_WAVES - 1) / (4 * LG_DUP_WAVES), LG_DUP_GRID));
        lg_duplicate<<<dgrid, LG_DUP_THREADS, 0, stream>>>(N, nblk, q.gx, kp.stored(), kp.store_drop, kp.gid_bits, sort_begin, sort_end, (uint32_t)cap, geo.touched,
                                                          geo.blk_off, geo.part_prefix, geo.counters, geo.offsets, geo.tinfo, bin.keys_in, q.ntiles, bin.ranges, hist,
                                                          kp.two_stage ? 0xFFFFFFFFu : 0u, bin.long_tiles);
    }
    KCHECK("lg_duplicate");
    {
        ProfScope ps(prof, "sort", stream);
        size_t tb = bin.sort_temp_bytes;
        // two-stage scheme: the last pass also leaves the tile ranges (no lg_tile_ranges launch)
        HIP_TRY(lg_sort_keys(bin.sort_temp, tb, bin.keys_in, bin.entries, (uint32_t)cap, sort_begin, sort_end, geo.counters, true, stream,
                             LG_SORT_POLL_BUDGET, kp.two_stage ? bin.ranges : nullptr, kp.tile_shift()));
    }
    KCHECK("lg_sort_keys");
    if (!kp.two_stage) {
        ProfScope ps(prof, "tile_ranges", stream);
        const uint32_t rgrid = (uint32_t)((cap + 255) / 256);
        lg_tile_ranges<<<rgrid, 256, 0, stream>>>(geo.counters, kp.tile_shift(), kp.gid_bits, kp.gid_mask, kp.store_drop, kp.store_drop,
                                                  bin.entries, bin.keys_in, geo.tinfo, bin.ranges, device_status());
    } else {
        // second stage: one WAVE per tile orders its list by depth in LDS (lists up to 1024 entries; up to 4096: a whole workgroup,
        // same launch); the few longer ones go through a persistent grid of 1024-thread workgroups (an empty launch otherwise)
        ProfScope ps(prof, "tile_sort", stream);
        lg_tile_sort<<<(q.ntiles + 3) / 4 + q.ntiles, LG_TS_THREADS, 0, stream>>>(q.ntiles, geo.counters, bin.ranges, bin.entries, kp.gid_bits, kp.gid_mask, kp.store_drop,
                                                                                  kp.depth_bits, geo.tinfo, bin.long_tiles, device_status());
        lg_tile_sort_long<<<std::min(q.ntiles, LG_TL_GRID), LG_TL_THREADS, 0, stream>>>(geo.counters, bin.ranges, bin.entries, bin.keys_in, kp.gid_bits, kp.gid_mask,
                                                                                        kp.store_drop, kp.depth_bits, geo.tinfo, bin.long_tiles);
    }
    KCHECK("lg_tile_sort");
    return LG_OK;
}

int Forward::blend()
{
    const int W = q.W, H = q.H, gx = q.gx, S = q.S;
    const uint32_t gid_mask = kp.gid_mask;
    {
        // (count / score accumulators of the count variant were cleared by lg_preprocess; the slots of the per-hit variants that do not merge, here)
        ProfScope ps(prof, plan.count ? "blend_fwd_count" : "blend_fwd", stream);
        if (plan.clear_slots) HIP_TRY(lg_zero_async(bin.keys_in, (size_t)cap * 8, stream));
        const dim3 grid(q.ntiles_pad + (plan.work_list_group ? 1 : 0)), block(256);
        blend_fwd_kernel(plan)<<<grid, block, 0, stream>>>(W, H, gx, q.ntiles, q.ntiles_pad, bin.ranges, bin.entries, gid_mask, geo.rec, v->bg, out_color, img.final_T,
                                                           img.n_contrib, out_count, (unsigned long long*)bin.keys_in, geo.tinfo, (uint32_t)cap, S, bin.ckpt,
                                                           bin.work, bin.meta, bin.par_work, geo.counters, plan.long_mode, bin.par_arrived);
    }
    KCHECK("lg_blend_fwd");
    // (a second HIP stream for the long-tile chain / for the memory-bound front of other views: EXPERIMENTS.md, "streams")
    // persistent grids over the par_work list left by the forward's work-list workgroup (meta[4] items; none on scenes
    // without outlier lists: each launch is then one scalar load per workgroup)
    const uint32_t pgrid = (uint32_t)std::min<int64_t>((int64_t)q.ntiles + cap / S + 1, LG_PAR_GRID);
    if (plan.long_chain == LG_CHAIN_COUNT) {
        ProfScope ps(prof, "blend_fwd_count_long", stream);
        const float band_mul = (v->flags & LG_FLAG_COUNT_WIDE_BAND) ? 4096.0f : 1.0f;
        lg_count_seg<<<pgrid, 256, 0, stream>>>(W, H, gx, S, bin.par_work, bin.meta, bin.ranges, bin.entries, gid_mask, geo.rec, bin.ckpt, bin.ckpt_last, bin.par_arrived, band_mul);
        lg_count_rewalk<<<pgrid, 256, 0, stream>>>(W, H, gx, S, bin.par_work, bin.meta, bin.ranges, bin.entries, gid_mask, geo.rec, bin.ckpt, bin.ckpt_last, out_count, band_mul);
        lg_count_fixup<<<std::min<uint32_t>(pgrid, 256u), 256, 0, stream>>>(W, H, gx, S, bin.par_work, bin.meta, bin.ranges, bin.entries, gid_mask, geo.rec, bin.ckpt_last, out_count);
        KCHECK("lg_count_long");
    } else if (plan.long_chain == LG_CHAIN_COLOR) {
        ProfScope ps(prof, "blend_fwd_long", stream);
        // (pass 2, the per-tile scan, runs inside the first launch: the workgroup that finishes a tile's last segment does it)
        lg_blend_fwd_seg<<<pgrid, 256, 0, stream>>>(W, H, gx, S, bin.par_work, bin.meta, bin.ranges, bin.entries, gid_mask, geo.rec, bin.ckpt, bin.ckpt_last,
                                                   bin.par_arrived, v->bg, out_color, img.final_T, img.n_contrib);
        lg_blend_fwd_rewalk<<<pgrid, 256, 0, stream>>>(W, H, gx, S, bin.par_work, bin.meta, bin.ranges, bin.entries, gid_mask, geo.rec, v->bg,
                                                      out_color, img.final_T, img.n_contrib, bin.ckpt, bin.ckpt_last);
        KCHECK("lg_blend_fwd_long");
    }
    return LG_OK;
}

int Forward::score()
{
    if (plan.score == LG_SCORE_NONE) return LG_OK;
    {
        ProfScope ps(prof, "score", stream);
        if (plan.score == LG_SCORE_SLOTS_MAX)
            lg_score_slots<true><<<(N + 255) / 256, 256, 0, stream>>>(N, geo.touched, geo.offsets, (const unsigned long long*)bin.keys_in, (uint32_t)cap, out_count, out_score, v->count_sum, geo.counters);
        else if (plan.score == LG_SCORE_SLOTS)
            lg_score_slots<false><<<(N + 255) / 256, 256, 0, stream>>>(N, geo.touched, geo.offsets, (const unsigned long long*)bin.keys_in, (uint32_t)cap, out_count, out_score, v->count_sum, geo.counters);
        else
            lg_score_kernel<<<(N + 255) / 256, 256, 0, stream>>>(N, out_count, plan.score == LG_SCORE_COUNT_OPACITY ? g->opacities : nullptr, out_score, v->count_sum);
    }
    KCHECK("lg_score_kernel");
    return LG_OK;
}

int Forward::epilogue()
{
    if (debug && N > 0) {
        // debug: the abort word as it stands at the END of the view (the radix sort's look-back can only report after K2)
        uint32_t h_abort = 0;
        HIP_TRY(hipMemcpyAsync(&h_abort, geo.counters, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (h_abort & LG_ABORT_SORT) return fail(LG_ERR_DEVICE, "radix sort look-back gave up (a predecessor tile never published): the view is void");
    }
    if (bounded && bounded->host_status) {
        // K2's words arrive while the blend kernels are still running.  Spin on word 0 (written last, released system-wide); every
        // few thousand polls ask the stream whether it is still working, so that a device error cannot turn into a host hang
        uint32_t w0 = __atomic_load_n(&vslot.p[0], __ATOMIC_ACQUIRE);
        for (uint64_t spins = 1; w0 == LG_STATUS_PENDING; spins++) {
            if ((spins & 0xFFFu) == 0u) {
                const hipError_t q = hipStreamQuery(stream);
                if (q != hipErrorNotReady) {                       // stream drained (or failed): the words are final
                    w0 = __atomic_load_n(&vslot.p[0], __ATOMIC_ACQUIRE);
                    if (w0 == LG_STATUS_PENDING) return fail(LG_ERR_DEVICE, "lg_forward_bounded: the status words never arrived", q);
                    break;
                }
            }
            __builtin_ia32_pause();
            w0 = __atomic_load_n(&vslot.p[0], __ATOMIC_ACQUIRE);
        }
        bounded->host_status[0] = w0;
        for (int k = 1; k < 4; k++) bounded->host_status[k] = vslot.p[k];
        g_stats.num_rendered = vslot.p[3];
    }
    return LG_OK;
}

static int forward_impl(const lg_view* v, const lg_gaussians* g, void* geom_p, void* img_p, lg_alloc_fn alloc, void* alloc_user,
                        const Bounded* bounded, int weight_policy, float* out_color, int32_t* out_radii, int32_t* out_count,
                        float* out_score, void** binning_out, int64_t* num_rendered, void* stream_p)
{
    int rc = check_args(v, g);
    if (rc != LG_OK) return rc;
    if (!geom_p || !img_p || !out_color || (!out_radii && g->N > 0) || (!alloc && !bounded)) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    const bool count = out_count != nullptr;
    if (count && !out_score) return fail(LG_ERR_INVALID_ARGUMENT, "count needs score");
    if (count && (weight_policy < 0 || weight_policy > 3)) return fail(LG_ERR_INVALID_ARGUMENT, "bad weight policy");
    // LG_FLAG_SCORE_MAX on a count forward: a per-hit policy (the maximum of equal addends is the addend) with the canonical exp (Python never
    // issues a hardware-exp count forward, and its maximum could not be pinned).  A colour forward ignores the flag, as it ignores the policy.
    const bool score_max = count && (v->flags & LG_FLAG_SCORE_MAX);
    if (score_max && weight_policy < LG_WEIGHT_ALPHA) return fail(LG_ERR_INVALID_ARGUMENT, "LG_FLAG_SCORE_MAX needs LG_WEIGHT_ALPHA or LG_WEIGHT_ALPHA_T");
    if (score_max && (v->flags & LG_FLAG_FAST_EXP)) return fail(LG_ERR_INVALID_ARGUMENT, "LG_FLAG_SCORE_MAX with LG_FLAG_FAST_EXP in a count forward");
    // per-hit weights are summed in Q24.40 per view: a Gaussian can collect at most 0.99 per pixel (a maximum has no such limit)
    if (count && !score_max && weight_policy >= LG_WEIGHT_ALPHA && (int64_t)v->image_width * v->image_height > (1ll << 24))
        return fail(LG_ERR_INVALID_ARGUMENT, "ALPHA / ALPHA_T weights: images beyond 2^24 pixels overflow the Q24.40 per-view sums");
    Forward f{};
    f.v = v; f.g = g; f.bounded = bounded; f.alloc = alloc; f.alloc_user = alloc_user; f.weight_policy = weight_policy;
    f.out_color = out_color; f.out_radii = out_radii; f.out_count = out_count; f.out_score = out_score;
    f.binning_out = binning_out; f.num_rendered = num_rendered;
    f.stream = (hipStream_t)stream_p; f.debug = v->flags & LG_FLAG_DEBUG; f.prof = v->flags & LG_FLAG_PROFILE;
    f.N = g->N; f.nblk = (f.N + LG_PP - 1) / LG_PP;
    f.q = view_geom(v, f.N);
    f.geo = carve_geom(geom_p, f.N);
    f.img = carve_img(img_p, f.q.W, f.q.H);
    if (binning_out) *binning_out = nullptr;
    if (num_rendered) *num_rendered = 0;
    if ((rc = f.front_end()) != LG_OK || (rc = f.binning()) != LG_OK || (rc = f.blend()) != LG_OK || (rc = f.score()) != LG_OK) return rc;
    return f.epilogue();
}


extern "C" int lg_forward(const lg_view* view, const lg_gaussians* g, void* geom, void* img, lg_alloc_fn alloc, void* alloc_user,
                          float* out_color, int32_t* out_radii, void** binning_out, int64_t* num_rendered, void* stream)
{
    return forward_impl(view, g, geom, img, alloc, alloc_user, nullptr, LG_WEIGHT_OPACITY, out_color, out_radii, nullptr, nullptr, binning_out,
                        num_rendered, stream);
}

extern "C" int lg_forward_count(const lg_view* view, const lg_gaussians* g, void* geom, void* img, lg_alloc_fn alloc, void* alloc_user,
                                int32_t weight_policy, float* out_color, int32_t* out_radii, int32_t* out_count, float* out_score,
                                void** binning_out, int64_t* num_rendered, void* stream)
{
    if (g && g->N > 0 && (!out_count || !out_score)) return fail(LG_ERR_INVALID_ARGUMENT, "count/score outputs required");
    return forward_impl(view, g, geom, img, alloc, alloc_user, nullptr, weight_policy, out_color, out_radii, out_count, out_score, binning_out,
                        num_rendered, stream);
}

extern "C" int lg_forward_bounded(const lg_view* view, const lg_gaussians* g, void* geom, void* img, void* binning, int64_t max_rendered,
                                  float max_depth, int32_t weight_policy, float* out_color, int32_t* out_radii, int32_t* out_count,
                                  float* out_score, uint32_t* status, uint32_t* host_status, void* stream)
{
    if (g && g->N > 0 && ((out_count == nullptr) != (out_score == nullptr))) return fail(LG_ERR_INVALID_ARGUMENT, "count and score go together");
    const Bounded b = { binning, max_rendered, max_depth, status, host_status };
    return forward_impl(view, g, geom, img, nullptr, nullptr, &b, weight_policy, out_color, out_radii, out_count, out_score, nullptr, nullptr, stream);
}

// the nine per-Gaussian gradient outputs of a backward, in the order of the C ABI's dL_d* arguments (the Python side's _GradSet.SLOTS)
struct GradOut { float *means2D, *means3D, *shs, *colors, *opacity, *scales, *rotations, *cov3D, *shs_rest; };
// what lg_backward_features adds to a backward: a loss on the feature image and / or on alpha (lg_features_bwd_geom, lg_features.h)
struct FeatGrad { const float* features; int C; const float* bg; const float* dL_dout; const float* dL_dalpha; };
// the rest of a backward call: K9's chunks and their callback (lg_backward_chunked), lg_backward_features' losses, lg_backward_abs' output
// what lg_backward_distortion adds: a loss on the distortion and / or the median map (lg_distortion_bwd, lg_distortion.h); dm_rows [R]
struct DistGrad { const float* m; int m_stride; const void* state; const float* dL_dD; const float* dL_dmed; float* dm_rows; };
struct BackwardOpts { int chunks; lg_chunk_fn on_chunk; void* user; const FeatGrad* fg = nullptr; float* means2D_abs = nullptr; const DistGrad* dg = nullptr; };

// K9 (lg_preprocess_bwd) over the moment rows [R][12] a blend backward left: sums every Gaussian's rows and chains them to every input.
// Shared by lg_backward / lg_backward_chunked (rows from K7) and lg_backward_features (rows from K7 and / or lg_features_bwd_geom).
static void preprocess_bwd_launch(const lg_view* v, const lg_gaussians* g, const int32_t* radii, const ViewState& s, const float* rows, const GradOut& d,
                                  bool rgb_only, hipStream_t stream, const BackwardOpts& o)
{
    const ViewGeom& q = s.q; const GeomView& geo = s.geo; const BinView& bin = s.bin;
    // K9 runs over Gaussian ranges: `chunks` launches of consecutive 64-Gaussian workgroups.  After each launch is enqueued
    // the caller is told (on_chunk): rows [first, first + count) of every gradient tensor are final once the stream reaches
    // that point -- a data-parallel trainer starts their all-reduce there, while K9 computes the next range.
    const int N = g->N, W = q.W, H = q.H, S = q.S;
    ProfScope ps(v->flags & LG_FLAG_PROFILE, "preprocess_bwd", stream);
    const int nblk = (N + LG_PP - 1) / LG_PP;
    const int chunks = std::max(1, std::min(o.chunks, nblk));
    const int per = (nblk + chunks - 1) / chunks;
    for (int first_blk = 0; first_blk < nblk; first_blk += per) {
        const int nb = std::min(per, nblk - first_blk);
        // (the view of a backward is the view of its forward: LG_FLAG_SAVE_SH_JACOBIAN says K1 left the SH direction Jacobians)
        const bool jac = (v->flags & LG_FLAG_SAVE_SH_JACOBIAN) && g->shs && (d.shs || rgb_only);
        preprocess_bwd_kernel(v->flags & LG_FLAG_RAW_PARAMS, jac, v->flags & LG_FLAG_ANTIALIAS)<<<nb, LG_PP, 0, stream>>>(
            N, first_blk, g->M, v->sh_degree, W, H, v->tanfovx, v->tanfovy, v->scale_modifier, v->viewmatrix, v->projmatrix, v->campos, g->means3D,
            g->shs, g->shs_rest, g->colors_precomp, g->opacities, g->scales, g->rotations, g->cov3D_precomp, radii, geo.rec, geo.counters, bin.meta,
            (uint32_t)S, geo.touched, geo.offsets, reinterpret_cast<const float4*>(rows), geo.shjac, d.means2D, d.means3D, d.shs, d.shs_rest,
            d.colors, d.opacity, d.scales, d.rotations, d.cov3D);
        if (o.on_chunk) o.on_chunk(o.user, first_blk * LG_PP, std::min(N - first_blk * LG_PP, nb * LG_PP));
    }
}

// ---- the walks over the lists of a forward (lg_features.h, lg_distortion.h): what their entry points (below) and backward_impl share ----
static int features_args(const char* who, const lg_view* v, int32_t N, const void* geom_p, const void* bin_p, int64_t R, int32_t C)
{
    const char* what = nullptr;
    const ViewFault vf = v ? check_view(v, N) : VIEW_OK;
    if (!v) what = "null view";
    else if (C < 1 || C > LG_FEATURES_MAX) what = "C must be 1 .. LG_FEATURES_MAX (64) channels";
    else if (N < 0 || N >= (1 << LG_ID_BITS)) what = "N out of range";
    else if (R < 0 || R >= (1ll << 30)) what = "num_rendered out of range";
    else if (vf == VIEW_BAD_SIZE) what = "bad image size";
    else if (vf == VIEW_BAD_SEGMENT) what = "lg_view.segment_length must be 0 or a multiple of 64";
    else if (!geom_p) what = "missing geom buffer";
    else if (N > 0 && R > 0 && !bin_p) what = "missing binning buffer";
    else if (vf == VIEW_TOO_LARGE) what = "image too large";
    return what ? refuse(who, what) : LG_OK;
}
// what a loss on the feature image needs (lg_backward_features, lg_backward_distortion)
static int features_grad_args(const char* who, int32_t N, const float* features, const float* dL_dout, const float* dL_dfeatures)
{
    if (N > 0 && !features && (dL_dout || dL_dfeatures)) return refuse(who, "missing features");
    if (N > 0 && dL_dfeatures && !dL_dout) return refuse(who, "dL_dfeatures without dL_dout");
    return LG_OK;
}
static LgFeatView features_view(const ViewState& s, int32_t N, int64_t R)
{
    LgFeatView f; const ViewGeom& q = s.q; const GeomView& geo = s.geo;
    f.W = q.W; f.H = q.H; f.gx = q.gx; f.ntiles = q.ntiles; f.N = N;
    f.live = (N > 0 && R > 0 && s.bin.ranges) ? 1 : 0;      // (ranges is the head of the binning buffer: NULL without one)
    f.cap = (uint32_t)R; f.gid_mask = q.gid_mask;
    f.rec = geo.rec; f.counters = geo.counters;
    f.ranges = f.live ? s.bin.ranges : nullptr; f.entries = f.live ? s.bin.entries : nullptr;
    return f;
}
// what a call that launches walks sets out with, taken apart by name where it is used (KCHECK reads `debug` and `stream`)
struct WalkCall { hipStream_t stream; bool debug, prof, exact; ViewState s; LgFeatView f; };
static WalkCall walk_call(const lg_view* v, int32_t N, const void* geom_p, const void* img_p, const void* bin_p, int64_t R, void* stream_p)
{
    const ViewState s = view_state(v, N, geom_p, img_p, bin_p, R);
    return { (hipStream_t)stream_p, bool(v->flags & LG_FLAG_DEBUG), bool(v->flags & LG_FLAG_PROFILE), !(v->flags & LG_FLAG_FAST_EXP), s, features_view(s, N, R) };
}
// the state of lg_blend_distortion: float4 (A, P1, P2, c) [H W] | uint32 med_pos [H W]
static size_t distortion_state_head(int W, int H) { return align_up((size_t)W * (size_t)H * sizeof(float4)); }
// channels of the next walk when rem are left: as many as the registers take -- one walk up to 32 channels, two up to 64
static int features_channel_group(int rem) { return rem <= 4 ? 4 : rem <= 16 ? 16 : 32; }
using FeaturesFwdKernel = decltype(&lg_features_fwd<4, true>);
static FeaturesFwdKernel features_fwd_kernel(int cg, bool exact)
{
    static const FeaturesFwdKernel k[3][2] = { { lg_features_fwd<4, false>, lg_features_fwd<4, true> }, { lg_features_fwd<16, false>, lg_features_fwd<16, true> },
                                               { lg_features_fwd<32, false>, lg_features_fwd<32, true> } };
    return k[cg == 4 ? 0 : cg == 16 ? 1 : 2][exact];
}
using FeaturesBwdKernel = decltype(&lg_features_bwd<4, true>);
static FeaturesBwdKernel features_bwd_kernel(int nv, bool exact)
{
    static const FeaturesBwdKernel k[3][2] = { { lg_features_bwd<4, false>, lg_features_bwd<4, true> }, { lg_features_bwd<8, false>, lg_features_bwd<8, true> },
                                               { lg_features_bwd<16, false>, lg_features_bwd<16, true> } };
    return k[nv == 4 ? 0 : nv == 8 ? 1 : 2][exact];
}
using FeaturesBwdGeomKernel = decltype(&lg_features_bwd_geom<4, true, true>);
static FeaturesBwdGeomKernel features_bwd_geom_kernel(int cg, bool exact, bool accum)
{
#define LG_FBG(CG) { { lg_features_bwd_geom<CG, false, false>, lg_features_bwd_geom<CG, false, true> }, { lg_features_bwd_geom<CG, true, false>, lg_features_bwd_geom<CG, true, true> } }
    static const FeaturesBwdGeomKernel k[3][2][2] = { LG_FBG(4), LG_FBG(16), LG_FBG(32) };
#undef LG_FBG
    return k[cg == 4 ? 0 : cg == 16 ? 1 : 2][exact][accum];
}
using DistortionBwdKernel = decltype(&lg_distortion_bwd<true, true>);
static DistortionBwdKernel distortion_bwd_kernel(bool exact, bool accum)
{
    static const DistortionBwdKernel k[2][2] = { { lg_distortion_bwd<false, false>, lg_distortion_bwd<false, true> }, { lg_distortion_bwd<true, false>, lg_distortion_bwd<true, true> } };
    return k[exact][accum];
}

static int backward_impl(const lg_view* v, const lg_gaussians* g, const int32_t* radii, const void* geom_p, const void* bin_p,
                         const void* img_p, int64_t R, const float* dL_dcolor, const GradOut& d, void* scratch, void* stream_p, const BackwardOpts& o)
{
    int rc = check_args(v, g);
    if (rc != LG_OK) return rc;
    if (g->N == 0) return LG_OK;   // empty model: torch hands over NULL pointers for empty tensors, and there is nothing to write
    // SH inputs without dL_dshs but WITH dL_dcolors: K9's rgb_only mode (dL/d rgb per Gaussian instead of the coefficient gradients;
    // lg_sh_grad_from_rgb rebuilds them) -- then dL_dshs_rest is not needed either
    const bool rgb_only = g->shs && !d.shs && d.colors;
    if (g->shs_rest && !d.shs_rest && !rgb_only) return fail(LG_ERR_INVALID_ARGUMENT, "missing gradient output for shs_rest");
    if (rgb_only && d.shs_rest) return fail(LG_ERR_INVALID_ARGUMENT, "dL_dshs_rest without dL_dshs");
    if (!radii || !geom_p || !bin_p || !img_p || (!dL_dcolor && !o.fg && !o.dg) || !d.means2D || !d.means3D || !d.opacity || !scratch)
        return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    if ((g->shs && !d.shs && !rgb_only) || (g->colors_precomp && !d.colors) || (g->scales && (!d.scales || !d.rotations)) ||
        (g->cov3D_precomp && !d.cov3D))
        return fail(LG_ERR_INVALID_ARGUMENT, "missing gradient output for a provided input");
    const int N = g->N;
    // S must be the forward's (same lg_view); the kernels compare it with meta[2] and refuse otherwise
    const auto [stream, debug, prof, exact, s, f] = walk_call(v, N, geom_p, img_p, bin_p, R, stream_p);
    const ViewGeom& q = s.q; const GeomView& geo = s.geo; const ImgView& img = s.img; const BinView& bin = s.bin;
    const int W = q.W, H = q.H, S = q.S;
    float* rows = (float*)scratch; // [R][12] gradient rows, every row written by lg_blend_bwd
    const uint32_t max_items = (uint32_t)(q.ntiles + R / S + 1);
    // (the work list of the backward blend -- one item per (tile, segment of S entries), longest first -- was left in the binning
    // buffer by the forward: one extra workgroup of lg_blend_fwd)
    if (R > 0 && dL_dcolor) {
        ProfScope ps(prof, "blend_bwd", stream);
        blend_bwd_kernel(exact, o.means2D_abs != nullptr)<<<max_items, 64, 0, stream>>>(
            W, H, q.gx, S, bin.work, bin.meta, bin.ranges, bin.entries, q.gid_mask, geo.tinfo, geo.rec, v->bg, img.final_T, img.n_contrib, dL_dcolor, bin.ckpt, rows);
    }
    KCHECK("lg_blend_bwd");
    if (o.means2D_abs) {
        // lg_backward_abs: floats 9 and 10 of the rows summed per Gaussian, in front of the first K9 chunk (K9 does not read them)
        {
            ProfScope ps(prof, "absgrad_rows", stream);
            lg_absgrad_rows<<<(N + LG_ABS_THREADS - 1) / LG_ABS_THREADS, LG_ABS_THREADS, 0, stream>>>(
                N, W, H, (uint32_t)R, radii, geo.rec, geo.counters, bin.meta, (uint32_t)S, geo.touched, geo.offsets,
                reinterpret_cast<const float4*>(rows), o.means2D_abs);
        }
        KCHECK("lg_absgrad_rows");
    }
    if (o.fg && R > 0) {
        // lg_backward_features: the moments of the feature / alpha loss join K7's in the same rows (lg_features.h), CG channels per walk;
        // the first walk writes whole rows, zeros included, when K7 did not run -- also when there is no image gradient at all
        if (o.fg->dL_dout || o.fg->dL_dalpha || !dL_dcolor) {
            const int nch = o.fg->dL_dout ? o.fg->C : 1;     // without dL_dout one walk: dL_dalpha's, or the zero rows
            bool accum = dL_dcolor != nullptr;
            for (int c0 = 0, cg; c0 < nch; c0 += cg) {
                cg = features_channel_group(nch - c0);
                {
                    ProfScope ps(prof, "features_bwd_geom", stream);
                    features_bwd_geom_kernel(cg, exact, accum)<<<q.ntiles_pad, 256, 0, stream>>>(f, (uint32_t)S, bin.meta, o.fg->C, c0, geo.tinfo, o.fg->features,
                                                                                                o.fg->bg, o.fg->dL_dout, o.fg->dL_dalpha, img.final_T, img.n_contrib, rows);
                }
                KCHECK("lg_features_bwd_geom");
                accum = true;
            }
        }
    }
    if (o.dg && R > 0) {
        // lg_backward_distortion: the moments of the distortion / median loss join the rows; the walk writes whole rows when it is the first
        const bool accum = dL_dcolor != nullptr || o.fg != nullptr;
        const float4* st = (const float4*)o.dg->state;
        const uint32_t* st_pos = (const uint32_t*)((const char*)o.dg->state + distortion_state_head(W, H));
        {
            ProfScope ps(prof, "distortion_bwd", stream);
            distortion_bwd_kernel(exact, accum)<<<q.ntiles_pad, 256, 0, stream>>>(
                f, (uint32_t)S, bin.meta, geo.tinfo, o.dg->m, o.dg->m_stride, st, st_pos, o.dg->dL_dD, o.dg->dL_dmed, img.final_T, img.n_contrib, rows, o.dg->dm_rows);
        }
        KCHECK("lg_distortion_bwd");
    }
    preprocess_bwd_launch(v, g, radii, s, rows, d, rgb_only, stream, o);
    KCHECK("lg_preprocess_bwd");
    if (debug && R > 0) {
        uint32_t h_seg = 0;
        HIP_TRY(hipMemcpyAsync(&h_seg, bin.meta + 2, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (h_seg != (uint32_t)S) return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward: lg_view.segment_length differs from the forward's (gradients are zero)");
        if ((v->flags & LG_FLAG_SAVE_SH_JACOBIAN) && g->shs && (d.shs || rgb_only)) {
            uint32_t h_mark = 0;
            HIP_TRY(hipMemcpyAsync(&h_mark, geo.counters + 9, 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (h_mark != LG_SHJAC_MAGIC)
                return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward: the view carries LG_FLAG_SAVE_SH_JACOBIAN but its forward did not (gradients are zero)");
        }
    }
    return LG_OK;
}

extern "C" int lg_backward(const lg_view* v, const lg_gaussians* g, const int32_t* radii, const void* geom_p, const void* bin_p,
                           const void* img_p, int64_t R, const float* dL_dcolor, float* dL_dmeans2D, float* dL_dmeans3D,
                           float* dL_dshs, float* dL_dcolors, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                           float* dL_dcov3D, float* dL_dshs_rest, void* scratch, void* stream_p)
{
    const GradOut d = { dL_dmeans2D, dL_dmeans3D, dL_dshs, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, dL_dshs_rest };
    return backward_impl(v, g, radii, geom_p, bin_p, img_p, R, dL_dcolor, d, scratch, stream_p, { 1, nullptr, nullptr });
}

extern "C" int lg_backward_chunked(const lg_view* v, const lg_gaussians* g, const int32_t* radii, const void* geom_p, const void* bin_p,
                                   const void* img_p, int64_t R, const float* dL_dcolor, float* dL_dmeans2D, float* dL_dmeans3D,
                                   float* dL_dshs, float* dL_dcolors, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                                   float* dL_dcov3D, float* dL_dshs_rest, void* scratch, void* stream_p, int32_t chunks,
                                   lg_chunk_fn on_chunk, void* user)
{
    const GradOut d = { dL_dmeans2D, dL_dmeans3D, dL_dshs, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, dL_dshs_rest };
    return backward_impl(v, g, radii, geom_p, bin_p, img_p, R, dL_dcolor, d, scratch, stream_p, { chunks, on_chunk, user });
}

// lg_backward_chunked that also leaves the absolute screen-space mean gradients (lg_absgrad.h; the view must carry LG_FLAG_ABSGRAD)
extern "C" int lg_backward_abs(const lg_view* v, const lg_gaussians* g, const int32_t* radii, const void* geom_p, const void* bin_p,
                               const void* img_p, int64_t R, const float* dL_dcolor, float* dL_dmeans2D, float* dL_dmeans3D,
                               float* dL_dshs, float* dL_dcolors, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                               float* dL_dcov3D, float* dL_dshs_rest, void* scratch, void* stream_p, int32_t chunks,
                               lg_chunk_fn on_chunk, void* user, float* dL_dmeans2D_abs)
{
    if (!v || !(v->flags & LG_FLAG_ABSGRAD)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward_abs: the view must carry LG_FLAG_ABSGRAD");
    if (!dL_dmeans2D_abs) return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward_abs: missing dL_dmeans2D_abs");
    if (!dL_dcolor) return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward_abs: missing dL_dcolor");
    if (R < 0 || R >= (1ll << 30)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward_abs: num_rendered out of range");
    const GradOut d = { dL_dmeans2D, dL_dmeans3D, dL_dshs, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, dL_dshs_rest };
    return backward_impl(v, g, radii, geom_p, bin_p, img_p, R, dL_dcolor, d, scratch, stream_p, { chunks, on_chunk, user, nullptr, dL_dmeans2D_abs });
}

// ---- camera pose gradients (lg_camera.h) ----
extern "C" size_t lg_camera_scratch_bytes(int32_t N)
{
    const size_t nwg = ((size_t)(N > 0 ? N : 1) + LG_CAM_THREADS - 1) / LG_CAM_THREADS;
    return align_up(nwg * LG_CAM_TERMS * sizeof(double));     // partials[workgroup][27]
}

extern "C" int lg_backward_camera(const lg_view* v, const lg_gaussians* g, const int32_t* radii, const void* geom_p, const void* bin_p,
                                  int64_t R, const void* backward_scratch, float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos,
                                  void* scratch, void* stream_p)
{
    int rc = check_args(v, g);
    if (rc != LG_OK) return rc;
    if (!dL_dviewmatrix || !dL_dprojmatrix || !dL_dcampos) return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward_camera: the three gradient outputs are required");
    if (!scratch) return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward_camera: missing scratch");
    if (R < 0 || R >= (1ll << 30)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward_camera: num_rendered out of range");
    if (g->N > 0) {
        if (!radii || !geom_p || !bin_p || !backward_scratch) return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward_camera: missing buffer");
        if (g->shs && !(v->flags & LG_FLAG_SAVE_SH_JACOBIAN))
            return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward_camera: SH inputs need LG_FLAG_SAVE_SH_JACOBIAN on the view (forward and backward)");
    }
    hipStream_t stream = (hipStream_t)stream_p;
    const bool debug = v->flags & LG_FLAG_DEBUG, prof = v->flags & LG_FLAG_PROFILE;
    const int N = g->N;
    const uint32_t nwg = N > 0 ? (uint32_t)(((size_t)N + LG_CAM_THREADS - 1) / LG_CAM_THREADS) : 0u;
    double* partials = (double*)scratch;
    if (N > 0) {
        const ViewState s = view_state(v, N, geom_p, nullptr, bin_p, R);
        const ViewGeom& q = s.q; const GeomView& geo = s.geo; const BinView& bin = s.bin;
        {
            ProfScope ps(prof, "camera_bwd", stream);
            // (LG_FLAG_ANTIALIAS: the compensation factor of the opacity depends on the camera -- those variants read the input opacities)
            camera_bwd_kernel(v->flags & LG_FLAG_RAW_PARAMS, v->flags & LG_FLAG_ANTIALIAS)<<<nwg, LG_CAM_THREADS, 0, stream>>>(
                N, g->M, v->sh_degree, q.W, q.H, v->tanfovx, v->tanfovy, v->scale_modifier, (uint32_t)R, v->viewmatrix, v->projmatrix, v->campos,
                g->means3D, g->shs, g->scales, g->rotations, g->cov3D_precomp, radii, geo.rec, geo.counters, bin.meta, (uint32_t)q.S, geo.touched,
                geo.offsets, reinterpret_cast<const float4*>(backward_scratch), geo.shjac, partials, g->opacities);
        }
        KCHECK("lg_camera_bwd");
    }
    {
        ProfScope ps(prof, "camera_reduce", stream);
        lg_camera_reduce<<<1, LG_CAM_THREADS, 0, stream>>>(nwg, partials, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos);
    }
    KCHECK("lg_camera_reduce");
    return LG_OK;
}

extern "C" int lg_sh_grad_from_rgb(int32_t N, int32_t M, int32_t sh_degree, int32_t V, const float* means3D, const float* campos,
                                   const float* drgb, int64_t view_stride, float divisor, int32_t accumulate, float* dL_dshs, float* dL_dshs_rest,
                                   void* stream_p)
{
    if (N < 0 || V < 1 || !sh_shape_ok(M, sh_degree))
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_sh_grad_from_rgb: N >= 0, V >= 1, M in {1, 4, 9, 16}, (D + 1)^2 <= M required");
    if (N == 0) return LG_OK;
    if (!means3D || !campos || !drgb || !dL_dshs || view_stride < 3 * (int64_t)N || !(divisor > 0.0f))
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_sh_grad_from_rgb: missing buffer, view_stride < 3 N or divisor <= 0");
    if (dL_dshs_rest && M == 1) dL_dshs_rest = nullptr;     // degree 0: nothing beyond the dc row
    hipStream_t stream = (hipStream_t)stream_p;
    lg_sh_grad_from_rgb_kernel<<<(N + LG_PP - 1) / LG_PP, LG_PP, 0, stream>>>(N, M, sh_degree, V, means3D, campos, drgb, (size_t)view_stride, divisor,
                                                                           accumulate ? 1 : 0, dL_dshs, dL_dshs_rest);
    KLAUNCHED("lg_sh_grad_from_rgb_kernel");
    return LG_OK;
}

extern "C" int lg_score_from_count(int32_t N, const int32_t* count, const float* weight, float* score, void* stream_p)
{
    if (N < 0 || (N > 0 && (!count || !score))) return fail(LG_ERR_INVALID_ARGUMENT, "bad arguments");
    if (N == 0) return LG_OK;
    hipStream_t stream = (hipStream_t)stream_p;
    lg_score_kernel<<<(N + 255) / 256, 256, 0, stream>>>(N, count, weight, score, nullptr);
    KLAUNCHED("lg_score_kernel");
    return LG_OK;
}

extern "C" size_t lg_prune_scratch_bytes(int32_t N)
{
    (void)N;
    return align_up(2 * sizeof(LgSelect));
}

extern "C" int lg_prune_epilogue(int32_t N, const float* scaling, const float* imp_list, float v_pow, double prune_percent,
                                 float* v_list, uint8_t* mask, float* thresholds, void* scratch, uint32_t flags, void* stream_p)
{
    if (N <= 0) return fail(LG_ERR_INVALID_ARGUMENT, "prune epilogue needs N >= 1 (the reference indexes an empty sort)");
    if (!scaling || !imp_list || !v_list || !mask || !thresholds || !scratch) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    if (!(prune_percent >= 0.0 && prune_percent <= 1.0)) return fail(LG_ERR_INVALID_ARGUMENT, "prune_percent must be in [0, 1]");
    hipStream_t stream = (hipStream_t)stream_p;
    const bool debug = flags & LG_FLAG_DEBUG, prof = flags & LG_FLAG_PROFILE;
    LgSelect* st = (LgSelect*)scratch;
    // prune.py:122-124: element `index = int(N * 0.9)` of the DESCENDING sort = ascending rank N - 1 - index
    const int index = (int)((double)N * 0.9);
    const uint32_t rank_volume = (uint32_t)(N - 1 - (index < N ? index : N - 1));
    // scene/gaussian_model.py:778-779: ascending index int(percent * (N - 1)), evaluated like Python (double)
    const uint32_t rank_score = (uint32_t)(prune_percent * (double)(N - 1));
    const int blocks = (int)std::min<int64_t>(((int64_t)N + 255) / 256, 2048);
    ProfScope ps(prof, "prune_epilogue", stream);
    HIP_TRY(hipMemsetAsync(st, 0, 2 * sizeof(LgSelect), stream));
    for (int p = 0; p < 4; p++) {
        lg_select_pass<0><<<blocks, 256, 0, stream>>>(N, p, rank_volume, scaling, &st[0]);
        KCHECK("lg_select_pass<volume>");
    }
    lg_v_imp_score_kernel<<<blocks, 256, 0, stream>>>(N, rank_volume, scaling, imp_list, v_pow, &st[0], v_list, &st[1], thresholds);
    KCHECK("lg_v_imp_score_kernel");
    for (int p = 1; p < 4; p++) {
        lg_select_pass<1><<<blocks, 256, 0, stream>>>(N, p, rank_score, v_list, &st[1]);
        KCHECK("lg_select_pass<score>");
    }
    lg_prune_mask_kernel<<<blocks, 256, 0, stream>>>(N, rank_score, v_list, &st[1], mask, thresholds);
    KCHECK("lg_prune_mask_kernel");
    return LG_OK;
}

// rank-th smallest element of values[0..N) by one radix select (four 8-bit histogram passes; exact: the element a sort puts
// at that index) and, when mask != NULL, mask[i] = values[i] <= that element.  The two halves of the prune epilogue around the
// reference's own torch.pow (prune.prune_epilogue): no sort, no host read-back.
extern "C" int lg_select_mask(int32_t N, const float* values, int64_t rank, uint8_t* mask, float* out_value, void* scratch, void* stream_p)
{
    if (N <= 0 || rank < 0 || rank >= N) return fail(LG_ERR_INVALID_ARGUMENT, "lg_select_mask needs N >= 1 and 0 <= rank < N");
    if (!values || !out_value || !scratch) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    LgSelect* st = (LgSelect*)scratch;
    const int blocks = (int)std::min<int64_t>(((int64_t)N + 255) / 256, 2048);
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(LgSelect), stream));
    for (int p = 0; p < 4; p++) {
        lg_select_pass<1><<<blocks, 256, 0, stream>>>(N, p, (uint32_t)rank, values, st);
        KLAUNCHED("lg_select_pass");
    }
    lg_select_finish_kernel<<<mask ? blocks : 1, 256, 0, stream>>>(N, (uint32_t)rank, values, st, mask, out_value);
    KLAUNCHED("lg_select_finish_kernel");
    return LG_OK;
}

extern "C" int lg_ordered_sum(int32_t V, int64_t n, const float* rows, int64_t row_stride, float* out, void* stream_p)
{
    if (V <= 0 || n < 0 || row_stride < n) return fail(LG_ERR_INVALID_ARGUMENT, "bad shape");
    if (n == 0) return LG_OK;
    if (!rows || !out) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    lg_ordered_sum_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(V, (size_t)n, rows, (size_t)row_stride, out);
    KLAUNCHED("lg_ordered_sum_kernel");
    return LG_OK;
}

// ---- compaction of the Gaussian tensors after a prune (scene/gaussian_model.py:564-600) ----
extern "C" size_t lg_compact_scratch_bytes(int32_t N)
{
    const size_t nb = ((size_t)(N > 0 ? N : 1) + LG_COMPACT_ROWS - 1) / LG_COMPACT_ROWS;
    return 2 * align_up(nb * 4);
}

extern "C" int lg_compact_plan(int32_t N, const uint8_t* keep, int32_t* dest, int32_t* count, void* scratch, void* stream_p)
{
    if (N < 0) return fail(LG_ERR_INVALID_ARGUMENT, "bad row count");
    if (!count || (N > 0 && (!keep || !dest || !scratch))) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    if (N == 0) { HIP_TRY(hipMemsetAsync(count, 0, 4, stream)); return LG_OK; }
    const int nb = (N + LG_COMPACT_ROWS - 1) / LG_COMPACT_ROWS;
    uint32_t* blk_sum = (uint32_t*)scratch;
    uint32_t* blk_off = (uint32_t*)((char*)scratch + align_up((size_t)nb * 4));
    lg_compact_count<<<nb, 256, 0, stream>>>(N, keep, blk_sum);
    KLAUNCHED("lg_compact_count");
    lg_scan_words<<<1, 1024, 0, stream>>>(nb, blk_sum, blk_off, count);
    KLAUNCHED("lg_scan_words");
    lg_compact_dest<<<nb, 256, 0, stream>>>(N, keep, blk_off, dest);
    KLAUNCHED("lg_compact_dest");
    return LG_OK;
}

// grid of the row moves (lg_compact_move, lg_densify_move): x strides over rows * widest words in workgroups of 1024, 8192 at the most; y = tensor
static dim3 row_move_grid(size_t rows, size_t widest, int num_tensors)
{
    const size_t blocks = std::min<size_t>((rows * widest + 1023) / 1024, 8192);
    return dim3((unsigned)std::max<size_t>(blocks, 1), (unsigned)num_tensors);
}

extern "C" int lg_compact_rows(int32_t N, const int32_t* dest, int32_t num_tensors, const void* const* src, void* const* dst,
                               const int32_t* row_bytes, void* stream_p)
{
    if (N < 0 || num_tensors < 0 || num_tensors > LG_COMPACT_MAX_TENSORS) return fail(LG_ERR_INVALID_ARGUMENT, "bad tensor count (max 32 per call)");
    if (N == 0 || num_tensors == 0) return LG_OK;
    if (!dest || !src || !dst || !row_bytes) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    LgCompactArgs a;
    memset(&a, 0, sizeof(a));
    size_t widest = 1;
    for (int t = 0; t < num_tensors; t++) {
        if (row_bytes[t] <= 0 || (row_bytes[t] & 3) || !src[t] || !dst[t] || ((uintptr_t)src[t] & 3) || ((uintptr_t)dst[t] & 3))
            return fail(LG_ERR_INVALID_ARGUMENT, "lg_compact_rows: rows must be non-empty multiples of 4 bytes, 4-byte aligned");
        a.src[t] = (const uint32_t*)src[t]; a.dst[t] = (uint32_t*)dst[t]; a.words[t] = (uint32_t)(row_bytes[t] / 4);
        widest = std::max<size_t>(widest, a.words[t]);
    }
    lg_compact_move<<<row_move_grid((size_t)N, widest, num_tensors), 256, 0, stream>>>(N, dest, a);
    KLAUNCHED("lg_compact_move");
    return LG_OK;
}

// ---- VecTree nearest-code search (vectree/vq.py:262-266) ----
extern "C" size_t lg_vq_scratch_bytes(int32_t K, int32_t d)
{
    const int dk2 = lg_vq_dk2(d);
    if (K <= 0 || d <= 0 || dk2 == 0) return 0;
    return align_up((size_t)lg_vq_kpad(K) * 2 * dk2 * sizeof(float));
}

extern "C" int lg_vq_nearest(int32_t n, int32_t d, int32_t K, const float* x, const float* codebook, int32_t* out_index, void* scratch,
                             uint32_t flags, void* stream_p)
{
    const int dk2 = lg_vq_dk2(d);
    if (n < 0 || K <= 0 || d <= 0 || dk2 == 0) return fail(LG_ERR_INVALID_ARGUMENT, "lg_vq_nearest: need n >= 0, K >= 1, 1 <= d <= 63");
    if (n == 0) return LG_OK;
    if (!x || !codebook || !out_index || !scratch) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    const bool debug = flags & LG_FLAG_DEBUG, prof = flags & LG_FLAG_PROFILE;
    const int Kpad = lg_vq_kpad(K), dk = 2 * dk2;
    float* cbA = (float*)scratch;
    ProfScope ps(prof, "vq_nearest", stream);
    lg_vq_prepare<<<(Kpad + 255) / 256, 256, 0, stream>>>(K, Kpad, d, dk, codebook, cbA);
    KCHECK("lg_vq_prepare");
    const unsigned grid = (unsigned)((n + 127) / 128);
    vq_nearest_kernel(dk2)<<<grid, 256, 0, stream>>>(n, d, Kpad, x, cbA, out_index);
    KCHECK("lg_vq_nearest_kernel");
    return LG_OK;
}

// ---- colours of a VecTree-compressed model (lg_vq_color.h) ----
extern "C" int lg_vq_colors(int32_t N, int32_t M, int32_t sh_degree, const float* means3D, const float* campos, const uint32_t* slot,
                            const void* rows_f16, int32_t row_stride_bytes, float* out_rgb, uint32_t flags, void* stream_p)
{
    if (N < 0 || !sh_shape_ok(M, sh_degree))
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_vq_colors: N >= 0, M in {1, 4, 9, 16}, (D + 1)^2 <= M required");
    if (row_stride_bytes < 6 * M || (row_stride_bytes & 15) != 0 || ((uintptr_t)rows_f16 & 15) != 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_vq_colors: rows must be 16-byte aligned, row_stride_bytes a multiple of 16 and >= 6 M");
    if (N == 0) return LG_OK;
    if (!means3D || !campos || !slot || !rows_f16 || !out_rgb) return fail(LG_ERR_INVALID_ARGUMENT, "lg_vq_colors: missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    const bool debug = flags & LG_FLAG_DEBUG, prof = flags & LG_FLAG_PROFILE;
    const uint32_t need = lg_vq_need_mask(M, sh_degree);
    const unsigned grid = (unsigned)((N + LG_PP - 1) / LG_PP);
    ProfScope ps(prof, "vq_colors", stream);
    vq_colors_kernel(M)<<<grid, LG_PP, 0, stream>>>(N, sh_degree, need, means3D, campos, slot, (const unsigned char*)rows_f16, (uint32_t)row_stride_bytes, out_rgb);
    KCHECK("lg_vq_colors_kernel");
    return LG_OK;
}

// ---- VecTree codebook training step (vectree/vq.py:262-299, training mode) ----
extern "C" size_t lg_vq_ema_scratch_bytes(int32_t n, int32_t K, int32_t d)
{
    if (n < 0 || n >= (1 << 30) || lg_vq_scratch_bytes(K, d) == 0) return 0;
    return carve_vq_ema(nullptr, (size_t)n, (size_t)K, (size_t)d).total;
}

// Groups n keys (code << 32 | element) by code: sorts them on the code bits, then leaves the start of each of the `lists` lists and the
// chunk offsets of the first K.  lg_vq_ema_step: lists = K, with the weight partials lg_vq_keys left; lg_vq_code_index: lists = K + 1 (the
// pseudo-code K of the non-VQ Gaussians included), without.  b: the caller's keys_in / keys_out / sort_temp (VqEmaView, VqIndexScratch).
template <class Bufs>
static int vq_group_by_code(const Bufs& b, uint32_t n, uint32_t K, uint32_t lists, uint32_t* start, uint32_t* chunk_off, uint32_t nwpart,
                            const float* wpart, float* scal, bool debug, hipStream_t stream)
{
    int code_bits = 1;
    while (code_bits < 31 && (1u << code_bits) < lists) code_bits++;
    size_t tb = b.sort_temp_bytes;
    HIP_TRY(lg_sort_keys(b.sort_temp, tb, b.keys_in, b.keys_out, n, 32, 32 + code_bits, nullptr, false, stream));
    KCHECK("lg_sort_keys");
    lg_vq_starts<<<(n + 255) / 256, 256, 0, stream>>>(n, lists, b.keys_out, start);
    KCHECK("lg_vq_starts");
    lg_vq_chunk_scan<<<1, LG_VQ_RED_THREADS, 0, stream>>>(K, start, chunk_off, nwpart, wpart, scal);
    KCHECK("lg_vq_chunk_scan");
    return LG_OK;
}

extern "C" int lg_vq_ema_step(int32_t n, int32_t d, int32_t K, const float* x, const float* weight, float* embed, float* cluster_size,
                              double decay, double eps, int32_t* out_index, void* scratch, uint32_t flags, void* stream_p)
{
    if (n <= 0 || n >= (1 << 30) || K <= 0 || d <= 0 || lg_vq_dk2(d) == 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_vq_ema_step: need 1 <= n < 2^30, K >= 1, 1 <= d <= 63");
    if (!x || !embed || !cluster_size || !out_index || !scratch) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    const bool debug = flags & LG_FLAG_DEBUG, prof = flags & LG_FLAG_PROFILE;
    const VqEmaView v = carve_vq_ema(scratch, (size_t)n, (size_t)K, (size_t)d);
    {
        ProfScope ps(prof, "vq_ema_search", stream);
        const int rc = lg_vq_nearest(n, d, K, x, embed, out_index, v.cbA, flags & ~(uint32_t)LG_FLAG_PROFILE, stream_p);
        if (rc != LG_OK) return rc;
    }
    const uint32_t un = (uint32_t)n, uK = (uint32_t)K;
    const uint32_t nwpart = (un + LG_VQ_WSUM_TILE - 1) / LG_VQ_WSUM_TILE;
    const uint32_t* sort_err = lg_sort_error_word(v.sort_temp, (size_t)n);
    {
        ProfScope ps(prof, "vq_ema_index", stream);
        lg_vq_keys<<<nwpart, 256, 0, stream>>>(un, uK, out_index, weight, v.keys_in, v.wpart);
        KCHECK("lg_vq_keys");
        const int rc = vq_group_by_code(v, un, uK, uK, v.start, v.chunk_off, nwpart, weight ? v.wpart : nullptr, v.scal, debug, stream);
        if (rc != LG_OK) return rc;
    }
    const float decay_f = (float)decay, one_minus = (float)(1.0 - decay);      // what torch makes of mul_(decay).add_(new, alpha = 1 - decay)
    {
        ProfScope ps(prof, "vq_ema_sum", stream);
        const unsigned grid = (unsigned)((v.max_chunks + 3) / 4);
        vq_chunk_sum_kernel(weight != nullptr)<<<grid, 256, 0, stream>>>(un, d, uK, x, weight, v.scal, v.keys_out, v.start, v.chunk_off, v.partial);
        KCHECK("lg_vq_chunk_sum");
        lg_vq_combine<<<(unsigned)(((size_t)K * (d + 1) + 255) / 256), 256, 0, stream>>>(uK, d, v.chunk_off, v.partial, v.esum, cluster_size, decay_f,
                                                                                          one_minus, sort_err);
        KCHECK("lg_vq_combine");
    }
    {
        ProfScope ps(prof, "vq_ema_epilogue", stream);
        lg_vq_size_sum<<<1, LG_VQ_RED_THREADS, 0, stream>>>(uK, cluster_size, v.scal);
        KCHECK("lg_vq_size_sum");
        lg_vq_epilogue<<<(unsigned)(((size_t)K * d + 255) / 256), 256, 0, stream>>>(uK, d, v.esum, cluster_size, v.scal, embed, decay_f, one_minus,
                                                                                    (float)eps, (float)((double)K * eps));
        KCHECK("lg_vq_epilogue");
    }
    return LG_OK;
}

// ---- backward of lg_vq_colors (lg_vq_color_bwd.h) ----
static bool vq_index_shape_ok(int32_t N, int32_t K) { return N >= 0 && N < (1 << 30) && K >= 1 && K <= (1 << 24); }

extern "C" size_t lg_vq_code_index_bytes(int32_t N, int32_t K)
{
    return vq_index_shape_ok(N, K) ? carve_vq_index(nullptr, (size_t)N, (size_t)K).total : 0;
}

extern "C" size_t lg_vq_code_index_scratch_bytes(int32_t N, int32_t K)
{
    return vq_index_shape_ok(N, K) ? carve_vq_index_scratch(nullptr, (size_t)N).total : 0;
}

extern "C" int lg_vq_code_index(int32_t N, int32_t K, const uint32_t* slot, void* index, void* scratch, void* stream_p)
{
    if (!vq_index_shape_ok(N, K)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_vq_code_index: need 0 <= N < 2^30, 1 <= K <= 2^24");
    if (!index || (N > 0 && (!slot || !scratch))) return fail(LG_ERR_INVALID_ARGUMENT, "lg_vq_code_index: missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    const VqIndexView v = carve_vq_index(index, (size_t)N, (size_t)K);
    if (N == 0) {                                   // every list empty: start = chunk_off = 0, no error
        HIP_TRY(hipMemsetAsync(index, 0, v.total, stream));
        return LG_OK;
    }
    const VqIndexScratch s = carve_vq_index_scratch(scratch, (size_t)N);
    const uint32_t un = (uint32_t)N, uK = (uint32_t)K;
    lg_vq_slot_keys<<<(un + 255) / 256, 256, 0, stream>>>(un, uK, slot, s.keys_in);
    KLAUNCHED("lg_vq_slot_keys");
    const int rc = vq_group_by_code(s, un, uK, uK + 1u, v.start, v.chunk_off, 0u, nullptr, nullptr, false, stream);
    if (rc != LG_OK) return rc;
    const uint32_t* sort_err = lg_sort_error_word(s.sort_temp, (size_t)N);
    lg_vq_index_ids<<<(un + 255) / 256, 256, 0, stream>>>(un, s.keys_out, sort_err, v.ids, v.err);
    KLAUNCHED("lg_vq_index_ids");
    return LG_OK;
}

extern "C" size_t lg_vq_colors_bwd_scratch_bytes(int32_t N, int32_t M, int32_t K)
{
    if (!vq_index_shape_ok(N, K) || M < 1 || M > 16) return 0;
    return align_up(std::max<size_t>(lg_vq_bwd_max_chunks((size_t)N, (size_t)K), 1) * 3 * (size_t)M * sizeof(float));
}

extern "C" int lg_vq_colors_bwd(int32_t N, int32_t M, int32_t sh_degree, int32_t K, int64_t n_rows, const float* means3D, const float* campos,
                                const uint32_t* slot, const void* rows_f16, int32_t row_stride_bytes, const float* dL_drgb, const void* index,
                                float* dL_drows, float* dL_dmeans3D, void* scratch, uint32_t flags, void* stream_p)
{
    if (!vq_index_shape_ok(N, K) || !sh_shape_ok(M, sh_degree) || n_rows < K || n_rows >= ((int64_t)1 << 31))
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_vq_colors_bwd: 0 <= N < 2^30, M in {1, 4, 9, 16}, (D + 1)^2 <= M, K <= n_rows < 2^31 required");
    if (row_stride_bytes < 6 * M || (row_stride_bytes & 15) != 0 || ((uintptr_t)rows_f16 & 15) != 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_vq_colors_bwd: rows must be 16-byte aligned, row_stride_bytes a multiple of 16 and >= 6 M");
    if (!dL_drows || !index || !scratch || !rows_f16 || (N > 0 && (!means3D || !campos || !slot || !dL_drgb)))
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_vq_colors_bwd: missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    const bool debug = flags & LG_FLAG_DEBUG, prof = flags & LG_FLAG_PROFILE;
    const uint32_t need = lg_vq_need_mask(M, sh_degree);
    const VqIndexView v = carve_vq_index(const_cast<void*>(index), (size_t)N, (size_t)K);
    const unsigned char* rows = (const unsigned char*)rows_f16;
    const uint32_t stride = (uint32_t)row_stride_bytes, uK = (uint32_t)K;
    float* partial = (float*)scratch;
    if (N > 0) {
        ProfScope ps(prof, "vq_colors_bwd_rows", stream);
        const unsigned grid = (unsigned)((N + LG_VQ_BWD_WAVE - 1) / LG_VQ_BWD_WAVE);
        vq_colors_bwd_rows_kernel(M)<<<grid, LG_VQ_BWD_WAVE, 0, stream>>>(N, sh_degree, need, uK, (uint32_t)n_rows, means3D, campos, slot, rows, stride, dL_drgb,
                                                                          dL_drows, dL_dmeans3D);
        KCHECK("lg_vq_colors_bwd_rows_kernel");
    }
    {
        ProfScope ps(prof, "vq_colors_bwd_codes", stream);
        const unsigned grid = (unsigned)lg_vq_bwd_max_chunks((size_t)N, (size_t)K);
        if (grid > 0) {
            vq_colors_bwd_chunk_kernel(M)<<<grid, LG_VQ_BWD_WAVE, 0, stream>>>(sh_degree, need, uK, means3D, campos, rows, stride, dL_drgb, v.ids, v.start,
                                                                               v.chunk_off, v.err, partial);
            KCHECK("lg_vq_colors_bwd_chunk_kernel");
        }
        lg_vq_colors_bwd_combine<<<(unsigned)(((size_t)K * 3 * M + 255) / 256), 256, 0, stream>>>(uK, (uint32_t)(3 * M), v.chunk_off, partial, v.err,
                                                                                                 dL_drows);
        KCHECK("lg_vq_colors_bwd_combine");
    }
    return LG_OK;
}

// ---- Adam / AdamW step (lg_adam.h) ----
// lg_adam_step and lg_adam_step_rows are one step (adam_step) over two table types.  These overloads are all the two differ in: where
// the dense part of an entry and of the table sits, the row refusals and row fields of a masked entry, and the kernel with its names.
static const lg_adam_tensor& adam_dense(const lg_adam_tensor& x) { return x; }
static const lg_adam_tensor& adam_dense(const lg_adam_rows_tensor& x) { return x.t; }
static LgAdamTable& adam_dense(LgAdamTable& a) { return a; }
static LgAdamTable& adam_dense(LgAdamRowsTable& r) { return r.a; }
static const char* adam_rows_fault(const lg_adam_tensor&) { return nullptr; }
static const char* adam_rows_fault(const lg_adam_rows_tensor& x)
{
    if (!x.row_mask) return nullptr;                // dense entry: rows is not looked at
    if (x.rows < 1) return "rows < 1 with a row_mask";
    if (x.t.numel % x.rows != 0) return "numel is not a multiple of rows";
    if (x.t.numel / x.rows > (int64_t)LG_ADAM_MAX_ROW_LEN) return "a row beyond 2^31 - 1 elements";
    return nullptr;
}
static void adam_rows_reset(LgAdamTable&) {}
static void adam_rows_reset(LgAdamRowsTable& r) { for (int k = 0; k < LG_ADAM_MAX_TENSORS; k++) r.row_len[k] = 1; }
static void adam_rows_fill(LgAdamTable&, int, const lg_adam_tensor&) {}
static void adam_rows_fill(LgAdamRowsTable& r, int k, const lg_adam_rows_tensor& x)
{
    if (!x.row_mask) return;
    r.row_mask[k] = x.row_mask;
    r.row_len[k] = (uint32_t)(x.t.numel / x.rows);
    r.row_rcp[k] = lg_adam_row_rcp(r.row_len[k]);
    r.row_thr[k] = lg_adam_row_thr(r.row_len[k]);
}
static int adam_launch(const LgAdamTable& a, uint32_t wgs, bool decoupled, bool prof, hipStream_t stream)
{
    ProfScope ps(prof, "adam", stream);
    adam_kernel(decoupled)<<<wgs, LG_ADAM_THREADS, 0, stream>>>(a);
    KLAUNCHED("lg_adam_kernel");
    return LG_OK;
}
static int adam_launch(const LgAdamRowsTable& r, uint32_t wgs, bool decoupled, bool prof, hipStream_t stream)
{
    ProfScope ps(prof, "adam_rows", stream);
    adam_rows_kernel(decoupled)<<<wgs, LG_ADAM_THREADS, 0, stream>>>(r);
    KLAUNCHED("lg_adam_rows_kernel");
    return LG_OK;
}

// check -> fill -> split -> launch.  A launch takes LG_ADAM_MAX_TENSORS entries and 2^31 - 1 workgroups; a step with more is split.
template <class Table, class Tensor>
static int adam_step(const char* who, int32_t num_tensors, const Tensor* tensors, double beta1, double beta2, double eps, uint32_t flags, void* stream_p)
{
    // everything is checked before the first HIP call: a refused step has touched nothing
    if (num_tensors < 0) return refuse(who, "num_tensors < 0");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return refuse(who, "betas must lie in [0, 1)");
    if (num_tensors > 0 && !tensors) return refuse(who, "missing tensor table");
    for (int t = 0; t < num_tensors; t++) {
        const lg_adam_tensor& x = adam_dense(tensors[t]);
        if (x.numel < 0) return refuse(who, "numel < 0");
        if (x.step < 1) return refuse(who, "step < 1 (the step being taken counts from 1)");
        if (x.numel == 0) continue;                     // skipped: its pointers, its mask and its rows are not looked at
        if (!x.param || !x.grad || !x.exp_avg || !x.exp_avg_sq) return refuse(who, "null param / grad / exp_avg / exp_avg_sq with numel > 0");
        if ((((uintptr_t)x.param | (uintptr_t)x.grad | (uintptr_t)x.exp_avg | (uintptr_t)x.exp_avg_sq) & 3) != 0)
            return refuse(who, "float32 tensors must be 4-byte aligned");
        if ((x.numel + LG_ADAM_SPAN - 1) / LG_ADAM_SPAN > 0x7FFFFFFFll) return refuse(who, "tensor beyond 2^31 - 1 spans");
        if (const char* what = adam_rows_fault(tensors[t])) return refuse(who, what);
    }
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE, decoupled = flags & LG_ADAM_DECOUPLED_WD;
    Table table;
    LgAdamTable& a = adam_dense(table);
    int filled = 0;
    uint32_t wgs = 0;
    auto reset = [&]() {
        memset(&table, 0, sizeof(table));
        for (int k = 0; k < LG_ADAM_MAX_TENSORS; k++) a.first_wg[k] = 0xFFFFFFFFu;
        adam_rows_reset(table);
        a.one_minus_beta1 = (float)(1.0 - beta1); a.beta2 = (float)beta2; a.one_minus_beta2 = (float)(1.0 - beta2); a.eps = (float)eps;
        filled = 0; wgs = 0;
    };
    reset();
    for (int t = 0; t < num_tensors; t++) {
        const lg_adam_tensor& x = adam_dense(tensors[t]);
        if (x.numel == 0) continue;
        const uint32_t need = (uint32_t)((x.numel + LG_ADAM_SPAN - 1) / LG_ADAM_SPAN);
        if (filled == LG_ADAM_MAX_TENSORS || (filled > 0 && wgs + need > 0x7FFFFFFFu)) {
            const int rc = adam_launch(table, wgs, decoupled, prof, stream);
            if (rc != LG_OK) return rc;
            reset();
        }
        const int k = filled++;
        a.param[k] = x.param; a.grad[k] = x.grad; a.exp_avg[k] = x.exp_avg; a.exp_avg_sq[k] = x.exp_avg_sq;
        a.numel[k] = x.numel;
        a.first_wg[k] = wgs;
        // torch's default step: the three scalars in double, each rounded once to float
        a.step_size[k] = (float)(x.lr / (1.0 - pow(beta1, (double)x.step)));
        a.bc2_sqrt[k] = (float)sqrt(1.0 - pow(beta2, (double)x.step));
        a.decay[k] = decoupled ? (float)(1.0 - x.lr * x.weight_decay) : (float)x.weight_decay;
        if ((((uintptr_t)x.param | (uintptr_t)x.grad | (uintptr_t)x.exp_avg | (uintptr_t)x.exp_avg_sq) & 15) == 0) a.vec_mask |= 1u << k;
        adam_rows_fill(table, k, tensors[t]);
        wgs += need;
    }
    if (filled > 0) return adam_launch(table, wgs, decoupled, prof, stream);
    return LG_OK;
}

extern "C" int lg_adam_step(int32_t num_tensors, const lg_adam_tensor* tensors, double beta1, double beta2, double eps, uint32_t flags,
                            void* stream_p)
{
    return adam_step<LgAdamTable>("lg_adam_step", num_tensors, tensors, beta1, beta2, eps, flags, stream_p);
}

// lg_adam_step with a byte mask of rows per entry (lg_adam_rows_kernel): the same step, plus the row geometry of the masked entries
extern "C" int lg_adam_step_rows(int32_t num_tensors, const lg_adam_rows_tensor* tensors, double beta1, double beta2, double eps,
                                 uint32_t flags, void* stream_p)
{
    return adam_step<LgAdamRowsTable>("lg_adam_step_rows", num_tensors, tensors, beta1, beta2, eps, flags, stream_p);
}

// ---- densification (lg_densify.h) ----
struct DensifyScratch { uint8_t* flags; uint4* blk_sum; uint4* blk_off; size_t total; };
static DensifyScratch carve_densify(void* base, int32_t N)
{
    DensifyScratch d; size_t off = 0; char* p = (char*)base;
    auto take = [&](size_t bytes) { void* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
    const size_t n = (size_t)(N > 0 ? N : 1), nb = (n + LG_DENSIFY_ROWS - 1) / LG_DENSIFY_ROWS;
    d.flags = (uint8_t*)take(n);
    d.blk_sum = (uint4*)take(nb * 16);
    d.blk_off = (uint4*)take(nb * 16);
    d.total = off;
    return d;
}
extern "C" size_t lg_densify_scratch_bytes(int32_t N) { return carve_densify(nullptr, N).total; }

#define LG_DENSIFY_MAX_ROWS (1 << 30)
extern "C" int lg_densify_stats(int32_t N, const float* viewspace_grad, const uint8_t* update_filter, const int32_t* radii,
                                float* max_radii2D, float* accum, float* denom, uint32_t flags, void* stream_p)
{
    if (N < 0 || N >= LG_DENSIFY_MAX_ROWS) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_stats: N outside [0, 2^30)");
    if (N == 0) return LG_OK;
    if (!viewspace_grad || !update_filter || !accum || !denom) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_stats: null viewspace_grad / update_filter / accum / denom");
    if (radii && !max_radii2D) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_stats: radii without max_radii2D");
    if ((((uintptr_t)viewspace_grad | (uintptr_t)radii | (uintptr_t)max_radii2D | (uintptr_t)accum | (uintptr_t)denom) & 3) != 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_stats: 32-bit tensors must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    ProfScope ps(prof, "densify_stats", stream);
    lg_densify_stats_kernel<<<(unsigned)((N + 255) / 256), 256, 0, stream>>>(N, viewspace_grad, update_filter, radii, max_radii2D, accum, denom);
    KLAUNCHED("lg_densify_stats_kernel");
    return LG_OK;
}

extern "C" int lg_densify_plan(int32_t N, const float* scaling, const float* opacity, const float* accum, const float* denom, float thr_g,
                               float thr_d, float thr_w, float min_opacity, int32_t use_extent, void* map, int32_t* record, void* scratch,
                               uint32_t flags, void* stream_p)
{
    if (N < 0 || N >= LG_DENSIFY_MAX_ROWS) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_plan: N outside [0, 2^30)");
    if (!(thr_g > 0.0f)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_plan: thr_g must be > 0 (clones are never split only then)");
    if (thr_d != thr_d || thr_w != thr_w || min_opacity != min_opacity) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_plan: a NaN threshold");
    if (!record) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_plan: null record");
    if (N > 0 && (!scaling || !opacity || !accum || !denom || !map || !scratch))
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_plan: null scaling / opacity / accum / denom / map / scratch");
    if ((((uintptr_t)scaling | (uintptr_t)opacity | (uintptr_t)accum | (uintptr_t)denom | (uintptr_t)record) & 3) != 0 || ((uintptr_t)map & 7) != 0 ||
        ((uintptr_t)scratch & 15) != 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_plan: misaligned tensor (float32: 4 bytes, map: 8, scratch: 16)");
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    ProfScope ps(prof, "densify_plan", stream);
    if (N == 0) { HIP_TRY(lg_zero_async(record, 32, stream)); return LG_OK; }
    const DensifyScratch d = carve_densify(scratch, N);
    const int nb = (N + LG_DENSIFY_ROWS - 1) / LG_DENSIFY_ROWS;
    const LgDensifyThresholds th = { thr_g, thr_d, thr_w, min_opacity, use_extent ? 1 : 0 };
    lg_densify_classify<<<nb, 256, 0, stream>>>(N, scaling, opacity, accum, denom, th, d.flags, d.blk_sum);
    KLAUNCHED("lg_densify_classify");
    lg_densify_scan<<<1, 1024, 0, stream>>>(nb, d.blk_sum, d.blk_off, record);
    KLAUNCHED("lg_densify_scan");
    lg_densify_map<<<nb, 256, 0, stream>>>(N, d.flags, d.blk_off, record, (uint2*)map);
    KLAUNCHED("lg_densify_map");
    return LG_OK;
}

extern "C" int lg_densify_rows(int32_t N, int64_t N_out, const void* map, const int32_t* record, int32_t num_tensors,
                               const lg_densify_tensor* tensors, const float* rotation, const float* scaling, const float* noise,
                               int64_t noise_rows, uint32_t flags, void* stream_p)
{
    if (N < 0 || N >= LG_DENSIFY_MAX_ROWS) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: N outside [0, 2^30)");
    if (N_out < 0 || N_out > 2 * (int64_t)N) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: N_out outside [0, 2 N]");
    if (num_tensors < 0 || num_tensors > LG_DENSIFY_MAX_TENSORS) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: num_tensors outside [0, 32]");
    if (noise_rows < 0 || (noise_rows > 0 && !noise)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: noise_rows < 0 or null noise");
    if (num_tensors > 0 && !tensors) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: missing tensor table");
    if (N_out == 0 || num_tensors == 0) return LG_OK;
    if (!map || !record || ((uintptr_t)map & 7) != 0 || ((uintptr_t)record & 3) != 0) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: null or misaligned map / record");
    LgDensifyArgs a;
    memset(&a, 0, sizeof(a));
    size_t widest = 1;
    for (int t = 0; t < num_tensors; t++) {
        const lg_densify_tensor& x = tensors[t];
        if (x.role < LG_DENSIFY_COPY || x.role > LG_DENSIFY_ZERO) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: unknown role");
        if (x.row_words <= 0) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: row_words must be > 0 (leave empty tensors out)");
        if (!x.dst || (x.role != LG_DENSIFY_ZERO && !x.src)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: null src / dst");
        if ((((uintptr_t)x.src | (uintptr_t)x.dst) & 3) != 0) return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: tensors must be 4-byte aligned");
        if ((x.role == LG_DENSIFY_XYZ || x.role == LG_DENSIFY_SCALING) && x.row_words != 3)
            return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: the xyz and scaling roles need row_words == 3");
        if (x.role == LG_DENSIFY_XYZ && (!rotation || !scaling || (((uintptr_t)rotation | (uintptr_t)scaling | (uintptr_t)noise) & 3) != 0))
            return fail(LG_ERR_INVALID_ARGUMENT, "lg_densify_rows: the xyz role needs rotation and scaling (4-byte aligned, like noise)");
        a.src[t] = (const uint32_t*)x.src; a.dst[t] = (uint32_t*)x.dst; a.words[t] = (uint32_t)x.row_words; a.role[t] = (uint32_t)x.role;
        widest = std::max<size_t>(widest, (size_t)x.row_words);
    }
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    ProfScope ps(prof, "densify_rows", stream);
    lg_densify_move<<<row_move_grid((size_t)N_out, widest, num_tensors), 256, 0, stream>>>(N_out, (const uint2*)map, record, a, rotation, scaling, noise, noise_rows);
    KLAUNCHED("lg_densify_move");
    return LG_OK;
}

// ---- 3DGS-MCMC (lg_mcmc.h, include/lightgaussian_mcmc.h) ----
struct McmcScratch { int32_t* cnt; float4* planned; size_t total; };
static McmcScratch carve_mcmc(void* base, int32_t N)
{
    McmcScratch d; size_t off = 0; char* p = (char*)base;
    auto take = [&](size_t bytes) { void* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
    const size_t n = (size_t)(N > 0 ? N : 1);
    d.cnt = (int32_t*)take(n * 4);
    d.planned = (float4*)take(n * 16);
    d.total = off;
    return d;
}
extern "C" size_t lg_mcmc_scratch_bytes(int32_t N) { return carve_mcmc(nullptr, N).total; }

#define LG_MCMC_MAX_ROWS (1 << 30)
extern "C" int lg_mcmc_noise(int32_t N, float* xyz, const float* scaling, const float* rotation, const float* opacity, const float* noise,
                             float c, float k, float x0, uint32_t flags, void* stream_p)
{
    if (N < 0 || N >= LG_MCMC_MAX_ROWS) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_noise: N outside [0, 2^30)");
    if (c != c || k != k || x0 != x0) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_noise: a NaN among c, k, x0");
    if (N == 0) return LG_OK;
    if (!xyz) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_noise: null xyz");
    if (!scaling) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_noise: null scaling");
    if (!rotation) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_noise: null rotation");
    if (!opacity) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_noise: null opacity");
    if (!noise) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_noise: null noise");
    if ((((uintptr_t)xyz | (uintptr_t)scaling | (uintptr_t)rotation | (uintptr_t)opacity | (uintptr_t)noise) & 3) != 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_noise: xyz / scaling / rotation / opacity / noise must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    ProfScope ps(prof, "mcmc_noise", stream);
    lg_mcmc_noise_kernel<<<(unsigned)((N + 255) / 256), 256, 0, stream>>>(N, xyz, scaling, rotation, opacity, noise, c, k, x0);
    KLAUNCHED("lg_mcmc_noise_kernel");
    return LG_OK;
}

extern "C" int lg_mcmc_plan(int32_t N, int32_t n, const int32_t* src, const float* opacity, const float* scaling, float min_opacity,
                            void* scratch, uint32_t flags, void* stream_p)
{
    if (N < 0 || N >= LG_MCMC_MAX_ROWS) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_plan: N outside [0, 2^30)");
    if (n < 0 || (N == 0 && n > 0)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_plan: n < 0, or draws from an empty model");
    if (!(min_opacity >= 0.0f && min_opacity < 1.0f)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_plan: min_opacity outside [0, 1)");
    if (N == 0) return LG_OK;
    if (n > 0 && !src) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_plan: null src");
    if (!opacity) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_plan: null opacity");
    if (!scaling) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_plan: null scaling");
    if (!scratch) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_plan: null scratch");
    if ((((uintptr_t)src | (uintptr_t)opacity | (uintptr_t)scaling) & 3) != 0 || ((uintptr_t)scratch & 15) != 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_plan: misaligned src / opacity / scaling (4 bytes) or scratch (16)");
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    const McmcScratch d = carve_mcmc(scratch, N);
    {
        ProfScope ps(prof, "mcmc_count", stream);
        HIP_TRY(lg_zero_async(d.cnt, (size_t)N * 4, stream));
        if (n > 0) {
            lg_mcmc_count_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(N, n, src, d.cnt);
            KLAUNCHED("lg_mcmc_count_kernel");
        }
    }
    if (n > 0) {
        ProfScope ps(prof, "mcmc_plan", stream);
        lg_mcmc_plan_kernel<<<(unsigned)((N + 255) / 256), 256, 0, stream>>>(N, d.cnt, opacity, scaling, min_opacity, d.planned);
        KLAUNCHED("lg_mcmc_plan_kernel");
    }
    return LG_OK;
}

extern "C" int lg_mcmc_rows(int32_t N, int64_t N_out, int32_t n, const int32_t* dst, const int32_t* src, const void* scratch,
                            int32_t num_tensors, const lg_densify_tensor* tensors, uint32_t flags, void* stream_p)
{
    if (N < 0 || N >= LG_MCMC_MAX_ROWS) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: N outside [0, 2^30)");
    if (N_out < (int64_t)N || N_out > 0x7FFFFFFFll) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: N_out outside [N, 2^31)");
    if (n < 0 || (N == 0 && n > 0)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: n < 0, or draws from an empty model");
    if (num_tensors < 0 || num_tensors > LG_DENSIFY_MAX_TENSORS) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: num_tensors outside [0, 32]");
    if (num_tensors > 0 && !tensors) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: null tensors");
    const bool inplace = N_out == (int64_t)N;
    if (N == 0 || num_tensors == 0 || (inplace && n == 0)) return LG_OK;
    if (n > 0 && !dst) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: null dst");
    if (n > 0 && !src) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: null src");
    if (!scratch) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: null scratch");
    if ((((uintptr_t)dst | (uintptr_t)src) & 3) != 0 || ((uintptr_t)scratch & 15) != 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: misaligned dst / src (4 bytes) or scratch (16)");
    LgDensifyArgs a;
    memset(&a, 0, sizeof(a));
    size_t widest = 1;
    for (int t = 0; t < num_tensors; t++) {
        const lg_densify_tensor& x = tensors[t];
        if (x.role < LG_MCMC_COPY || x.role > LG_MCMC_SCALING) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: tensors: unknown role");
        if (x.row_words <= 0) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: tensors: row_words must be > 0 (leave empty tensors out)");
        if (!x.src || !x.dst) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: tensors: null src / dst");
        if ((((uintptr_t)x.src | (uintptr_t)x.dst) & 3) != 0) return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: tensors: src / dst must be 4-byte aligned");
        if ((x.role == LG_MCMC_OPACITY && x.row_words != 1) || (x.role == LG_MCMC_SCALING && x.row_words != 3))
            return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: tensors: the opacity role needs row_words == 1, the scaling role 3");
        if (inplace != (x.src == x.dst))
            return fail(LG_ERR_INVALID_ARGUMENT, "lg_mcmc_rows: tensors: src == dst exactly when N_out == N (in place)");
        a.src[t] = (const uint32_t*)x.src; a.dst[t] = (uint32_t*)x.dst; a.words[t] = (uint32_t)x.row_words; a.role[t] = (uint32_t)x.role;
        widest = std::max<size_t>(widest, (size_t)x.row_words);
    }
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    const McmcScratch d = carve_mcmc(const_cast<void*>(scratch), N);
    ProfScope ps(prof, "mcmc_rows", stream);
    lg_mcmc_move<<<row_move_grid((inplace ? 0 : (size_t)N) + (size_t)n, widest, num_tensors), 256, 0, stream>>>(
        N, N_out, n, dst, src, d.cnt, d.planned, a, inplace ? 1 : 0);
    KLAUNCHED("lg_mcmc_move");
    return LG_OK;
}

// ---- 3D smoothing filter (lg_filter3d.h) ----
extern "C" size_t lg_filter3d_scratch_bytes(int32_t N) { (void)N; return align_up((size_t)LG_F3D_MAX_WGS * sizeof(float)); }

extern "C" int lg_filter3d_update(int32_t N, const float* means3D, int32_t V, const lg_filter_camera* cameras, float* filter3d, uint8_t* seen,
                                  void* scratch, uint32_t flags, void* stream_p)
{
    if (N < 0 || N >= LG_ROWS_MAX) return fail(LG_ERR_INVALID_ARGUMENT, "lg_filter3d_update: N outside [0, 2^30)");
    if (V < 1) return fail(LG_ERR_INVALID_ARGUMENT, "lg_filter3d_update: V < 1 (the filter needs at least one camera)");
    if (!means3D || !cameras || !filter3d || !scratch) return fail(LG_ERR_INVALID_ARGUMENT, "lg_filter3d_update: null means3D / cameras / filter3d / scratch");
    if ((((uintptr_t)means3D | (uintptr_t)cameras | (uintptr_t)filter3d | (uintptr_t)scratch) & 3) != 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_filter3d_update: 32-bit tensors must be 4-byte aligned");
    if (N == 0) return LG_OK;
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    const unsigned wgs = (unsigned)std::min<int64_t>(((int64_t)N + LG_F3D_THREADS - 1) / LG_F3D_THREADS, LG_F3D_MAX_WGS);
    float* partial = (float*)scratch;
    {
        ProfScope ps(prof, "filter3d_update", stream);
        lg_filter3d_update_kernel<<<wgs, LG_F3D_THREADS, 0, stream>>>(N, means3D, V, cameras, filter3d, seen, partial);
        KLAUNCHED("lg_filter3d_update_kernel");
    }
    {
        ProfScope ps(prof, "filter3d_reduce", stream);
        lg_filter3d_fill_kernel<<<wgs, LG_F3D_THREADS, 0, stream>>>(N, (int)wgs, partial, filter3d);
        KLAUNCHED("lg_filter3d_fill_kernel");
    }
    return LG_OK;
}

static int lg_filter3d_check(const char* who, int32_t N, std::initializer_list<const void*> ptrs, bool* vec)
{
    if (N < 0 || N >= LG_ROWS_MAX) return refuse(who, "N outside [0, 2^30)");
    uintptr_t all = 0;
    for (const void* p : ptrs) {
        if (!p) return refuse(who, "null tensor");
        all |= (uintptr_t)p;
    }
    if (all & 3) return refuse(who, "float32 tensors must be 4-byte aligned");
    *vec = (all & 15) == 0;
    return LG_OK;
}

extern "C" int lg_filter3d_apply(int32_t N, const float* scaling, const float* opacity, const float* filter3d, float* out_scaling,
                                 float* out_opacity, uint32_t flags, void* stream_p)
{
    bool vec = false;
    const int rc = lg_filter3d_check("lg_filter3d_apply", N, { scaling, opacity, filter3d, out_scaling, out_opacity }, &vec);
    if (rc != LG_OK || N == 0) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    ProfScope ps(prof, "filter3d_apply", stream);
    const unsigned wgs = lg_rows4_wgs(N, LG_F3D_THREADS);
    filter3d_apply_kernel(flags & LG_FILTER3D_RAW)<<<wgs, LG_F3D_THREADS, 0, stream>>>(N, vec, scaling, opacity, filter3d, out_scaling, out_opacity);
    KLAUNCHED("lg_filter3d_apply_kernel");
    return LG_OK;
}

extern "C" int lg_filter3d_apply_bwd(int32_t N, const float* scaling, const float* opacity, const float* filter3d, const float* dL_dout_scaling,
                                     const float* dL_dout_opacity, float* dL_dscaling, float* dL_dopacity, uint32_t flags, void* stream_p)
{
    bool vec = false;
    const int rc = lg_filter3d_check("lg_filter3d_apply_bwd", N, { scaling, opacity, filter3d, dL_dout_scaling, dL_dout_opacity, dL_dscaling, dL_dopacity }, &vec);
    if (rc != LG_OK || N == 0) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    ProfScope ps(prof, "filter3d_apply_bwd", stream);
    const unsigned wgs = lg_rows4_wgs(N, LG_F3D_THREADS);
    filter3d_apply_bwd_kernel(flags & LG_FILTER3D_RAW)<<<wgs, LG_F3D_THREADS, 0, stream>>>(N, vec, scaling, opacity, filter3d, dL_dout_scaling, dL_dout_opacity,
                                                                                           dL_dscaling, dL_dopacity);
    KLAUNCHED("lg_filter3d_apply_bwd_kernel");
    return LG_OK;
}

// ---- normals and the depth-normal consistency loss (lg_normals.h, include/lightgaussian_normals.h) ----
struct NamedPtr { const char* name; const void* p; };
// null and alignment checks that name the argument; all16: every pointer is 16-byte aligned
static int normals_ptrs(const char* who, std::initializer_list<NamedPtr> ptrs, bool* all16 = nullptr)
{
    char what[96];
    uintptr_t all = 0;
    for (const NamedPtr& a : ptrs) {
        if (!a.p) { snprintf(what, sizeof(what), "null %s", a.name); return refuse(who, what); }
        if ((uintptr_t)a.p & 3) { snprintf(what, sizeof(what), "%s must be 4-byte aligned", a.name); return refuse(who, what); }
        all |= (uintptr_t)a.p;
    }
    if (all16) *all16 = (all & 15) == 0;
    return LG_OK;
}
static int normals_image(const char* who, int32_t H, int32_t W, float tanfovx, float tanfovy)
{
    if (H < 1 || H > LG_NRM_MAX_DIM) return refuse(who, "H outside [1, 32768]");
    if (W < 1 || W > LG_NRM_MAX_DIM) return refuse(who, "W outside [1, 32768]");
    if (tanfovx != tanfovx) return refuse(who, "tanfovx is NaN");
    if (tanfovy != tanfovy) return refuse(who, "tanfovy is NaN");
    return LG_OK;
}

extern "C" int lg_normal_rows(int32_t N, const float* xyz, const float* scaling, const float* rotation, const float* viewmatrix, float* rows,
                              uint32_t flags, void* stream_p)
{
    const char* who = "lg_normal_rows";
    if (N < 0 || N >= LG_ROWS_MAX) return refuse(who, "N outside [0, 2^30)");
    bool vec = false;
    int rc = normals_ptrs(who, { { "xyz", xyz }, { "scaling", scaling }, { "rotation", rotation }, { "rows", rows } }, &vec);
    if (rc == LG_OK) rc = normals_ptrs(who, { { "viewmatrix", viewmatrix } });
    if (rc != LG_OK || N == 0) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    ProfScope ps(flags & LG_FLAG_PROFILE, "normal_rows", stream);
    lg_normal_rows_kernel<<<lg_rows4_wgs(N, LG_NRM_THREADS), LG_NRM_THREADS, 0, stream>>>(N, vec, xyz, scaling, rotation, viewmatrix, rows);
    KLAUNCHED("lg_normal_rows_kernel");
    return LG_OK;
}

extern "C" int lg_normal_rows_bwd(int32_t N, const float* xyz, const float* scaling, const float* rotation, const float* viewmatrix,
                                  const float* dL_drows, float* dL_dxyz, float* dL_drotation, uint32_t flags, void* stream_p)
{
    const char* who = "lg_normal_rows_bwd";
    if (N < 0 || N >= LG_ROWS_MAX) return refuse(who, "N outside [0, 2^30)");
    bool vec = false;
    int rc = normals_ptrs(who, { { "xyz", xyz }, { "scaling", scaling }, { "rotation", rotation }, { "dL_drows", dL_drows }, { "dL_dxyz", dL_dxyz },
                                 { "dL_drotation", dL_drotation } }, &vec);
    if (rc == LG_OK) rc = normals_ptrs(who, { { "viewmatrix", viewmatrix } });
    if (rc != LG_OK || N == 0) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    ProfScope ps(flags & LG_FLAG_PROFILE, "normal_rows_bwd", stream);
    lg_normal_rows_bwd_kernel<<<lg_rows4_wgs(N, LG_NRM_THREADS), LG_NRM_THREADS, 0, stream>>>(N, vec, xyz, scaling, rotation, viewmatrix, dL_drows, dL_dxyz, dL_drotation);
    KLAUNCHED("lg_normal_rows_bwd_kernel");
    return LG_OK;
}

extern "C" int lg_depth_normals(int32_t H, int32_t W, const float* depth, float tanfovx, float tanfovy, float* normals, uint32_t flags, void* stream_p)
{
    const char* who = "lg_depth_normals";
    int rc = normals_image(who, H, W, tanfovx, tanfovy);
    if (rc == LG_OK) rc = normals_ptrs(who, { { "depth", depth }, { "normals", normals } });
    if (rc != LG_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    ProfScope ps(flags & LG_FLAG_PROFILE, "depth_normals", stream);
    lg_normal_fwd<false><<<dim3(lg_nrm_strips(W, LG_NRM_FWD_COLS), lg_nrm_segs(H)), 64, 0, stream>>>(H, W, tanfovx, tanfovy, depth, nullptr, nullptr, nullptr,
                                                                                                 normals, nullptr);
    KLAUNCHED("lg_normal_fwd");
    return LG_OK;
}

extern "C" int lg_depth_normals_bwd(int32_t H, int32_t W, const float* depth, float tanfovx, float tanfovy, const float* dL_dnormals,
                                    float* dL_ddepth, uint32_t flags, void* stream_p)
{
    const char* who = "lg_depth_normals_bwd";
    int rc = normals_image(who, H, W, tanfovx, tanfovy);
    if (rc == LG_OK) rc = normals_ptrs(who, { { "depth", depth }, { "dL_dnormals", dL_dnormals }, { "dL_ddepth", dL_ddepth } });
    if (rc != LG_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    ProfScope ps(flags & LG_FLAG_PROFILE, "depth_normals_bwd", stream);
    lg_normal_bwd<false><<<dim3(lg_nrm_strips(W, LG_NRM_BWD_COLS), lg_nrm_segs(H)), 64, 0, stream>>>(H, W, tanfovx, tanfovy, depth, dL_dnormals, nullptr, nullptr,
                                                                                                 nullptr, 0.0f, nullptr, dL_ddepth);
    KLAUNCHED("lg_normal_bwd");
    return LG_OK;
}

extern "C" size_t lg_normal_loss_scratch_bytes(int32_t H, int32_t W)
{
    if (H < 1 || W < 1 || H > LG_NRM_MAX_DIM || W > LG_NRM_MAX_DIM) return 0;
    return align_up((size_t)lg_nrm_strips(W, LG_NRM_FWD_COLS) * lg_nrm_segs(H) * sizeof(float));
}

extern "C" int lg_normal_loss(int32_t H, int32_t W, const float* normal_map, const float* depth, const float* alpha, const float* weight,
                              float tanfovx, float tanfovy, float* loss, float* depth_normals, void* scratch, uint32_t flags, void* stream_p)
{
    const char* who = "lg_normal_loss";
    int rc = normals_image(who, H, W, tanfovx, tanfovy);
    if (rc == LG_OK) rc = normals_ptrs(who, { { "normal_map", normal_map }, { "depth", depth }, { "alpha", alpha }, { "loss", loss }, { "scratch", scratch } });
    if (rc == LG_OK && weight) rc = normals_ptrs(who, { { "weight", weight } });
    if (rc == LG_OK && depth_normals) rc = normals_ptrs(who, { { "depth_normals", depth_normals } });
    if (rc != LG_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    const dim3 grid(lg_nrm_strips(W, LG_NRM_FWD_COLS), lg_nrm_segs(H));
    float* partials = (float*)scratch;
    {
        ProfScope ps(prof, "normal_loss", stream);
        lg_normal_fwd<true><<<grid, 64, 0, stream>>>(H, W, tanfovx, tanfovy, depth, normal_map, alpha, weight, depth_normals, partials);
        KLAUNCHED("lg_normal_fwd");
    }
    {
        ProfScope ps(prof, "normal_loss_reduce", stream);
        lg_mean_finalize<1><<<1, 256, 0, stream>>>((int)(grid.x * grid.y), 1.0 / ((double)H * W), partials, loss);
        KLAUNCHED("lg_mean_finalize");
    }
    return LG_OK;
}

extern "C" int lg_normal_loss_bwd(int32_t H, int32_t W, const float* normal_map, const float* depth, const float* alpha, const float* weight,
                                  float tanfovx, float tanfovy, const float* dL_dloss, float* dL_dnormal_map, float* dL_ddepth, uint32_t flags,
                                  void* stream_p)
{
    const char* who = "lg_normal_loss_bwd";
    int rc = normals_image(who, H, W, tanfovx, tanfovy);
    if (rc == LG_OK) rc = normals_ptrs(who, { { "normal_map", normal_map }, { "depth", depth }, { "alpha", alpha }, { "dL_dloss", dL_dloss },
                                              { "dL_dnormal_map", dL_dnormal_map }, { "dL_ddepth", dL_ddepth } });
    if (rc == LG_OK && weight) rc = normals_ptrs(who, { { "weight", weight } });
    if (rc != LG_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    ProfScope ps(flags & LG_FLAG_PROFILE, "normal_loss_bwd", stream);
    lg_normal_bwd<true><<<dim3(lg_nrm_strips(W, LG_NRM_BWD_COLS), lg_nrm_segs(H)), 64, 0, stream>>>(
        H, W, tanfovx, tanfovy, depth, normal_map, alpha, weight, dL_dloss, (float)(1.0 / ((double)H * W)), dL_dnormal_map, dL_ddepth);
    KLAUNCHED("lg_normal_bwd");
    return LG_OK;
}

// ---- TSDF fusion and marching tetrahedra (lg_tsdf.h, include/lightgaussian_mesh.h) ----
static bool positive_finite(float v) { return v > 0.0f && v <= 3.402823466e+38f; }
static bool finite_f(float v) { return v - v == 0.0f; }
// the checks of a volume every entry point shares; *vec: tsdf, weight and color are 16-byte aligned
static int tsdf_volume(const char* who, const lg_tsdf_volume* vol, bool* vec = nullptr)
{
    if (!vol) return refuse(who, "null volume");
    if (vol->nx < 1 || vol->ny < 1 || vol->nz < 1) return refuse(who, "nx, ny, nz must be at least 1");
    if ((int64_t)vol->nx * vol->ny >= LG_TSDF_MAX_POINTS || (int64_t)vol->nx * vol->ny * vol->nz >= LG_TSDF_MAX_POINTS)
        return refuse(who, "nx ny nz outside [1, 2^29)");
    if (!positive_finite(vol->voxel_size)) return refuse(who, "voxel_size must be positive and finite");
    if (!positive_finite(vol->trunc)) return refuse(who, "trunc must be positive and finite");
    for (int a = 0; a < 3; a++)
        if (!finite_f(vol->origin[a])) return refuse(who, "origin must be finite");
    bool all16 = false;
    int rc = normals_ptrs(who, { { "tsdf", vol->tsdf }, { "weight", vol->weight } }, &all16);
    if (rc == LG_OK && vol->color) {
        rc = normals_ptrs(who, { { "color", vol->color } });
        all16 = all16 && ((uintptr_t)vol->color & 15) == 0;
    }
    if (vec) *vec = all16;
    return rc;
}
static size_t tsdf_points(const lg_tsdf_volume* vol) { return (size_t)vol->nx * (size_t)vol->ny * (size_t)vol->nz; }

static LgTsdfLattice tsdf_lattice(const float* origin, float voxel, float trunc) { return { { origin[0], origin[1], origin[2] }, voxel, trunc }; }
static LgTsdfCam tsdf_cam(const lg_tsdf_view& v) { return { v.W, v.H, v.tanfovx, v.tanfovy, v.depth_max, v.z_min, v.alpha_min }; }

// The checks of the views lg_tsdf_integrate, lg_blocks_touch and lg_blocks_integrate share.  need_color: the volume keeps colour and the
// call reads views[i].color.  align_color: views[i].color is held to 4-byte alignment; the dense entry does so even for a volume that
// keeps no colour, the block entries only when the call reads it.
static int tsdf_views(const char* who, int32_t n_views, const lg_tsdf_view* views, bool need_color, bool align_color)
{
    if (n_views < 0) return refuse(who, "n_views < 0");
    if (n_views > 0 && !views) return refuse(who, "null views");
    for (int i = 0; i < n_views; i++) {
        const lg_tsdf_view& v = views[i];
        char what[96];
        auto bad = [&](const char* text) { snprintf(what, sizeof(what), "views[%d]: %s", i, text); return refuse(who, what); };
        if (v.H < 1 || v.H > LG_TSDF_MAX_DIM) return bad("H outside [1, 32768]");
        if (v.W < 1 || v.W > LG_TSDF_MAX_DIM) return bad("W outside [1, 32768]");
        if (v.tanfovx != v.tanfovx) return bad("tanfovx is NaN");
        if (v.tanfovy != v.tanfovy) return bad("tanfovy is NaN");
        if (v.alpha_min != v.alpha_min || v.depth_max != v.depth_max || v.z_min != v.z_min) return bad("alpha_min, depth_max or z_min is NaN");
        if (!v.viewmatrix) return bad("null viewmatrix");
        if (!v.depth) return bad("null depth");
        if (need_color && !v.color) return bad("null color for a volume that keeps colour");
        if (((uintptr_t)v.viewmatrix | (uintptr_t)v.depth | (uintptr_t)(align_color ? v.color : nullptr) | (uintptr_t)v.alpha) & 3)
            return bad("viewmatrix, depth, color and alpha must be 4-byte aligned");
    }
    return LG_OK;
}
// views[first .. first + n) as the by-value argument of an integrate kernel; color: the volume keeps colour
static LgTsdfBatch tsdf_batch(const lg_tsdf_view* views, int first, int n, bool color)
{
    LgTsdfBatch b;
    memset(&b, 0, sizeof(b));
    for (int k = 0; k < n; k++) {
        const lg_tsdf_view& v = views[first + k];
        b.v[k] = { v.viewmatrix, v.depth, color ? v.color : nullptr, v.alpha, tsdf_cam(v) };
    }
    return b;
}

extern "C" int lg_tsdf_integrate(const lg_tsdf_volume* vol, int32_t n_views, const lg_tsdf_view* views, uint32_t flags, void* stream_p)
{
    const char* who = "lg_tsdf_integrate";
    bool vec = false;
    int rc = tsdf_volume(who, vol, &vec);
    if (rc == LG_OK) rc = tsdf_views(who, n_views, views, vol->color != nullptr, true);
    if (rc != LG_OK) return rc;
    if (n_views == 0) return LG_OK;
    hipStream_t stream = (hipStream_t)stream_p;
    const LgMeshDims d = { vol->nx, vol->ny, vol->nz };
    const LgTsdfLattice g = tsdf_lattice(vol->origin, vol->voxel_size, vol->trunc);
    const unsigned wgs = (unsigned)lg_tsdf_bricks(vol->nx, vol->ny, vol->nz);
    for (int first = 0; first < n_views; first += LG_TSDF_BATCH) {
        const int n = std::min(LG_TSDF_BATCH, n_views - first);
        const LgTsdfBatch b = tsdf_batch(views, first, n, vol->color != nullptr);
        ProfScope ps(flags & LG_FLAG_PROFILE, "tsdf_integrate", stream);
        if (vol->color) lg_tsdf_integrate_kernel<true><<<wgs, LG_TSDF_THREADS, 0, stream>>>(d, g, vec, n, b, vol->tsdf, vol->weight, vol->color);
        else lg_tsdf_integrate_kernel<false><<<wgs, LG_TSDF_THREADS, 0, stream>>>(d, g, vec, n, b, vol->tsdf, vol->weight, nullptr);
        KLAUNCHED("lg_tsdf_integrate_kernel");
    }
    return LG_OK;
}

extern "C" size_t lg_mesh_scratch_bytes(int32_t nx, int32_t ny, int32_t nz)
{
    if (nx < 1 || ny < 1 || nz < 1 || (int64_t)nx * ny >= LG_TSDF_MAX_POINTS || (int64_t)nx * ny * nz >= LG_TSDF_MAX_POINTS) return 0;
    const size_t P = (size_t)nx * (size_t)ny * (size_t)nz;
    return carve_mesh(nullptr, P, lg_mesh_blocks(P), 0).total;
}

// The checks the count and emit calls of both volumes share, after the volume's own.
static int mesh_args(const char* who, float iso, float min_weight, const void* scratch)
{
    if (!finite_f(iso)) return refuse(who, "iso must be finite");
    if (!positive_finite(min_weight)) return refuse(who, "min_weight must be positive and finite");
    if (!scratch) return refuse(who, "null scratch");
    if ((uintptr_t)scratch & 255) return refuse(who, "scratch must be 256-byte aligned");
    return LG_OK;
}
static int mesh_counts_ptr(const char* who, const int64_t* counts)
{
    if (!counts) return refuse(who, "null counts");
    if ((uintptr_t)counts & 7) return refuse(who, "counts must be 8-byte aligned");
    return LG_OK;
}
// What an emit call does before its launch: the ranges of n_vertices and n_faces, the output pointers, then the read-back of the counts
// that `count_fn` left in scratch (16 bytes, one synchronise) and the refusal of sizes that differ from them.
static int mesh_emit_args(const char* who, const char* count_fn, bool keeps_color, const LgMeshScratch& s, int64_t n_vertices, int64_t n_faces,
                          const float* vertices, const float* colors, const int32_t* faces, hipStream_t stream)
{
    if (n_vertices < 0 || n_vertices >= (1ll << 31)) return refuse(who, "n_vertices outside [0, 2^31)");
    if (n_faces < 0 || n_faces >= (1ll << 31)) return refuse(who, "n_faces outside [0, 2^31)");
    if (colors && !keeps_color) return refuse(who, "colors for a volume that keeps no colour");
    int rc = LG_OK;
    if (n_vertices > 0) {
        rc = normals_ptrs(who, { { "vertices", vertices } });
        if (rc == LG_OK && colors) rc = normals_ptrs(who, { { "colors", colors } });
    }
    if (rc == LG_OK && n_faces > 0) rc = normals_ptrs(who, { { "faces", faces } });
    if (rc != LG_OK) return rc;
    int64_t h_counts[2] = { -1, -1 };
    HIP_TRY(hipMemcpyAsync(h_counts, s.counts, 16, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const char* names[2] = { "n_vertices", "n_faces" };
    const int64_t given[2] = { n_vertices, n_faces };
    for (int c = 0; c < 2; c++)
        if (h_counts[c] != given[c]) {
            char what[112];
            snprintf(what, sizeof(what), "%s differs from the count %s left in scratch", names[c], count_fn);
            return refuse(who, what);
        }
    return LG_OK;
}

extern "C" int lg_mesh_count(const lg_tsdf_volume* vol, float iso, float min_weight, void* scratch, int64_t* counts, uint32_t flags, void* stream_p)
{
    const char* who = "lg_mesh_count";
    int rc = tsdf_volume(who, vol);
    if (rc == LG_OK) rc = mesh_args(who, iso, min_weight, scratch);
    if (rc == LG_OK) rc = mesh_counts_ptr(who, counts);
    if (rc != LG_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    const size_t P = tsdf_points(vol), nb = lg_mesh_blocks(P);
    const LgMeshScratch s = carve_mesh(scratch, P, nb, 0);
    const LgMeshDims d = { vol->nx, vol->ny, vol->nz };
    {
        ProfScope ps(prof, "mesh_count", stream);
        lg_mesh_count_kernel<<<(unsigned)nb, 256, 0, stream>>>(d, P, iso, min_weight, vol->tsdf, vol->weight, s.vmask, s.fcount, s.blk, s.blk + nb);
        KLAUNCHED("lg_mesh_count_kernel");
    }
    {
        ProfScope ps(prof, "mesh_scan", stream);
        lg_mesh_scan_kernel<<<2, 1024, 0, stream>>>(nb, s.blk, counts, s.counts);
        KLAUNCHED("lg_mesh_scan_kernel");
        lg_mesh_prefix_kernel<4, false><<<(unsigned)nb, 256, 0, stream>>>(P, s.vmask, s.fcount, s.blk, s.blk + nb, s.vprefix, s.fprefix);
        KLAUNCHED("lg_mesh_prefix_kernel");
    }
    return LG_OK;
}

extern "C" int lg_mesh_emit(const lg_tsdf_volume* vol, float iso, float min_weight, void* scratch, int64_t n_vertices, int64_t n_faces, float* vertices,
                            float* colors, int32_t* faces, uint32_t flags, void* stream_p)
{
    const char* who = "lg_mesh_emit";
    int rc = tsdf_volume(who, vol);
    if (rc == LG_OK) rc = mesh_args(who, iso, min_weight, scratch);
    if (rc != LG_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    const size_t P = tsdf_points(vol);
    const LgMeshScratch s = carve_mesh(scratch, P, lg_mesh_blocks(P), 0);
    rc = mesh_emit_args(who, "lg_mesh_count", vol->color != nullptr, s, n_vertices, n_faces, vertices, colors, faces, stream);
    if (rc != LG_OK) return rc;
    if (n_vertices == 0 && n_faces == 0) return LG_OK;
    const LgMeshDims d = { vol->nx, vol->ny, vol->nz };
    ProfScope ps(flags & LG_FLAG_PROFILE, "mesh_emit", stream);
    lg_mesh_emit_kernel<<<(unsigned)((P + 255) / 256), 256, 0, stream>>>(d, P, tsdf_lattice(vol->origin, vol->voxel_size, vol->trunc), iso, min_weight, vol->tsdf,
                                                                          vol->weight, vol->color, s.vprefix, s.fprefix, s.vmask, s.fcount, n_vertices, n_faces,
                                                                          vertices, colors, faces);
    KLAUNCHED("lg_mesh_emit_kernel");
    return LG_OK;
}

// ---- block-sparse TSDF volume (lg_blocks.h, include/lightgaussian_blocks.h) ----
// the checks of a block volume every entry point shares
static int block_volume(const char* who, const lg_block_volume* vol, const char* name = "volume")
{
    char what[96];
    auto bad = [&](const char* text) { snprintf(what, sizeof(what), "%s: %s", name, text); return refuse(who, what); };
    if (!vol) return bad("null volume");
    if (vol->n_blocks < 0 || vol->n_blocks >= LG_BLK_MAX_BLOCKS) return bad("n_blocks outside [0, 2^20): n_blocks 512 must stay below 2^29");
    if (!positive_finite(vol->voxel_size)) return bad("voxel_size must be positive and finite");
    if (!(vol->trunc > 0.0f && vol->trunc <= 4.0f * vol->voxel_size)) return bad("trunc must lie in (0, 4 voxel_size]");
    for (int a = 0; a < 3; a++)
        if (!finite_f(vol->origin[a])) return bad("origin must be finite");
    if (vol->n_blocks == 0) return LG_OK;
    if (!vol->keys) return bad("null keys");
    if ((uintptr_t)vol->keys & 7) return bad("keys must be 8-byte aligned");
    if (!vol->tsdf) return bad("null tsdf");
    if (!vol->weight) return bad("null weight");
    if ((uintptr_t)vol->tsdf & 15) return bad("tsdf must be 16-byte aligned");
    if ((uintptr_t)vol->weight & 15) return bad("weight must be 16-byte aligned");
    if ((uintptr_t)vol->color & 15) return bad("color must be 16-byte aligned");
    return LG_OK;
}
static LgTsdfLattice block_lattice(const lg_block_volume* vol) { return tsdf_lattice(vol->origin, vol->voxel_size, vol->trunc); }
static int64_t block_touch_waves(int32_t n_views, const lg_tsdf_view* views, int64_t* pixels = nullptr)
{
    int64_t waves = 0, px = 0;
    for (int i = 0; i < n_views; i++) { waves += lg_blk_touch_waves(views[i].W, views[i].H); px += (int64_t)views[i].W * views[i].H; }
    if (pixels) *pixels = px;
    return waves;
}
// scratch of lg_blocks_touch: [2] int64 totals, then wave_n [2][waves]
static size_t block_touch_bytes(int64_t waves) { return align_up(16) + align_up((size_t)std::max<int64_t>(waves, 1) * 8); }

extern "C" size_t lg_blocks_touch_scratch_bytes(int32_t n_views, const lg_tsdf_view* views)
{
    if (n_views < 0 || (n_views > 0 && !views)) return 0;
    for (int i = 0; i < n_views; i++)
        if (views[i].W < 1 || views[i].W > LG_TSDF_MAX_DIM || views[i].H < 1 || views[i].H > LG_TSDF_MAX_DIM) return 0;
    return block_touch_bytes(block_touch_waves(n_views, views));
}

extern "C" int lg_blocks_touch(const lg_block_volume* vol, int32_t n_views, const lg_tsdf_view* views, int64_t capacity, int64_t* candidates, int64_t* stats,
                               void* scratch, uint32_t flags, void* stream_p)
{
    const char* who = "lg_blocks_touch";
    int rc = block_volume(who, vol);
    if (rc == LG_OK) rc = tsdf_views(who, n_views, views, false, false);
    if (rc != LG_OK) return rc;
    if (capacity < 0 || capacity >= (1ll << 30)) return refuse(who, "capacity outside [0, 2^30)");
    if (capacity > 0 && !candidates) return refuse(who, "null candidates");
    if ((uintptr_t)candidates & 7) return refuse(who, "candidates must be 8-byte aligned");
    if (!stats) return refuse(who, "null stats");
    if ((uintptr_t)stats & 7) return refuse(who, "stats must be 8-byte aligned");
    if (!scratch) return refuse(who, "null scratch");
    if ((uintptr_t)scratch & 255) return refuse(who, "scratch must be 256-byte aligned");
    int64_t pixels = 0;
    const int64_t waves = block_touch_waves(n_views, views, &pixels);
    if (pixels >= LG_BLK_TOUCH_MAX_PIXELS) return refuse(who, "views: 2^26 pixels or more in one call");
    hipStream_t stream = (hipStream_t)stream_p;
    int64_t* totals = (int64_t*)scratch;
    uint32_t* wave_n = (uint32_t*)((char*)scratch + align_up(16));
    const LgTsdfLattice g = block_lattice(vol);
    ProfScope ps(flags & LG_FLAG_PROFILE, "blocks_touch", stream);
    for (int emit = 0; emit < 2; emit++) {
        uint32_t wave_base = 0;
        for (int first = 0; first < n_views; first += LG_TSDF_BATCH) {
            const int n = std::min(LG_TSDF_BATCH, n_views - first);
            LgBlkTouchBatch b;
            memset(&b, 0, sizeof(b));
            uint32_t end = 0;
            for (int k = 0; k < n; k++) {
                const lg_tsdf_view& v = views[first + k];
                end += lg_blk_touch_waves(v.W, v.H);
                b.v[k] = { v.viewmatrix, v.depth, v.alpha, tsdf_cam(v), end, (uint32_t)((v.W + LG_BLK_TOUCH_TILE - 1) / LG_BLK_TOUCH_TILE) };
            }
            const unsigned wgs = (end + 3) / 4;
            if (emit) lg_blk_touch_kernel<true><<<wgs, 256, 0, stream>>>(g, n, b, end, wave_base, (uint32_t)waves, wave_n, capacity, candidates);
            else lg_blk_touch_kernel<false><<<wgs, 256, 0, stream>>>(g, n, b, end, wave_base, (uint32_t)waves, wave_n, capacity, candidates);
            KLAUNCHED("lg_blk_touch_kernel");
            wave_base += end;
        }
        if (!emit) {
            // channel 0: candidates per wave -> exclusive prefix, total to stats[1]; channel 1: skipped pixels, total to stats[2]
            lg_mesh_scan_kernel<<<2, 1024, 0, stream>>>((size_t)waves, wave_n, stats + 1, totals);
            KLAUNCHED("lg_mesh_scan_kernel");
        }
    }
    if (capacity > 0) {
        lg_blk_pad_kernel<<<(unsigned)std::min<int64_t>((capacity + 255) / 256, 1024), 256, 0, stream>>>(totals, capacity, candidates);
        KLAUNCHED("lg_blk_pad_kernel");
    }
    return LG_OK;
}

// scratch of lg_blocks_merge: keys_in [n], sorted [n], blk [ceil(n / 1024)], [2] int64, the sort's temp storage
struct LgBlkMergeScratch { uint64_t* keys_in; uint64_t* sorted; uint32_t* blk; int64_t* copy; void* sort_temp; size_t sort_bytes, total; };
static LgBlkMergeScratch carve_blk_merge(void* base, size_t n)
{
    LgBlkMergeScratch s; size_t off = 0; char* p = (char*)base;
    auto take = [&](size_t bytes) { void* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
    const size_t m = std::max<size_t>(n, 1);
    s.keys_in = (uint64_t*)take(m * 8);
    s.sorted = (uint64_t*)take(m * 8);
    s.blk = (uint32_t*)take((m + 1023) / 1024 * 4);
    s.copy = (int64_t*)take(16);
    s.sort_bytes = lg_sort_layout(m).total;
    s.sort_temp = take(s.sort_bytes);
    s.total = off;
    return s;
}
extern "C" size_t lg_blocks_merge_scratch_bytes(int64_t n) { return (n < 0 || n >= (1ll << 30)) ? 0 : carve_blk_merge(nullptr, (size_t)n).total; }

extern "C" int lg_blocks_merge(int64_t n_old, const int64_t* old_keys, int64_t n_add, const int64_t* add_keys, int64_t* merged, int64_t* count, void* scratch,
                               uint32_t flags, void* stream_p)
{
    const char* who = "lg_blocks_merge";
    if (n_old < 0 || n_old >= LG_BLK_MAX_BLOCKS) return refuse(who, "n_old outside [0, 2^20)");
    if (n_add < 0 || n_old + n_add >= (1ll << 30)) return refuse(who, "n_add negative or n_old + n_add >= 2^30");
    if (n_old > 0 && !old_keys) return refuse(who, "null old_keys");
    if (n_add > 0 && !add_keys) return refuse(who, "null add_keys");
    if (n_old + n_add > 0 && !merged) return refuse(who, "null merged");
    if (!count) return refuse(who, "null count");
    if (((uintptr_t)old_keys | (uintptr_t)add_keys | (uintptr_t)merged | (uintptr_t)count) & 7) return refuse(who, "old_keys, add_keys, merged and count must be 8-byte aligned");
    if (!scratch) return refuse(who, "null scratch");
    if ((uintptr_t)scratch & 255) return refuse(who, "scratch must be 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_p;
    const size_t n = (size_t)(n_old + n_add), nb = (n + 1023) / 1024;
    const LgBlkMergeScratch s = carve_blk_merge(scratch, n);
    ProfScope ps(flags & LG_FLAG_PROFILE, "blocks_touch", stream);
    if (n > 0) {
        lg_blk_concat_kernel<<<(unsigned)std::min<size_t>((n + 255) / 256, 2048), 256, 0, stream>>>((size_t)n_old, old_keys, (size_t)n_add, add_keys, s.keys_in);
        KLAUNCHED("lg_blk_concat_kernel");
        size_t tb = s.sort_bytes;
        HIP_TRY(lg_sort_keys(s.sort_temp, tb, s.keys_in, s.sorted, (uint32_t)n, 0, 64, nullptr, false, stream));
        lg_blk_unique_kernel<false><<<(unsigned)nb, 256, 0, stream>>>(n, s.sorted, s.blk, merged, nullptr, count);
        KLAUNCHED("lg_blk_unique_kernel");
    }
    lg_mesh_scan_kernel<<<1, 1024, 0, stream>>>(nb * (n > 0), s.blk, count, s.copy);
    KLAUNCHED("lg_mesh_scan_kernel");
    if (n > 0) {
        lg_blk_unique_kernel<true><<<(unsigned)nb, 256, 0, stream>>>(n, s.sorted, s.blk, merged, lg_sort_error_word(s.sort_temp, n), count);
        KLAUNCHED("lg_blk_unique_kernel");
    }
    return LG_OK;
}

extern "C" int lg_blocks_regrid(const lg_block_volume* from, const lg_block_volume* to, uint32_t flags, void* stream_p)
{
    const char* who = "lg_blocks_regrid";
    int rc = block_volume(who, from, "from");
    if (rc == LG_OK) rc = block_volume(who, to, "to");
    if (rc != LG_OK) return rc;
    if (to->n_blocks == 0) return LG_OK;
    if (from->n_blocks > 0 && (from->color != nullptr) != (to->color != nullptr)) return refuse(who, "from and to: both keep colour or neither does");
    hipStream_t stream = (hipStream_t)stream_p;
    ProfScope ps(flags & LG_FLAG_PROFILE, "blocks_regrid", stream);
    if (to->color) lg_blk_regrid_kernel<true><<<(unsigned)to->n_blocks, LG_BLK_THREADS, 0, stream>>>(from->n_blocks, from->keys, to->keys, from->tsdf, from->weight, from->color, to->tsdf, to->weight, to->color);
    else lg_blk_regrid_kernel<false><<<(unsigned)to->n_blocks, LG_BLK_THREADS, 0, stream>>>(from->n_blocks, from->keys, to->keys, from->tsdf, from->weight, nullptr, to->tsdf, to->weight, nullptr);
    KLAUNCHED("lg_blk_regrid_kernel");
    return LG_OK;
}

extern "C" int lg_blocks_integrate(const lg_block_volume* vol, int32_t n_views, const lg_tsdf_view* views, uint32_t flags, void* stream_p)
{
    const char* who = "lg_blocks_integrate";
    int rc = block_volume(who, vol);
    if (rc == LG_OK) rc = tsdf_views(who, n_views, views, vol->color != nullptr, vol->color != nullptr);
    if (rc != LG_OK) return rc;
    if (n_views == 0 || vol->n_blocks == 0) return LG_OK;
    hipStream_t stream = (hipStream_t)stream_p;
    const LgTsdfLattice g = block_lattice(vol);
    for (int first = 0; first < n_views; first += LG_TSDF_BATCH) {
        const int n = std::min(LG_TSDF_BATCH, n_views - first);
        const LgTsdfBatch b = tsdf_batch(views, first, n, vol->color != nullptr);
        ProfScope ps(flags & LG_FLAG_PROFILE, "blocks_integrate", stream);
        if (vol->color) lg_blk_integrate_kernel<true><<<(unsigned)vol->n_blocks, LG_BLK_THREADS, 0, stream>>>(g, vol->keys, n, b, vol->tsdf, vol->weight, vol->color);
        else lg_blk_integrate_kernel<false><<<(unsigned)vol->n_blocks, LG_BLK_THREADS, 0, stream>>>(g, vol->keys, n, b, vol->tsdf, vol->weight, nullptr);
        KLAUNCHED("lg_blk_integrate_kernel");
    }
    return LG_OK;
}

// scratch of the mesh calls of n blocks: one workgroup of the count kernel and one row of nbr per block
static LgMeshScratch carve_blk_mesh(void* base, size_t n) { return carve_mesh(base, n * LG_BLK_POINTS, n, n); }
extern "C" size_t lg_blocks_mesh_scratch_bytes(int32_t n_blocks)
{
    return (n_blocks < 0 || n_blocks >= LG_BLK_MAX_BLOCKS) ? 0 : carve_blk_mesh(nullptr, (size_t)n_blocks).total;
}

extern "C" int lg_blocks_mesh_count(const lg_block_volume* vol, float iso, float min_weight, void* scratch, int64_t* counts, uint32_t flags, void* stream_p)
{
    const char* who = "lg_blocks_mesh_count";
    int rc = block_volume(who, vol);
    if (rc == LG_OK) rc = mesh_args(who, iso, min_weight, scratch);
    if (rc == LG_OK) rc = mesh_counts_ptr(who, counts);
    if (rc != LG_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    const bool prof = flags & LG_FLAG_PROFILE;
    const uint32_t n = (uint32_t)vol->n_blocks;
    const LgMeshScratch s = carve_blk_mesh(scratch, n);
    if (n > 0) {
        ProfScope ps(prof, "blocks_mesh_count", stream);
        lg_blk_nbr_kernel<<<(n * 8 + 255) / 256, 256, 0, stream>>>((int)n, vol->keys, s.nbr);
        KLAUNCHED("lg_blk_nbr_kernel");
        lg_blk_mesh_count_kernel<<<n, LG_BLK_MESH_THREADS, 0, stream>>>(n, iso, min_weight, s.nbr, vol->tsdf, vol->weight, s.vmask, s.fcount, s.blk, s.blk + n);
        KLAUNCHED("lg_blk_mesh_count_kernel");
    }
    {
        ProfScope ps(prof, "blocks_mesh_scan", stream);
        lg_mesh_scan_kernel<<<2, 1024, 0, stream>>>((size_t)n, s.blk, counts, s.counts);
        KLAUNCHED("lg_mesh_scan_kernel");
        if (n > 0) {
            static_assert(LG_BLK_POINTS == LG_BLK_MESH_THREADS * 2, "WHOLE: a block is exactly the points of one workgroup, so P = 512 n has no partial one");
            lg_mesh_prefix_kernel<2, true><<<n, LG_BLK_MESH_THREADS, 0, stream>>>((size_t)n * LG_BLK_POINTS, s.vmask, s.fcount, s.blk, s.blk + n, s.vprefix, s.fprefix);
            KLAUNCHED("lg_mesh_prefix_kernel");
        }
    }
    return LG_OK;
}

extern "C" int lg_blocks_mesh_emit(const lg_block_volume* vol, float iso, float min_weight, void* scratch, int64_t n_vertices, int64_t n_faces, float* vertices,
                                   float* colors, int32_t* faces, uint32_t flags, void* stream_p)
{
    const char* who = "lg_blocks_mesh_emit";
    int rc = block_volume(who, vol);
    if (rc == LG_OK) rc = mesh_args(who, iso, min_weight, scratch);
    if (rc != LG_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    const uint32_t n = (uint32_t)vol->n_blocks;
    const LgMeshScratch s = carve_blk_mesh(scratch, n);
    rc = mesh_emit_args(who, "lg_blocks_mesh_count", vol->color != nullptr, s, n_vertices, n_faces, vertices, colors, faces, stream);
    if (rc != LG_OK) return rc;
    if (n == 0 || (n_vertices == 0 && n_faces == 0)) return LG_OK;
    ProfScope ps(flags & LG_FLAG_PROFILE, "blocks_mesh_emit", stream);
    lg_blk_mesh_emit_kernel<<<n, LG_BLK_MESH_THREADS, 0, stream>>>(n, block_lattice(vol), iso, min_weight, vol->keys, s.nbr, vol->tsdf, vol->weight, vol->color,
                                                                   s.vprefix, s.fprefix, s.vmask, s.fcount, n_vertices, n_faces, vertices, colors, faces);
    KLAUNCHED("lg_blk_mesh_emit_kernel");
    return LG_OK;
}

extern "C" size_t lg_knn_scratch_bytes(int32_t P) { return P < 0 ? 0 : carve_knn(nullptr, P).total; }

extern "C" int lg_knn3_mean_dist2(int32_t P, const float* points, float* mean_dist2, void* scratch, uint32_t flags, void* stream_p)
{
    if (P < 0) return fail(LG_ERR_INVALID_ARGUMENT, "bad point count");
    if (P == 0) return LG_OK;
    if (!points || !mean_dist2 || !scratch) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    const bool debug = flags & LG_FLAG_DEBUG, prof = flags & LG_FLAG_PROFILE;
    KnnView kv = carve_knn(scratch, P);
    ProfScope ps(prof, "knn3", stream);
    HIP_TRY(hipMemsetAsync(kv.box, 0xFF, 12, stream));                 // min keys
    HIP_TRY(hipMemsetAsync(kv.box + 3, 0, 64 - 12, stream));           // max keys, open-point counters
    const int nb = (P + 255) / 256;
    lg_knn_bbox<<<std::min(nb, 1024), 256, 0, stream>>>(P, points, kv.box);
    KCHECK("lg_knn_bbox");
    int key_bits = 1;
    while ((1u << key_bits) < kv.cap) key_bits++;
    for (int level = 0; level < LG_KNN_LEVELS; level++) {
        lg_knn_cells<<<nb, 256, 0, stream>>>(P, kv.cap, level, points, kv.box, kv.pairs_in);
        KCHECK("lg_knn_cells");
        size_t tb = kv.sort_temp_bytes;
        HIP_TRY(lg_sort_keys(kv.sort_temp, tb, kv.pairs_in, kv.pairs_out, (uint32_t)P, 32, 32 + key_bits, nullptr, false, stream));
        HIP_TRY(hipMemsetAsync(kv.cell_start, 0, (size_t)kv.cap * 4, stream));
        HIP_TRY(hipMemsetAsync(kv.cell_end, 0, (size_t)kv.cap * 4, stream));
        lg_knn_ranges<<<nb, 256, 0, stream>>>(P, points, kv.pairs_out, kv.cell_start, kv.cell_end, kv.sorted, lg_sort_error_word(kv.sort_temp, (size_t)P), kv.box);
        KCHECK("lg_knn_ranges");
        uint32_t* open_in = (level & 1) ? kv.open_a : kv.open_b;
        uint32_t* open_out = (level & 1) ? kv.open_b : kv.open_a;
        const int max_rings = level == LG_KNN_LEVELS - 1 ? (1 << 30) : LG_KNN_RINGS;
        lg_knn_query<<<nb, 256, 0, stream>>>(P, kv.cap, level, max_rings, points, kv.box, kv.sorted, kv.cell_start, kv.cell_end, open_in,
                                             kv.box + 8 + (level > 0 ? level - 1 : 0), open_out, kv.box + 8 + level, mean_dist2);
        KCHECK("lg_knn_query");
    }
    // one 4-byte read-back at the end (distCUDA2 runs once per training run, scene/gaussian_model.py:152): did any level's sort give up?
    uint32_t h_err = 0;
    HIP_TRY(hipMemcpyAsync(&h_err, kv.box + 15, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h_err) return fail(LG_ERR_DEVICE, "lg_knn3_mean_dist2: the radix sort of a grid level gave up (look-back poll budget exhausted): the distances are void");
    return LG_OK;
}

extern "C" size_t lg_loss_state_bytes(int32_t C, int32_t H, int32_t W)
{
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return carve_loss(nullptr, C, H, W).total;
}

// what the two loss entry points check and derive: the state carved (the backward reads what the forward left there) and the grid of
// one wave per (strip of 64 columns, LG_LOSS_TH rows, plane).  out: the buffer the call writes
static int loss_args(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, const void* state, const float* out, LossView* lv, dim3* grid)
{
    if (C <= 0 || H <= 0 || W <= 0 || C > 65535) return fail(LG_ERR_INVALID_ARGUMENT, "bad image shape");
    if (!img || !gt || !state || !out) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    *lv = carve_loss(const_cast<void*>(state), C, H, W);
    *grid = dim3(lg_loss_strips(W), lg_loss_segs(H), C);
    if (grid->y > 65535) return fail(LG_ERR_INVALID_ARGUMENT, "image too large");
    return LG_OK;
}

extern "C" int lg_loss_forward(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, void* state, float* out_l1_ssim,
                               uint32_t flags, void* stream_p)
{
    LossView lv; dim3 grid;
    const int rc = loss_args(C, H, W, img, gt, state, out_l1_ssim, &lv, &grid);
    if (rc != LG_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    const bool debug = flags & LG_FLAG_DEBUG, prof = flags & LG_FLAG_PROFILE;
    if (flags & LG_FLAG_L1_ONLY) {
        ProfScope ps(prof, "l1_fwd", stream);
        const size_t n = (size_t)C * H * W;
        const int blocks = (int)std::min<size_t>((n + 1023) / 1024, (size_t)grid.x * grid.y * grid.z);   // partials has one slot per tile
        lg_l1_fwd<<<blocks, 256, 0, stream>>>(n, img, gt, lv.partials);
        KCHECK("lg_l1_fwd");
        lg_mean_finalize<2><<<1, 256, 0, stream>>>(blocks, 1.0 / (double)n, (const float*)lv.partials, out_l1_ssim);
        KCHECK("lg_mean_finalize");
        return LG_OK;
    }
    {
        ProfScope ps(prof, "loss_fwd", stream);
        lg_loss_fwd<<<grid, LG_LOSS_STRIP, 0, stream>>>(H, W, img, gt, lv.dmu1, lv.dsig1, lv.dsig12, lv.partials);
        KCHECK("lg_loss_fwd");
        lg_mean_finalize<2><<<1, 256, 0, stream>>>((int)(grid.x * grid.y * grid.z), 1.0 / ((double)C * H * W), (const float*)lv.partials, out_l1_ssim);
        KCHECK("lg_mean_finalize");
    }
    return LG_OK;
}

extern "C" int lg_loss_backward(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, const void* state,
                                const float* dL_dl1, float scale_l1, const float* dL_dssim, float scale_ssim, float* dL_dimg,
                                uint32_t flags, void* stream_p)
{
    LossView lv; dim3 grid;
    const int rc = loss_args(C, H, W, img, gt, state, dL_dimg, &lv, &grid);
    if (rc != LG_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_p;
    const bool debug = flags & LG_FLAG_DEBUG, prof = flags & LG_FLAG_PROFILE;
    if (flags & LG_FLAG_L1_ONLY) {
        ProfScope ps(prof, "l1_bwd", stream);
        const size_t n = (size_t)C * H * W;
        lg_l1_bwd<<<(int)std::min<size_t>((n + 1023) / 1024, 65535 * 16), 256, 0, stream>>>(n, img, gt, dL_dl1, scale_l1 / (float)n, dL_dimg);
        KCHECK("lg_l1_bwd");
        return LG_OK;
    }
    {
        ProfScope ps(prof, "loss_bwd", stream);
        lg_loss_bwd<<<grid, LG_LOSS_STRIP, 0, stream>>>(H, W, img, gt, lv.dmu1, lv.dsig1, lv.dsig12, dL_dl1, scale_l1, dL_dssim, scale_ssim,
                                              (float)(1.0 / ((double)C * H * W)), dL_dimg);
        KCHECK("lg_loss_bwd");
    }
    return LG_OK;
}

// ------------------------------------------------------------------------------------------------
// feature blending over the lists of a forward (lg_features.h)
extern "C" size_t lg_features_scratch_bytes(int32_t N, int64_t num_rendered, int32_t C)
{
    (void)N;
    if (C < 1 || C > LG_FEATURES_MAX || num_rendered < 0) return 0;
    return align_up((size_t)(num_rendered > 0 ? num_rendered : 1) * (size_t)lg_features_chunk(num_rendered, C) * sizeof(float));
}

extern "C" int lg_blend_features(const lg_view* v, int32_t N, const void* geom_p, const void* bin_p, int64_t R, const float* features, int32_t C,
                                 const float* bg_features, float* out, float* alpha, void* stream_p)
{
    int rc = features_args("lg_blend_features", v, N, geom_p, bin_p, R, C);
    if (rc != LG_OK) return rc;
    if (!out || (N > 0 && !features)) return fail(LG_ERR_INVALID_ARGUMENT, "lg_blend_features: missing features / out buffer");
    const auto [stream, debug, prof, exact, s, f] = walk_call(v, N, geom_p, nullptr, bin_p, R, stream_p);
    const ViewGeom& q = s.q;
    for (int c0 = 0, cg; c0 < C; c0 += cg) {
        cg = features_channel_group(C - c0);
        {
            ProfScope ps(prof, "features_fwd", stream);
            features_fwd_kernel(cg, exact)<<<q.ntiles_pad, 256, 0, stream>>>(f, C, c0, features, bg_features, out, alpha);
        }
        KCHECK("lg_features_fwd");
    }
    return LG_OK;
}

// the launches of lg_blend_features_backward (arguments checked by the caller)
static int features_backward_run(const lg_view* v, int32_t N, const void* geom_p, const void* bin_p, int64_t R, const float* dL_dout, int32_t C,
                                 float* dL_dfeatures, void* scratch, void* stream_p)
{
    const auto [stream, debug, prof, exact, s, f] = walk_call(v, N, geom_p, nullptr, bin_p, R, stream_p);
    const ViewGeom& q = s.q; const GeomView& geo = s.geo;
    float* rows = (float*)scratch;        // [R][cw] partial rows of the current chunk of channels, every row written by lg_features_bwd
    const int chunk = lg_features_chunk(R, C);
    for (int cb = 0; cb < C; cb += chunk) {
        const int cw = std::min(chunk, C - cb);
        if (f.live) {
            for (int c0 = cb; c0 < cb + cw;) {
                const int rem = cb + cw - c0, nv = rem <= 4 ? 4 : rem <= 8 ? 8 : 16;
                {
                    ProfScope ps(prof, "features_bwd", stream);
                    features_bwd_kernel(nv, exact)<<<q.ntiles_pad, 256, 0, stream>>>(f, c0, cb + cw, cb, cw, geo.tinfo, dL_dout, rows);
                }
                KCHECK("lg_features_bwd");
                c0 += nv;
            }
        }
        {
            ProfScope ps(prof, "features_gather", stream);
            const size_t n = (size_t)N * cw;
            lg_features_gather<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(N, C, cb, cw, f.live, f.cap, geo.touched, geo.offsets, geo.counters, rows, dL_dfeatures);
        }
        KCHECK("lg_features_gather");
    }
    return LG_OK;
}

extern "C" int lg_blend_features_backward(const lg_view* v, int32_t N, const void* geom_p, const void* bin_p, int64_t R, const float* dL_dout, int32_t C,
                                          float* dL_dfeatures, void* scratch, void* stream_p)
{
    int rc = features_args("lg_blend_features_backward", v, N, geom_p, bin_p, R, C);
    if (rc != LG_OK) return rc;
    if (N == 0) return LG_OK;             // nothing to write
    if (!dL_dout || !dL_dfeatures || !scratch) return fail(LG_ERR_INVALID_ARGUMENT, "lg_blend_features_backward: missing dL_dout / dL_dfeatures / scratch buffer");
    return features_backward_run(v, N, geom_p, bin_p, R, dL_dout, C, dL_dfeatures, scratch, stream_p);
}

// lg_backward with a loss on the feature image and on alpha next to (or instead of) the colour loss: K7 when dL_dcolor is given, the
// geometry walks of lg_features_bwd_geom into the same moment rows, K9 once, then dL_dfeatures as lg_blend_features_backward computes it.
// scratch = the moment rows [R][12] | the partial rows of lg_blend_features_backward.
extern "C" size_t lg_backward_features_scratch_bytes(int32_t N, int64_t num_rendered, int32_t C)
{
    if (C < 1 || C > LG_FEATURES_MAX || num_rendered < 0) return 0;
    return lg_backward_scratch_bytes(N, num_rendered) + lg_features_scratch_bytes(N, num_rendered, C);
}

extern "C" int lg_backward_features(const lg_view* v, const lg_gaussians* g, const int32_t* radii, const void* geom_p, const void* bin_p,
                                    const void* img_p, int64_t R, const float* dL_dcolor, const float* features, int32_t C,
                                    const float* bg_features, const float* dL_dout, const float* dL_dalpha, float* dL_dmeans2D,
                                    float* dL_dmeans3D, float* dL_dshs, float* dL_dcolors, float* dL_dopacity, float* dL_dscales,
                                    float* dL_drotations, float* dL_dcov3D, float* dL_dshs_rest, float* dL_dfeatures, void* scratch,
                                    void* stream_p)
{
    if (!g) return fail(LG_ERR_INVALID_ARGUMENT, "lg_backward_features: null gaussians");
    int rc = features_args("lg_backward_features", v, g->N, geom_p, bin_p, R, C);
    if (rc != LG_OK) return rc;
    if ((rc = features_grad_args("lg_backward_features", g->N, features, dL_dout, dL_dfeatures)) != LG_OK) return rc;
    const FeatGrad fg = { features, C, bg_features, dL_dout, dL_dalpha };
    const GradOut d = { dL_dmeans2D, dL_dmeans3D, dL_dshs, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, dL_dshs_rest };
    rc = backward_impl(v, g, radii, geom_p, bin_p, img_p, R, dL_dcolor, d, scratch, stream_p, { 1, nullptr, nullptr, &fg, nullptr });
    if (rc != LG_OK || g->N == 0 || !dL_dfeatures) return rc;
    return features_backward_run(v, g->N, geom_p, bin_p, R, dL_dout, C, dL_dfeatures, (char*)scratch + lg_backward_scratch_bytes(g->N, R), stream_p);
}

// ---- depth distortion and median depth (lg_distortion.h, include/lightgaussian_distortion.h) ----
extern "C" size_t lg_distortion_state_bytes(int32_t W, int32_t H)
{
    if (W < 1 || H < 1) return 0;
    return distortion_state_head(W, H) + align_up((size_t)W * (size_t)H * sizeof(uint32_t));
}

static int distortion_args(const char* who, const lg_view* v, int32_t N, const void* geom_p, const void* bin_p, int64_t R, int32_t C, const float* m,
                           int32_t m_stride, const void* state)
{
    if (C < 0 || C > LG_FEATURES_MAX) return refuse(who, "C must be 0 .. LG_FEATURES_MAX (64) channels");
    int rc = features_args(who, v, N, geom_p, bin_p, R, C > 0 ? C : 1);
    if (rc != LG_OK) return rc;
    if (m_stride < 1) return refuse(who, "m_stride must be at least 1");
    if (N > 0 && !m) return refuse(who, "missing m");
    if (!state) return refuse(who, "missing state buffer");
    return LG_OK;
}

extern "C" int lg_blend_distortion(const lg_view* v, int32_t N, const void* geom_p, const void* bin_p, int64_t R, const float* m, int32_t m_stride,
                                   float* distortion, float* median, void* state, void* stream_p)
{
    int rc = distortion_args("lg_blend_distortion", v, N, geom_p, bin_p, R, 0, m, m_stride, state);
    if (rc != LG_OK) return rc;
    if (!distortion) return refuse("lg_blend_distortion", "missing distortion map");
    const auto [stream, debug, prof, exact, s, f] = walk_call(v, N, geom_p, nullptr, bin_p, R, stream_p);
    const ViewGeom& q = s.q;
    {
        ProfScope ps(prof, "distortion_fwd", stream);
        distortion_fwd_kernel(exact)<<<q.ntiles_pad, 256, 0, stream>>>(
            f, m, m_stride, distortion, median, (float4*)state, (uint32_t*)((char*)state + distortion_state_head(q.W, q.H)));
    }
    KCHECK("lg_distortion_fwd");
    return LG_OK;
}

// scratch = the moment rows [R][12] | the partial rows of lg_blend_features_backward (C > 0) | the dm rows [R]
static size_t distortion_scratch_features(int32_t N, int64_t R, int32_t C) { return C > 0 ? lg_features_scratch_bytes(N, R, C) : 0; }
extern "C" size_t lg_backward_distortion_scratch_bytes(int32_t N, int64_t num_rendered, int32_t C)
{
    if (C < 0 || C > LG_FEATURES_MAX || num_rendered < 0) return 0;
    return lg_backward_scratch_bytes(N, num_rendered) + distortion_scratch_features(N, num_rendered, C) +
           align_up((size_t)(num_rendered > 0 ? num_rendered : 1) * sizeof(float));
}

extern "C" int lg_backward_distortion(const lg_view* v, const lg_gaussians* g, const int32_t* radii, const void* geom_p, const void* bin_p,
                                      const void* img_p, int64_t R, const float* dL_dcolor, const float* features, int32_t C,
                                      const float* bg_features, const float* dL_dout, const float* dL_dalpha, float* dL_dmeans2D,
                                      float* dL_dmeans3D, float* dL_dshs, float* dL_dcolors, float* dL_dopacity, float* dL_dscales,
                                      float* dL_drotations, float* dL_dcov3D, float* dL_dshs_rest, float* dL_dfeatures, const float* m,
                                      int32_t m_stride, const void* state, const float* dL_ddistortion, const float* dL_dmedian, float* dL_dm,
                                      void* scratch, void* stream_p)
{
    const char* who = "lg_backward_distortion";
    if (!g) return refuse(who, "null gaussians");
    int rc = distortion_args(who, v, g->N, geom_p, bin_p, R, C, m, m_stride, state);
    if (rc != LG_OK) return rc;
    const int N = g->N;
    if ((rc = features_grad_args(who, N, features, dL_dout, dL_dfeatures)) != LG_OK) return rc;
    if (C == 0 && dL_dout) return refuse(who, "dL_dout without channels (C is 0)");
    if (N > 0 && !dL_dm) return refuse(who, "missing dL_dm");
    if (N == 0) return LG_OK;       // nothing to write
    if (!scratch) return refuse(who, "missing scratch buffer");
    char* feat_scratch = (char*)scratch + lg_backward_scratch_bytes(N, R);
    float* dm_rows = (float*)(feat_scratch + distortion_scratch_features(N, R, C));
    const FeatGrad fg = { features, C, bg_features, dL_dout, dL_dalpha };
    const DistGrad dg = { m, m_stride, state, dL_ddistortion, dL_dmedian, dm_rows };
    const GradOut d = { dL_dmeans2D, dL_dmeans3D, dL_dshs, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, dL_dshs_rest };
    rc = backward_impl(v, g, radii, geom_p, bin_p, img_p, R, dL_dcolor, d, scratch, stream_p,
                       { 1, nullptr, nullptr, (dL_dout || dL_dalpha) ? &fg : nullptr, nullptr, &dg });
    if (rc != LG_OK) return rc;
    if (dL_dfeatures) {
        rc = features_backward_run(v, N, geom_p, bin_p, R, dL_dout, C, dL_dfeatures, feat_scratch, stream_p);
        if (rc != LG_OK) return rc;
    }
    const auto [stream, debug, prof, exact, s, f] = walk_call(v, N, geom_p, nullptr, bin_p, R, stream_p);
    // (a segment length other than the forward's: lg_distortion_bwd wrote zero dm rows)
    {
        ProfScope ps(prof, "distortion_gather", stream);
        lg_features_gather<<<(unsigned)(((size_t)N + 255) / 256), 256, 0, stream>>>(N, 1, 0, 1, f.live, f.cap, s.geo.touched, s.geo.offsets, s.geo.counters, dm_rows, dL_dm);
    }
    KCHECK("lg_features_gather");
    return LG_OK;
}

// ---- sensitivity pruning score (lg_sensitivity.h, include/lightgaussian_sensitivity.h) ----
// scratch = the moment rows [num_rendered][12]
extern "C" size_t lg_sensitivity_scratch_bytes(int32_t N, int64_t num_rendered)
{
    (void)N;
    if (num_rendered < 0) return 0;
    return align_up((size_t)(num_rendered > 0 ? num_rendered : 1) * LG_SENS_NV * sizeof(float));
}

extern "C" int lg_sensitivity_accumulate(const lg_view* v, const lg_gaussians* g, const int32_t* radii, const void* geom_p, const void* bin_p,
                                         const void* img_p, int64_t R, double* H, void* scratch, void* stream_p)
{
    const char* who = "lg_sensitivity_accumulate";
    int rc = check_args(v, g);
    if (rc != LG_OK) return rc;
    if (v->flags & LG_FLAG_ANTIALIAS) return refuse(who, "LG_FLAG_ANTIALIAS is not supported (the compensated opacity depends on the covariance)");
    if ((v->flags & (LG_FLAG_SKIP_COLOR | LG_FLAG_SCORE_MAX)) || v->count_sum) return refuse(who, "needs the buffers of a colour forward, not of a count forward");
    if (R < 0 || R >= (1ll << 30)) return refuse(who, "num_rendered out of range");
    if (g->N == 0) return LG_OK;          // nothing to add
    if (!H) return refuse(who, "missing H");
    if (g->cov3D_precomp) return refuse(who, "needs scales and rotations (cov3D_precomp has no scale to differentiate)");
    if (!radii || !geom_p || !img_p || !scratch) return refuse(who, "missing buffer");
    if (R > 0 && !bin_p) return refuse(who, "missing binning buffer");
    const int N = g->N;
    const auto [stream, debug, prof, exact, s, f] = walk_call(v, N, geom_p, img_p, bin_p, R, stream_p);
    if (!f.live) return LG_OK;            // no instances: every H keeps its value
    const ViewGeom& q = s.q; const GeomView& geo = s.geo; const ImgView& img = s.img; const BinView& bin = s.bin;
    float* rows = (float*)scratch;        // [R][12] moment rows, every row written by lg_sensitivity_walk
    {
        ProfScope ps(prof, "sensitivity_walk", stream);
        sensitivity_walk_kernel(exact)<<<q.ntiles_pad, 256, 0, stream>>>(f, (uint32_t)q.S, bin.meta, geo.tinfo, v->bg, img.final_T, img.n_contrib, rows);
    }
    KCHECK("lg_sensitivity_walk");
    {
        ProfScope ps(prof, "sensitivity_accum", stream);
        sensitivity_accum_kernel(v->flags & LG_FLAG_RAW_PARAMS)<<<(unsigned)(((size_t)N + LG_SENS_THREADS - 1) / LG_SENS_THREADS), LG_SENS_THREADS, 0, stream>>>(
            N, q.W, q.H, v->tanfovx, v->tanfovy, v->scale_modifier, (uint32_t)R, v->viewmatrix, v->projmatrix, g->means3D, g->scales, g->rotations, radii,
            geo.rec, geo.counters, bin.meta, (uint32_t)q.S, geo.touched, geo.offsets, reinterpret_cast<const float4*>(rows), H);
    }
    KCHECK("lg_sensitivity_accum");
    return LG_OK;
}

extern "C" int lg_sensitivity_score(int32_t N, const double* H, const float* scales, double* out, void* stream_p)
{
    if (N < 0 || N >= LG_ROWS_MAX) return refuse("lg_sensitivity_score", "N out of range");
    if (N == 0) return LG_OK;
    if (!H || !out) return refuse("lg_sensitivity_score", "missing H / out");
    hipStream_t stream = (hipStream_t)stream_p;
    lg_sensitivity_score_kernel<<<(unsigned)(((size_t)N + LG_SENS_THREADS - 1) / LG_SENS_THREADS), LG_SENS_THREADS, 0, stream>>>(N, H, scales, out);
    KLAUNCHED("lg_sensitivity_score_kernel");
    return LG_OK;
}

// diagnostics: Gaussian id of the last contributor of every pixel (0xFFFFFFFF: none) from the state a forward saved -- the
// implementation-independent form of n_contrib (which is a position in THIS library's culled tile lists)
__global__ void __launch_bounds__(256)
lg_debug_last_contributor_kernel(int W, int H, int gx, const uint2* __restrict__ ranges, const uint64_t* __restrict__ entries, uint32_t gid_mask,
                                 const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ counters, uint32_t* __restrict__ out)
{
    const size_t pid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pid >= (size_t)W * H) return;
    const int x = (int)(pid % (size_t)W), y = (int)(pid / (size_t)W);
    const uint32_t n = counters[0] == 0u ? n_contrib[pid] : 0u;
    out[pid] = n > 0u ? ((uint32_t)entries[ranges[(y / LG_TILE) * gx + x / LG_TILE].x + n - 1u] & gid_mask) : 0xFFFFFFFFu;
}
extern "C" int lg_debug_tile_lists(const lg_view* v, const void* bin_p, int64_t R, uint32_t* out_ranges, uint64_t* out_entries, void* stream_p)
{
    if (!v || !bin_p || !out_ranges || !out_entries || R < 0 || v->image_width <= 0 || v->image_height <= 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_debug_tile_lists: missing buffer");
    const ViewState s = view_state(v, 0, nullptr, nullptr, bin_p, R);
    const ViewGeom& q = s.q; const BinView& bin = s.bin;
    hipError_t e = hipMemcpyAsync(out_ranges, bin.ranges, (size_t)q.ntiles * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream_p);
    if (e == hipSuccess && R > 0) e = hipMemcpyAsync(out_entries, bin.entries, (size_t)R * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream_p);
    if (e != hipSuccess) return fail(LG_ERR_DEVICE, "lg_debug_tile_lists copy", e);
    return LG_OK;
}

extern "C" int lg_debug_view_meta(const lg_view* v, const void* bin_p, int64_t R, uint32_t* out_meta16, void* stream_p)
{
    if (!v || !bin_p || !out_meta16 || R < 0 || v->image_width <= 0 || v->image_height <= 0) return fail(LG_ERR_INVALID_ARGUMENT, "lg_debug_view_meta: missing buffer");
    const BinView bin = view_state(v, 0, nullptr, nullptr, bin_p, R).bin;
    hipError_t e = hipMemcpyAsync(out_meta16, bin.meta, 64, hipMemcpyDeviceToDevice, (hipStream_t)stream_p);
    if (e != hipSuccess) return fail(LG_ERR_DEVICE, "lg_debug_view_meta copy", e);
    return LG_OK;
}

extern "C" int lg_debug_last_contributor(const lg_view* v, int32_t N, const void* geom_p, const void* bin_p, const void* img_p, int64_t R,
                                         uint32_t* out_ids, void* stream_p)
{
    if (!v || N <= 0 || !geom_p || !bin_p || !img_p || !out_ids || v->image_width <= 0 || v->image_height <= 0)
        return fail(LG_ERR_INVALID_ARGUMENT, "lg_debug_last_contributor: missing buffer");
    const ViewState s = view_state(v, N, geom_p, img_p, bin_p, R);
    const ViewGeom& q = s.q; const GeomView& geo = s.geo; const ImgView& img = s.img; const BinView& bin = s.bin;
    const int W = q.W, H = q.H;
    const size_t P = (size_t)W * H;
    lg_debug_last_contributor_kernel<<<(unsigned)((P + 255) / 256), 256, 0, (hipStream_t)stream_p>>>(W, H, q.gx, bin.ranges, bin.entries, q.gid_mask, img.n_contrib,
                                                                                                  geo.counters, out_ids);
    KLAUNCHED("lg_debug_last_contributor");
    return LG_OK;
}

// diagnostics: the K4 radix sort on its own (stand-alone histogram pass + onesweep passes)
extern "C" size_t lg_debug_sort_temp_bytes(int64_t n) { return n < 0 ? 0 : lg_sort_layout((size_t)n).total; }
extern "C" int lg_debug_sort_keys(int64_t n, const uint64_t* keys_in, uint64_t* keys_out, int32_t begin_bit, int32_t end_bit, void* temp,
                                  void* stream_p)
{
    if (n < 0 || n >= (1ll << 30) || begin_bit < 0 || end_bit > 64 || end_bit <= begin_bit) return fail(LG_ERR_INVALID_ARGUMENT, "bad sort arguments");
    if (n == 0) return LG_OK;
    if (!keys_in || !keys_out || !temp) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    const LgSortLayout L = lg_sort_layout((size_t)n);
    size_t tb = L.total;
    HIP_TRY(lg_sort_keys(temp, tb, keys_in, keys_out, (uint32_t)n, begin_bit, end_bit, nullptr, false, (hipStream_t)stream_p));
    uint32_t h_err = 0;
    HIP_TRY(hipMemcpyAsync(&h_err, lg_sort_error_word(temp, (size_t)n), 4, hipMemcpyDeviceToHost, (hipStream_t)stream_p));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_p));
    if (h_err & LG_ABORT_SORT) return fail(LG_ERR_DEVICE, "radix sort look-back gave up (a predecessor tile never published)");
    return LG_OK;
}

// diagnostics: the failure path of the look-back.  One digit pass is launched with its ticket counter preset to 1, so the tile
// that runs has a predecessor (tile 0) that does not exist and never publishes; with a small poll budget the look-back must give
// up, set the error word and return -- LG_ERR_DEVICE here -- instead of hanging the device or passing a wrong order on silently.
extern "C" int lg_debug_sort_orphan(int64_t n, const uint64_t* keys_in, uint64_t* keys_out, void* temp, void* stream_p)
{
    if (n <= 0 || n > LG_SORT_TILE) return fail(LG_ERR_INVALID_ARGUMENT, "lg_debug_sort_orphan: 1 <= n <= one sort tile");
    if (!keys_in || !keys_out || !temp) return fail(LG_ERR_INVALID_ARGUMENT, "missing buffer");
    hipStream_t stream = (hipStream_t)stream_p;
    const LgSortLayout L = lg_sort_layout((size_t)2 * LG_SORT_TILE);
    char* base = (char*)temp;
    HIP_TRY(lg_zero_async(base, lg_sort_clear_bytes(L, 1), stream));
    const uint32_t one = 1u;
    HIP_TRY(hipMemcpyAsync(base + L.ticket_off, &one, 4, hipMemcpyHostToDevice, stream));
    uint32_t* tickets = (uint32_t*)(base + L.ticket_off);
    uint32_t* err = lg_sort_error_word(temp, (size_t)2 * LG_SORT_TILE);
    // n_arg = one tile beyond the orphan so that tile 1 is inside the key range; it sorts keys_in[0..n) as its own keys
    lg_onesweep_pass<<<1, LG_SORT_BLOCK, 0, stream>>>(keys_in - LG_SORT_TILE, keys_out - LG_SORT_TILE, nullptr, (uint32_t)(LG_SORT_TILE + n), 0, 8,
                                                       (uint32_t*)(base + L.hist_off), tickets, (uint32_t*)(base + L.state_off), err, 64u, nullptr, 0);
    KLAUNCHED("lg_onesweep_pass");
    uint32_t h_err = 0;
    HIP_TRY(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h_err & LG_ABORT_SORT) return fail(LG_ERR_DEVICE, "radix sort look-back gave up (a predecessor tile never published)");
    return LG_OK;
}

// The four status words of a view as they stand when `stream` reaches this call: { abort flags, prefiltered violation,
// largest depth bit pattern, instance count }.  One blocking 16-byte read.  abort bit 2 (LG_ABORT_SORT) can only be set
// after the words lg_forward_bounded hands out were written, so a caller that must know reads them here.
extern "C" int lg_view_status(const void* geom, int32_t N, uint32_t* out4, void* stream_p)
{
    if (!geom || !out4 || N < 0) return fail(LG_ERR_INVALID_ARGUMENT, "lg_view_status: missing buffer");
    GeomView geo = carve_geom(const_cast<void*>(geom), N);
    hipStream_t stream = (hipStream_t)stream_p;
    HIP_TRY(hipMemcpyAsync(out4, geo.counters, 16, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (out4[0] & LG_ABORT_SORT) return fail(LG_ERR_DEVICE, "radix sort look-back gave up (a predecessor tile never published): the view is void");
    return LG_OK;
}

// diagnostics: the activations of the fused-getter path (K1 / K9, RAW) on their own, in several candidate operation orders,
// to be compared bit for bit with torch.exp / F.normalize / torch.sigmoid (tools/activation_probe.py)
__global__ void lg_debug_activations_kernel(int n, const float* __restrict__ s, const float* __restrict__ r, const float* __restrict__ o,
                                            float* __restrict__ out_s, float* __restrict__ out_r, float* __restrict__ out_o)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_s[i] = expf(s[i]);
    out_o[i] = lg_sigmoid(o[i]);
    out_o[n + i] = 1.0f / (1.0f + __expf(-o[i]));
    const float a = r[4 * i], b = r[4 * i + 1], c = r[4 * i + 2], d = r[4 * i + 3];
    const float n0 = fmaxf(sqrtf(((a * a + b * b) + c * c) + d * d), 1e-12f);
    const float n1 = fmaxf(sqrtf((a * a + b * b) + (c * c + d * d)), 1e-12f);
    const float n2 = fmaxf(sqrtf(fmaf(d, d, fmaf(c, c, fmaf(b, b, a * a)))), 1e-12f);
    const float n3 = fmaxf(sqrtf((a * a + c * c) + (b * b + d * d)), 1e-12f);
    const float nn[4] = {n0, n1, n2, n3};
    for (int v = 0; v < 4; v++) {
        out_r[(size_t)v * 4 * n + 4 * i] = a / nn[v]; out_r[(size_t)v * 4 * n + 4 * i + 1] = b / nn[v];
        out_r[(size_t)v * 4 * n + 4 * i + 2] = c / nn[v]; out_r[(size_t)v * 4 * n + 4 * i + 3] = d / nn[v];
    }
}
extern "C" int lg_debug_activations(int32_t n, const float* s, const float* r, const float* o, float* out_s, float* out_r, float* out_o, void* stream_p)
{
    if (n <= 0) return LG_OK;
    lg_debug_activations_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream_p>>>(n, s, r, o, out_s, out_r, out_o);
    KLAUNCHED("lg_debug_activations");
    return LG_OK;
}

extern "C" int lg_debug_reduce9(const float* in_64x9, float* out_9, void* stream_p)
{
    lg_debug_reduce9_kernel<<<1, 64, 0, (hipStream_t)stream_p>>>(in_64x9, out_9);
    KLAUNCHED("lg_debug_reduce9");
    return LG_OK;
}

#ifndef LG_BUILD_ID
#define LG_BUILD_ID "unknown"
#endif
extern "C" const char* lg_build_id(void) { return LG_BUILD_ID; }
extern "C" int lg_abi_version(void) { return LG_ABI_VERSION; }
extern "C" const char* lg_last_error(void) { return g_err.c_str(); }
extern "C" int lg_last_stats(lg_stats* out)
{
    if (!out) return LG_ERR_INVALID_ARGUMENT;
    *out = g_stats;
    return LG_OK;
}

extern "C" void lg_profile_reset(void)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& p : g_prof)
        for (auto& ev : p.pending) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    g_prof.clear();
}

extern "C" int lg_profile_read(lg_kernel_time* out, int cap)
{
    int n = 0;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& p : g_prof) {
        for (auto& ev : p.pending) {
            float ms = 0.0f;
            if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
                p.ms += ms; p.n += 1;
            }
            (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second);
        }
        p.pending.clear();
        if (out && n < cap) {
            memset(&out[n], 0, sizeof(lg_kernel_time));
            strncpy(out[n].name, p.name.c_str(), sizeof(out[n].name) - 1);
            out[n].total_ms = p.ms; out[n].launches = p.n;
        }
        n++;
    }
    return n;
}

