/*
 * lightgaussian.h -- C ABI of the MI355X-native LightGaussian rasterizer (liblightgaussian_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of VITA-Group/LightGaussian: the differentiable
 * tile rasterizer + per-Gaussian Global-Significance accumulation + its backward.  In the
 * reference that path lives in the un-vendored CUDA extension
 *     submodules/compress-diff-gaussian-rasterization            (/root/reference/.gitmodules:6-8)
 * and is reached only through
 *     gaussian_renderer/__init__.py:14-17   (import of GaussianRasterizationSettings / GaussianRasterizer)
 *     gaussian_renderer/__init__.py:52-68   (settings record, 13 fields)
 *     gaussian_renderer/__init__.py:106-115 (render call, returns color, radii)
 *     gaussian_renderer/__init__.py:209-218 (count call, returns count, score, color, radii)
 * The published extension exposes three torch-typed entry points behind that Python API
 * (rasterize_gaussians / count_gaussians / rasterize_gaussians_backward).  The entry points below
 * are what a binding of that path binds instead: plain device pointers, sizes and a stream --
 * no torch types.  INTEGRATION.md shows the ctypes stub.
 * Beyond the reference's three: feature / depth / alpha maps over a view's tile lists (lg_blend_features, lg_backward_features) and the
 * gradient with respect to the camera itself (lg_backward_camera: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos), which the reference's
 * backward treats as a constant.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory owned by the caller, fp32 contiguous unless noted
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it
 *   - functions return LG_OK or a negative error code; lg_last_error() gives the message
 *   - the library keeps no state between calls that can change a result (re-entrant per stream): everything a view depends
 *     on travels in lg_view / lg_gaussians and in the caller's buffers.  What it does keep is bookkeeping only: the
 *     thread-local text of lg_last_error() / lg_last_stats(), a pool of pinned 64-byte read-back slots, and the optional
 *     LG_FLAG_PROFILE event list
 */
#ifndef LIGHTGAUSSIAN_H
#define LIGHTGAUSSIAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 7 (round 6): lg_view.count_sum (running hit count fused into the score kernel); the ALPHA / ALPHA_T weight policies are exact
 *    64-bit fixed-point sums (Q24.40; out_score bit-reproducible, out_count / out_score written by lg_score_slots) instead of
 *    float atomics; images beyond 2^24 pixels are refused for them.  LG_FLAG_BWD_SPLAT_PARALLEL (prototype kernel) removed.
 * 6 (round 5): geom buffer layout of round 4 ([N][9] SH direction Jacobian, counters[9]), LG_FLAG_SAVE_SH_JACOBIAN as part of the
 *    forward / backward contract, lg_debug_* moved to lightgaussian_debug.h (all three shipped under 5 -- ADVICE r4), plus this
 *    round's additions: lg_backward's rgb_only mode, lg_sh_grad_from_rgb, LG_FLAG_BWD_SPLAT_PARALLEL.
 * 5 (round 3): stateless library -- segment length and long-tile mode travel in lg_view. */
#define LG_ABI_VERSION 7

enum {
    LG_OK = 0,
    LG_ERR_INVALID_ARGUMENT = -1, /* bad sizes / exclusive inputs violated (reference: Python Exception before launch) */
    LG_ERR_DEVICE = -2,           /* HIP error (reference: std::runtime_error -> RuntimeError) */
    LG_ERR_ALLOC = -3,            /* binning allocator callback returned NULL */
    LG_ERR_PREFILTERED = -4       /* prefiltered=1 but a Gaussian failed the frustum test */
};

/* per-hit weight of the significance score; OPACITY is LightGaussian's GS_j = sum 1(hit) * sigma_j */
enum { LG_WEIGHT_ONE = 0, LG_WEIGHT_OPACITY = 1, LG_WEIGHT_ALPHA = 2, LG_WEIGHT_ALPHA_T = 3 };

/* flags */
enum {
    LG_FLAG_DEBUG = 1,     /* sync + check after every kernel (reference: raster_settings.debug, gaussian_renderer/__init__.py:64) */
    LG_FLAG_FAST_EXP = 2,  /* hardware exp/rcp in the blend kernels (training renders): image/gradients agree with the
                              canonical path to ~1e-6, far inside the 1e-4 contract; never used for count renders,
                              whose integer outputs are bit-pinned */
    LG_FLAG_PROFILE = 4,   /* record per-kernel hipEvent timings, read back with lg_profile_read() */
    LG_FLAG_SKIP_COLOR = 16, /* significance-only forward (lg_forward_count): K1 does not read the SH rows and the blend kernel
                              neither accumulates colour nor writes out_color / the per-pixel state (their contents are
                              undefined); counts, scores and radii are unaffected.  Used by the sharded prune pass. */
    LG_FLAG_L1_ONLY = 32,  /* lg_loss_forward / lg_loss_backward only: mean |img - gt| without the SSIM work (out[1] = 0);
                              forward and backward must agree */
    /* cross-check switches (never needed in production): */
    LG_FLAG_NARROW_KEY = 64,     /* lay the sort key out as if only 40 bits were available (exercises the beyond-64-bit layout on small scenes) */
    LG_FLAG_SORT_ALL_BITS = 128, /* one-stage sort: every stored key bit through the global radix passes (the round-2 scheme) instead of the
                                    default two stages -- radix passes on the tile bits, then each list ordered by depth inside LDS.  Same lists. */
    LG_FLAG_K1_LDS = 256,        /* K1 stages SH rows through LDS instead of per-lane reads */
    LG_FLAG_LONG_SERIAL = 512,   /* long per-tile lists of the hardware-exp colour forward: walk every list serially inside the blend kernel */
    LG_FLAG_LONG_PARALLEL = 1024, /* ... walk the segments of EVERY multi-segment list in parallel (lg_blend_fwd_seg, which also scans, / lg_blend_fwd_rewalk).
                              Neither flag (default): only lists longer than two segments and four times the view's mean list --
                              decided on the device from this view's own instance count, so the choice never depends on what the
                              process rendered before.  Images of the parallel walk agree with the serial one to float rounding
                              (regrouped transmittance products), n_contrib exactly.  Canonical colour forwards, count forwards that return an
                              image and the float weight policies always walk serially; the significance-only count pass (LG_FLAG_SKIP_COLOR,
                              integer weights) has a parallel walk of its own since round 5 (lg_count_seg / _rewalk / _fixup), taken ONLY when
                              LG_FLAG_LONG_PARALLEL is set (measured slower than the serial walk with several views in flight, which is how
                              the pass runs by default); its counts are bit-identical to the serial walk's.
                              No counterpart in the reference (its renderCUDA walks every list serially). */
    LG_FLAG_SAVE_SH_JACOBIAN = 2048, /* forward: this view will be differentiated -- K1 leaves d rgb / d (view direction) of every visible
                                        Gaussian (36 bytes) in the geom buffer, and lg_backward (which finds a marker word there) does not read
                                        the SH coefficients again: 388 MB less per view at 3 M Gaussians.  Without the flag the backward
                                        works as before.  No effect on any result (same operations in the same order). */
    LG_FLAG_COUNT_WIDE_BAND = 8192, /* tests only: the parallel long-tile walk of the significance-only pass compares regrouped transmittances with
                                       the 1e-4 threshold through an error band; this widens the band 4096 x, sending a fifth of the saturating pixels
                                       through the exact fix-up pass instead of a handful per view.  Counts must not change. */
    LG_FLAG_ANTIALIAS = 16384, /* opacity compensation of the fixed 0.3-pixel screen-space blur (Mip-Splatting's 2D filter, the `antialiasing`
                                  switch of upstream 3DGS): with S the 2D covariance of a splat before the blur, K1 scales its opacity by
                                  rho = sqrt(max(0.000025, det S / det(S + 0.3 I))) -- in the blend record and in the alpha >= 1/255 footprint
                                  cull; radii and the reference tile rectangles do not change -- and K9 / lg_camera_bwd carry the gradient
                                  through rho to the opacity, the covariance, the mean and the camera.  Honoured by lg_forward,
                                  lg_forward_count, lg_forward_bounded, lg_backward, lg_backward_chunked, lg_backward_features and
                                  lg_backward_camera; ignored by everything else (lg_blend_features and its backward read the records the
                                  forward left).  The forward of a view and EVERY backward of that view must carry the same value: a backward
                                  that disagrees differentiates another function than the one rendered (nothing detects it).  The
                                  LG_WEIGHT_OPACITY score keeps the raw opacity (a property of the model, not of the view); hit counts and
                                  the per-hit weights follow the compensated alpha.  Without the flag every kernel launched is unchanged. */
    LG_FLAG_ABSGRAD = 32768,   /* this view's backward is lg_backward_abs, which also leaves the ABSOLUTE screen-space mean gradients (AbsGS's
                                  homodirectional gradient, gsplat's `absgrad`).  Read by lg_backward_abs alone, which refuses a view without it;
                                  every forward and every other backward ignores it: without lg_backward_abs every kernel launched and every
                                  bit produced is unchanged. */
    /* (65536 is LG_FLAG_SCORE_MAX, a flag of the count forwards declared in the extension header lightgaussian_score.h: the bit is taken) */
    /* (4096 was LG_FLAG_BWD_SPLAT_PARALLEL, the round-5 prototype of the backward blend on the other parallel axis: removed in ABI 7) */
    LG_FLAG_RAW_PARAMS = 8 /* "fused getters" (SURVEY 8f row 1): the inputs are GaussianModel's RAW parameters and the
                              activations of scene/gaussian_model.py:98-118 run inside the kernels: scales = log-scales (exp),
                              rotations = unnormalised quaternions (normalize), opacities = logits (sigmoid), shs = _features_dc
                              [N,1,3] with shs_rest = _features_rest [N,M-1,3] (no torch.cat).  Gradients are w.r.t. the raw tensors. */
};

/* GaussianRasterizationSettings (gaussian_renderer/__init__.py:52-66), minus f_count which selects the entry point */
typedef struct lg_view {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    const float* bg;         /* [3] */
    float scale_modifier;
    const float* viewmatrix; /* [4,4] world_view_transform (row-vector convention, scene/cameras.py:70-72) */
    const float* projmatrix; /* [4,4] full_proj_transform (scene/cameras.py:80-84) */
    int32_t sh_degree;       /* active degree D; the coefficient count M is in lg_gaussians */
    const float* campos;     /* [3] */
    int32_t prefiltered;
    uint32_t flags;          /* LG_FLAG_* */
    int32_t segment_length;  /* per-tile lists longer than this many entries are processed by the backward as independent segments,
                                from checkpoints the forward leaves (long-tile robustness).  0 = default (512); otherwise a
                                multiple of 64 (small values exist for tests).  The SAME lg_view must be handed to lg_forward* and
                                to the lg_backward of that view, and to lg_binning_bytes: the forward records the value in the
                                binning buffer and a backward called with another one writes zero gradients (LG_FLAG_DEBUG: error). */
    int32_t* count_sum;      /* lg_forward_count / lg_forward_bounded with count outputs, optional (NULL: off): a running per-Gaussian hit
                                count [N] int32 to which this view's out_count is ADDED by the kernel that writes out_score -- the
                                `gaussian_list += gaussians_count` of prune_list (prune.py:144-155) without a launch of its own.  Plain
                                read-modify-write, not atomic: one view at a time per accumulator (views in flight on several streams
                                use one accumulator per stream).  Ignored by lg_forward and lg_backward. */
} lg_view;

/* the 8 tensor kwargs of GaussianRasterizer.forward (gaussian_renderer/__init__.py:106-115); means2D is gradient-only */
typedef struct lg_gaussians {
    int32_t N;                   /* number of Gaussians */
    int32_t M;                   /* SH coefficients per channel in `shs` (1,4,9,16); 0 when colors_precomp is used */
    const float* means3D;        /* [N,3] */
    const float* shs;            /* [N,M,3] or NULL */
    const float* colors_precomp; /* [N,3]   or NULL   (exactly one of shs / colors_precomp) */
    const float* opacities;      /* [N,1] */
    const float* scales;         /* [N,3]   or NULL */
    const float* rotations;      /* [N,4]   or NULL   (r,x,y,z) */
    const float* cov3D_precomp;  /* [N,6]   or NULL   (exactly one of scales+rotations / cov3D_precomp) */
    const float* shs_rest;       /* [N,M-1,3] or NULL; only with LG_FLAG_RAW_PARAMS (then shs is [N,1,3]) */
} lg_gaussians;

/* Scratch sizing.  geom: per-Gaussian projected state; img: per-pixel state; binning: (tile,Gaussian)
 * instance lists for `num_rendered` instances; backward scratch: one 48-byte gradient row per instance. */
size_t lg_geom_bytes(int32_t N);
size_t lg_img_bytes(int32_t width, int32_t height);
size_t lg_binning_bytes(int64_t num_rendered, int32_t width, int32_t height, int32_t segment_length /* lg_view.segment_length */);
size_t lg_backward_scratch_bytes(int32_t N, int64_t num_rendered);

/* Called once per forward, after the instance count is known, to obtain the binning buffer
 * (same role as the resize-callbacks of the published extension). Must return a device pointer
 * valid on `stream` with at least `bytes` bytes, or NULL. */
typedef void* (*lg_alloc_fn)(void* user, size_t bytes);

/*
 * Forward render  (replaces rasterize_gaussians; Python call site gaussian_renderer/__init__.py:106-115).
 *   out_color [3,H,W]   out_radii [N] int32 (>0 <=> rasterised)
 *   geom / img: caller scratch of lg_geom_bytes / lg_img_bytes (kept for backward)
 *   *binning_out / *num_rendered: the buffer returned by `alloc` and the instance count (kept for backward)
 * One blocking device->host read of the instance count happens inside (as in the reference extension).
 */
int lg_forward(const lg_view* view, const lg_gaussians* g, void* geom, void* img, lg_alloc_fn alloc, void* alloc_user,
               float* out_color, int32_t* out_radii, void** binning_out, int64_t* num_rendered, void* stream);

/*
 * Forward render + Global Significance accumulation  (replaces count_gaussians; call site
 * gaussian_renderer/__init__.py:209-218 with f_count=True).
 *   out_count [N] int32: number of pixels each Gaussian contributed to
 *   out_score [N] fp32 : per-view significance; for ONE/OPACITY weights it is bit-identical to
 *                        out_count[j] sequential float additions of the weight (what per-hit
 *                        atomicAdd produces), computed from the exact integer count.
 */
int lg_forward_count(const lg_view* view, const lg_gaussians* g, void* geom, void* img, lg_alloc_fn alloc, void* alloc_user,
                     int32_t weight_policy, float* out_color, int32_t* out_radii, int32_t* out_count, float* out_score,
                     void** binning_out, int64_t* num_rendered, void* stream);

/*
 * Capacity-bounded forward: the same render (plain when out_count/out_score are NULL, else + significance) WITHOUT the
 * blocking device->host read of the instance count that lg_forward -- like the reference extension, whose Python side
 * sizes its binning buffer from num_rendered (SURVEY 8b "one blocking D->H read of R per forward") -- performs.  The
 * caller supplies the binning buffer for up to `max_rendered` instances (lg_binning_bytes(max_rendered, W, H, S); e.g.
 * 1.25x the previous view's count) and an upper bound `max_depth` of the view-space depth (the camera's zfar), which fixes
 * the key layout on the host.  Nothing is read back and every launch is stream-ordered, so a view's forward + backward can
 * be issued from one host thread onto several streams, or captured into a hipGraph.
 *   status: device uint32[4], written on `stream` = { abort flags, prefiltered violation, largest depth bit pattern,
 *           instance count R }.  abort bit 0: R > max_rendered; bit 1: a depth beyond max_depth; bit 2 (added to `status` by a
 *           later kernel if it ever happens; `host_status` has left for the host by then -- see lg_view_status): the radix
 *           sort's look-back gave up.  When status[0] != 0 the
 *           view was abandoned on the device (every later kernel returns at once; outputs undefined, gradients of a
 *           following lg_backward are zero) and the caller re-runs it through lg_forward -- the only host decision left.
 *   host_status: NULL, or HOST uint32[4] receiving the same four words before the call returns ("validated" mode; `status`
 *           is not written then).  The scan kernel writes them straight into pinned host memory of the library (no copy node)
 *           and the call waits for them only after the rest of the view is enqueued: the host learns R and the abort flags
 *           synchronously -- a wrapper can fall back to
 *           lg_forward at once and stay a safe drop-in -- while the device goes straight from the scan into the sort and
 *           the blend (the exact forward leaves it idle for the host's wake-up + allocation + launches, ~70 us per view).
 * Backward: lg_backward(..., binning, num_rendered = max_rendered, ...) with scratch lg_backward_scratch_bytes(N, max_rendered).
 */
int lg_forward_bounded(const lg_view* view, const lg_gaussians* g, void* geom, void* img, void* binning, int64_t max_rendered,
                       float max_depth, int32_t weight_policy, float* out_color, int32_t* out_radii, int32_t* out_count,
                       float* out_score, uint32_t* status, uint32_t* host_status, void* stream);

/*
 * Backward  (replaces rasterize_gaussians_backward).  dL_dcolor [3,H,W] -> dense gradients, zero for
 * Gaussians that were not rasterised.  Output pointers may be NULL when the matching input was NULL.
 *   dL_dmeans2D [N,3] (NDC units, z = 0; consumed by scene/gaussian_model.py:784-788)
 *   dL_dmeans3D [N,3]  dL_dshs [N,M,3]  dL_dcolors [N,3]  dL_dopacity [N,1]
 *   dL_dscales [N,3]   dL_drotations [N,4]  dL_dcov3D [N,6]  dL_dshs_rest [N,M-1,3] (RAW_PARAMS only, else NULL)
 *   scratch: lg_backward_scratch_bytes(N, num_rendered)
 * geom / img are read-only here; inside `binning` lg_backward fills one reserved array (the dispatch order of its
 * per-tile kernel) -- idempotent, so retain_graph-style repeated backward calls on the same saved state are fine.
 */
int lg_backward(const lg_view* view, const lg_gaussians* g, const int32_t* radii, const void* geom, const void* binning,
                const void* img, int64_t num_rendered, const float* dL_dcolor, float* dL_dmeans2D, float* dL_dmeans3D,
                float* dL_dshs, float* dL_dcolors, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                float* dL_dcov3D, float* dL_dshs_rest, void* scratch, void* stream);

/* SH inputs with dL_dshs == NULL and dL_dcolors != NULL ("rgb_only", round 5): lg_backward writes dL/d(rgb) per Gaussian [N,3] -- the
 * gradient of the colour the SH expansion produced, clamped channels zeroed -- to dL_dcolors INSTEAD of the coefficient gradients
 * (dL_dshs_rest must be NULL too); dL_dmeans3D still contains the view-direction term.  The coefficient gradient of one view is the
 * outer product basis(dir) x dRGB; lg_sh_grad_from_rgb rebuilds it (bit for bit what lg_backward would have written), for V views at
 * once, summed in view order and divided by `divisor`:
 *     dL_dshs[i][k][c] = ( [accumulate: the value already there +] sum_v basis_k(normalize(means3D[i] - campos[v])) * drgb[v][i][c] ) / divisor
 * (accumulate != 0 continues a running sum over several calls -- a camera batch per rank; pass divisor 1 until the last call)
 * A data-parallel trainer exchanges 12 bytes per Gaussian and view (all-gather of dRGB + the camera centres) instead of all-reducing
 * 12 M bytes (192 at degree 3), and every rank ends with identical bits (lightgaussian_amd.parallel.SHGradExchange).  The reference's
 * trainers run one process per GPU with no gradient exchange at all (scripts/run_prune_finetune.sh:58-96); its extension has no counterpart.
 *   drgb: V blocks of [N,3] floats, `view_stride` floats apart; campos [V][3]; dL_dshs [N,M,3], or with dL_dshs_rest != NULL the
 *   GaussianModel split: dL_dshs = _features_dc gradient [N,1,3], dL_dshs_rest = _features_rest gradient [N,M-1,3]. */
int lg_sh_grad_from_rgb(int32_t N, int32_t M, int32_t sh_degree, int32_t V, const float* means3D, const float* campos,
                        const float* drgb, int64_t view_stride, float divisor, int32_t accumulate, float* dL_dshs, float* dL_dshs_rest,
                        void* stream);

/* lg_backward with the per-Gaussian stage (K9) split into `chunks` launches over consecutive Gaussian ranges.  on_chunk(user,
 * first, count) is called on the HOST right after the launch covering Gaussians [first, first + count) has been enqueued: from
 * that point of `stream` on, rows [first, first + count) of every gradient tensor are final.  A data-parallel trainer
 * records an event there and all-reduces those rows on a side stream while K9 computes the next range (SURVEY 8f row 3:
 * gradient all-reduce overlapped with K7-K9; lightgaussian_amd.parallel.OverlappedGradAllReduce).  The reference's
 * distill_train.py:124-166 has no such hook -- its extension returns all gradients at once. */
typedef void (*lg_chunk_fn)(void* user, int32_t first, int32_t count);
int lg_backward_chunked(const lg_view* view, const lg_gaussians* g, const int32_t* radii, const void* geom, const void* binning,
                        const void* img, int64_t num_rendered, const float* dL_dcolor, float* dL_dmeans2D, float* dL_dmeans3D,
                        float* dL_dshs, float* dL_dcolors, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                        float* dL_dcov3D, float* dL_dshs_rest, void* scratch, void* stream, int32_t chunks, lg_chunk_fn on_chunk,
                        void* user);

/* lg_backward_chunked that ALSO writes dL_dmeans2D_abs [N,3]: per Gaussian the sum over pixels of |dL/dmean2D| instead of the |sum|
 * that dL_dmeans2D holds -- signed per-pixel pulls on a large splat straddling fine structure cancel in the latter and it is never
 * densified (AbsGS; gsplat's `absgrad`).  With t = G dL/dalpha and dx = x_g - px of a (pixel, Gaussian) pair and the splat's conic
 * (ha, nb, hc) = (-A/2, -B, -C/2) and record opacity op (the compensated one under LG_FLAG_ANTIALIAS):
 *     abs.x = 0.5 W op sum_pairs |t (2 ha dx + nb dy)|     abs.y = 0.5 H op sum_pairs |t (2 hc dy + nb dx)|     abs.z = 0
 * in the NDC units of dL_dmeans2D, so abs >= |dL_dmeans2D| component-wise up to rounding.  The per-pair magnitudes exist only inside the
 * backward blend: its ABS variant carries them in floats 9 and 10 of the 48-byte gradient rows (zeros otherwise), and one more
 * kernel (lg_absgrad_rows) sums them per Gaussian in slot order between the blend and the first chunk of the per-Gaussian stage:
 * deterministic, no atomics.  Scratch size and every other output are those of lg_backward_chunked, bit for bit.  Rows of Gaussians with
 * radii <= 0, and all rows after an abandoned forward or with a segment_length other than the forward's, are exact zeros.
 * The view must carry LG_FLAG_ABSGRAD and dL_dcolor and dL_dmeans2D_abs must not be NULL (also for N = 0): LG_ERR_INVALID_ARGUMENT otherwise.
 * lg_backward_camera may follow on the same scratch (it reads floats 0..8 of the rows).  lg_backward_features has no such variant.
 * LG_FLAG_PROFILE adds an "absgrad_rows" entry. */
int lg_backward_abs(const lg_view* view, const lg_gaussians* g, const int32_t* radii, const void* geom, const void* binning,
                    const void* img, int64_t num_rendered, const float* dL_dcolor, float* dL_dmeans2D, float* dL_dmeans3D,
                    float* dL_dshs, float* dL_dcolors, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                    float* dL_dcov3D, float* dL_dshs_rest, void* scratch, void* stream, int32_t chunks, lg_chunk_fn on_chunk,
                    void* user, float* dL_dmeans2D_abs /* [N,3], z = 0 */);

/* score[j] = seqsum32(weight[j], count[j]) on the device (weight NULL => 1.0).  Used by the sharded
 * prune pass to rebuild per-view scores from integer counts. */
int lg_score_from_count(int32_t N, const int32_t* count, const float* weight, float* score, void* stream);

/* --- prune epilogue -------------------------------------------------------------
 * Replaces prune.py:112-128 calculate_v_imp_score() followed by the mask of scene/gaussian_model.py:776-782
 * prune_gaussians(), entirely on the device (two radix selects instead of two sorts + host indexing; no synchronisation):
 *   volume = (s0*s1)*s2 of the ACTIVATED scaling [N,3]; kth = element int(N*0.9) of its DESCENDING sort;
 *   v_list[i] = powf(volume[i] / kth, v_pow) * imp_list[i];
 *   thr = element int(prune_percent*(N-1)) of v_list's ASCENDING sort;  mask[i] = v_list[i] <= thr  (ties pruned).
 * v_list [N] float, mask [N] uint8 (1 = prune), thresholds: device float[2] = {kth, thr};
 * scratch: lg_prune_scratch_bytes(N) device bytes.  N == 0 is an error (the reference raises IndexError). */
size_t lg_prune_scratch_bytes(int32_t N);
int lg_prune_epilogue(int32_t N, const float* scaling, const float* imp_list, float v_pow, double prune_percent,
                      float* v_list, uint8_t* mask, float* thresholds, void* scratch, uint32_t flags, void* stream);

/* One radix select: out_value[0] = the rank-th smallest (0-based) of values[0..N) -- exactly the element a sort puts at that
 * index -- and, when mask != NULL, mask[i] = values[i] <= out_value (uint8).  The two order statistics of the epilogue
 * above, usable around the reference's own torch.pow so that v_list and the mask stay bit-identical to prune.py:112-128 /
 * scene/gaussian_model.py:776-782 (lightgaussian_amd.prune.prune_epilogue).  scratch: lg_prune_scratch_bytes(N). */
int lg_select_mask(int32_t N, const float* values, int64_t rank, uint8_t* mask, float* out_value, void* scratch, void* stream);

/* --- compaction after a prune --------------------------------------------------
 * Replaces the tensor surgery of GaussianModel.prune_points / _prune_optimizer (scene/gaussian_model.py:564-600): every
 * parameter, both Adam moments of every parameter and the three bookkeeping tensors are indexed with the keep-mask there
 * (21 boolean-index kernels, each with a nonzero() + host sync).  lg_compact_plan: dest[i] = row of i among the kept rows
 * (order preserved) or -1, *count = number kept (device int32; the ONE value the host reads to size the outputs).
 * lg_compact_rows: moves the rows of up to 32 tensors in one launch; src/dst/row_bytes are HOST arrays of num_tensors device
 * pointers / row sizes in bytes (multiples of 4); dst[t] holds >= *count rows.  Result == tensor[keep] bit for bit.
 * keep: uint8 [N] (1 = keep).  scratch: lg_compact_scratch_bytes(N). */
size_t lg_compact_scratch_bytes(int32_t N);
int lg_compact_plan(int32_t N, const uint8_t* keep, int32_t* dest, int32_t* count, void* scratch, void* stream);
int lg_compact_rows(int32_t N, const int32_t* dest, int32_t num_tensors, const void* const* src, void* const* dst,
                    const int32_t* row_bytes, void* stream);

/* --- VecTree nearest-code search (second half) ----------------------------------
 * Replaces vectree/vq.py:262-266 (EuclideanCodebook.forward: dist = -torch.cdist(flatten, embed, p=2); embed_ind =
 * dist.argmax(-1)) as driven by vectree/vectree.py:87-101: out_index[i] = argmin_c |x[i] - codebook[c]|^2, ties to the lowest
 * c.  x [n,d], codebook [K,d] fp32 device (d <= 63: 27 / 48 in the reference, K = 8192), out_index [n] int32.
 * f32 MFMA (v_mfma_f32_32x32x2_f32, exact f32) on |c|^2 - 2 x.c with a fused per-point argmin; scratch:
 * lg_vq_scratch_bytes(K, d) (the augmented codebook, rebuilt by every call). */
size_t lg_vq_scratch_bytes(int32_t K, int32_t d);
int lg_vq_nearest(int32_t n, int32_t d, int32_t K, const float* x, const float* codebook, int32_t* out_index, void* scratch,
                  uint32_t flags, void* stream);

/* --- VecTree codebook training step ----------------------------------------------------------------
 * One iteration of the importance-weighted EMA k-means of vectree/vq.py:262-299 (EuclideanCodebook.forward in training mode,
 * temperature 0, no DDP, threshold_ema_dead_code 0), as vectree/vectree.py:196-204 drives it (n = 80 000 sampled rows, K = 8192,
 * d = 27 / 48).  With w = weight * n / sum(weight) (all ones when weight is NULL):
 *     out_index[i] = argmin_c |x[i] - embed[c]|^2 on the codebook as handed in (lg_vq_nearest, ties to the lowest c)
 *     size[c] = sum of w[i], esum[c] = sum of w[i] * x[i] over the rows with out_index[i] == c
 *     cluster_size <- decay * cluster_size + (1 - decay) * size
 *     smoothed = (cluster_size + eps) / (sum(cluster_size) + K * eps) * sum(cluster_size)          (the updated cluster_size)
 *     embed <- decay * embed + (1 - decay) * esum / smoothed[:, None]                              (a code without rows decays)
 * x [n,d], weight [n] or NULL, embed [K,d] in/out, cluster_size [K] in/out: fp32 device; out_index [n] int32.
 * No n x K intermediate and no float atomics: the rows of every code are listed in ascending row order (stable radix sort of
 * (code, row) on the code bits) and added in that order inside chunks of 256 rows; a code's chunk sums are added in chunk order
 * -- the result is a function of the inputs alone, bit for bit.  Every launch on `stream`, no host synchronisation; an all-zero
 * weight gives the reference's NaN.  scratch: lg_vq_ema_scratch_bytes(n, K, d), linear in n and K * d; 0 for the shapes
 * lg_vq_scratch_bytes refuses (and for n >= 2^30).  lg_vq_ema_step needs n >= 1. */
size_t lg_vq_ema_scratch_bytes(int32_t n, int32_t K, int32_t d);
int lg_vq_ema_step(int32_t n, int32_t d, int32_t K, const float* x, const float* weight, float* embed, float* cluster_size,
                   double decay, double eps, int32_t* out_index, void* scratch, uint32_t flags, void* stream);

/* --- colours of a VecTree-compressed model ----------------------------------------------------------
 * The read side of the reference's extreme_saving model (vectree/utils.py:5-65 load_vqgaussian, scene/gaussian_model.py:420-461
 * load_vq) without the dequantised table: out_rgb[i] = max(eval_sh(sh_degree, row(slot[i]), normalize(means3D[i] - campos)) + 0.5, 0),
 * the colors_precomp of lg_gaussians, by the same lg_sh_to_rgb K1 evaluates on a float32 SH tensor -- equal to the dense path's
 * colours bit for bit.  rows_f16: fp16 table, row r at rows_f16 + r * row_stride_bytes (16-byte aligned base, stride a multiple
 * of 16 and >= 6 M), 3 M halfs per row in the file's order f_dc_0..2, f_rest_0.. (channel-major: coefficient m >= 1 of channel c
 * at 3 + c (M - 1) + m - 1); by convention the K codebook rows, then the non-VQ rows.  slot [N] uint32: row of each Gaussian,
 * NOT range-checked (the table's length is not an argument).  M in {1, 4, 9, 16}, (sh_degree + 1)^2 <= M: only the 16-byte
 * chunks holding an active coefficient are read.  Per Gaussian: 12 + 4 + 6 (sh_degree + 1)^2 bytes read, 12 written.
 * means3D [N,3], campos [3], out_rgb [N,3]: fp32 device.  One launch on `stream`, no host synchronisation.
 * flags: LG_FLAG_DEBUG, LG_FLAG_PROFILE. */
int lg_vq_colors(int32_t N, int32_t M, int32_t sh_degree, const float* means3D, const float* campos, const uint32_t* slot,
                 const void* rows_f16, int32_t row_stride_bytes, float* out_rgb, uint32_t flags, void* stream);

/* --- backward of lg_vq_colors: fine-tuning a compressed model in place -------------------------------
 * dL_drgb [N,3] (what lg_backward leaves for colors_precomp) -> the gradient of the row table and the colour part of dL/dmeans3D:
 *   dL_drows[r][idx(M,k,c)] = sum over i with slot[i] = r of  [rgb_{i,c} not clamped] B_k(normalize(means3D[i] - campos)) dL_drgb[i][c]
 *                             for k < (sh_degree + 1)^2;  exactly 0 for the other columns and for a codebook row no Gaussian uses
 *   dL_dmeans3D[i]          = the view-direction term (colour -> direction -> position); NULL: not computed
 * dL_drows is [n_rows][3 M] float32, UNPADDED, columns in the file's order of a row (see lg_vq_colors).  The arithmetic per
 * Gaussian is the dense backward's own (the values of the fp16 row the forward read, the clamp re-evaluated from them): the
 * gradient row of a Gaussian with a row of its own equals the dense model's dL/dSH row bit for bit.
 * Rows r >= K (one Gaussian each, by the format) are written by their Gaussian; a slot >= n_rows is ignored.  Rows r < K are a
 * segmented sum over the model's code index.  SUMMATION ORDER: the Gaussians of a code are added in ascending Gaussian index
 * inside chunks of 256 consecutive list entries, acc = acc + term starting from 0; the chunk sums are then added in chunk order.
 * No float atomics: the result is a function of the arguments alone, bit-identical run to run and across streams.
 * Every element of dL_drows is final when the call's work on `stream` completes (no caller-side clear).
 *
 * lg_vq_code_index builds the index of a model ONCE (the assignment does not change during fine-tuning): slot [N] uint32,
 * slot < K = a code; index: lg_vq_code_index_bytes(N, K) device bytes that must stay alive and unmodified while used;
 * scratch: lg_vq_code_index_scratch_bytes(N, K) device bytes, free again when the stream has passed the call.
 * lg_vq_colors_bwd: scratch of lg_vq_colors_bwd_scratch_bytes(N, M, K) device bytes (the chunk sums), private to the stream.
 * 0 <= N < 2^30, 1 <= K <= 2^24, K <= n_rows < 2^31 (the size queries return 0 otherwise).  All launches on `stream`, no host
 * synchronisation.  flags: LG_FLAG_DEBUG, LG_FLAG_PROFILE. */
size_t lg_vq_code_index_bytes(int32_t N, int32_t K);
size_t lg_vq_code_index_scratch_bytes(int32_t N, int32_t K);
int lg_vq_code_index(int32_t N, int32_t K, const uint32_t* slot, void* index, void* scratch, void* stream);
size_t lg_vq_colors_bwd_scratch_bytes(int32_t N, int32_t M, int32_t K);
int lg_vq_colors_bwd(int32_t N, int32_t M, int32_t sh_degree, int32_t K, int64_t n_rows, const float* means3D, const float* campos,
                     const uint32_t* slot, const void* rows_f16, int32_t row_stride_bytes, const float* dL_drgb, const void* index,
                     float* dL_drows, float* dL_dmeans3D, void* scratch, uint32_t flags, void* stream);

/* --- Adam / AdamW step ------------------------------------------------------------------------------
 * The optimizer.step() of the reference's training_setup (scene/gaussian_model.py: torch.optim.AdamW(l, lr=0.0, eps=1e-15) over six
 * one-tensor groups with an lr each) for a caller without torch: applies grad to param and to the two moments lg_compact_rows moves.
 * Per element, float32, correctly rounded divide / sqrt, the sum closing each line one explicit fmaf, nothing else contracted, t = step:
 *     g' = g + weight_decay * p  (L2 form, only for weight_decay != 0)     p = p * (1 - lr * weight_decay)  (LG_ADAM_DECOUPLED_WD)
 *     exp_avg    = exp_avg + (1 - beta1) * (g' - exp_avg)
 *     exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) * (g' * g')
 *     p          = p - step_size * (exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps)),   step_size = lr / (1 - beta1^t)
 * step_size, sqrt(1 - beta2^t), 1 - lr * weight_decay, 1 - beta1 and 1 - beta2 are evaluated in double and rounded once to float:
 * torch's default (non-fused, non-capturable) Adam / AdamW.  No amsgrad, no maximize.  Non-finite gradients propagate.
 * tensors: HOST array; the four device tensors of an entry are float32, contiguous, numel elements each and do not overlap.
 * Entries with numel == 0 are skipped.  The table travels in the kernel arguments, LG_ADAM_MAX_TENSORS (8) tensors per launch:
 * no device allocation, no host-to-device copy, no synchronisation, every launch on `stream`.  A workgroup owns one span of
 * LG_ADAM_SPAN (4096) elements of one tensor; 16-byte aligned tensors go through 16-byte loads and stores.  28 bytes of traffic
 * per element.  flags: LG_ADAM_DECOUPLED_WD, LG_FLAG_PROFILE (one "adam" entry per launch); LG_FLAG_DEBUG does not apply.
 * LG_ERR_INVALID_ARGUMENT, before any device call: num_tensors < 0, a beta outside [0, 1), numel < 0, step < 1, a null or
 * misaligned pointer with numel > 0. */
typedef struct lg_adam_tensor {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;   /* device, float32, contiguous */
    int64_t numel;
    double lr, weight_decay;
    int64_t step;                      /* the step being taken, >= 1 */
} lg_adam_tensor;
#define LG_ADAM_DECOUPLED_WD 1u          /* AdamW: p *= 1 - lr*wd; otherwise g += wd*p (Adam's L2 form) */
#define LG_ADAM_MAX_TENSORS 8            /* tensors per launch */
#ifndef LG_ADAM_SPAN
#define LG_ADAM_SPAN 4096                /* elements per workgroup (a build-time choice of the library, by measurement) */
#endif
int lg_adam_step(int32_t num_tensors, const lg_adam_tensor* tensors /* host */, double beta1, double beta2, double eps,
                 uint32_t flags, void* stream);

/* lg_adam_step over the rows a byte mask names (a view's visibility_filter, or the union of several views'): a tensor [rows, ...] of
 * row_len = numel / rows elements per row is stepped with `rows` mask bytes.
 *   row whose byte is non-zero   every element takes exactly lg_adam_step's arithmetic, with the same host-side constants; bias
 *                                correction uses the entry's own `step`
 *   row whose byte is zero       param, exp_avg and exp_avg_sq keep their bits: no moment decay, no weight decay in either form, and
 *                                the row's gradient is never read (a NaN there changes nothing)
 * This is NOT dense Adam, where an unseen row coasts on its momentum.  An entry with row_mask == NULL is a dense entry: lg_adam_step's
 * update inside the same launch (rows is not looked at).  row_mask has byte alignment; no byte outside [row_mask, row_mask + rows) is
 * read.  A 16-byte access wholly in unseen rows is neither loaded nor stored.  Same table by value, LG_ADAM_MAX_TENSORS entries per
 * launch, same flags; LG_FLAG_PROFILE records one "adam_rows" entry per launch.
 * LG_ERR_INVALID_ARGUMENT, before any device call: every case of lg_adam_step, and with a row_mask rows < 1, numel not a multiple of
 * rows, a row of more than 2^31 - 1 elements. */
typedef struct lg_adam_rows_tensor {
    lg_adam_tensor t;
    const uint8_t* row_mask;           /* device, `rows` bytes, non-zero = step the row; NULL = dense entry */
    int64_t rows;
} lg_adam_rows_tensor;
int lg_adam_step_rows(int32_t num_tensors, const lg_adam_rows_tensor* tensors /* host */, double beta1, double beta2, double eps,
                      uint32_t flags, void* stream);

/* --- densification: view statistics and clone / split / prune ---------------------------------------
 * GaussianModel.add_densification_stats and densify_and_prune (scene/gaussian_model.py:602-761, 784-788) for float32 device tensors.
 * lg_densify_stats, one launch, no read-back: for every row i with update_filter[i] != 0
 *     accum[i] += sqrt(fma(g[i][1], g[i][1], g[i][0]^2))   denom[i] += 1    max_radii2D[i] = max(max_radii2D[i], (float) radii[i])  (radii != NULL)
 * viewspace_grad float32 [N,3], update_filter uint8 / bool [N], radii int32 [N] or NULL (then max_radii2D is not looked at).
 * lg_densify_plan: with s = exp(scaling row), m = max s, sigma = sigmoid(opacity), g = accum / denom (NaN -> 0) per row
 *     clone  = g >= thr_g && m <= thr_d          split = g >= thr_g && m > thr_d
 *     pruned(sigma, mu) = sigma < min_opacity || (use_extent && mu > thr_w)
 * writes the source map of the output rows, in this order: originals with !split that are not pruned(sigma, m); clones of those;
 * first children, then second children, of the split rows that are not pruned(sigma, m / 1.6f) -- each group in source order.
 * map: 2 N entries of two uint32 {source row, kind << 30 | k}, kind 0 original, 1 clone, 2 first child, 3 second child; k = rank of the
 * parent among ALL split rows (its noise rows are k and n_s + k).  record: 8 int32 on the device {N_out, n_keep, n_clone, n_s,
 * n_child, 0, 0, 0}.  The thresholds are floats: evaluate them in double and round once.  thr_g must be > 0, N < 2^30.
 * scratch: lg_densify_scratch_bytes(N).
 * lg_densify_rows, one launch (grid.y = tensor), writes N_out rows of up to LG_DENSIFY_MAX_TENSORS tensors from the map.  tensors is a
 * HOST array; src has N rows and dst N_out rows of row_words 32-bit words (> 0), contiguous; src and dst do not overlap.  role:
 *     LG_DENSIFY_COPY     every output row is its source row, bit for bit
 *     LG_DENSIFY_MOMENT   originals copied, new rows zero
 *     LG_DENSIFY_XYZ      children: R(q / |q|) (noise * exp(scaling)) + xyz, q = (r, x, y, z); row_words 3
 *     LG_DENSIFY_SCALING  children: log(exp(scaling) / 1.6f); row_words 3
 *     LG_DENSIFY_ZERO     every output row zero (src is not looked at)
 * rotation [N,4], scaling [N,3]: the model's raw rows; noise float32 [noise_rows,3], noise_rows >= 2 n_s (unit normal).
 * flags: LG_FLAG_PROFILE ("densify_stats", "densify_plan", "densify_rows").  LG_ERR_INVALID_ARGUMENT before any device call. */
typedef struct lg_densify_tensor {
    const void* src; void* dst;        /* device */
    int32_t row_words;
    int32_t role;
} lg_densify_tensor;
#define LG_DENSIFY_COPY 0
#define LG_DENSIFY_MOMENT 1
#define LG_DENSIFY_XYZ 2
#define LG_DENSIFY_SCALING 3
#define LG_DENSIFY_ZERO 4
#define LG_DENSIFY_MAX_TENSORS 32
size_t lg_densify_scratch_bytes(int32_t N);
int lg_densify_stats(int32_t N, const float* viewspace_grad, const uint8_t* update_filter, const int32_t* radii, float* max_radii2D,
                     float* accum, float* denom, uint32_t flags, void* stream);
int lg_densify_plan(int32_t N, const float* scaling, const float* opacity, const float* accum, const float* denom, float thr_g,
                    float thr_d, float thr_w, float min_opacity, int32_t use_extent, void* map, int32_t* record, void* scratch,
                    uint32_t flags, void* stream);
int lg_densify_rows(int32_t N, int64_t N_out, const void* map, const int32_t* record, int32_t num_tensors,
                    const lg_densify_tensor* tensors /* host */, const float* rotation, const float* scaling, const float* noise,
                    int64_t noise_rows, uint32_t flags, void* stream);

/* --- feature blending over a view's tile lists ------------------------------------------------------
 * lg_blend_features composites C further per-Gaussian channels with the blending weights w = alpha T of a view whose forward has
 * run: it reads only what that forward left in `geom` and `binning` (the same lg_view -- image size, segment_length, LG_FLAG_FAST_EXP
 * -- and the same N and num_rendered as that call; for lg_forward_bounded num_rendered is max_rendered).  Per pixel, front to back over
 * the tile's sorted list with the forward's own pair step (canonical arithmetic, or the guarded hardware exp under LG_FLAG_FAST_EXP: the
 * include / exclude decisions are the forward's):
 *     F_c = fma(f_c, alpha T, F_c),  T = T (1 - alpha),  stop at T (1 - alpha) < 1e-4;   out_c = fma(T, bg_c, F_c).
 * features [N][C] float32, 1 <= C <= LG_FEATURES_MAX; bg_features [C] or NULL (zeros); out [C][H][W]; alpha [H][W] or NULL: the sum
 * of the weights, accumulated as a channel of ones -- bit for bit what blending a column of ones gives, 1 - T up to rounding.
 * In canonical mode a triple of channels equals lg_forward's image of the same colours_precomp bit for bit.  A view the forward
 * abandoned on the device (lg_forward_bounded) yields bg_features / 0.  No host round trip, no allocation, every launch on `stream`.
 * lg_blend_features_backward: dL_dfeatures [N][C] = sum over pixels of w dL_dout -- the gradient with respect to `features` only
 * (the geometry gradient: lg_backward_features below).  No float atomics, no memset: one row of partial sums per (tile, Gaussian) instance, then one ordered
 * sum per Gaussian; rows of Gaussians without instances are exact zeros and the result is bit-identical run to run.
 * scratch: lg_features_scratch_bytes(N, num_rendered, C) device bytes (the channels are processed in chunks where [num_rendered][C]
 * floats would exceed 1 GiB).  flags of the view that apply: LG_FLAG_FAST_EXP, LG_FLAG_PROFILE ("features_fwd", "features_bwd",
 * "features_gather"), LG_FLAG_DEBUG (synchronise and check after every launch). */
#define LG_FEATURES_MAX 64
size_t lg_features_scratch_bytes(int32_t N, int64_t num_rendered, int32_t C);
int lg_blend_features(const lg_view* view, int32_t N, const void* geom, const void* binning, int64_t num_rendered,
                      const float* features, int32_t C, const float* bg_features, float* out, float* alpha, void* stream);
int lg_blend_features_backward(const lg_view* view, int32_t N, const void* geom, const void* binning, int64_t num_rendered,
                               const float* dL_dout, int32_t C, float* dL_dfeatures, void* scratch, void* stream);

/* lg_backward_features: lg_backward for a loss on the feature image `out`, on `alpha` and on the colour image of ONE forward -- the
 * geometry gradient of lg_blend_features.  Any of dL_dcolor [3][H][W], dL_dout [C][H][W], dL_dalpha [H][W] may be NULL (all three:
 * zero geometry gradients).  Order on `stream`: K7 (lg_blend_bwd) when dL_dcolor is given; lg_features_bwd_geom, one back-to-front walk
 * of the tile lists per group of up to 32 channels (dL_dalpha rides with the first), which adds the six pixel-offset moments of the
 * feature / alpha loss to the per-instance rows K7 wrote (or writes the rows when K7 did not run); K9 (lg_preprocess_bwd) ONCE; then
 * dL_dfeatures [N][C] (or NULL) exactly as lg_blend_features_backward computes it.  view, gaussians, radii, geom, binning, img,
 * num_rendered and the gradient outputs dL_dmeans2D .. dL_dshs_rest: as for lg_backward, same rules (an output per provided input);
 * features, C, bg_features: as handed to lg_blend_features.  A view the forward abandoned, or a segment_length other than the
 * forward's, yields zero gradients.  No float atomics, no memset: bit-identical run to run.
 * scratch: lg_backward_features_scratch_bytes(N, num_rendered, C) device bytes.  Profile entry of the walks: "features_bwd_geom". */
size_t lg_backward_features_scratch_bytes(int32_t N, int64_t num_rendered, int32_t C);
int lg_backward_features(const lg_view* view, const lg_gaussians* g, const int32_t* radii, const void* geom, const void* binning,
                         const void* img, int64_t num_rendered, const float* dL_dcolor, const float* features, int32_t C,
                         const float* bg_features, const float* dL_dout, const float* dL_dalpha, float* dL_dmeans2D,
                         float* dL_dmeans3D, float* dL_dshs, float* dL_dcolors, float* dL_dopacity, float* dL_dscales,
                         float* dL_drotations, float* dL_dcov3D, float* dL_dshs_rest, float* dL_dfeatures, void* scratch,
                         void* stream);

/* --- camera pose gradients ---------------------------------------------------------------------------
 * lg_backward_camera: dL/dviewmatrix [16], dL/dprojmatrix [16], dL/dcampos [3] of the loss whose backward has just run -- the
 * backward treats lg_view.viewmatrix / projmatrix / campos as constants; this call differentiates with respect to them (pose
 * refinement).  Call it AFTER lg_backward, lg_backward_chunked or lg_backward_features of the same view (same lg_view, lg_gaussians,
 * radii, geom, binning, num_rendered), on the same stream, before `backward_scratch` -- the scratch buffer of that backward, which
 * still holds the per-instance moment rows -- is reused.  Row-vector layout m[4 row + column], as the inputs.  Column 3 of the view
 * matrix and column 2 of the projection matrix take no part in the forward: their gradients are exact zeros.  The published
 * conventions of the backward hold here too (no gradient through the +-1.3 tan(fov) clamp, the 0.2 near plane or the radius).
 * lg_camera_bwd (one lane per Gaussian) gathers each visible Gaussian's rows again, forms its 27 camera terms in float32 and sums them
 * in float64 in a fixed order (wave butterfly, waves in order, one plain store per workgroup); lg_camera_reduce (one workgroup) adds
 * the workgroup partials in a fixed order and rounds once to float32.  No atomics, no memset: bit-identical run to run.  A view the
 * forward abandoned, a segment_length other than the forward's or a forward without LG_FLAG_SAVE_SH_JACOBIAN yield exact zeros, as
 * lg_backward; N == 0 writes zeros.  SH inputs need LG_FLAG_SAVE_SH_JACOBIAN on the view (LG_ERR_INVALID_ARGUMENT otherwise): the
 * camera centre enters through the view direction, whose Jacobian K1 saved.  The three outputs are required.
 * scratch: lg_camera_scratch_bytes(N) device bytes.  Profile entries: "camera_bwd", "camera_reduce". */
size_t lg_camera_scratch_bytes(int32_t N);
int lg_backward_camera(const lg_view* view, const lg_gaussians* g, const int32_t* radii, const void* geom, const void* binning,
                       int64_t num_rendered, const void* backward_scratch, float* dL_dviewmatrix, float* dL_dprojmatrix,
                       float* dL_dcampos, void* scratch, void* stream);

/* --- 3D smoothing filter (Mip-Splatting's 3D filter; lg_filter3d.h) -----------
 * A Gaussian that no training camera samples at more than 1 / t samples per world unit must not be narrower than that sampling
 * allows: filter3d = sqrtf(0.2f) t is added (as a variance, filter3d^2) to each squared scale, and the opacity is scaled so that the
 * Gaussian keeps its integral.
 *
 * lg_filter3d_update: for every mean p and every camera n of the DEVICE table `cameras` (viewmatrix in the row-vector layout of
 * lg_view.viewmatrix), in float32 with explicit fmaf and correctly rounded divisions (lg_math.h: lg_filter3d_term):
 *     (x, y, z) = view-space p     fx = W / (2 tanfovx)   fy = H / (2 tanfovy)     u = x / z * fx + 0.5 W    v = y / z * fy + 0.5 H
 *     seen_n = z > 0.2 && -0.15 W <= u <= 1.15 W && -0.15 H <= v <= 1.15 H          (a NaN compares false: unseen)
 *     t_n = z / fx                       world units per pixel at p
 * filter3d[i] = sqrtf(0.2f) min over the seeing cameras of t_n -- the paper's maximal sampling rate; with cameras of one focal length
 * it is the published code's min depth / max focal.  A row no camera sees gets the largest filter3d of the seen rows (as published);
 * when no row is seen at all every value is 0, the identity of the apply (the published code raises there).  seen (optional):
 * 1 / 0 per row.  Two launches on `stream` ("filter3d_update": one lane per Gaussian, the camera table staged through LDS 64 cameras
 * at a time, one partial maximum per workgroup with a plain store; "filter3d_reduce": every workgroup takes the maximum of the at
 * most 2048 partials in a fixed order and fills the unseen rows of its stride).  No atomics, no memset, no host read-back:
 * bit-identical run to run.  scratch: lg_filter3d_scratch_bytes(N) device bytes, 4-byte aligned.
 *
 * lg_filter3d_apply, one elementwise launch ("filter3d_apply").  With LG_FILTER3D_RAW scaling [N,3] holds log-scales r and opacity
 * [N] logits o, in and out -- the domain LG_FLAG_RAW_PARAMS reads:
 *     u_k = expf(r_k)^2 + f^2    r'_k = 0.5 logf(u_k)    w_k = expf(r_k)^2 / u_k    c = sqrtf(w_0 w_1 w_2)
 *     y = sigmoid(o) c           o' = logf(y / (1 - y))                   (y == 0 gives -inf: opacity 0 in K1, culled)
 * without it scales s and opacities sigma:  s'_k = sqrtf(s_k^2 + f^2),  sigma' = sigma c.  A row with f == 0 is copied bit for bit.
 * lg_filter3d_apply_bwd ("filter3d_apply_bwd"): the gradients with respect to scaling and opacity from those with respect to the
 * outputs, w_k, c, y recomputed from the inputs by the forward's operations; the filter takes none.  Raw:
 *     dL/dr_k = g_r'_k w_k + g_o' (1 - w_k) / (1 - y)       dL/do = g_o' (1 - sigmoid(o)) / (1 - y)
 * (1 - w_k evaluated as f^2 / u_k and 1 - sigmoid(o) as sigmoid(-o): the same in real arithmetic, no cancellation).  A row with
 * f == 0 copies its incoming gradients bit for bit.  Outputs must not overlap inputs.  Tensors whose pointers are all 16-byte
 * aligned go through 16-byte accesses, others one dword at a time.
 *
 * All three: LG_ERR_INVALID_ARGUMENT before any device call for N < 0, N >= 2^30, V < 1, a null or misaligned (4 bytes) pointer;
 * N == 0 is a no-op.  flags: LG_FILTER3D_RAW (apply), LG_FLAG_PROFILE. */
typedef struct lg_filter_camera {
    float viewmatrix[16];
    float tanfovx, tanfovy;
    int32_t width, height;
} lg_filter_camera;                     /* 80 bytes */
#define LG_FILTER3D_RAW 1u              /* scaling = log-scales, opacity = logits, in and out; otherwise activated values */
size_t lg_filter3d_scratch_bytes(int32_t N);
int lg_filter3d_update(int32_t N, const float* means3D, int32_t V, const lg_filter_camera* cameras, float* filter3d, uint8_t* seen,
                       void* scratch, uint32_t flags, void* stream);
int lg_filter3d_apply(int32_t N, const float* scaling, const float* opacity, const float* filter3d, float* out_scaling,
                      float* out_opacity, uint32_t flags, void* stream);
int lg_filter3d_apply_bwd(int32_t N, const float* scaling, const float* opacity, const float* filter3d, const float* dL_dout_scaling,
                          const float* dL_dout_opacity, float* dL_dscaling, float* dL_dopacity, uint32_t flags, void* stream);

/* out[j] = (((rows[0][j] + rows[1][j]) + rows[2][j]) + ...) over V rows of n floats (row pitch row_stride floats): the
 * sequential in-place float accumulation of per-view scores in prune.py:144-155, in view order, as one launch. */
int lg_ordered_sum(int32_t V, int64_t n, const float* rows, int64_t row_stride, float* out, void* stream);

/* --- distCUDA2 (first half) -------------------------------------------------------
 * Replaces the reference's simple-knn extension: submodules/simple-knn/spatial.cu:15-27 distCUDA2() ->
 * simple_knn.cu:185-221 SimpleKNN::knn(): mean_dist2[i] = (d0 + d1 + d2) / 3 with d0 <= d1 <= d2 the three smallest
 * squared Euclidean distances from points[i] to the OTHER points (by index: coincident points count with distance 0;
 * fewer than 4 points leave FLT_MAX placeholders in the sum, as in simple_knn.cu:150,182).  Exact.
 * points [P,3] fp32 device, mean_dist2 [P] fp32 device, scratch: lg_knn_scratch_bytes(P) device bytes.  No host sync. */
size_t lg_knn_scratch_bytes(int32_t P);
int lg_knn3_mean_dist2(int32_t P, const float* points, float* mean_dist2, void* scratch, uint32_t flags, void* stream);

/* --- photometric loss of the training step -------------------------------------
 * Replaces utils/loss_utils.py:18-19 l1_loss() and :46-85 ssim() (11x11 Gaussian window sigma 1.5 of :26-43,
 * conv2d zero padding 5, C1 = 0.01^2, C2 = 0.03^2, mean over all C*H*W), as combined at prune_finetune.py:161-164:
 *     loss = (1 - lambda) * l1 + lambda * (1 - ssim).
 * img, gt: [C,H,W] fp32 device.  state: lg_loss_state_bytes(C,H,W) device bytes, written by forward, read by backward.
 * out_l1_ssim: device float[2] = {mean |img-gt|, mean ssim_map}.
 * backward: dL_dimg [C,H,W] = scale_l1 * *dL_dl1 * d l1/d img + scale_ssim * *dL_dssim * d ssim/d img; dL_dl1 / dL_dssim are
 * DEVICE scalars (the autograd gradients; NULL => that term is 0), so the call never synchronises.
 * flags: LG_FLAG_DEBUG, LG_FLAG_PROFILE, LG_FLAG_L1_ONLY. */
size_t lg_loss_state_bytes(int32_t C, int32_t H, int32_t W);
int lg_loss_forward(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, void* state, float* out_l1_ssim,
                    uint32_t flags, void* stream);
int lg_loss_backward(int32_t C, int32_t H, int32_t W, const float* img, const float* gt, const void* state,
                     const float* dL_dl1, float scale_l1, const float* dL_dssim, float scale_ssim, float* dL_dimg,
                     uint32_t flags, void* stream);

/* The four status words of a view as they stand when `stream` reaches this call (one blocking 16-byte read): { abort flags,
 * prefiltered violation, largest depth bit pattern, instance count }.  abort bit 2: a look-back of the radix sort exhausted its
 * poll budget (a predecessor tile never published: a device fault, never observed) -- the view was left EMPTY instead of being
 * blended from a wrong order, and this call (like any forward with LG_FLAG_DEBUG) returns LG_ERR_DEVICE. */
int lg_view_status(const void* geom, int32_t N, uint32_t* out4 /* host */, void* stream);

/* Byte offset, inside the geom buffer of a forward over N Gaussians, of uint8 visible[N] (1 = radii > 0): the reference's
 * `visibility_filter = radii > 0` (gaussian_renderer/__init__.py:121) without a kernel of its own. */
size_t lg_geom_visible_offset(int32_t N);

/* The lg_debug_* entry points (stand-alone sort passes, tile-list dumps, the wave reduction on its own ...) are exported by the
 * library for tests/ and tools/ only; they are declared in include/lightgaussian_debug.h and are not part of the drop-in ABI. */

/* --- introspection / measurement ------------------------------------------------------------ */
int lg_abi_version(void);
const char* lg_last_error(void);
/* 12 hex digits identifying the kernel sources the library was built from (sha1 of csrc/ + this header); the profile
 * summaries under profiles/ record it and bench.py quotes PMC-derived numbers only when it matches the loaded library */
const char* lg_build_id(void);

/* Per-kernel timings recorded when LG_FLAG_PROFILE is set (hipEvents on the launch stream).
 * lg_profile_read synchronises the stream-recorded events, then fills up to `cap` entries. */
typedef struct lg_kernel_time {
    char name[32];
    double total_ms;
    int64_t launches;
} lg_kernel_time;
int lg_profile_read(lg_kernel_time* out, int cap);
void lg_profile_reset(void);

/* statistics of the most recent forward on this thread (for bench roofline accounting) */
typedef struct lg_stats {
    int64_t num_rendered;  /* instances after exact footprint culling */
    int64_t num_visible;   /* -1: not tracked on the device (count radii > 0 instead) */
} lg_stats;
int lg_last_stats(lg_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* LIGHTGAUSSIAN_H */
