/*
 * splatraster.h — C ABI of the MI355X-native differentiable Gaussian tile rasterizer
 * and of the 3-nearest-neighbour distance kernel used to seed Gaussian scales.
 *
 * This is the drop-in boundary for SplatLoc's native hot path.  The reference binds
 * this path through two CUDA extension modules whose sources are NOT vendored in
 * /root/reference (empty submodule dirs, .gitmodules:1-9):
 *
 *   diff_gauss.GaussianRasterizer.forward / backward
 *       call site  gaussian_splatting/gaussian_renderer/__init__.py:117-126  (forward)
 *       settings   gaussian_splatting/gaussian_renderer/__init__.py:42-55
 *       backward   triggered by train_gaussians.py:229 and :286 (loss.backward())
 *   simple_knn._C.distCUDA2
 *       call site  gaussian_splatting/scene/gaussian_model.py:18,206
 *   tinycudann.Encoding (the multiresolution grid encodings of FeatureDecoder)
 *       call site  models/encoding.py:3,33-46 (built), models/decoders.py:63 (called)
 *   utils.selection.gaussian_selectition (landmark selection)
 *       call site  test.py:39 (import), test.py:564 (called by --eval_selection)
 *   utils.match_utils.HungarianMatcher / hungarian_solve, LocalizeQuery.get_frusm_pts (2D-3D matching)
 *       call site  test.py:247-378 (match_feature, --eval_pose)
 *   pycolmap.absolute_pose_estimation via solve_pose (absolute pose: P3P LO-RANSAC and refinement)
 *       call site  test.py:64-84 (solve_pose), test.py:345 (called by match_feature, --eval_pose)
 *   utils.fusion_utils.TSDFVolumeTorch.integrate / get_mesh's vertex gather (feature-TSDF fusion)
 *       call site  pre_process/gen_3d_fusion_feature.py:70-94 (run_feature_fusion)
 *
 * Everything here is plain C: raw device pointers, sizes, an opaque stream handle
 * (hipStream_t passed as void*), int status codes.  No torch types, no exceptions.
 * All float tensors are fp32, row-major, contiguous, resident in device memory.
 *
 * Memory ownership: the caller owns every buffer.  Scratch state that must survive
 * from forward to backward lives in three caller-allocated opaque buffers
 * (geometry / binning / image), sized by the *_bytes() queries below, so a framework's
 * caching allocator owns all device memory and several frames can be alive at once
 * (train_gaussians.py:195-229 keeps 5 forwards alive before one backward).
 */
#ifndef SPLATRASTER_H
#define SPLATRASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped on every change of a signature or buffer layout; the Python binding refuses a library
 * whose splatraster_abi_version() differs (a stale in-tree .so would otherwise be called through
 * ctypes with mismatched arguments) */
#define SPLATRASTER_ABI_VERSION 20

#define SPLATRASTER_TILE 16 /* tile edge in pixels (16x16 = 256 pixels = 4 wave64) */

/* status codes */
#define SPLATRASTER_OK 0
#define SPLATRASTER_ERR_BAD_ARG 1      /* null pointer / inconsistent sizes / both-or-neither inputs */
#define SPLATRASTER_ERR_HIP 2          /* a HIP runtime call or kernel launch failed (incl. a wedged look-back: hard spin bound -> trap) */
#define SPLATRASTER_ERR_UNSUPPORTED 3  /* e.g. sh_degree > 3 */
#define SPLATRASTER_ERR_OVERFLOW 4     /* tile instance count does not fit the binning buffer */
#define SPLATRASTER_WARN_LOOKBACK_STALL 5 /* splatraster_poll_errors() only: a scan / sort block waited longer than the soft
                                          * spin bound for a predecessor; NOT an error of any frame (results are late, never wrong) */

/*
 * Mirror of diff_gauss.GaussianRasterizationSettings
 * (gaussian_renderer/__init__.py:42-55) minus the tensors, which are passed as pointers.
 */
typedef struct splatraster_settings {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    float scale_modifier;
    int32_t sh_degree;   /* active SH degree (0..3); only used when shs != NULL */
    int32_t sh_coeffs;   /* M: coefficients per colour channel stored in shs [P, M, 3]; 0 when shs == NULL */
    int32_t channels;    /* C: composited channels. colors_precomp is [P, C]; with shs, C must be 3 */
    int32_t bg_channels; /* number of valid floats behind bg; channels >= bg_channels read 0 (train_gaussians.py:70 passes 3 for C = 4) */
    int32_t prefiltered;
    int32_t debug;       /* bit 1 (SPLATRASTER_SETTINGS_FORWARD_ONLY): no backward will read this frame's buffers — the render stage
                          * then skips what only a backward uses (the dead marks of the wide forward); other bits: unused */
} splatraster_settings;
#define SPLATRASTER_SETTINGS_FORWARD_ONLY 2

/* ---- buffer sizing ------------------------------------------------------------------ */

/* per-Gaussian forward state: projected centre, depth, conic+opacity, tile counts,
 * depth-sorted order, instance offsets, SH colours + clamp flags. */
size_t splatraster_geometry_bytes(int32_t P);
/* per-tile-instance state for R = num_rendered instances: sorted point list and the
 * sort's ping-pong buffers, the [tiles] range table, the per-instance payload (32-byte record
 * + quadrant reach mask) and, when channels % 4 != 0, the 16-byte-aligned feature table. */
size_t splatraster_binning_bytes(int32_t P, int64_t R, int32_t width, int32_t height, int32_t channels);
/* per-pixel forward state needed by backward: final transmittance, last contributor (its position in the tile's list), and behind
 * them what the compact payload adds: the last contributor's position in the list's compact stream (a third 4-byte plane: 12 bytes
 * per pixel) and the [2 * tiles] table of the compact ranges. */
size_t splatraster_image_bytes(int32_t width, int32_t height);

/* ---- forward ------------------------------------------------------------------------- */

/*
 * Stage 1 of forward (replaces the preprocess + InclusiveSum part of the reference
 * extension's forward).  Projects all P Gaussians, depth-sorts them, counts the tiles
 * each touches, and returns the total number of (tile, Gaussian) instances in
 * *num_rendered (one stream synchronisation to read a single int64).
 *
 * Exactly one of shs / colors_precomp and exactly one of (scales, rotations) /
 * cov3D_precomp must be non-NULL, as the reference wrapper enforces.
 *
 * radii [P] int32 is an output tensor (returned 4th by GaussianRasterizer.forward).
 */
int splatraster_forward_geometry(const splatraster_settings* s, int32_t P,
                                 const float* means3D,       /* [P,3] */
                                 const float* shs,           /* [P,M,3] or NULL */
                                 const float* opacities,     /* [P,1] */
                                 const float* scales,        /* [P,3] or NULL */
                                 const float* rotations,     /* [P,4] (w,x,y,z) or NULL */
                                 const float* cov3D_precomp, /* [P,6] or NULL */
                                 const float* viewmatrix,    /* [4,4] row-vector convention */
                                 const float* projmatrix,    /* [4,4] view @ proj */
                                 const float* campos,        /* [3] */
                                 void* geometry, int32_t* radii, int64_t* num_rendered,
                                 void* stream);

/*
 * Stage 2 of forward: instance emission, stable tile-bucket radix sort, tile ranges and
 * front-to-back alpha compositing.  R must be the value stage 1 returned and `binning`
 * must hold splatraster_binning_bytes(P, R, W, H, C) bytes.
 *
 * Outputs: out_color [C,H,W], out_depth [1,H,W], out_alpha [1,H,W]
 * (the first three members of the tuple GaussianRasterizer.forward returns,
 * gaussian_renderer/__init__.py:117).
 */
int splatraster_forward_render(const splatraster_settings* s, int32_t P, int64_t R,
                               const float* bg,             /* [bg_channels] */
                               const float* colors_precomp, /* [P,C] or NULL when shs were given */
                               void* geometry, void* binning, void* image,
                               float* out_color, float* out_depth, float* out_alpha,
                               void* stream);

/* ---- backward ------------------------------------------------------------------------ */

/*
 * Full backward (replaces the reference extension's rasterize_gaussians_backward).
 * Gradient outputs are OVERWRITTEN (zeroed inside).  dL_dmeans2D is [P,3] with
 * z = 0 and xy in NDC units (pixel gradient x 0.5*W / 0.5*H), which is what
 * GaussianModel.add_densification_stats reads (gaussian_model.py:677-679).
 * Optional outputs (dL_dshs, dL_dcov3D, dL_dscales, dL_drotations, dL_dcolors) may be
 * NULL when the matching forward input was NULL.
 */
int splatraster_backward(const splatraster_settings* s, int32_t P, int64_t R,
                         const float* bg, const float* means3D, const float* shs,
                         const float* colors_precomp, const float* opacities,
                         const float* scales, const float* rotations,
                         const float* cov3D_precomp, const float* viewmatrix,
                         const float* projmatrix, const float* campos,
                         const int32_t* radii,
                         void* geometry /* read + its backward scratch area is written */,
                         const void* binning, const void* image,
                         const float* out_color, const float* out_depth, const float* out_alpha,
                         const float* dL_dout_color, /* [C,H,W] */
                         const float* dL_dout_depth, /* [1,H,W] or NULL (= zeros) */
                         const float* dL_dout_alpha, /* [1,H,W] or NULL (= zeros) */
                         float* dL_dmeans3D,   /* [P,3] */
                         float* dL_dmeans2D,   /* [P,3] */
                         float* dL_dcolors,    /* [P,C] or NULL */
                         float* dL_dopacities, /* [P,1] */
                         float* dL_dscales,    /* [P,3] or NULL */
                         float* dL_drotations, /* [P,4] or NULL */
                         float* dL_dcov3D,     /* [P,6] or NULL */
                         float* dL_dshs,       /* [P,M,3] or NULL */
                         /* pose-gradient extension (no counterpart in the reference):
                          * exact derivative w.r.t. the camera tensors, or NULL to skip */
                         float* dL_dviewmatrix, /* [4,4] or NULL */
                         float* dL_dprojmatrix, /* [4,4] or NULL */
                         float* dL_dcampos,     /* [3] or NULL (non-zero only with shs) */
                         void* stream);

/* ---- a WINDOW of views in one launch sequence -------------------------------------------- */

/*
 * SplatLoc.map renders `window_size` (5) views of one Gaussian scene, sums their losses and runs ONE
 * backward (train_gaussians.py:195-229); color_refinement and eval_rendering call the rasterizer once per
 * view.  The reference extension has only the per-view call, so that loop is 5 x (preprocess, two sorts,
 * compositing) + autograd's accumulation of 5 gradient sets.  These entry points take the V <= 8 views of a
 * window at once: one preprocess over the P Gaussians for all views, ONE depth sort of the V * P (view,
 * Gaussian) rows, ONE tile sort keyed by (view, tile), one compositing grid over V * tiles * 4 quadrant-waves —
 * a 640x480 frame alone leaves most of an MI355X idle — and a backward that sums the V views into ONE set of
 * parameter gradients.  Results per view are bit-identical to V calls of the functions above (both sorts are
 * stable: every (view, tile) list is in (depth, index) order); only the float-atomic summation order of the
 * gradients differs, as it does from run to run anyway.  All views share the settings' image size, channel
 * count, scale modifier and background; tanfovx / tanfovy are per view (settings->tanfovx/y are ignored here).
 * Colours must be precomputed (`colors_precomp`, SplatLoc's configuration): view-dependent SH colours stay on the
 * per-view call (SPLATRASTER_ERR_UNSUPPORTED here).  The pose-gradient extension has a window entry point of its own,
 * splatraster_backward_window_cameras below: the camera gradients of every view and NO parameter gradients (pose refinement
 * freezes the map); splatraster_backward_window itself returns parameter gradients only, and
 * splatraster_backward_window_joint returns both from one compositing backward.
 */
#define SPLATRASTER_MAX_WINDOW_VIEWS 8

typedef struct splatraster_window_view {
    const float* viewmatrix; /* [4,4] device memory, row-vector convention */
    const float* projmatrix; /* [4,4] view @ proj */
    const float* campos;     /* [3] or NULL (unused with precomputed colours) */
    float tanfovx, tanfovy;
    int32_t* radii;          /* [P] int32: forward output (4th member of the tuple), read again by the backward */
    float* out_color;        /* [C,H,W] forward output; read by the backward */
    float* out_depth;        /* [1,H,W] */
    float* out_alpha;        /* [1,H,W] */
    /* backward only (ignored by the forward calls) */
    const float* dL_dout_color; /* [C,H,W]; or [color_grad_channels,H,W] when that is in [1, C) */
    const float* dL_dout_depth; /* [1,H,W] or NULL (= zeros) */
    const float* dL_dout_alpha; /* [1,H,W] or NULL (= zeros) */
    float* dL_dmeans2D;         /* [P,3] output: per view, as GaussianModel.add_densification_stats reads it */
    /* SplatLoc's render() hands the colour buffer out as TWO tensors, render = image[:3] and kp_prob = image[-1]
     * (gaussian_renderer/__init__.py:133-135), and the losses produce their gradients separately — through autograd
     * each arrives zero-padded to [C,H,W] and the two are added (five elementwise kernels per view).  A caller that
     * has the two gradients apart passes them apart: color_grad_channels = C - 1 planes behind dL_dout_color and the
     * last channel's plane behind dL_dout_last, or NULL when that channel did not reach the loss (color_refinement:
     * RGB only, train_gaussians.py:283-285) — the backward then skips the channel altogether.  0 = all C planes are
     * behind dL_dout_color (the plain call).  Wider tables ([rgb | features | kp_score]): any g in [1, C) — the first g
     * planes behind dL_dout_color, the last channel behind dL_dout_last, the channels in between without a gradient
     * (their planes are neither read nor built).  One value per launch. */
    const float* dL_dout_last;  /* [1,H,W] or NULL */
    int32_t color_grad_channels; /* 0 (= C), or g in [1, C) */
} splatraster_window_view;

size_t splatraster_window_geometry_bytes(int32_t P, int32_t n_views);
size_t splatraster_window_binning_bytes(int32_t P, int32_t n_views, int64_t R_total, int32_t width, int32_t height,
                                        int32_t channels);
size_t splatraster_window_image_bytes(int32_t width, int32_t height, int32_t n_views);

/* Stage 1: num_rendered[v] = tile instances of view v (one stream synchronisation for the whole window). */
int splatraster_forward_window_geometry(const splatraster_settings* s, int32_t n_views,
                                        const splatraster_window_view* views, int32_t P,
                                        const float* means3D, const float* opacities, const float* scales,
                                        const float* rotations, const float* cov3D_precomp, void* geometry,
                                        int64_t* num_rendered /* [n_views] */, void* stream);
/* Stage 2: `binning` holds splatraster_window_binning_bytes(P, n_views, sum(num_rendered), W, H, C) bytes. */
int splatraster_forward_window_render(const splatraster_settings* s, int32_t n_views,
                                      const splatraster_window_view* views, int32_t P,
                                      const int64_t* num_rendered, const float* bg, const float* colors_precomp,
                                      void* geometry, void* binning, void* image, void* stream);
/* Backward of the whole window: the parameter gradients are the SUM over the views (written once, overwritten),
 * dL_dmeans2D per view.  `bg`: the background the forward was given (NULL = zeros) — the back-to-front walk starts every pixel
 * at A = bg . g - g_A (round 4; rounds 1-3 took the background's share from the forward's colour planes, which the backward
 * no longer reads). */
int splatraster_backward_window(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                int32_t P, const int64_t* num_rendered, const float* bg, const float* means3D,
                                const float* colors_precomp, const float* scales, const float* rotations,
                                const float* cov3D_precomp, void* geometry, const void* binning, const void* image,
                                float* dL_dmeans3D,   /* [P,3] */
                                float* dL_dcolors,    /* [P,C] */
                                float* dL_dopacities, /* [P,1] */
                                float* dL_dscales,    /* [P,3] or NULL */
                                float* dL_drotations, /* [P,4] or NULL */
                                float* dL_dcov3D,     /* [P,6] or NULL */
                                void* stream);

/* Camera gradients of the n_views <= 8 views of a window, and nothing per Gaussian (pose refinement of a window of query frames
 * against a frozen map): the accumulator fill and the compositing backward of splatraster_backward_window (the
 * deterministic debug mode included), then ONE kernel with a thread per (view, Gaussian) that reduces the 27 partial sums of
 * every view — per wave, per block, one atomic per value and block into one of the view's replicated sets, the view's last block
 * (a ticket; no block waits for another) writes the view's outputs.  dL_dviewmatrix / dL_dprojmatrix [n_views,4,4] and
 * dL_dcampos [n_views,3] (may be NULL; zeros: a window has precomputed colours only) are written in full, zeros for a view that
 * sees nothing and when P == 0.  views[v].dL_dmeans2D is not written and may be NULL.  `workspace`: device memory of
 * splatraster_window_camera_workspace_bytes(n_views) bytes (0 for n_views outside 1 .. 8), zeroed by this call on `stream`.
 * n_views outside 1 .. 8 or a NULL required pointer: SPLATRASTER_ERR_BAD_ARG before any launch.  No host synchronisation. */
size_t splatraster_window_camera_workspace_bytes(int32_t n_views);
int splatraster_backward_window_cameras(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                        int32_t P, const int64_t* num_rendered, const float* bg, const float* means3D,
                                        const float* colors_precomp, const float* scales, const float* rotations,
                                        const float* cov3D_precomp, void* geometry, const void* binning, const void* image,
                                        void* workspace,
                                        float* dL_dviewmatrix, /* [n_views,4,4] */
                                        float* dL_dprojmatrix, /* [n_views,4,4] */
                                        float* dL_dcampos,     /* [n_views,3] or NULL */
                                        void* stream);

/* Parameter gradients AND camera gradients of the n_views <= 8 views of a window in one launch sequence (key-frame poses
 * optimised together with the map over a window): ONE accumulator fill and ONE compositing backward (the
 * deterministic debug mode and the compact payload stream included), the colour gather / copy of splatraster_backward_window,
 * then ONE per-Gaussian kernel that reads every (view, Gaussian) row once, sums the views' parameter gradients in view order —
 * the outputs of splatraster_backward_window, views[v].dL_dmeans2D included — and reduces the 27 camera partial sums of every view
 * the way splatraster_backward_window_cameras does (replicated sets, one ticket per view; no block waits for another).  The
 * argument rules are those of the two calls together; `workspace` and the camera outputs are that call's: [n_views,4,4],
 * [n_views,4,4] and [n_views,3] (may be NULL; zeros), written in full, zeros for a view that sees nothing and when P == 0.
 * n_views outside 1 .. 8 or a NULL required pointer: SPLATRASTER_ERR_BAD_ARG before any launch.  No host synchronisation.  For
 * n_views == 1 the results are those of splatraster_backward with its three camera outputs, up to float summation order.
 * Precomputed colours only, and no raw-parameter variant: splatraster_backward_window_raw returns no camera gradient. */
int splatraster_backward_window_joint(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                      int32_t P, const int64_t* num_rendered, const float* bg, const float* means3D,
                                      const float* colors_precomp, const float* scales, const float* rotations,
                                      const float* cov3D_precomp, void* geometry, const void* binning, const void* image,
                                      float* dL_dmeans3D,   /* [P,3] */
                                      float* dL_dcolors,    /* [P,C] */
                                      float* dL_dopacities, /* [P,1] */
                                      float* dL_dscales,    /* [P,3] or NULL */
                                      float* dL_drotations, /* [P,4] or NULL */
                                      float* dL_dcov3D,     /* [P,6] or NULL */
                                      void* workspace,      /* splatraster_window_camera_workspace_bytes(n_views), zeroed by the call */
                                      float* dL_dviewmatrix, /* [n_views,4,4] */
                                      float* dL_dprojmatrix, /* [n_views,4,4] */
                                      float* dL_dcampos,     /* [n_views,3] or NULL; zeros */
                                      void* stream);

/* The same backward, writing the gradients of SplatLoc's RAW parameters directly (SH degree 0, scales + rotations; what
 * gaussian_model.py:78-105 and gaussian_renderer/__init__.py:84-102 put between the optimiser tensors and the rasterizer call):
 *   scales = exp(scaling), rotations = normalize(rotation), opacities = sigmoid(opacity),
 *   colors_precomp = [clamp_min(C0 f_dc + 0.5, 0) | extra]                                       (C = 3 + extra_channels)
 * The chain through these activations and the sum of the accumulator rows' colour columns run inside the per-Gaussian
 * backward kernel: no dL/dcolors / dL/dopacities / dL/dscales / dL/drotations tensors, no second pass over them.  `scales`,
 * `rotations`, `colors_precomp` are the ACTIVATED tensors the forward was given; results are bit-identical to
 * splatraster_backward_window followed by splatraster_activate_backward.  extra_channels <= 1 (C <= 4: the accumulator rows' colour
 * columns share the 64-byte line of the moments the kernel reads anyway); wider layouts: SPLATRASTER_ERR_UNSUPPORTED — use the plain call. */
/* Stage 1 of the window forward from the RAW parameters: the activations run inside the projection kernel, which uses the activated
 * values and writes them — `scales`, `rotations`, `opacities`, `colors` are OUTPUTS of this call (the render stage takes `colors` as
 * its colors_precomp, the backward `scales` / `rotations`) — bit-identical to splatraster_activate_forward followed by
 * splatraster_forward_window_geometry. */
typedef struct splatraster_raw_forward {
    const float* scaling;  /* [P,3] */
    const float* rotation; /* [P,4] */
    const float* opacity;  /* [P]   logits */
    const float* f_dc;     /* [P,3] */
    const float* extra;    /* [P,extra_channels] or NULL */
    int32_t extra_channels;
    float* scales;         /* [P,3]   out */
    float* rotations;      /* [P,4]   out */
    float* opacities;      /* [P]     out */
    float* colors;         /* [P,3 + extra_channels] out */
} splatraster_raw_forward;
int splatraster_forward_window_geometry_raw(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                            int32_t P, const float* means3D, const splatraster_raw_forward* raw, void* geometry,
                                            int64_t* num_rendered /* [n_views] */, void* stream);

typedef struct splatraster_raw_params {
    const float* scaling;  /* [P,3] */
    const float* rotation; /* [P,4] */
    const float* opacity;  /* [P]   logits */
    const float* f_dc;     /* [P,3] */
    int32_t extra_channels;
    float* dL_dscaling;    /* [P,3] */
    float* dL_drotation;   /* [P,4] */
    float* dL_dopacity;    /* [P]   */
    float* dL_df_dc;       /* [P,3] */
    float* dL_dextra;      /* [P,extra_channels] or NULL */
    /* optional (NULL: none): SplatLoc.map's isotropic regulariser (train_gaussians.py:221-228; splatraster_isotropic_loss's row_grad and
     * out) adds reg_weight * reg_out[1] * reg_row_grad[i] to dL/dscales[i, :] before the chain through exp */
    const float* reg_row_grad; /* [P] */
    const float* reg_out;      /* [2] (device) */
    float reg_weight;
} splatraster_raw_params;
int splatraster_backward_window_raw(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                    int32_t P, const int64_t* num_rendered, const float* bg, const float* means3D,
                                    const float* colors_precomp, const float* scales, const float* rotations, void* geometry,
                                    const void* binning, const void* image, const splatraster_raw_params* raw,
                                    float* dL_dmeans3D /* [P,3] */, void* stream);

/* ---- bounded window forward: no host wait for the instance count ------------------------------------------------------
 * splatraster_forward_window_geometry stops the host until the instance count R is known, because the caller sizes `binning`
 * by it.  The bounded calls take a `binning` of splatraster_window_binning_bytes(P, n_views, capacity, W, H, C) bytes instead, run
 * geometry and render as ONE launch sequence, return no count, wait on no event and read nothing on the host that this frame
 * writes (the front end's wide-list hint word is a hint from earlier frames).  R stays on the device.  A frame with
 * R <= capacity is bit-identical to the two-stage forward (every output, point_list[:R], the range table, n_contrib, final_T).
 * A frame that does not fit writes no key, no list, no payload word; its range table is all [0, 0), it renders the background,
 * its backward yields zero gradients and nothing beyond `capacity` elements of any per-instance array is touched; the sequence
 * records itself in the status block.
 *
 * Status block (64 bytes, owned by the library; one per optimisation loop).  `overflow` is STICKY: once set, every later bounded
 * sequence with this status has an effective capacity of 0 (it renders background, whatever its own capacity) and every gated
 * Adam launch (splatraster_adam_step_gated) returns without touching anything, until splatraster_bounded_status_clear.  A loop
 * can therefore run ahead of the device: when it later reads `overflow`, nothing has changed since the parameters sequence
 * `first_tag` started from; it synchronises once, grows `binning` to hold `first_total`, clears the status and replays from
 * `first_tag`.  splatraster_bounded_status_read copies the host-mapped mirror and never synchronises: its fields are those of
 * some recent moment each, copied in this order: last_tag, then overflow, then the rest.  Every sequence in front of `last_tag`
 * has finished, so overflow == 0 in the same copy says that none of THEM overflowed (the sequence `last_tag` itself still
 * may).  A set flag is a hint until it is read again behind a stream synchronisation, which gives the consistent record.
 * splatraster_bounded_status_clear is a kernel in stream order and also zeroes the mirror from the host at once, so a caller
 * that has synchronised the stream reads a clear block immediately.
 *
 * Binned front end only (small and medium frames — the host-bound ones; the radix front end sizes its sort grids by R on the
 * host): where the two-stage forward would take the radix front end (and for P == 0) the bounded calls return
 * SPLATRASTER_ERR_UNSUPPORTED before any launch.  0 <= capacity < 2^31.
 *
 * Backward of a bounded frame: splatraster_backward_window, _raw, _joint and _cameras use num_rendered only to lay out `binning`
 * (and skip the compositing launch when it sums to 0); pass num_rendered = {capacity, 0, ...}. */
typedef struct splatraster_bounded_status {
    uint32_t total;       /* R of the last bounded sequence (saturated at 2^32 - 1) */
    uint32_t overflow;    /* 0 or 1, sticky */
    uint32_t first_tag;   /* tag of the first sequence that did not fit (valid while overflow == 1) */
    uint32_t first_total; /* that sequence's R */
    uint32_t last_tag;    /* tag of the last bounded sequence */
    uint32_t reserved[11];
} splatraster_bounded_status;
int splatraster_bounded_status_create(void** handle);          /* on the current device; the block starts cleared */
int splatraster_bounded_status_destroy(void* handle);          /* the caller has synchronised every stream that used it */
int splatraster_bounded_status_read(const void* handle, splatraster_bounded_status* out);   /* host read of the mirror: no synchronisation */
int splatraster_bounded_status_clear(void* handle, void* stream);                           /* stream-ordered */
/* 1 when the bounded calls accept this shape under the present settings (the two-stage forward would take the binned front end), else 0 */
int splatraster_forward_window_bounded_supported(int32_t P, int32_t n_views, int32_t width, int32_t height);
int splatraster_forward_window_bounded(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                       int32_t P, const float* means3D, const float* opacities, const float* scales,
                                       const float* rotations, const float* cov3D_precomp, const float* bg,
                                       const float* colors_precomp, void* geometry, void* binning, void* image,
                                       int64_t capacity, uint32_t tag, void* status, void* stream);
/* (raw-parameter mode: `raw->colors`, an output of this call, is the colour table the render stage reads) */
int splatraster_forward_window_bounded_raw(const splatraster_settings* s, int32_t n_views, const splatraster_window_view* views,
                                           int32_t P, const float* means3D, const splatraster_raw_forward* raw, const float* bg,
                                           void* geometry, void* binning, void* image, int64_t capacity, uint32_t tag,
                                           void* status, void* stream);

/* ---- auxiliary entry points ---------------------------------------------------------- */

/* present[i] = 1 when Gaussian i passes the near-plane test (view-space z > 0.2).
 * Mirrors GaussianRasterizer.markVisible of the extension's Python wrapper. */
int splatraster_mark_visible(int32_t P, const float* means3D, const float* viewmatrix,
                             const float* projmatrix, uint8_t* present, void* stream);

/* Debug / test introspection: byte offsets of the arrays inside the opaque buffers. */
typedef struct splatraster_geometry_layout {
    size_t rec0;          /* 32-byte records, stride 32: float4 at rec0 + 32 i = pixel x, pixel y, view depth, radius (float, 0 = culled) */
    size_t rec1;          /* = rec0 + 16: float4 at rec1 + 32 i = conic a, b, c, opacity */
    size_t tiles_touched; /* uint32[P] (original index order) */
    size_t depth_order;   /* uint32[P]: Gaussian indices (bits 0..23; bits 24..31 = min(tiles_touched, 255)), stable-sorted by depth bits (culled last) */
    size_t offsets;       /* uint32[P]: inclusive scan of tiles_touched in depth_order */
    size_t rgb;           /* float[3P]: SH colours (only with shs) */
    size_t clamped;       /* uint8[3P]: SH clamp flags (only with shs) */
    size_t total;
} splatraster_geometry_layout;
typedef struct splatraster_binning_layout {
    size_t point_list; /* uint32[R]: Gaussian index per instance, sorted by (tile, depth, index) */
    size_t tile_list;  /* uint32[R]: tile id per sorted instance */
    size_t ranges;     /* uint32[2*tiles]: [start, end) per tile */
    size_t total;
} splatraster_binning_layout;
typedef struct splatraster_image_layout {
    size_t final_T;   /* float[H*W] */
    size_t n_contrib; /* uint32[H*W] */
    size_t total;     /* (behind the two planes, at 2 * n_contrib and 3 * n_contrib: uint32[H*W] n_contrib_c and uint32[2*tiles] cranges,
                       *  written by forwards that stream the compact payload; splatraster_debug_set_payload_compact) */
} splatraster_image_layout;
int splatraster_get_geometry_layout(int32_t P, splatraster_geometry_layout* out);
int splatraster_get_binning_layout(int32_t P, int64_t R, int32_t width, int32_t height, int32_t channels,
                                   splatraster_binning_layout* out);
int splatraster_get_image_layout(int32_t width, int32_t height, splatraster_image_layout* out);
/* the same for the buffers of a window: arrays indexed by Gaussian hold n_views * P rows (row v * P + i), the
 * instance lists hold rows and GLOBAL tile ids v * tiles + t, `ranges` has 2 * n_views * tiles entries and the
 * per-pixel planes n_views * H * W */
int splatraster_get_window_geometry_layout(int32_t P, int32_t n_views, splatraster_geometry_layout* out);
int splatraster_get_window_binning_layout(int32_t P, int32_t n_views, int64_t R_total, int32_t width, int32_t height,
                                          int32_t channels, splatraster_binning_layout* out);
int splatraster_get_window_image_layout(int32_t width, int32_t height, int32_t n_views, splatraster_image_layout* out);

/* Stable LSD radix sort of (key, value) pairs on key bits [0, key_bits); exposed so the
 * sort can be tested and timed on its own.  tmp must hold splatraster_sort_tmp_bytes(n).  The sort moves whole 8-bit
 * digits: it orders by bits [0, 8 * ceil(key_bits / 8)), and key bits at or above that ride along unsorted. */
size_t splatraster_sort_tmp_bytes(int64_t n);
int splatraster_sort_pairs_u32(int64_t n, uint32_t* keys, uint32_t* vals, int32_t key_bits,
                               void* tmp, void* stream);

/* ---- test hooks of the scan and the sort (tests/test_gpu_scan_sort_edges.py); no product code calls them ---- */

/* Host only, no HIP call: the form a sort of n keys takes.  0 nothing to do (n or key_bits 0), 1 one-sweep with 2048-key
 * tiles, 2 one-sweep with 4096-key tiles, 3 histogram / scan / scatter kernels per pass, 4 the same on uint16_t keys
 * (keys16 != 0: the answer for splatraster_debug_sort_pairs_k16); +8 when the table scan of a pass takes three kernels.
 * -1: arguments the sort itself refuses (n < 0, key_bits outside [0, 32], keys16 where the sort has no uint16_t form). */
int splatraster_debug_sort_path(int64_t n, int32_t key_bits, int32_t keys16);
/* Host only: the form a scan of n words takes.  0 nothing to do, 1 one-pass decoupled look-back, 2 three kernels; -1: n < 0. */
int splatraster_debug_scan_path(int64_t n);
/* bytes of `tmp` for splatraster_debug_scan_u32 */
size_t splatraster_debug_scan_tmp_bytes(int64_t n);
/* The device-wide prefix sum that every stage uses.  out[i] = sum of v[0..i] (inclusive) or v[0..i) (exclusive) mod 2^32,
 * *total (optional) the exact 64-bit sum; a tile of 2048 consecutive values must sum below 2^32.  v[i] = in[i], or with `perm`
 * in[perm[i] & 0xFFFFFF], where bits 24..31 of perm[i] hold min(in[row], 255) and rows are < n (the packed depth order of the
 * rasterizer).  in == out is allowed without `perm`; `exclusive` requires it, and takes no perm and no span_owner.  span_owner
 * (inclusive only, span > 0): for every b < span_cap with b * span < total, span_owner[b] = the i with
 * out[i - 1] <= b * span < out[i]; other entries are not written, and the three-kernel form writes none.  The call clears the
 * state it needs in `tmp` itself.  Bad arguments are refused before any HIP call. */
int splatraster_debug_scan_u32(int64_t n, const uint32_t* in, const uint32_t* perm, uint32_t* out, uint64_t* total,
                               int32_t exclusive, uint32_t* span_owner, uint32_t span, uint32_t span_cap, void* tmp,
                               void* stream);
/* splatraster_sort_pairs_u32 in the uint16_t form of the tile sort: on entry the first half of `keys` holds n uint16_t keys,
 * on return `keys` holds the n sorted keys as uint32_t.  key_bits <= 16 and a size at which splatraster_debug_sort_path(n,
 * key_bits, 1) is not -1, else SPLATRASTER_ERR_BAD_ARG.  tmp must hold splatraster_sort_tmp_bytes(n). */
int splatraster_debug_sort_pairs_k16(int64_t n, uint32_t* keys, uint32_t* vals, int32_t key_bits, void* tmp, void* stream);

/* ---- parameter activations + SH / feature packing -------------------- */

/* The elementwise work between SplatLoc's raw optimiser tensors and the rasterizer call, as one
 * kernel each way.  Replaces, with identical results:
 *   scales    = exp(_scaling)             gaussian_model.py:78-80; an isotropic [P,1] model is
 *                                         repeated to 3 columns (gaussian_renderer/__init__.py:73-76)
 *   rotations = normalize(_rotation)      gaussian_model.py:82-84 (eps 1e-12)
 *   opacities = sigmoid(_opacity)         gaussian_model.py:101-103
 *   colors    = cat(clamp_min(eval_sh(active_sh_degree, cat(f_dc, f_rest), normalize(xyz - campos))
 *                             + 0.5, 0), extra)
 *                                         gaussian_renderer/__init__.py:84-102, sh_utils.py:55-118
 * sh_coeffs = (max_sh_degree + 1)^2 >= (active_sh_degree + 1)^2, active_sh_degree in [0, 3];
 * f_dc is [P,1,3], f_rest [P,sh_coeffs-1,3] (NULL when sh_coeffs == 1); scaling_cols is 3 or 1;
 * extra is [P,extras] (SplatLoc: the kp_score column) or NULL with extras == 0. */
int splatraster_activate_forward(int32_t P, int32_t sh_coeffs, int32_t active_sh_degree,
                                 int32_t scaling_cols, int32_t extras,
                                 const float* xyz, const float* f_dc, const float* f_rest,
                                 const float* scaling, const float* rotation, const float* opacity,
                                 const float* extra, const float* campos,
                                 float* scales /* [P,3] */, float* rotations /* [P,4] */,
                                 float* opacities /* [P,1] */, float* colors /* [P,3+extras] */,
                                 void* stream);
/* Gradients w.r.t. the raw tensors given dL/d(scales, rotations, opacities, colors); recomputes
 * the activations from the raw inputs (nothing is saved by the forward).  dL_dxyz receives ONLY
 * the view-direction term of the SH colour (zero at degree 0; the rasterizer's own dL/dmeans3D
 * is added by the caller) and may be NULL; dL_df_rest / dL_dextra may be NULL when empty.
 * The camera centre gets no gradient. */
int splatraster_activate_backward(int32_t P, int32_t sh_coeffs, int32_t active_sh_degree,
                                  int32_t scaling_cols, int32_t extras,
                                  const float* xyz, const float* f_dc, const float* f_rest,
                                  const float* scaling, const float* rotation, const float* opacity,
                                  const float* campos,
                                  const float* dL_dscales, const float* dL_drotations,
                                  const float* dL_dopacities, const float* dL_dcolors,
                                  float* dL_dxyz, float* dL_df_dc, float* dL_df_rest, float* dL_dscaling,
                                  float* dL_drotation, float* dL_dopacity, float* dL_dextra, void* stream);

/* Per-view densification statistics, in place: for every Gaussian with
 * radii > 0:  max_radii2D = max(max_radii2D, radii) (train_gaussians.py:240-244),
 * xyz_gradient_accum += ||viewspace_grad[:2]||, denom += 1 (gaussian_model.py:677-679). */
int splatraster_densification_stats(int32_t P, const float* viewspace_grad /* [P,3] */, const int32_t* radii,
                                    float* xyz_gradient_accum /* [P,1] */, float* denom /* [P,1] */,
                                    float* max_radii2D /* [P] */, void* stream);
/* The same for the n_views <= SPLATRASTER_MAX_WINDOW_VIEWS views of a window in ONE launch, in view order (host arrays
 * of device pointers).  xyz_gradient_accum == denom == NULL: only max_radii2D is updated — the statistics line of
 * SplatLoc.color_refinement (train_gaussians.py:293-294); viewspace_grads may then be NULL. */
int splatraster_densification_stats_window(int32_t P, int32_t n_views, const float* const* viewspace_grads,
                                           const int32_t* const* radii, float* xyz_gradient_accum, float* denom,
                                           float* max_radii2D, void* stream);

/* ---- densify / clone / split / prune + Adam over the parameter groups -------- */

/* The raw (pre-activation) parameter tensors of the reference's GaussianModel, in the group order of
 * GaussianModel.training_setup (gaussian_model.py:254-297): row-major [P, width], fp32, device memory.
 * The same struct carries the Adam moments (exp_avg / exp_avg_sq of each group; NULL = the group has no
 * optimizer state — SplatLoc's marker never receives a gradient in map()). */
typedef struct splatraster_model {
    int32_t P;
    int32_t f_rest_width;  /* 3 * ((max_sh_degree + 1)^2 - 1); 0 in SplatLoc (f_rest is [P, 0, 3]) */
    int32_t marker_width;  /* 1 (0 = absent) */
    int32_t kp_width;      /* columns of _kp_score (1 in SplatLoc) */
    int32_t scaling_width; /* 3, or 1 for an isotropic model */
    float* xyz;            /* [P,3] */
    float* f_dc;           /* [P,1,3] */
    float* f_rest;         /* [P,f_rest_width] */
    float* opacity;        /* [P,1]  logit */
    float* marker;         /* [P,marker_width] */
    float* kp_score;       /* [P,kp_width] */
    float* scaling;        /* [P,scaling_width]  log */
    float* rotation;       /* [P,4]  un-normalised quaternion (w,x,y,z) */
} splatraster_model;

/* GaussianModel.densify_and_prune(max_grad, min_opacity, extent, max_screen_size)
 * (gaussian_model.py:655-675 with densify_and_clone :632-653, densify_and_split :590-630, prune_points
 * :510-526 and the optimizer surgery :477-587) as one compaction:
 *   plan   decides clone / split / prune per row from xyz_gradient_accum / denom, the scales, opacity and
 *          (primitive_reg) the marker, scans the keep flags and returns the new row count (one
 *          device->host read: it sizes the caller's allocations);
 *   apply  writes the re-sized parameter tensors and Adam moments in the reference's row order
 *          [originals | clones | split children copy 0 | copy 1]; new rows get zero moments.
 * The caller zeroes the statistics afterwards (densification_postfix resets xyz_gradient_accum, denom
 * AND max_radii2D, gaussian_model.py:585-587 — which is why max_screen_size can only act as the on/off
 * switch of the world-size prune: use_size_prune = (max_screen_size != 0)).
 * Split children: xyz + R(q/|q|) (z * exp(scaling)), z ~ N(0, I).  unit_noise [2,P,3] supplies z by
 * (copy, source row) when given (tests: the recorded table of tests/golden/densify.npz); otherwise z is
 * drawn from Philox4x32-10 keyed by (seed, draw_id, source row, copy), so data-parallel replicas that pass
 * the same (seed, draw_id) split identically without a broadcast. */
size_t splatraster_densify_workspace_bytes(int32_t P);
int splatraster_densify_plan(const splatraster_model* model, const float* xyz_gradient_accum /* [P,1] */,
                             const float* denom /* [P,1] */, float max_grad, float min_opacity, float extent,
                             float percent_dense, int32_t use_size_prune, int32_t primitive_reg, void* workspace,
                             int32_t* new_P, void* stream);
/* The same plan from the two FINISHED size thresholds.  The reference compares float32 scales with the Python
 * doubles `percent_dense * extent` and `0.1 * extent`, i.e. with the float32 rounding of a DOUBLE product; the
 * float32 product splatraster_densify_plan forms from its float arguments differs from that by one ulp for about
 * a quarter of all extents, which moves a Gaussian whose largest scale sits on the threshold from split to clone.
 * size_split = (float)(percent_dense * extent), size_prune = (float)(0.1 * extent), both products in double. */
int splatraster_densify_plan_thresholds(const splatraster_model* model, const float* xyz_gradient_accum /* [P,1] */,
                                        const float* denom /* [P,1] */, float max_grad, float min_opacity,
                                        float size_split, float size_prune, int32_t use_size_prune,
                                        int32_t primitive_reg, void* workspace, int32_t* new_P, void* stream);
int splatraster_densify_apply(const splatraster_model* model, const splatraster_model* exp_avg /* or NULL */,
                              const splatraster_model* exp_avg_sq /* or NULL */, const float* unit_noise /* or NULL */,
                              uint64_t seed, uint64_t draw_id, void* workspace /* from plan */, int32_t new_P,
                              splatraster_model* out_model, splatraster_model* out_exp_avg,
                              splatraster_model* out_exp_avg_sq, int32_t* source_row /* [new_P] or NULL */,
                              int32_t* source_kind /* [new_P] or NULL: 0 original, 1 clone, 2 / 3 split child */,
                              void* stream);

/* Key-frame insertion, GaussianModel.extend_from_pcd -> densification_postfix -> cat_tensors_to_optimizer
 * (gaussian_model.py:222-241, :528-587; once per key-frame, train_gaussians.py:173-177): the `extra->P` new rows are
 * appended to the 8 parameter tensors and ZERO rows to the Adam moments of every group that has state — ONE launch
 * instead of 24 torch.cat + 16 zeros_like.  out_* hold model->P + extra->P rows; exp_avg / exp_avg_sq (and their
 * outputs) may be NULL, or carry NULL members for groups without state.  The caller resets the densification
 * statistics, as densification_postfix does (:585-587). */
int splatraster_model_append(const splatraster_model* model, const splatraster_model* exp_avg /* or NULL */,
                             const splatraster_model* exp_avg_sq /* or NULL */, const splatraster_model* extra,
                             splatraster_model* out_model, splatraster_model* out_exp_avg,
                             splatraster_model* out_exp_avg_sq, void* stream);

/* One torch.optim.Adam step (no weight decay, no amsgrad: gaussian_model.py:287) over up to 16 parameter
 * groups in ONE launch.  `step` is the group's step count AFTER this step (>= 1): the bias corrections
 * and 1 - beta are formed on the host in double like torch does (hence the double betas).  A group with grad == NULL is skipped (torch
 * semantics: no state is touched).  row_gate (or NULL): per-ROW gate values; rows with
 * gate > row_gate_threshold see a ZERO gradient — the key-primitive freeze `get_xyz.grad[key_mask] = 0`
 * of train_gaussians.py:231-234 (gate = the marker, threshold 0.005) without its .cpu() sync. */
typedef struct splatraster_adam_group {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    const float* row_gate;
    int64_t numel;
    int32_t row_width; /* elements per row (for row_gate) */
    float lr;
    double step;
} splatraster_adam_group;
int splatraster_adam_step(int32_t n_groups, const splatraster_adam_group* groups, double beta1, double beta2, double eps,
                          float row_gate_threshold, void* stream);
/* splatraster_adam_step and, in the same launch, the statistics line of SplatLoc.color_refinement (train_gaussians.py:293-294):
 * max_radii2D[i] = max(max_radii2D[i], radii[i]) wherever radii[i] > 0 (radii: the int32 [P] output of the frame's forward).
 * n_groups may be 0 (only the statistics). */
int splatraster_adam_step_radii(int32_t n_groups, const splatraster_adam_group* groups, double beta1, double beta2, double eps,
                                float row_gate_threshold, int32_t P, const int32_t* radii, float* max_radii2D, void* stream);

/* The two launches above behind a bounded status block (splatraster_bounded_status_create): while its `overflow` word is set every
 * block returns before it touches a parameter, a moment or max_radii2D; with the word clear the results are bit-identical to the
 * ungated calls.  The word is read on the device, in stream order: no host synchronisation. */
int splatraster_adam_step_gated(int32_t n_groups, const splatraster_adam_group* groups, double beta1, double beta2, double eps,
                                float row_gate_threshold, const void* status, void* stream);
int splatraster_adam_step_radii_gated(int32_t n_groups, const splatraster_adam_group* groups, double beta1, double beta2, double eps,
                                      float row_gate_threshold, int32_t P, const int32_t* radii, float* max_radii2D,
                                      const void* status, void* stream);

/* Isotropic scale regulariser of SplatLoc.map (train_gaussians.py:222-228):
 *   mask = marker > 0.005;  loss = mean_{mask} | mean_k scaling[i,k] / (0.02 (1 - marker_i)) - 1 |
 * scaling is the ACTIVATED [P, scaling_cols] tensor.  row_grad[i] = d|x_i - 1| / d scaling[i,k] (equal for
 * every k; 0 outside the mask); out[0] = loss, out[1] = 1 / |mask| (both 0 for an empty mask), so
 * d loss / d scaling[i,k] = out[1] * row_grad[i].  No host synchronisation. */
size_t splatraster_isotropic_loss_workspace_bytes(int32_t P);
int splatraster_isotropic_loss(int32_t P, int32_t scaling_cols, const float* scaling, const float* marker,
                               float* row_grad /* [P] */, float* out /* [2] */, void* workspace, void* stream);

/* ---- per-view mapping loss + gradient ---------------------------------- */

/* loss = get_loss_mapping(config, image, depth, viewpoint, opacity) (utils/utils.py:55-82; exposure
 * affine exp(a) image + b unless exposure == NULL, i.e. initialization=True)
 *      + get_loss_marker(config, marker, viewpoint.kp_score) (train_gaussians.py:38-42),
 * the per-view sum of train_gaussians.py:217-218, and its gradient w.r.t. the rendered buffers,
 * in one pass.  image / g_image are 3 planes of H*W floats with plane stride H*W (they may point
 * into a [C,H,W] render and its gradient), marker / g_marker one plane.  kp is the float32
 * key-point score map used as the (soft) BCE target, `gt.view(-1).float()` at train_gaussians.py:40
 * (a bool mask is passed as 0.0 / 1.0).  out[4] = { rgbd loss, marker loss, dL/dexposure_a, dL/dexposure_b } (device).
 * pixels <= 0: SPLATRASTER_ERR_BAD_ARG, and a workspace size of 0 (as the other loss stages answer a non-positive size). */
size_t splatraster_mapping_loss_workspace_bytes(int32_t pixels);
int splatraster_mapping_loss(int32_t pixels, const float* image, const float* depth, const float* marker,
                             const float* gt_image, const float* gt_depth, const float* kp,
                             float rgb_boundary_threshold, const float* exposure /* [2] = a, b or NULL */,
                             float* g_image, float* g_depth, float* g_marker, float* out /* [4] */,
                             void* workspace, void* stream);

/* The same for the n_views <= SPLATRASTER_MAX_WINDOW_VIEWS views of a window (the loop train_gaussians.py:195-219 sums the
 * per-view losses with weight 1) in ONE launch pair: `views` is a HOST array of per-view device pointers, out is [n_views][4]
 * (device), workspace n_views x splatraster_mapping_loss_workspace_bytes(pixels).  Per-view results are bit-identical to
 * n_views calls of splatraster_mapping_loss (same blocks, same summation order). */
typedef struct splatraster_loss_view {
    const float* image;    /* 3 planes */
    const float* depth;
    const float* marker;
    const float* gt_image; /* 3 planes */
    const float* gt_depth;
    const float* kp;
    const float* exposure; /* [2] = a, b or NULL */
    float* g_image;        /* 3 planes */
    float* g_depth;
    float* g_marker;
} splatraster_loss_view;
int splatraster_mapping_loss_window(int32_t n_views, int32_t pixels, const splatraster_loss_view* views,
                                    float rgb_boundary_threshold, float* out /* [n_views][4] */, void* workspace,
                                    void* stream);

/* Colour-refinement loss (train_gaussians.py:283-285):
 *   loss = (1 - lambda_dssim) l1_loss(image, gt) + lambda_dssim (1 - ssim(image, gt))
 * with l1_loss / ssim of gaussian_splatting/utils/loss_utils.py:21-22, 42-102 (11x11 Gaussian
 * window, sigma 1.5, zero padding), and its gradient w.r.t. image.  image, gt, g_image: [C,H,W].
 * out[3] = { l1, ssim, loss } (device). */
size_t splatraster_refinement_loss_workspace_bytes(int32_t channels, int32_t height, int32_t width);
int splatraster_refinement_loss(int32_t channels, int32_t height, int32_t width, float lambda_dssim,
                                const float* image, const float* gt, float* g_image, float* out /* [3] */,
                                void* workspace, void* stream);

/* Per-frame metrics of eval_rendering (utils/eval_utils.py:45-52): image = clamp(render, 0, 1), mask = gt > 0 per element,
 *   psnr = 20 log10(1 / sqrt(mean_{mask} (image - gt)^2))   (gaussian_splatting/utils/image_utils.py:19-21)
 *   ssim = ssim(image, gt)                                  (loss_utils.py:61-102)
 * render, gt: [C,H,W] (render is clamped on load; nothing is written back).  out[4] = { psnr, ssim, masked mse, mask count }
 * (device).  LPIPS (a learned network, torchmetrics) is not part of this library. */
size_t splatraster_eval_metrics_workspace_bytes(int32_t channels, int32_t height, int32_t width);
int splatraster_eval_metrics(int32_t channels, int32_t height, int32_t width, const float* render, const float* gt,
                             float* out /* [4] */, void* workspace, void* stream);

/* ---- simple_knn._C.distCUDA2 (gaussian_model.py:206) ---------------------------------- */

size_t splatknn_workspace_bytes(int32_t N);
/* out[i] = mean of the squared distances from points[i] to its 3 nearest other points.  Exact: a tiled brute force below
 * 10 000 points, an exact uniform-grid search from there on (SplatLoc passes 5-20 k per key-frame) — same distance
 * arithmetic, bit-identical results.  No host synchronisation. */
int splatknn_dist2(int32_t N, const float* points /* [N,3] */, float* out /* [N] */,
                   void* workspace, void* stream);

/* test hook: point count from which splatknn_dist2 takes the grid search (< 0 restores the default 10 000) */
int splatknn_debug_set_grid_min(int32_t n);

/* ---- tinycudann.Encoding: multiresolution grid encoding (models/encoding.py:33-46) -------------------------------------
 * Restatement of tiny-cuda-nn's public grid-encoding definition.  Level l of L:
 *   scale_l = exp2f(l * log2f(per_level_scale)) * base_res - 1,  res_l = ceilf(scale_l) + 1          (f32, on the host, once)
 *   size_l  = next_multiple(res_l^D, 8) (at most 2^31 - 1 before rounding), then capped: Hash at 2^log2_T, Tiled at base_res^D,
 *             Dense not at all;  offset_l = sum of the sizes below l;  n_params = F * sum of all sizes
 *   params[(offset_l + index) * F + f]  (level-major table)
 * A point x [D] (not clamped to [0, 1]) at level l: pos = fmaf(scale_l, x_d, 0.5f), cell = (uint32)(int)floorf(pos),
 * frac = pos - floorf(pos); each of the 2^D corners is indexed densely (sum cell_d * res_l^d, stopping once the stride passes
 * size_l) or, for Hash when res_l^D > size_l, by XOR_d cell_d * {1, 2654435761, 805459861}_d; then % size_l.  The output row
 * of a point holds level l's F features in columns [l*F, l*F + F): the sum over corners of prod_d (frac_d | 1 - frac_d) *
 * corner feature.  D in {2, 3}, F in {1, 2, 4, 8}, 1 <= L <= 32, 1 <= log2_T <= 30, linear interpolation only. */
#define SPLATRASTER_GRID_MAX_LEVELS 32
#define SPLATRASTER_GRID_HASH 0
#define SPLATRASTER_GRID_DENSE 1
#define SPLATRASTER_GRID_TILED 2
typedef struct splatraster_grid_layout {
    int32_t n_dims;        /* D */
    int32_t n_levels;      /* L */
    int32_t n_features;    /* F per level */
    int32_t grid_type;     /* SPLATRASTER_GRID_* */
    uint32_t offset[SPLATRASTER_GRID_MAX_LEVELS];      /* in table entries of F floats */
    uint32_t size[SPLATRASTER_GRID_MAX_LEVELS];        /* entries of level l */
    uint32_t resolution[SPLATRASTER_GRID_MAX_LEVELS];  /* res_l */
    float scale[SPLATRASTER_GRID_MAX_LEVELS];          /* scale_l */
    int64_t n_params;      /* floats in the parameter table */
} splatraster_grid_layout;

/* Host only (never touches the GPU): fills `out` for the configuration; SPLATRASTER_ERR_UNSUPPORTED outside the limits above
 * or when the table would exceed 2^31 entries, SPLATRASTER_ERR_BAD_ARG for non-positive base_res / per_level_scale. */
int splatraster_grid_encoding_layout(int32_t n_dims, int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size,
                                     int32_t base_resolution, double per_level_scale, int32_t grid_type,
                                     splatraster_grid_layout* out);
/* out [N, L*F] = encoding of x [N, D].  `layout` as filled by splatraster_grid_encoding_layout (re-validated: its offsets must
 * be the running sum of its sizes); params [n_params].  params must be 16-byte aligned.  No host synchronisation. */
int splatraster_grid_encoding_forward(const splatraster_grid_layout* layout, int64_t N, const float* x, const float* params,
                                      float* out, void* stream);
/* Gradients of a loss L given dL_dout [N, L*F]: dL_dparams [n_params] (may be NULL) is ACCUMULATED with float atomics
 * (zero it first; the last bits depend on arrival order), dL_dx [N, D] (may be NULL) is written. */
int splatraster_grid_encoding_backward(const splatraster_grid_layout* layout, int64_t N, const float* x, const float* params,
                                       const float* dL_dout, float* dL_dparams, float* dL_dx, void* stream);

/* ---- FeatureDecoder: models/decoders.py:43-68 and the training step of train_decoder.py:20-25,48-51,64-78; INTEGRATION.md §19 ----
 * out[n] = f / |f|,  f = W_{n-1} relu(... relu(W_0 enc(xn)) ...),  xn = (float)((x - lo) / (hi - lo)) computed in f64 from the f64
 * (or exactly widened f32) point and rounded once; enc = the grid encoding above (bit-identical to
 * splatraster_grid_encoding_forward); W_l [dims[l+1], dims[l]] row-major f32 without bias (torch.nn.Linear.weight).  Every dot
 * product is an f32 fmaf chain from a zero accumulator with k ascending (v_mfma_f32_32x32x2_f32).  |f| = sqrtf(sum of squares), the
 * squares summed per block of 32 columns by a butterfly over lane distances 16, 8, 4, 2, 1 and the blocks' sums added in ascending
 * column order; the quotient is a division, so a zero row gives NaN as the reference does.
 * Supported shapes: the grid configurations above with dims[0] = L*F a multiple of 16 up to 64; 2 <= n_layers <= 8; one hidden width
 * dims[1] = ... = dims[n_layers-1] in {32, 64, 128}; dims[n_layers] a multiple of 32 up to 256.  Anything else:
 * SPLATRASTER_ERR_BAD_ARG, before any launch. */
#define SPLATRASTER_DECODER_MAX_LAYERS 8
typedef struct splatraster_decoder_layout {
    splatraster_grid_layout grid;
    double bound[3][2];    /* scene.bound: {lo, hi} per dimension (the first n_dims rows are read) */
    int32_t n_layers;      /* Linear layers */
    int32_t dims[SPLATRASTER_DECODER_MAX_LAYERS + 1];   /* dims[0] = L*F, dims[l+1] = rows of W_l */
} splatraster_decoder_layout;

/* Host only.  *workspace_bytes: the backward's workspace for N points (per-workgroup weight-gradient slabs, per-tile loss terms,
 * dL/d(encoded)); *activation_bytes: the activation record of a training forward over N points, floats in this order:
 * encoded [N, dims[0]], post-ReLU h_1 .. h_{n-1} [N, H] each, unnormalised f [N, O], |f| [N], xn [N, D].  Either may be NULL. */
int splatraster_decoder_workspace_bytes(const splatraster_decoder_layout* layout, int64_t N, size_t* workspace_bytes,
                                        size_t* activation_bytes);
/* out [N, O].  x [N, D] f32, or f64 when x_is_f64; table [grid.n_params]; weights: HOST array of n_layers device pointers.
 * activations: NULL (inference: nothing but `out` is written) or activation_bytes of device memory, filled for the backward.
 * table, out, activations and every weight must be 16-byte aligned.  One launch, no host synchronisation. */
int splatraster_decoder_forward(const splatraster_decoder_layout* layout, int64_t N, const void* x, int32_t x_is_f64,
                                const float* table, const float* const* weights, float* out, float* activations, void* stream);
/* Backward of the forward that filled `activations` (N >= 1).  Exactly one of dL_dout [N, O] and targets [N, O] is given.
 * With targets the loss is train_decoder.py's cos_loss, 1 - mean_i cos(out_i, t_i) with
 * cos = (y . t) / (max(|y|, 1e-8) max(|t|, 1e-8)) as torch.cosine_similarity defines it; *loss (device, may be NULL) receives it,
 * summed in a fixed order (per row: 8 ascending chains over O/8 columns, butterfly 1, 2, 4; rows of a 32-point tile ascending;
 * tiles in 256 strided ascending chains and a binary tree), and dL/dout is formed in the same pass.
 * dL_dweights [sum_l dims[l+1]*dims[l]] (layer 0 first, each laid out like its weight) is WRITTEN: per-workgroup partial sums in
 * the workspace, added in ascending workgroup order, so it is bit-reproducible run to run.  dL_dtable [grid.n_params] (may be
 * NULL) is ACCUMULATED by the float atomics of splatraster_grid_encoding_backward (zero it first; arrival-ordered).  dL_dx [N, D]
 * (may be NULL) is written, with respect to the NORMALISED point xn.  Three launches, no host synchronisation. */
int splatraster_decoder_backward(const splatraster_decoder_layout* layout, int64_t N, const float* table,
                                 const float* const* weights, const float* activations, const float* dL_dout, const float* targets,
                                 float* loss, float* dL_dweights, float* dL_dtable, float* dL_dx, void* workspace, void* stream);
/* One torch.optim.Adam step (no amsgrad) over both parameter groups of train_decoder.py:48-51 in one launch, `step` = 1 for the
 * first: g += weight_decay * p (weights only); m += (g - m)(1 - beta1); v = v beta2 + (1 - beta2) g g;
 * p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps).  Dense over the table (an entry with zero gradient
 * still moves through its momentum).  w_grad / w_m / w_v: flat, laid out as dL_dweights; t_*: [grid.n_params].  Every gradient
 * read is written back as zero, so the next backward needs no memset. */
int splatraster_decoder_adam(const splatraster_decoder_layout* layout, float* const* weights, float* w_grad, float* w_m, float* w_v,
                             float* table, float* t_grad, float* t_m, float* t_v, int64_t step, double lr_weights, double lr_table,
                             double beta1, double beta2, double eps_weights, double eps_table, double weight_decay, void* stream);

/* ---- landmark selection: utils/selection.py:91-157 (gaussian_selectition), INTEGRATION.md §16 ----------------------------
 * Scores.  Point p [N,3] against view i of w2c [M,4,4] (row-major world-to-camera) and K [3,3] (f64, row-major, HOST memory),
 * all arithmetic f64 from the f32 inputs, no FP contraction:
 *   pc = R_i p + t_i; visible iff !(pc.z < 0.01) and, with (u, v) = (K pc)_{0,1} / (K pc)_2, 0 < u < width, 0 < v < height
 *   d = depths[i, (int)v, (int)u] ([M, height, width] f32); diff = |pc.z - d| kept iff diff < 0.3 and d > 0.02
 *   depth_mean / depth_std (ddof 0) over the kept diffs, NaN when none was kept
 *   b = R_i^T (p - t_i) / |.|, H = mean over visible views of (I - b b^T), span = acos(clip(1 - 2 lmin/lmax, 0, 1)), 0 if none
 *   score = min(2, 0.05/mean) + min(2, 0.05/std) + span with python's min (NaN -> 2; a zero mean or std -> 2)
 * n_visible / n_depth [N] i32, the others [N] f64.  No host synchronisation. */
int splatraster_landmark_scores(int64_t N, int32_t M, const float* points, const float* w2c, const double* K,
                                const float* depths, int32_t width, int32_t height, int32_t* n_visible, int32_t* n_depth,
                                double* depth_mean, double* depth_std, double* span, double* score, void* stream);
/* device workspace of splatraster_landmark_select for N points and num landmarks */
size_t splatraster_landmark_workspace_bytes(int64_t N, int32_t num);
/* Greedy pick of `num` landmarks among points [N,3] (f32) by score [N] (f64), as the reference's loop: candidates walked by
 * score descending, ties the larger index first; rank 0 is taken; then passes at radius, radius/2, ...: a candidate is taken
 * unless a landmark taken before it lies at f64 distance sqrt((dx^2 + dy^2) + dz^2) < radius; stop at num.  out_idx [num]
 * (device) receives the point indices in pick order; *n_passes (host, may be NULL) the passes run.  Synchronises the stream
 * once per pass (the landmark count is read back).  SPLATRASTER_ERR_BAD_ARG for num outside [1, N], a radius that is not
 * positive and finite, or when the radius underflows to 0 first (fewer than num distinct positions). */
int splatraster_landmark_select(int64_t N, const float* points, const double* score, int32_t num, double radius,
                                int32_t* out_idx, int32_t* n_passes, void* workspace, void* stream);

/* ---- feature-TSDF fusion: utils/fusion_utils.py:112-181 (integrate), 277-288 (the vertex gather of get_mesh), INTEGRATION.md §20
 * The volume in the reference's layout, all f32 and contiguous: tsdf [X,Y,Z], weight [X,Y,Z], color [X,Y,Z,3], feat [X,Y,Z,C]
 * (16-byte aligned); axis[a] [dim[a]] f32 are the voxel centres along axis a (the host builds them with the reference's
 * promotion chain).  dim[0]*dim[1]*dim[2] <= 2^30; feat_dim a multiple of 4 in [4, 256].  Element offsets are 64-bit. */
#define SPLATRASTER_FUSION_MAX_FRAMES 8
#define SPLATRASTER_FUSION_MAX_FEAT_DIM 256
typedef struct splatraster_fusion_volume {
    int32_t dim[3];
    int32_t feat_dim;
    const float* axis[3];
    float* tsdf;
    float* weight;
    float* color;
    float* feat;
} splatraster_fusion_volume;
/* Host only: bytes of the four volumes, and of the device workspace of splatraster_fusion_surface_count / _extract.
 * SPLATRASTER_ERR_BAD_ARG (both set to 0) for a dimension < 1, more than 2^30 voxels or an unsupported feat_dim. */
int splatraster_fusion_bytes(int32_t X, int32_t Y, int32_t Z, int32_t feat_dim, size_t* volume_bytes, size_t* surface_bytes);
/* Integrates F <= 8 frames, in order, in one launch: depth [F,H,W], color_im [F,H,W,3], feat_im [F,H,W,C] (device f32, feat_im
 * 16-byte aligned); world2cam [F,12] (rows 0..2 of the world-to-camera matrices) and intrinsics [F,4] (fx, fy, cx, cy) in HOST
 * memory.  Per voxel centre p and frame, every operation rounded to f32 on its own:
 *   cam = ((m0 px + m1 py) + m2 pz) + m3 per row; skipped unless cam.z > 0
 *   pix = rint((cam.xy * f) / cam.z + c) (half to even); skipped outside [0, W) x [0, H)
 *   d = depth[pix]; diff = d - cam.z; skipped unless d > 0 and diff >= -sdf_trunc; dist = min(diff / sdf_trunc, 1)
 *   w' = w + obs_weight; tsdf = (w tsdf + obs dist) / w'; color = clamp(rint((w color + obs color_im[pix]) / w'), 0, 255);
 *   feat = clamp((w feat + obs feat_im[pix]) / w', 0, 255); weight = w'
 * A batch gives bit for bit what F single-frame calls give.  H, W <= 32768.  No host synchronisation. */
int splatraster_fusion_integrate(const splatraster_fusion_volume* volume, int32_t F, int32_t H, int32_t W, const float* depth,
                                 const float* color_im, const float* feat_im, const float* world2cam, const float* intrinsics,
                                 float obs_weight, float sdf_trunc, void* stream);
/* Surface vertices: one per grid edge (voxel n to its +x, +y or +z neighbour) whose end values a, b satisfy
 * (a < level) != (b < level).  level = `level` when use_level, else 0.5f * (min + max) of tsdf (NaN ignored), reduced on the
 * device; it is stored as the f32 at offset 0 of the workspace.  Counts the vertices, scans the counts and returns the total in
 * *n_vertices (HOST); synchronises the stream once.  volume->feat and ->axis are not read. */
int splatraster_fusion_surface_count(const splatraster_fusion_volume* volume, int32_t use_level, float level, void* workspace,
                                     int64_t* n_vertices, void* stream);
/* Writes the M = *n_vertices vertices of the preceding count (same workspace, unchanged tsdf), in ascending (voxel linear index,
 * axis) order: verts [M,3] f32 in voxel units (i + (level - a) / (b - a) along the edge's axis), points [M,3] f64 =
 * (double)(verts * (float)voxel_size) + origin (origin: 3 doubles in HOST memory), index [M] i64 = linear index of the voxel
 * rint(verts) (half to even), colors [M,3] u8 = floor(color[index]), feats [M,C] = feat[index] (16-byte aligned). */
int splatraster_fusion_surface_extract(const splatraster_fusion_volume* volume, const void* workspace, double voxel_size,
                                       const double* origin, int64_t M, float* verts, double* points, int64_t* index,
                                       uint8_t* colors, float* feats, void* stream);
/* Surface mesh over those vertices (get_mesh of utils/fusion_utils.py:271-289; the triangulation and the normals are the
 * project's own rule).  A cell is the cube of 8 voxels from (x, y, z) to (x+1, y+1, z+1); cells are walked in
 * linear [X-1, Y-1, Z-1] order.  Corner c of a cell lies at (c & 1, (c >> 1) & 1, (c >> 2) & 1); bit c of its case is set when
 * tsdf(corner c) < level (NaN: not set); edge e = axis * 4 + k runs along `axis` from the corner whose offset along the lower of
 * the two other axes is k & 1 and along the higher one (k >> 1) & 1.  The table (csrc/fusion_mesh.h, derived at compile time)
 * gives each case up to 5 triangles as edge ids; the vertex of an edge is the surface vertex of (the voxel the edge starts at,
 * axis).  (p1 - p0) x (p2 - p0) of every triangle points towards increasing tsdf.
 * Host only: bytes of the mesh workspace.  SPLATRASTER_ERR_BAD_ARG as splatraster_fusion_bytes; SPLATRASTER_ERR_OVERFLOW when
 * 5 * cells does not fit 32 bits. */
int splatraster_fusion_mesh_bytes(int32_t X, int32_t Y, int32_t Z, size_t* mesh_bytes);
/* Counts the triangles of every cell, scans the counts and returns the total in *n_faces (HOST); synchronises the stream once.
 * splatraster_fusion_surface_count must have run on surface_workspace for the same, unchanged tsdf: it supplies the level and the
 * vertex offsets.  SPLATRASTER_ERR_OVERFLOW when the vertex total or the face total exceeds 2^31 - 1 (the faces are int32). */
int splatraster_fusion_mesh_count(const splatraster_fusion_volume* volume, const void* surface_workspace, void* mesh_workspace,
                                  int64_t* n_faces, void* stream);
/* Writes faces [F,3] i32 (vertex ids into the surface extract's rows, cells ascending, a cell's triangles in table order) and
 * normals [M,3] f32, one per vertex in the surface extract's order.  Normal of the vertex on the edge from voxel n to its
 * neighbour n' along an axis, end values a and b, every operation rounded to f32 on its own: the gradient g(v) of the tsdf at a
 * voxel is 0.5f * (t[i+1] - t[i-1]) per axis (t[1] - t[0] and t[last] - t[last-1] at the ends, 0 on an axis of one voxel);
 * q = (level - a) / (b - a); g = g(n) + q * (g(n') - g(n)); len = sqrtf((g0 g0 + g1 g1) + g2 g2); normal = g / len when len is
 * positive and finite, else (0, 0, 0).  M and F as returned by the two counts.  A smaller F (M) writes the first F (M) rows only;
 * a larger F writes the counted faces and leaves the remaining rows at -1; a larger M leaves the remaining rows untouched.
 * F = 0 writes no face, M = 0 no normal (the pointer may then be NULL).  SPLATRASTER_ERR_BAD_ARG for F > 5 * cells, M > 3 * voxels,
 * a negative count or a missing pointer.  No host synchronisation. */
int splatraster_fusion_mesh_extract(const splatraster_fusion_volume* volume, const void* surface_workspace,
                                    const void* mesh_workspace, int64_t M, int64_t F, int32_t* faces, float* normals, void* stream);
/* Host only: copies the 256 x 16 bytes of the triangulation table (row of a case: byte 0 the triangle count, bytes 1..15 edge
 * ids, 0xFF where unused). */
int splatraster_debug_mc_table(uint8_t* out);

/* ---- 2D-3D matching: test.py:247-378 (get_frusm_pts, match_feature), utils/match_utils.py (hungarian_solve), INTEGRATION.md §17
 * Exact rectangular assignment (scipy.optimize.linear_sum_assignment, Crouse's shortest augmenting path): for the same f64 cost
 * matrix the same assignment as scipy, ties included.  Problem b is the ORIENTED [nr, nc] f64 matrix (nr <= nc, row-major) at
 * element `offset` of `costs`; `transposed` != 0 says it is the transpose of the caller's matrix.  Limits: 1 <= nr <= nc <=
 * SPLATRASTER_LSAP_MAX_NC and nr * nc < 2^31 (SPLATRASTER_ERR_OVERFLOW beyond them, SPLATRASTER_ERR_BAD_ARG for nr < 1 or nc < nr).
 * maximize != 0 solves on -cost.  Problem b writes nr pairs at row_ind / col_ind [sum of nr] (int64, device) from slot
 * sum_{b' < b} nr_b', in the caller's orientation: untransposed (i, col of row i) for i = 0..nr-1; transposed the caller's rows
 * ascending and their columns.  status[b] (device) receives SPLATRASTER_LSAP_OK, _INVALID (a NaN or, after the sign, a -inf
 * entry) or _INFEASIBLE (no finite assignment), steps[b] the Dijkstra steps taken.  The problem table is host memory; no host
 * synchronisation.  The column / row state lives in LDS when nc <= 4096 (splatraster_debug_set_lsap_lds(1), the default) and
 * in `workspace` otherwise (splatraster_lsap_workspace_bytes; 0 bytes when every problem fits the LDS). */
#define SPLATRASTER_LSAP_MAX_NC 65535
#define SPLATRASTER_LSAP_OK 0
#define SPLATRASTER_LSAP_INVALID 1
#define SPLATRASTER_LSAP_INFEASIBLE 2
typedef struct splatraster_lsap_problem {
    int64_t offset;
    int32_t nr, nc;
    int32_t transposed;
    int32_t reserved;
} splatraster_lsap_problem;
size_t splatraster_lsap_workspace_bytes(int32_t B, const splatraster_lsap_problem* problems);
int splatraster_lsap(int32_t B, const splatraster_lsap_problem* problems, const double* costs, int32_t maximize,
                     int64_t* row_ind, int64_t* col_ind, int32_t* status, int32_t* steps, void* workspace, void* stream);
/* test hook: 1 (default) keeps the solver state of problems with nc <= 4096 in LDS, 0 forces the global workspace for every
 * problem.  Results never depend on it. */
int splatraster_debug_set_lsap_lds(int mode);
/* hungarian_solve's cost: d1 [D, N1], d2 [D, N2] f32 (columns are descriptors), each column divided by max(||x||, 1e-12)
 * (F.normalize(p=2, dim=0)); sim = d1^T d2 in f32 (one FMA chain over D per entry), sim < threshold -> 0, cost = 1 - sim (f32),
 * written widened to f64 in the solver's orientation: [N1, N2] when N1 <= N2, else [N2, N1] (its transpose).  norms [N1 + N2]
 * (device) receives the denominators.  splatraster_match_sims gathers the thresholded similarity of K pairs (i1[k], i2[k])
 * (int64 indices into d1 / d2, device) with the same arithmetic as the matrix.  No host synchronisation. */
int splatraster_match_cost(int32_t D, int32_t N1, int32_t N2, const float* d1, const float* d2, float threshold, float* norms,
                           double* cost, void* stream);
int splatraster_match_sims(int32_t D, int32_t N1, int32_t N2, const float* d1, const float* d2, const float* norms,
                           float threshold, int64_t K, const int64_t* i1, const int64_t* i2, float* sims, void* stream);
/* get_frusm_pts without the decoder.  points [N,3] f32 (device); w2c [4,4] and K [3,3] f64 row-major (HOST).  All arithmetic in
 * f64 from the f32 inputs: pc = R p + t, (u, v) = (K pc)_{0,1} / (K pc)_2; kept iff pc.z > 0.05, 0 <= u < width, 0 <= v < height
 * and, in key-Gaussian mode (marker != NULL, [N] f32), marker > marker_threshold (compared in f32 like the reference).
 * Subset mode (marker == NULL): the kept points in index order.  Key-Gaussian mode: every pixel of kp_mask [height, width] (u8,
 * == 1 is a keypoint, every other value is not; row-major order) is back-projected with depth [height, width] f32, c2w [4,4]
 * (f64, HOST) and kp_K = (fx, fy, cx, cy) (HOST): x = (col - cx) * d / fx, y = (row - cy) * d / fy, z = d, q = R x + t; its nearest kept point (distance
 * sqrt((dx^2 + dy^2) + dz^2) in f64, ties the smaller index) is emitted, in keypoint order, when closer than 0.1.
 * A keypoint whose q is not finite (depth inf or NaN) or reaches 1e15 in magnitude is not searched and emits nothing; depth 0
 * gives q = t and follows the rule.
 * Outputs (device): out_idx [n] i32 point indices, out_xyz [n,3] f32, out_uv [n,2] f64 projections, *out_count (int64, device) =
 * n; capacity N (subset) or width * height (key mode).  workspace: splatraster_frustum_workspace_bytes(N, width, height).  No
 * host synchronisation. */
size_t splatraster_frustum_workspace_bytes(int64_t N, int32_t width, int32_t height);
int splatraster_frustum_candidates(int64_t N, const float* points, const float* marker, float marker_threshold, const double* w2c,
                                   const double* K, int32_t width, int32_t height, const uint8_t* kp_mask, const float* depth,
                                   const double* c2w, const double* kp_K, int32_t* out_idx, float* out_xyz, double* out_uv,
                                   int64_t* out_count, void* workspace, void* stream);

/* ---- absolute pose: test.py:64-84 (solve_pose -> pycolmap.absolute_pose_estimation), INTEGRATION.md §18 -------------------
 * P3P LO-RANSAC and a robust refinement for B problems of different sizes.  Problem b holds n correspondences at element
 * `offset` of points2d [*, 2] and points3d [*, 3] (f64, device) and a pinhole camera (fx, fy, cx, cy).  The pose is
 * world-to-camera: x_cam = R X + t.  Everything is f64 and compiled without FP contraction; the definitions below are exact.
 *
 * Residual of (R, t) at correspondence i: (x, y, z) = R X + t with x = ((R00*X0 + R01*X1) + R02*X2) + t0 (same for y, z);
 *   du = u - (fx * (x / z) + cx), dv = v - (fy * (y / z) + cy), r = du*du + dv*dv (no +0.5 shift of the keypoints).
 *   i is an inlier iff z > 0 and r <= thr2, thr2 = max_error_px * max_error_px.
 * Support: (inlier count, sum of r over the inliers).  A model is better with more inliers; at equal counts with the smaller
 *   sum; then the lower trial, then the lower solution index (slot = 4 * trial + solution).
 * Sampler (stateless): mix(x) = splitmix64's finaliser: x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *   x = (x ^ (x >> 27)) * 0x94D049BB133111EB; x ^ (x >> 31) (uint64 wrap-around).  h_d = mix(mix(seed) ^ (3 * trial + d))
 *   for draw d = 0, 1, 2.  i0 = h_0 mod n; i1 = h_1 mod (n - 1), +1 if >= i0; i2 = h_2 mod (n - 2), +1 if >= min(i0, i1),
 *   +1 more if then >= max(i0, i1).  The problem's position in the batch is not hashed, so a problem draws the same samples
 *   alone or in a batch.
 * Minimal solver: Grunert's P3P on the bearings normalize((u - cx) / fx, (v - cy) / fy, 1): the quartic in v = s3 / s1
 *   (Haralick et al. 1994), its real roots by Ferrari's resolvent (largest cubic root in closed form, 2 Newton steps on the
 *   cubic, 2 on the quartic), u = s2 / s1 from v, the depths polished by 3 Newton steps on the three cosine-law equations, and
 *   (R, t) from the orthonormal frames of the two triangles (t from the centroids).  Up to 4 models per trial; v <= 0, u <= 0, a
 *   degenerate triangle (|e1 x e2| <= 1e-10 |e1| |e2|, a zero side) or a non-finite entry drops a model.  Never NaN.
 * Trials run in batches of SPLATRASTER_PNP_BATCH.  After each batch, with k the best inlier count: required = max_num_trials
 *   if k == 0 or k / n < min_inlier_ratio; else p3 = (k / n)^3, required = min_num_trials if p3 >= 1, else
 *   ceil(log(1 - confidence) / log(1 - p3)) clipped to [min_num_trials, max_num_trials] (max_num_trials if the log is 0).
 *   A problem finishes when its trials (a multiple of the batch) reach the required count.
 * LO: when a batch's best model beats the running best, up to 4 rounds of { up to 10 Gauss-Newton steps of sum r over the
 *   inliers of the round's start model (rotation by the so(3) exponential, left-multiplied; t additive), re-score on all n };
 *   a round is kept if its support is better, and LO stops at the first round that is not.
 * Success: a best model with >= 4 inliers.  Final refinement: Levenberg-Marquardt on sum log(1 + r) over the RANSAC inliers,
 *   at most 100 iterations, stopping when the relative cost change or the step norm falls below 1e-10; a non-finite result is
 *   SPLATRASTER_PNP_NONFINITE.  num_inliers / inlier_mask are those of the RANSAC model, before refinement.
 * Every reduction has a fixed order (no atomics): outputs are bit-identical from run to run and between a batch and single
 *   calls.  n < 4 gives SPLATRASTER_PNP_NO_MODEL without any trial.
 * Outputs (device): R_out [B, 9] (row-major), t_out [B, 3] f64, num_inliers [B] i32, inlier_mask [sum n] u8, status [B] i32,
 *   trials [B] i32.  One stream synchronisation per batch of trials (the "all finished" flag).  workspace:
 *   splatraster_pnp_workspace_bytes.  Limits: n <= SPLATRASTER_PNP_MAX_N, B <= 65535, 1 <= min_num_trials <= max_num_trials. */
#define SPLATRASTER_PNP_BATCH 1024
#define SPLATRASTER_PNP_MAX_N (1 << 20)
#define SPLATRASTER_PNP_OK 0
#define SPLATRASTER_PNP_NO_MODEL 1
#define SPLATRASTER_PNP_NONFINITE 2
typedef struct splatraster_pnp_problem {
    int64_t offset;
    int32_t n;
    int32_t reserved;
    double fx, fy, cx, cy;
} splatraster_pnp_problem;
typedef struct splatraster_pnp_options {
    double max_error_px;
    double min_inlier_ratio;
    double confidence;
    uint64_t seed;
    int32_t min_num_trials, max_num_trials;
} splatraster_pnp_options;
size_t splatraster_pnp_workspace_bytes(int32_t B, const splatraster_pnp_problem* problems, const splatraster_pnp_options* options);
int splatraster_pnp(int32_t B, const splatraster_pnp_problem* problems, const splatraster_pnp_options* options,
                    const double* points2d, const double* points3d, double* R_out, double* t_out, int32_t* num_inliers,
                    uint8_t* inlier_mask, int32_t* status, int32_t* trials, void* workspace, void* stream);
/* test entries (same workspace, no host synchronisation).  hypotheses: trials trial0 .. trial0 + ntrials - 1 of every problem
 * (ntrials <= SPLATRASTER_PNP_BATCH): samples [B, ntrials, 3] i32, models [B, ntrials, 4, 12] f64 (R row-major, t; slots past
 * nmodels unwritten), nmodels [B, ntrials] i32.  score: the support of M given models [B, M, 12] per problem: count [B, M] i32,
 * sum [B, M] f64. */
int splatraster_pnp_hypotheses(int32_t B, const splatraster_pnp_problem* problems, const splatraster_pnp_options* options,
                               int64_t trial0, int32_t ntrials, const double* points2d, const double* points3d, int32_t* samples,
                               double* models, int32_t* nmodels, void* workspace, void* stream);
int splatraster_pnp_score(int32_t B, const splatraster_pnp_problem* problems, const splatraster_pnp_options* options, int32_t M,
                          const double* models, const double* points2d, const double* points3d, int32_t* count, double* sum,
                          void* workspace, void* stream);

/* ---- localisation: retrieval and pose errors (pre_process/gen_netvlad_retrieval.py:32-34, utils/eval_utils.py:75-145,
 * test.py:81-82), INTEGRATION.md §21 ------------------------------------------------------------------------------------------
 * Retrieval: the k most similar database rows of every query row, similarity and selection fused (the Q x N matrix never exists
 * in global memory).  query [Q, D], db [N, D] f32 row-major (device); rows need not be unit length.  sims [Q, k] (f32) is the dot
 * product of the query row and the selected database row, accumulated in f32 (the order is the kernel's); idx [Q, k] (int64) the
 * database rows.  Within a query row: similarity descending, equal similarities (-0 == +0) by database index ascending.
 * Limits: 1 <= k <= min(N, SPLATRASTER_RETRIEVAL_MAX_K), D >= 1, Q >= 0, 1 <= N < 2^31; anything else is
 * SPLATRASTER_ERR_BAD_ARG without a launch.  status [1] (i32, device) receives SPLATRASTER_RETRIEVAL_OK, or _NONFINITE when a
 * computed similarity is NaN (idx / sims are then unspecified).  workspace (splatraster_retrieval_workspace_bytes; may be 0 bytes,
 * then NULL is accepted) holds one k-entry list per (query, slice of the database): O(Q k slices), at most 64 slices, nothing
 * that grows with Q * N.  No host synchronisation. */
#define SPLATRASTER_RETRIEVAL_MAX_K 128
#define SPLATRASTER_RETRIEVAL_OK 0
#define SPLATRASTER_RETRIEVAL_NONFINITE 1
size_t splatraster_retrieval_workspace_bytes(int64_t Q, int64_t N, int32_t D, int32_t k);
int splatraster_retrieval_topk(int64_t Q, int64_t N, int32_t D, int32_t k, const float* query, const float* db, int64_t* idx,
                               float* sims, int32_t* status, void* workspace, void* stream);
/* eval_pose for B poses (f64 row-major rotations [B,3,3], translations [B,3], device).  Per pose and per rotation: the quaternion
 * of SO3_to_quat in f64 (branch on R22 < 0, then R00 > R11; else on R00 < -R11; (v * 0.5) / sqrt(scale)), divided by
 * max(norm, 1e-12), rounded to f32; d = |q_gt . q_est| in f32, d > (float)(1 - 1e-7) -> that bound;
 * theta_deg = 2 * acos(d) * 180 / pi in f32 (never below 0.05595 degrees); dist = ||t_est - t_gt|| in f64.  valid (u8 [B] or NULL):
 * rows with valid == 0 get NaN in both outputs.  No host synchronisation. */
int splatraster_pose_errors(int64_t B, const double* R_est, const double* t_est, const double* R_gt, const double* t_gt,
                            const uint8_t* valid, float* theta_deg, double* dist, void* stream);
/* solve_pose's conversion for B poses: R_out = R^T, t_out[i] = fma(-R[2][i], t[2], fma(-R[1][i], t[1], -R[0][i] * t[0])) (f64,
 * device; the rounding of a three-term FMA chain in ascending order).  No host synchronisation. */
int splatraster_pose_invert(int64_t B, const double* R, const double* t, double* R_out, double* t_out, void* stream);

/* ---- pose refinement on the device (build extension, DESIGN.md §6.8: the reference's rasterizer returns no camera gradient
 * and nothing calls its utils/optimization_utils.py:5-66 pose helpers) ------------------------------------------------------
 * L = mean |color - target_color| + depth_weight * mean |depth - target_depth| and its gradient planes in one pass;
 * `*loss_out += L` (a float atomic: zero it before the first call; monitoring value).  target_depth may be NULL (no depth
 * term; g_depth, when given, is zeroed). */
int splatraster_l1_rgbd_loss(int64_t n_color, const float* color, const float* target_color, int64_t n_depth, const float* depth,
                             const float* target_depth, float depth_weight, float* g_color, float* g_depth, float* loss_out,
                             void* stream);
/* One Adam step on a camera pose and the camera tensors of the new pose, without leaving the device.
 * The pose is W2C = T(w, t) @ W2C_init with an axis-angle w and a translation t — at_to_transform_matrix of
 * utils/optimization_utils.py:31-42 (Rodrigues made regular at w = 0) —, the camera tensors are what
 * utils/camera_utils.py:129-139 derives from it: viewmatrix = W2C^T, projmatrix = viewmatrix @ projection_matrix,
 * campos = -R^T t.  state [20 floats, device]: w[3], t[3], Adam exp_avg[6], exp_avg_sq[6], step, pad — all zero at the start.
 * advance != 0: chains dL_dviewmatrix [16], dL_dprojmatrix [16], dL_dcampos [3 or NULL] (splatraster_backward's outputs) to
 * (w, t), takes the torch.optim.Adam step (lr_rot for w, lr_trans for t) and writes the NEW pose's tensors;
 * advance == 0: only writes the tensors of the current state (the first iteration).  All matrices row-major [4, 4]. */
int splatraster_pose_step(const float* dL_dviewmatrix, const float* dL_dprojmatrix, const float* dL_dcampos, const float* W2C_init,
                          const float* projection_matrix, float lr_rot, float lr_trans, float beta1, float beta2, float eps,
                          int advance, float* state, float* viewmatrix, float* projmatrix, float* campos, void* stream);

/* The two calls above for the 1 <= n_views <= 8 frames of a window, ONE launch each (splatloc_amd.pose.refine_poses).
 * splatraster_l1_rgbd_loss_window: every view has n_color colour and n_depth depth elements; loss_out[v] += L of view v; the
 * gradient planes are bit-identical to n_views single calls (a sign times a constant per element).  target_depth NULL in a
 * view: no depth term there, its g_depth (when given) is zeroed. */
typedef struct splatraster_l1_view {
    const float* color;        /* [n_color] */
    const float* target_color; /* [n_color] */
    const float* depth;        /* [n_depth]; may be NULL when target_depth is */
    const float* target_depth; /* [n_depth] or NULL */
    float* g_color;            /* [n_color] out */
    float* g_depth;            /* [n_depth] out, or NULL */
} splatraster_l1_view;
int splatraster_l1_rgbd_loss_window(int32_t n_views, const splatraster_l1_view* views /* host array */, int64_t n_color,
                                    int64_t n_depth, float depth_weight, float* loss_out /* [n_views] device */, void* stream);
/* splatraster_pose_step for n cameras, one thread per camera, the single call's arithmetic: state [n,20], dL_dviewmatrix /
 * dL_dprojmatrix [n,16], dL_dcampos [n,3] or NULL, W2C_init [n,4,4], ONE projection_matrix [4,4] shared by the cameras; outputs
 * viewmatrix / projmatrix [n,4,4], campos [n,3] or NULL.  A camera's result does not depend on its slot or on n. */
int splatraster_pose_step_window(int32_t n, const float* dL_dviewmatrix, const float* dL_dprojmatrix, const float* dL_dcampos,
                                 const float* W2C_init, const float* projection_matrix, float lr_rot, float lr_trans, float beta1,
                                 float beta2, float eps, int advance, float* state, float* viewmatrix, float* projmatrix,
                                 float* campos, void* stream);

/* ---- per-stage timing (HIP events on the launch stream) ----------------------------- */

/* Stage ids: every kernel group of the path is bracketed by a hipEvent pair when timing
 * is enabled (process-wide switch; off by default).  An event record between two kernels
 * costs ~10 us of idle GPU on MI355X, so a throughput measurement should select only the
 * stage it needs (splatraster_timing_select) and take the full breakdown in a separate run. */
#define SPLATRASTER_STAGE_PREPROCESS 0     /* preprocess_kernel */
#define SPLATRASTER_STAGE_DEPTH_SORT 1     /* depth keys + P-sized radix sort */
#define SPLATRASTER_STAGE_SCAN 2           /* inclusive scan of tiles_touched */
#define SPLATRASTER_STAGE_EMIT 3           /* emit_kernel */
#define SPLATRASTER_STAGE_TILE_SORT 4      /* R-sized radix sort on tile id */
#define SPLATRASTER_STAGE_RANGES 5         /* clearing the per-tile range table when nothing was emitted; the launch order of small grids (tile_order_kernel) */
#define SPLATRASTER_STAGE_COMPOSITE_FWD 6  /* composite_fwd_kernel */
#define SPLATRASTER_STAGE_COMPOSITE_BWD 7  /* composite_bwd_kernel (the accumulator memset before it is not bracketed) */
#define SPLATRASTER_STAGE_PREPROCESS_BWD 8 /* preprocess_bwd_kernel */
#define SPLATRASTER_STAGE_PAYLOAD 9        /* payload_kernel / ranges_kernel + payload_tile_kernel: per-instance records, reach masks, tile ranges */
#define SPLATRASTER_STAGE_COUNT 10

int splatraster_timing_enable(int on);            /* all stages on / off */
int splatraster_timing_select(uint32_t stage_mask); /* bit s set: time stage s only */
/* Waits for all recorded events, ADDS elapsed milliseconds / launch counts per stage into
 * ms[SPLATRASTER_STAGE_COUNT] / counts[SPLATRASTER_STAGE_COUNT], then clears the records. */
int splatraster_timing_collect(double* ms, int64_t* counts);

/* ---- frame preparation: image gradients, grad mask, masked medians (csrc/image_ops.hip) ----------- */

/* The frame-preparation step of SplatLoc's key-frame loop and of test.py: image_gradient / image_gradient_mask (utils/utils.py:4-38),
 * Camera.compute_grad_mask (utils/camera_utils.py:145-172) and get_median_depth (utils/utils.py:85-96), for N frames per call,
 * asynchronous on `stream`, nothing read back.  All tensors are contiguous device arrays; argument checks come before any launch.
 *
 * Arithmetic (float32, every operation rounding on its own, no contraction): gray = ((r + g) + b) / 3; the plane is padded by one
 * pixel with reflect padding (the border is not repeated); grad_v = (1/32) sum of [[3,10,3],[0,0,0],[-3,-10,-3]] * p and
 * grad_h = (1/32) sum of [[3,0,-3],[10,0,-10],[3,0,-3]] * p, cross-correlation, the nine products added row-major starting from
 * the first (zero taps included: 0 * NaN is NaN); a pixel is valid when all nine |p| > eps; the intensity is
 * x = sqrt((grad_v valid)^2 + (grad_h valid)^2) with a correctly rounded square root.  A median is the LOWER median, element
 * (n - 1) / 2 of the ascending order, and NaN when any selected element is NaN. */

/* Gradients and validity of every plane of image [N,C,H,W] (H, W >= 2; N * C <= 65535): grad_v, grad_h [N,C,H,W] float and
 * valid [N,C,H,W] bytes (1 / 0); each output may be NULL, not all three.  Needs no workspace. */
int splatraster_image_gradient(int32_t N, int32_t C, int32_t H, int32_t W, const float* image, float eps, float* grad_v,
                               float* grad_h, uint8_t* valid, void* stream);

#define SPLATRASTER_GRAD_MASK_REPLICA 0  /* per-block medians on a 32 x 32 grid of blocks */
#define SPLATRASTER_GRAD_MASK_GLOBAL 1   /* one median per frame (every other dataset type) */
/* Bytes of workspace a grad-mask call of this shape needs (0 is possible: then workspace may be NULL); have_intensity: the call
 * passes an intensity output. */
int splatraster_grad_mask_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t mode, int32_t have_intensity, size_t* bytes);
/* images [N,3,H,W] -> out [N,1,H,W].
 * REPLICA: bh = H / 32, bw = W / 32 (integer division); for block (r, c), t = median(x over the block) * edge_threshold and
 *   out = (x > t && t < 1) ? 1 : 0 (the reference writes 1 where x > t, then 0 where the result <= t: with t >= 1 its ones go too);
 *   t NaN (a NaN in the block, inf * 0): the block keeps x.  Rows at or beyond 32 bh and columns at or beyond 32 bw keep x.  The
 *   output is float (out_u8 != 0: SPLATRASTER_ERR_UNSUPPORTED); H < 32 or W < 32 (the reference takes the median of an empty block
 *   and raises): SPLATRASTER_ERR_BAD_ARG.  thresholds (optional): [N,32,32], t of every block.
 * GLOBAL: out = x > median(x over the frame) * edge_threshold, as float 0 / 1 or, with out_u8, as bytes.  thresholds (optional): [N].
 * intensity (optional): [N,1,H,W], x of every pixel.  workspace_bytes below the query's answer: SPLATRASTER_ERR_BAD_ARG. */
int splatraster_grad_mask(int32_t N, int32_t H, int32_t W, const float* images, float edge_threshold, float eps, int32_t mode,
                          int32_t out_u8, void* out, float* intensity, float* thresholds, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Test hook, host only: the internal path the REPLICA mode takes for H x W frames.  0: none (H or W below 32 or above 65536);
 * 1: fused, a block's halo and intensities in 19 KB of LDS (n = bh bw <= 2048, halo (bh + 2)(bw + 2) <= 2560); 2: fused in 145 KB
 * (n <= 16384, halo <= 20480); 3: the gradient kernel, then a per-block select over global memory. */
int splatraster_debug_image_ops_path(int32_t H, int32_t W);

/* Lower median of the selected elements of each of N rows of n <= 2^31 values [N,n]: element i is selected when
 * (!positive_only || value > 0) && (!opacity || opacity[i] > opacity_min) && (!mask || mask[i] != 0) (get_median_depth:
 * positive_only = 1, opacity_min = 0.95).  Negative values order correctly (-0 below +0).  Outputs per row: median [N] (NaN for an
 * empty selection: the reference raises there); optional std [N] (unbiased, NaN for fewer than two elements), count [N] and
 * valid [N,n] bytes (the selection).  The count, the rank and the result stay on the device. */
int splatraster_masked_median_workspace_bytes(int32_t N, int64_t n, size_t* bytes);
int splatraster_masked_median(int32_t N, int64_t n, const float* values, int32_t positive_only, const float* opacity,
                              float opacity_min, const uint8_t* mask, float* median, float* std, int64_t* count, uint8_t* valid,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- SuperPoint head: scores, NMS, keypoint selection, descriptors (csrc/superpoint_head.hip) ------ */

/* Everything behind SuperPoint's two convolution heads, for B images per call, asynchronous on `stream`, nothing read back.  Inputs
 * are the raw head outputs: semi [B,65,Hc,Wc] (the logits of convPb) and coarse [B,256,Hc,Wc] (the output of convDb); H = 8 Hc,
 * W = 8 Wc.  All tensors are contiguous float32 device arrays.  Argument checks come before any launch: B, Hc, Wc (H, W) >= 1, else
 * SPLATRASTER_ERR_BAD_ARG; B H W < 2^31, else SPLATRASTER_ERR_UNSUPPORTED; null or misaligned pointers, a radius outside 0..8,
 * max_keypoints outside 1..65535, a negative (or NaN) threshold, a negative border: SPLATRASTER_ERR_BAD_ARG.
 *
 * hloc's SuperPoint is not part of the reference tree; these definitions are the contract:
 *  scores   p = softmax(semi) over the 65 channels in float32: m = max, e_c = expf(x_c - m), s = e_0 + e_1 + ... + e_64 in that order,
 *           p_c = e_c / s.  Channel 64 is dropped; S[b, 8i + u, 8j + v] = p[b, 8u + v, i, j].
 *  NMS      pool(X) = maximum over the (2r + 1)^2 window clipped to the image.  M0 = (S == pool(S)); twice: Supp = pool(M) > 0,
 *           Q = where(Supp, 0, S), M |= (Q == pool(Q)) & ~Supp; N = where(M, S, 0).  Equal scores on a plateau all survive; r = 0: N = S.
 *  select   candidates: N > threshold (strict), border <= row < H - border, border <= col < W - border; n of them in an image.
 *           n <= K: the keypoints in row-major order.  n > K: the K largest scores in descending order, equal scores by ascending
 *           row-major index.  keypoints [B,K,2] as (x, y) = (col, row), scores [B,K], count [B] = min(n, K), candidates [B] = n;
 *           rows at and beyond count are zero.  Candidate scores are positive.
 *  sample   d^ = coarse / max(|coarse|, 1e-12) over the channels.  For a keypoint (x, y), in float32 without contraction:
 *           gx = ((x - 3.5) / (8 Wc - 4.5)) * 2 - 1, ix = ((gx + 1) / 2) * (Wc - 1), gy and iy likewise with Hc; the bilinear
 *           interpolation of d^ at (ix, iy), neighbours outside the grid reading 0, normalised once more with the same eps.
 *           descriptors [B,256,K], columns at and beyond count[b] zero.  A finite keypoint far outside the image has no neighbour
 *           inside the grid: a zero column.  Non-finite keypoints give NaN in the restatement and are outside the contract.
 *  dense    the same at every pixel (x, y) of rows [row0, row0 + rows): out [B,rows,W,256], channel-last. */

/* Host only, never touches the device: the tile of outputs one NMS workgroup owns for radii 0..4.  Radii 5..8 use tiles of half
 * that side, so every edge of the reported tile is a tile edge at every radius. */
int splatraster_sp_nms_tile(int32_t* tile_h, int32_t* tile_w);
/* Host only: bytes of workspace for B images of H x W pixels and up to max_keypoints keypoints; serves every call below of that
 * shape (sample and dense_descriptors use only its first part and accept any max_keypoints in the query). */
int splatraster_sp_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t max_keypoints, size_t* bytes);
/* scores [B,8 Hc,8 Wc], 16-byte aligned. */
int splatraster_sp_scores(int32_t B, int32_t Hc, int32_t Wc, const float* semi, float* scores, void* stream);
/* out [B,H,W]; any H, W >= 1; out must not alias scores unless radius is 0. */
int splatraster_sp_nms(int32_t B, int32_t H, int32_t W, const float* scores, int32_t radius, float* out, void* stream);
int splatraster_sp_select(int32_t B, int32_t H, int32_t W, const float* nms, float threshold, int32_t max_keypoints, int32_t border,
                          float* keypoints, float* scores, int32_t* count, int32_t* candidates, void* workspace, size_t workspace_bytes,
                          void* stream);
/* keypoints [B,K,2] need not be integers; count [B] (clamped to 0..K). */
int splatraster_sp_sample(int32_t B, int32_t Hc, int32_t Wc, const float* coarse, int32_t K, const float* keypoints, const int32_t* count,
                          float* descriptors, void* workspace, size_t workspace_bytes, void* stream);
/* 0 <= row0, rows >= 1, row0 + rows <= 8 Hc; out 16-byte aligned. */
int splatraster_sp_dense_descriptors(int32_t B, int32_t Hc, int32_t Wc, const float* coarse, int32_t row0, int32_t rows, float* out,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- NetVLAD head: soft assignment, VLAD aggregation, whitening (csrc/netvlad_head.hip) ----------- */

/* Everything behind NetVLAD's convolution stack, for B images per call, asynchronous on `stream`, nothing read back, no host
 * synchronisation.  All tensors are contiguous float32 device arrays.  hloc's NetVLAD layer is not part of the reference tree, so it
 * is unpinned; these definitions are this project's own contract, modelled on that layer:
 *  inputs     features [B,D,N], the backbone's map with N = h w locations, channel-major; score_w [K,D]; score_b [K] or NULL;
 *             centers [D,K].
 *  assign     inv[b,n] = 1 / max(sqrt(sum_d x[d,n]^2), 1e-12); xh[d,n] = x[d,n] * inv[b,n];
 *             s[k,n] = sum_d score_w[k,d] * xh[d,n] (+ score_b[k]); a = softmax of s over k in float32: m = max, e_k = expf(s_k - m),
 *             the sum in ascending k, a_k = e_k / sum.  Outputs assign [B,K,N] and inv_norm [B,N].  An all-zero location has xh = 0 and
 *             takes part with a = softmax(score_b).
 *  aggregate  V[d,k] = sum_n a[k,n] * xh[d,n] - centers[d,k] * sum_n a[k,n]: the GEMM form, which equals the literal
 *             sum_n a[k,n] (xh[d,n] - centers[d,k]) up to rounding; the two differ in a column whose residuals cancel (the literal
 *             form subtracts before it sums and keeps the small result's relative accuracy; this form's error is relative to
 *             sum |a xh| + |c| sum a).  Flag INTRANORM: V[:,k] /= max(||V[:,k]||_2, 1e-12) over d.  Flattened as v[b, d * K + k].
 *             Flag L2NORM: v /= max(||v||_2, 1e-12).  Flags 0: the raw V.  Reads features, assign, inv_norm and centers; never
 *             recomputes the softmax.
 *  project    y[b,o] = sum_i weight[o,i] * x[b,i] (+ bias[o]), weight [O,I] (nn.Linear's layout), bias [O] or NULL.  Flag L2NORM:
 *             y /= max(||y||_2, 1e-12).  x must not alias y.
 * Limits: 1 <= K <= SPLATRASTER_NETVLAD_MAX_K; D, N, O, I >= 1; B >= 0 (B = 0 returns SPLATRASTER_OK without a launch);
 * D * K < 2^31; one workgroup per (image, step of locations), per (image, block of d rows) and per (tile of o rows, slice of I, block of
 * images): each of these counts < 2^31.  Anything else, an unknown flag bit, a NULL or 4-byte-misaligned pointer, or a workspace
 * below the query's answer: SPLATRASTER_ERR_BAD_ARG before any launch.  Non-finite inputs are outside the contract (no loop depends
 * on data: they terminate).
 * Determinism: no float atomics; every sum has an order fixed by the shape alone; results are bit-identical run to run, and row b
 * of every output is bit-identical whatever B is. */
#define SPLATRASTER_NETVLAD_MAX_K 64
#define SPLATRASTER_NETVLAD_INTRANORM 1
#define SPLATRASTER_NETVLAD_L2NORM 2
/* Host only, never touches the device: the tile constants the launch geometry is built from.  n_step: locations per assign
 * workgroup and per aggregation step; d_tile: d rows per aggregation workgroup; i_slice: columns of I per projection workgroup
 * (the slices' partial sums are added in ascending order); o_tile / b_tile: weight rows and images of a projection tile. */
int splatraster_netvlad_tiles(int32_t* n_step, int32_t* d_tile, int32_t* i_slice, int32_t* o_tile, int32_t* b_tile);
/* Host only: bytes of workspace that serve every call below for B images of a [D,N] map, K clusters and an O x (D K) whitening
 * (pass O = 1 for a head without one).  Only project uses it (I / i_slice partial sums per output, rounded up); assign and aggregate
 * accept any workspace, NULL included.  (Named _size: the *_bytes queries are the ones tabulated in tests/test_host_workspace_sizes.py;
 * this one's sizes are pinned by tests/test_host_netvlad_head.py.) */
int splatraster_netvlad_workspace_size(int32_t B, int32_t D, int32_t K, int32_t N, int32_t O, size_t* bytes);
int splatraster_netvlad_assign(int32_t B, int32_t D, int32_t K, int32_t N, const float* features, const float* score_w,
                               const float* score_b, float* assign, float* inv_norm, void* workspace, size_t workspace_bytes,
                               void* stream);
int splatraster_netvlad_aggregate(int32_t B, int32_t D, int32_t K, int32_t N, const float* features, const float* assign,
                                  const float* inv_norm, const float* centers, int32_t flags, float* v, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* float4 loads where I % 4 == 0 and x and weight are 16-byte aligned, scalar loads otherwise: the same sums either way. */
int splatraster_netvlad_project(int32_t B, int32_t O, int64_t I, const float* x, const float* weight, const float* bias, int32_t flags,
                                float* y, void* workspace, size_t workspace_bytes, void* stream);

/* ---- convolution backbones: SuperPoint's encoder, NetVLAD's VGG16 trunk (csrc/conv2d.hip) --------- */

/* The layer both networks repeat, for B images per call, asynchronous on `stream`, nothing read back, no host synchronisation, no
 * float atomics.  All tensors are contiguous float32 NCHW device arrays.  Neither network's source is part of the reference tree, so
 * parity is unpinned; the layer below and the two layer tables of splatloc_amd/convnet.py are this project's
 * own contract.
 *  conv2d      out[b,co,y,x] = sum_{ci,ky,kx} weight[co,ci,ky,kx] * xp[b,ci,y + ky - p,x + kx - p] (+ bias[co]): cross-correlation,
 *              stride 1, ksize 1 or 3, p = (ksize - 1) / 2, xp = x padded with ZEROS; weight [Cout,Cin,ksize,ksize] (torch's layout),
 *              bias [Cout] or NULL.  Flag RELU: max(out, 0).  Flag POOL2: a 2x2 max pool with stride 2 in floor mode, applied after
 *              bias and ReLU, from the accumulators: out is [B,Cout,H/2,W/2], an odd last row or column is dropped, and the
 *              unpooled map is never written.  out must not alias x.
 *  THE CHAIN   every output is one float32 fmaf chain from zero, then + bias.  With C = ci_chunk of splatraster_conv2d_tiles:
 *                  acc = 0
 *                  for c0 = 0, C, 2 C, ... < Cin:  for ky = 0 .. ksize - 1:  for kx = 0 .. ksize - 1:  for ci = c0 .. c0 + C - 1:
 *                      acc = fmaf(weight[co,ci,ky,kx], xp[b,ci,y + ky - p,x + kx - p], acc)
 *                  out = acc + bias[co]
 *              where a channel ci >= Cin and a padded tap contribute fmaf(0, 0, acc) and fmaf(w, 0, acc), which are acc exactly: a
 *              border pixel and a channel tail follow the same statement.  The order is a function of (Cin, ksize) and C alone: not of
 *              B, of the pixel's position, of Cout or of the launch.  Cin = 1 and Cin = 3 take the same path (a chunk padded with
 *              zero channels), so there is no path hook.
 * Limits: B >= 0 (B = 0 returns SPLATRASTER_OK without a launch); Cin, Cout, H, W >= 1 (H, W >= 2 with POOL2); Cin H W, Cout H W and
 * ci_chunk H W < 2^31; one workgroup per (image, tile of channels, tile of pixels): that count < 2^31.  Anything else, a ksize outside
 * {1, 3}, an unknown flag bit, a NULL x, weight or out, or a 4-byte-misaligned pointer: SPLATRASTER_ERR_BAD_ARG before any device work.
 * The layer uses no workspace: any `workspace`, NULL included, is accepted.  All offsets are 64-bit.  Results are bit-identical run
 * to run, and image b of the output is bit-identical whatever B is. */
#define SPLATRASTER_CONV_RELU 1
#define SPLATRASTER_CONV_POOL2 2
/* Host only, never touches the device: the launch geometry.  co_tile: output channels per workgroup; px_rows x px_cols: its tile of
 * output pixels (both even: a pool window never straddles a tile); ci_chunk: input channels staged per step, the C of the chain. */
int splatraster_conv2d_tiles(int32_t* co_tile, int32_t* px_rows, int32_t* px_cols, int32_t* ci_chunk);
int splatraster_conv2d(int32_t B, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t ksize, const float* x, const float* weight,
                       const float* bias, int32_t flags, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* NetVLAD's input normalisation: rgb [B,3,H,W] in [0,1] -> out[b,c,y,x] = min(max(rgb * 255, 0), 255) - mean[c] with mean =
 * (123.68, 116.779, 103.939) in R, G, B order; three float32 operations, each rounded on its own.  A pass of its own, so the first
 * convolution pads with zeros and not with -mean.  B >= 0; H, W >= 1; 3 H W < 2^31; out may alias rgb. */
int splatraster_netvlad_preprocess(int32_t B, int32_t H, int32_t W, const float* rgb, float* out, void* stream);

/* ---- misc ---------------------------------------------------------------------------- */

/* The decoupled look-backs of the one-pass scan and of the one-sweep radix sort never give up with a
 * partial prefix (that would be a silently mis-sorted frame).  Soft bound: a block that has waited longer
 * than the spin limit raises a flag in host-mapped memory and keeps waiting — the frame stays correct, so
 * forward / backward / sort_pairs still return OK; splatraster_poll_errors() (exact after a stream
 * synchronize) returns SPLATRASTER_WARN_LOOKBACK_STALL once per raised flag, for monitoring.  Hard bound
 * (2^30 spins): the block traps, the kernel aborts and the following HIP calls fail -> SPLATRASTER_ERR_HIP:
 * a wedged device is a fault, never a silent hang. */
int splatraster_poll_errors(void);
/* test hooks: SOFT spin bound of the look-backs (default 1 << 24; 0 makes every block that has to wait at
 * all report), and y[i] = the device's 2^x (the alpha arithmetic shared with the CPU oracle). */
int splatraster_debug_set_spin_limit(uint32_t limit);
/* Deterministic debug mode of the backward (process-wide switch, default off).  The compositing backward sums
 * per-(wave, Gaussian) partials into per-Gaussian rows with float atomics, whose arrival order — and therefore the last bits of
 * every gradient — changes from run to run.  With the switch on,
 *   (1) each partial is converted to fixed point and accumulated with 64-bit INTEGER atomics (associative: the totals are
 *       bit-reproducible); the fixed point is chosen PER ELEMENT, 2^-44 of the largest partial the element receives
 *       (a first pass of the kernel takes that maximum, also an associative reduction) — round 3's single 2^-40 quantised the
 *       small rows of a large scene;
 *   (2) the per-pixel state of the back-to-front walk (T, A) is carried in double; split launches are not used.
 * Two passes of the kernel (~2.5 x slower).  Meant for regression hunting and the strictest tests.  (The NORMAL path is accurate
 * per gradient row since round 4 — it walks the lists back to front like the lineage; rounds 1-3 walked front to back and
 * carried an absolute float32 error in the suffix sum.) */
int splatraster_debug_set_deterministic(int on);
/* A/B hook: launches of the C = 4..15 backward with at most this many quadrant-waves take the small-layout panel
 * variant (HISTORY.md §11); < 0 restores the built-in default. */
int splatraster_debug_set_small_panel_max_waves(int waves);
/* A/B hook: narrow-layout launches (C <= 4) with at most this many quadrant-waves split every list of >= 256 entries in
 * four for the backward (the forward checkpoints every pixel's state at the quarter points of its tile's list; DESIGN.md §6.3, HISTORY.md §11).
 * 0 = never, < 0 or > 6144 = the built-in default 6144 (one 640x480 frame).  Must not change between a forward and its backward. */
int splatraster_debug_set_split_max_waves(int waves);
/* A/B / test hook: the forward of narrow layouts (C <= 4) walks the longest tile lists of a launch with a TEAM of four waves per
 * quadrant (two evaluate alpha for a step of candidates, one runs the transmittance chain a step behind, one accumulates
 * another step behind).  -1 (default): on the launches that are also split for the backward (at most 6144
 * quadrant lists: one 640x480 frame), 0: never, 1: every narrow launch of at most 32768 quadrant lists, 2 (tests): the same and a team for each of the 128 longest lists
 * whether or not they stand out.  Results never depend on it (bit-identical images, T, n_contrib, segment records). */
int splatraster_debug_set_fwd_team(int mode);
/* A/B / test hook: instance count from which the per-instance payload is written with streaming (non-temporal) stores
 * (HISTORY.md §11); < 0 restores the built-in default (8 Mi instances), 0 = always.  Results never depend on it. */
int splatraster_debug_set_payload_stream_min(int64_t instances);
/* A/B / test hook: the per-instance payload the compositing kernels stream (irec, ipack) holds only the instances that reach a
 * quadrant of their tile, each list compacted in place.  -1 (default): on behind the radix front end for launches
 * of one wave per quadrant over whole lists (not the team forward, not the split launches); 0: off — the full stream, one entry per
 * instance.  radii, num_rendered, point_list, tile_list, ranges, n_contrib and final_T never depend on it; colours, depth and
 * alpha are bit-identical for C <= 4 and C = 32..35 (C >= 36: which candidates share a pair-sum changes the last bit).  The
 * backward reads a binning buffer the way its render stage wrote it, whatever the switch says by then. */
int splatraster_debug_set_payload_compact(int mode);
/* A/B / test hook: the forward of wide layouts (C > 4) marks, in bits 28..31 of the payload word, the list entries it evaluated for a
 * quadrant without any pixel still accumulating AND past the alpha test (occluded footprints, Gaussians that pass between pixel
 * centres), and the backward does not walk them.  A render whose settings carry SPLATRASTER_SETTINGS_FORWARD_ONLY writes
 * no marks (a backward over it would walk every entry: correct, only slower).  1 (default): on; 0: the backward ignores the marks (the forward keeps
 * writing them).  Images, final_T, n_contrib and the lists never depend on it; gradients are bit-identical in the deterministic mode
 * and sums over the same pixels in the same order otherwise (which candidates share a pair or a flush group changes). */
int splatraster_debug_set_dead_marks(int on);
/* A/B / test hook: which front end orders the tile instances.  -1 (default): the binned front end (counting sort by
 * (view, tile) + one LDS sort per tile) for windows of at most 6144 (view, tile) lists — SplatLoc's own
 * 640x480 frames, singly or five at a time — and the two global radix sorts otherwise; 0: the radix sorts always; 1: the
 * binned front end whenever the shape allows (at most 16 384 tiles per view).  Both produce bit-identical point lists,
 * ranges and payloads.  The render stage follows the choice the GEOMETRY stage made for its geometry buffer: a change between the
 * two stages of a forward takes effect at the next geometry stage. */
int splatraster_debug_set_front_end(int mode);
/* A/B / test hook of the binned front end: the per-tile sort launch exists for lists of up to 2048 keys (128 threads, every
 * tile of a 640x480 frame resident at once) and of up to 4096 (256 threads); by default the library follows a hint the kernel
 * raises when it meets a list beyond 2048 keys (longer lists than the chosen launch holds go to the long-list launch either
 * way).  2048 / 4096 force an instantiation, any other value restores the default.  Results never depend on it. */
int splatraster_debug_set_tile_sort_cap(int keys);
/* Measurement hook.  The binned front end's two sort launches (lists up to the tile launch's cap | longer lists, which that launch
 * finds in the scanned table itself) are independent: 0 (default) = both on the caller's stream; -1 = the long-list launch on an
 * internal side stream — forked behind the key scatter, joined before the compositing grid — when a list beyond 2048 keys was seen
 * in the last 64 frames; 1 = always.  Measured a wash at Replica scale (profiles/r06_ab_probes.txt #6).  Results never depend on it. */
int splatraster_debug_set_sort_fork(int mode);
int splatraster_debug_exp2(int64_t n, const float* x, float* y, void* stream);
/* test hook: fills the LDS of every compute unit with `pattern` (e.g. a NaN's bits): enough workgroups of 64 KB each to cover
 * the whole array.  The compositing kernels read rows of their LDS staging buffers that a round did not write (the absent second
 * member of a round's last pair); their results must not depend on what the LDS held before the launch. */
int splatraster_debug_poison_lds(uint32_t pattern, void* stream);

const char* splatraster_error_string(int status);
/* last HIP error text recorded by this thread (empty string when none). */
const char* splatraster_last_hip_error(void);
int splatraster_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SPLATRASTER_H */
