/*
 * nsr.h -- C ABI of libnsr.so, the MI355X-native NICE-SLAM render hot path.
 *
 * Every entry point replaces a piece of the reference's *Python* interface (the reference has no
 * native code).  Citations are relative to the reference tree:
 *
 *   nsr_get_samples      <- src/common.py:125-134  get_samples (after the torch.randint draw)
 *   nsr_aabb_keep        <- src/Mapper.py:471-481, src/Tracker.py:95-104  bounding-box pre-filter (mask, no compaction)
 *   nsr_pack_params      <- (none) operand re-layout of src/conv_onet/models/decoder.py parameters
 *   nsr_render_fwd       <- src/utils/Renderer.py:63-198  Renderer.render_batch_ray  (forward)
 *                           incl. eval_points (:23-61), NICE.forward (decoder.py:312-342),
 *                           raw2outputs_nerf_color (src/common.py:204-245)
 *   nsr_render_bwd       <- the autograd backward of the above (src/Mapper.py:503, src/Tracker.py:125)
 *   nsr_eval_points_fwd  <- src/utils/Renderer.py:23-61   Renderer.eval_points (forward only)
 *   nsr_masked_adam      <- src/Mapper.py:368-379,394-401,504,511-519  masked write-back + Adam on one feature grid
 *   nsr_masked_adam_multi <- the same for all grids of a stage, step counts on the device (capturable)
 *   nsr_flat_adam        <- src/Mapper.py:368-387,504, src/Tracker.py:214-222,127  torch.optim.Adam on the dense rest of the
 *                           callers' optimiser (decoder parameter blobs, camera tensors), one launch pair, capturable
 *   nsr_get_samples_window <- src/Mapper.py:437-481  sampling loop over the mapping window + bounding-box pre-filter
 *   nsr_get_samples_window_fused <- the same as the first launch of a fused iteration: + the pixel draw of src/common.py:99 and the
 *                           zero fill that `loss.backward()` (src/Mapper.py:503) relies on, inside the one launch (ABI 7)
 *   nsr_get_samples_window_sharded <- the same for one rank of a ray-sharded iteration: + the batch-global max(gt_depth) of
 *                           src/utils/Renderer.py:109,144 over ALL ranks' draws, without a collective (ABI 8)
 *   nsr_pose_grad        <- autograd of src/common.py:74-88 for that window (local BA, src/Mapper.py:417-419)
 *   nsr_pack_rows        <- (none) gather / scatter of the voxel rows + blobs that travel in the multi-GPU all-reduce
 *   nsr_mc_* / nsr_point_masks / nsr_cc_* <- src/utils/Mesher.py:53-212,349-574  marching cubes, point_masks, mesh.split
 *   nsr_nn_* / nsr_sample_surface / nsr_dist_stats / nsr_icp_stats / nsr_transform_points / nsr_cull_vertices
 *   nsr_meshdist_* / nsr_face_normals / nsr_normal_stats
 *                        <- src/tools/eval_recon.py:24-59,91-117, src/tools/cull_mesh.py:45-75  reconstruction evaluation
 *   nsr_raster_* / nsr_depth_error / nsr_view_unseen
 *                        <- src/tools/eval_recon.py:131-211  depth rendering and the 2-D depth metric
 *   nsr_frame_out_size / nsr_frame_workspace_bytes / nsr_frame_prepare
 *                        <- src/utils/datasets.py:77-113  BaseDataset.__getitem__ between the decoded files and the tensors
 *
 * Conventions
 *   - all pointers are DEVICE pointers owned by the caller (PyTorch); the library never frees or
 *     retains them beyond the call.  No torch types cross this boundary.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises.
 *   - every function returns 0 on success; on failure a non-zero code and nsr_last_error()
 *     (thread-local, valid until the next failing call on that thread) describes it.
 *   - feature grids are fp32, 32 channels, CHANNELS-LAST: element (z,y,x,c) at ((z*Y+y)*X+x)*32+c.
 *     This is the physical layout of a torch tensor of logical shape [1,32,Z,Y,X] in
 *     torch.channels_last_3d memory format (reference logical shape: src/NICE_SLAM.py:218-222).
 *   - decoder parameters are ONE flat fp32 blob per decoder in the order of the reference module's
 *     named_parameters() (decoder.py:124-159 / :235-245), see nsr_param_count().
 */
#ifndef NSR_H_
#define NSR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSR_VERSION 8

/* stages of NICE.forward (decoder.py:312-342) */
enum { NSR_STAGE_COARSE = 0, NSR_STAGE_MIDDLE = 1, NSR_STAGE_FINE = 2, NSR_STAGE_COLOR = 3 };
/* decoder / grid slots */
enum { NSR_COARSE = 0, NSR_MIDDLE = 1, NSR_FINE = 2, NSR_COLOR = 3 };

#define NSR_MAX_SAMPLES 64

typedef struct nsr_grid {
    const float *feat;   /* [Z][Y][X][32] */
    float *dfeat;        /* gradient accumulator, same layout, caller-zeroed; NULL = not needed */
    int32_t Z, Y, X;     /* Z * Y * X < 2^25 voxels (a grid is addressed with 32-bit byte offsets: 4 GB)   */
    int32_t pad_;
    double lo[3];        /* normalisation box of the decoder reading this grid, xyz order          */
    double hi[3];        /* (decoder .bound, src/NICE_SLAM.py:152-157; coarse = scene bound * 2)   */
} nsr_grid;

typedef struct nsr_decoder {
    const float *params; /* flat blob, nsr_param_count(slot) floats                                */
    const float *packed; /* MFMA operand stream written by nsr_pack_params, nsr_packed_count(slot) */
    float *dparams;      /* flat gradient blob (caller-zeroed) or NULL                             */
} nsr_decoder;

typedef struct nsr_render_args {
    int32_t stage;            /* NSR_STAGE_*                                                        */
    int32_t n_samples;        /* uniform samples per ray  (cfg rendering.N_samples)                 */
    int32_t n_surface;        /* near-surface samples; forced to 0 when gt_depth == NULL or coarse  */
    int32_t pad_;
    int64_t n_rays;
    const float *rays_o;      /* [N][3] */
    const float *rays_d;      /* [N][3] */
    const float *gt_depth;    /* [N] or NULL (Renderer.py:88-96)                                    */
    const float *gt_max;      /* device scalar: max over the WHOLE batch of gt_depth (Renderer.py:109,144);
                                 required when gt_depth != NULL.  Kept on device: no host sync.     */
    double bound_lo[3];       /* Renderer.bound (un-enlarged): far_bb and the in-bound test         */
    double bound_hi[3];
    float t_uniform[NSR_MAX_SAMPLES];   /* torch.linspace(0,1,n_samples) fp32 (Renderer.py:152)     */
    double t_surface[NSR_MAX_SAMPLES];  /* torch.linspace(0,1,n_surface).double() (Renderer.py:132) */
    nsr_grid grid[4];         /* slots NSR_COARSE..NSR_COLOR; unused slots may be zeroed            */
    nsr_decoder dec[4];
    /* outputs */
    double *depth;            /* [N]    */
    double *var;              /* [N]    */
    float *rgb;               /* [N][3] */
    float *raw;               /* [N][S][4] decoder output after the out-of-bound override, S = n_samples+n_surface;
                                 written by fwd, read by bwd.  May be NULL for a forward-only call.  */
    double *zvals;            /* [N][S] sorted sample depths, written by fwd when non-NULL; required (like acts and raw) by a call
                                 that will be differentiated                                                            */
    /* --- fused mapping loss (src/Mapper.py:487-493), optional: all NULL / 0 for the plain renderer ------------------
     * fwd with loss != NULL adds   sum over rays r with keep[r] of  [gt_depth[r] > 0] |gt_depth[r] - depth[r]|   (gt_depth
     *                              as passed in this block, also in the coarse stage whose SAMPLING ignores it)
     *                              + (colour stage) w_color * sum_c |gt_color[r][c] - rgb[r][c]|     to *loss (fp64)
     * and writes that sum's derivative w.r.t. each ray's outputs to dl_depth / dl_rgb -- exactly the arrays
     * nsr_render_bwd takes as d_depth / d_rgb (d_var = NULL), so the caller's loss and its backward cost no launch. */
    const float *gt_color;    /* [N][3] */
    const uint8_t *keep;      /* [N] ray mask of the callers' bounding-box pre-filter (nsr_aabb_keep / nsr_get_samples_window);
                                 NULL = every ray counts.  With skip_masked the kernels read it through the scalar cache one
                                 aligned 32-bit word at a time: the buffer must be readable up to the next 4-byte boundary
                                 behind its last byte (any allocator's padding; do not hand in the tail of a page-exact mapping) */
    double *loss;             /* device scalar, caller-zeroed */
    double *dl_depth;         /* [N]    out, optional */
    float *dl_rgb;            /* [N][3] out, optional */
    float w_color;            /* cfg mapping.w_color_loss */
    int32_t acts_masks_only;  /* with `acts`: 1 = the backward will want no parameter gradients (tracking), the forward only
                                 writes the relu masks (1 of the 13 KB per tile and decoder); 0 = everything.  ABI 8: bits 1..3 say the
                                 same for ONE decoder pass each (2: middle -- or the coarse stage's only pass --, 4: fine, 8: colour): a
                                 decoder nobody will step (src/Mapper.py:335-341 steps the colour decoder only) saves its masks only */
    /* --- saved decoder activations + workspace of the split backward (ABI 3/4; required for a call that will be differentiated since
     * ABI 6).  nsr_acts_floats(stage, n_rays, n_samples + n_surface) floats, device, uninitialised: nsr_render_fwd (given acts, zvals
     * and raw) runs as sample placement -> decoder passes -> compositor and writes, per decoder pass and 16-point tile of the sample list,
     * the five hidden states, the decoder's grid features and the relu masks (13 KB), the sample positions (fp64 and fp32) and, with the
     * fused loss, d raw; nsr_render_bwd, given the SAME pointer, runs dX / dW / finalize over them.  NULL, or given without zvals
     * or raw: forward only (one launch, nothing saved, the buffer stays untouched); nsr_render_bwd then fails. */
    float *acts;
    void *ev_pass_start;      /* ABI 6, optional hipEvent_t pair recorded on `stream` right before / after the decoder-pass kernel of */
    void *ev_pass_stop;       /* a differentiated forward (the forward's dominant kernel); NULL = no timing                           */
    int32_t skip_masked;      /* ABI 6, with `keep`: 1 = rays with keep[r] == 0 are REMOVED from the batch like the reference's
                                 compaction does (src/Mapper.py:471-481, src/Tracker.py:95-104: `batch_rays_d[inside_mask]`): no
                                 decoder evaluation, outputs depth = var = rgb = 0, no loss term, no gradient.  Their slots of
                                 raw / zvals / acts stay unwritten.  nsr_render_bwd must be given the same keep / skip_masked.
                                 Honoured by calls that will be differentiated (acts + zvals + raw given); a forward-only call
                                 renders every ray.  0 (default): keep only masks the fused loss; every ray is rendered. */
    int32_t pad2_;
    const uint8_t *grad_voxel_mask[4]; /* ABI 8, opt-in, read by nsr_render_bwd only: per grid slot a [Z][Y][X] byte mask (the layout
                                 nsr_frustum_mask writes and nsr_masked_adam takes) of the voxels whose gradient the caller will
                                 CONSUME.  With `frustum_feature_selection` the mapper's optimiser holds only `val[mask]`
                                 (src/Mapper.py:315-333,394-401): the reference's autograd scatters into the whole grid and
                                 `val.grad[~mask]` is never read.  Given a mask, the backward's scatter skips voxels whose byte is 0:
                                 dfeat of voxels inside the mask equals the dense run's (up to the order of the atomic adds),
                                 dfeat of voxels outside stays as the caller left it (zero).  Ray / pose and decoder gradients are
                                 unaffected (they never depended on dfeat).  NULL (default) = the reference's dense gradient. */
} nsr_render_args;

typedef struct nsr_bwd_args {
    const double *d_depth;    /* [N]    dL/d depth   */
    const double *d_var;      /* [N]    dL/d var, may be NULL (== 0)  */
    const float *d_rgb;       /* [N][3] dL/d rgb, may be NULL (== 0)  */
    const double *depth;      /* [N]    forward result (needed for the variance term) */
    float *d_rays_o;          /* [N][3] caller-zeroed, or NULL */
    float *d_rays_d;          /* [N][3] caller-zeroed, or NULL */
    float *workspace;         /* nsr_bwd_workspace_floats() floats, contents undefined */
    int64_t workspace_floats;
    int32_t max_blocks;       /* persistent-grid cap used to size the workspace (0 = library default) */
    int32_t overwrite_dparams; /* 0: every nsr_decoder.dparams is ACCUMULATED into (autograd semantics, caller-zeroed for a
                                 fresh gradient); 1: it is OVERWRITTEN (saves the caller the zero fill) */
    void *ev_start;           /* optional hipEvent_t pair recorded on `stream` right before the first / after the last */
    void *ev_stop;            /* kernel of the backward; NULL = no timing                                               */
    const double *grad_scale; /* optional DEVICE scalar every output gradient (d_depth, d_var, d_rgb) is multiplied by -- the
                                 incoming gradient of a loss node fused around the render (no host sync, no extra launch);
                                 NULL = 1 */
    int32_t loss_grads_from_forward; /* ABI 6, opt-in.  1: d_depth / d_rgb ARE nsr_render_args.dl_depth / dl_rgb exactly as the forward's
                                 loss epilogue wrote them (same pointers, contents unmodified, d_var NULL): the backward then uses
                                 the per-sample `d raw` that epilogue already left in `acts` and skips the compositor backward (one
                                 launch).  0 (default): d_depth / d_var / d_rgb are read as given -- a caller may mask or re-weight
                                 dl_* in place before the backward.  Only grad_scale is applied on top in either case. */
    int32_t pad_;
    void *ev_dx_done;         /* ABI 6, optional hipEvent_t recorded behind the dX kernel / behind the dW kernel: with ev_start / ev_stop */
    void *ev_dw_done;         /* they give the time of each kernel of the backward (dX | dW | finalize)                                 */
} nsr_bwd_args;

int nsr_version(void);
const char *nsr_last_error(void);

/* number of fp32 parameters of decoder slot `slot` (coarse 6 337 / middle 15 800 / fine 20 920 / color 15 899) */
int64_t nsr_param_count(int slot);
/* number of floats of the packed operand stream for decoder slot `slot` */
int64_t nsr_packed_count(int slot);
/* size of nsr_render_args.acts in floats (-1 on bad arguments) */
int64_t nsr_acts_floats(int stage, int64_t n_rays, int n_samples_total);

/* floats of scratch nsr_render_bwd needs for (stage, n_rays, max_blocks) */
int64_t nsr_bwd_workspace_floats(int stage, int64_t n_rays, int n_samples_total, int max_blocks);

int nsr_pack_params(int slot, const float *params, float *packed, void *stream);

int nsr_render_fwd(const nsr_render_args *a, void *stream);
int nsr_render_bwd(const nsr_render_args *a, const nsr_bwd_args *b, void *stream);

/* Renderer.eval_points forward: p [M][3] fp64 world points -> out [M][4] fp32 (rgb, occ) */
int nsr_eval_points_fwd(const nsr_render_args *a, const double *points, int64_t n_points, float *out, void *stream);

/* get_samples after the index draw: flat indices into the crop [H0,H1)x[W0,W1) (row-major) ->
 * rays + gathered depth/colour.  c2w is a row-major 3x4 (or 4x4) fp32 matrix with row stride c2w_stride. */
int nsr_get_samples(const int64_t *indices, int64_t n, int32_t H0, int32_t H1, int32_t W0, int32_t W1,
                    int32_t W_full, float fx, float fy, float cx, float cy,
                    const float *c2w, int32_t c2w_stride, const float *depth, const float *color,
                    float *rays_o, float *rays_d, float *out_depth, float *out_color, void *stream);

/* --- the mapper's sampling loop in one launch -----------------------------------------------------------------------------
 * Replaces, for the K frames of the mapping window, the K get_samples calls + torch.cat of src/Mapper.py:437-468 and the
 * bounding-box pre-filter of :471-481 (as a mask, like nsr_aabb_keep): indices [K][n] (row-major flat indices into the crop,
 * one draw per frame), frames[k] = that frame's depth [H][W], colour [H][W][3] and pose (row-major 3x4 or 4x4, row stride
 * c2w_stride floats), all device pointers; outputs are the concatenation over frames, [K*n] rays.  keep / kept_max optional
 * (kept_max caller-zeroed).  bound_lo / bound_hi: HOST arrays of 3 doubles.  K <= 32. */
typedef struct nsr_frame {
    const float *depth;
    const float *color;
    const float *c2w;
    int32_t c2w_stride;
    int32_t pad_;
} nsr_frame;
int nsr_get_samples_window(const int64_t *indices, int32_t K, int64_t n, int32_t H0, int32_t H1, int32_t W0, int32_t W1,
                           int32_t W_full, float fx, float fy, float cx, float cy, const nsr_frame *frames,
                           float *rays_o, float *rays_d, float *out_depth, float *out_color,
                           const double *bound_lo, const double *bound_hi, uint8_t *keep, float *kept_max, void *stream);
/* The same with the pixel draw of src/common.py:99 (`torch.randint(h * w, (n,))`, one call per keyframe there) inside the
 * kernel: ray t of the window takes one uniform index in [0, crop_h * crop_w) from philox4x32-10 (counter = (t, calls so far),
 * key = seed) and the drawn indices are written to indices_out [K * n] (for nsr_pose_grad and the caller).  rng_state: three
 * uint64 on the device -- {seed, calls so far, 0} -- owned by the caller and advanced by the kernel, so that a captured graph
 * draws afresh on every replay without the host.  Same distribution as the reference's draw, not the same stream. */
int nsr_get_samples_window_draw(int64_t *indices_out, uint64_t *rng_state, int32_t K, int64_t n, int32_t H0, int32_t H1, int32_t W0,
                                int32_t W1, int32_t W_full, float fx, float fy, float cx, float cy, const nsr_frame *frames,
                                float *rays_o, float *rays_d, float *out_depth, float *out_color,
                                const double *bound_lo, const double *bound_hi, uint8_t *keep, float *kept_max, void *stream);
/* The window kernel as the FIRST launch of a fused iteration (ABI 7): beside the sampling it zero-fills the iteration's gradient
 * buffer -- x-blocks of its own that store zeros over zero[0 .. zero_floats) (16-byte aligned) while the others place the rays:
 * the fill is bandwidth, the sampling a chain of latencies, side by side they cost the longer of the two instead of two launches
 * (src/Mapper.py:503: `loss.backward()` accumulates into zeroed .grad tensors; Mapper.py:437-481 for the sampling) -- and its last
 * block to finish writes the iteration's 16-byte header {loss accumulator (fp64) = 0, kept_max, 0.f}: nothing has to be zeroed
 * before the launch.  indices: [K * n] or NULL (then drawn as in nsr_get_samples_window_draw and written to indices_out).
 * state: four uint64 on the device -- {seed, calls so far, 0, 0} -- owned by the caller; words 2 and 3 are the launch's hand-off
 * (blocks done, bit pattern of the running maximum) and are zero again when it ends; two launches that share a state must not
 * overlap.  header must be 16-byte aligned (one 16-byte store), state 8-byte aligned.  K, n >= 1. */
int nsr_get_samples_window_fused(const int64_t *indices, int64_t *indices_out, uint64_t *state, int32_t K, int64_t n, int32_t H0, int32_t H1,
                                 int32_t W0, int32_t W1, int32_t W_full, float fx, float fy, float cx, float cy, const nsr_frame *frames,
                                 float *rays_o, float *rays_d, float *out_depth, float *out_color,
                                 const double *bound_lo, const double *bound_hi, uint8_t *keep, float *header,
                                 float *zero, int64_t zero_floats, void *stream);
/* The fused window launch of ONE RANK of a ray-sharded mapping iteration (ABI 8; one process per GPU): the in-kernel
 * pixel draw of nsr_get_samples_window_fused for this rank's state, and -- instead of an all-reduce of the kept rays' maximum depth,
 * the one scalar of the WHOLE batch the render needs (src/utils/Renderer.py:109,144) -- the same draw REPEATED for the other ranks:
 * peer_seeds (HOST array, n_peers <= 15 entries) are the seeds of their states, every rank has made the same number of calls (the
 * call counter of `state` is used for all of them), keyframes and poses are replicated: extra blocks re-draw peer p's pixels, gather
 * their depths and apply the bounding-box pre-filter (src/Mapper.py:471-481) without writing any ray, and the header's kept maximum
 * becomes the maximum over the union batch -- bit-identical on every rank, no collective between the sampling and the render.
 * header: 16-byte aligned; state: 8-byte aligned (also required by nsr_get_samples_window_fused). */
int nsr_get_samples_window_sharded(int64_t *indices_out, uint64_t *state, const uint64_t *peer_seeds, int32_t n_peers, int32_t K, int64_t n,
                                   int32_t H0, int32_t H1, int32_t W0, int32_t W1, int32_t W_full, float fx, float fy, float cx, float cy,
                                   const nsr_frame *frames, float *rays_o, float *rays_d, float *out_depth, float *out_color,
                                   const double *bound_lo, const double *bound_hi, uint8_t *keep, float *header,
                                   float *zero, int64_t zero_floats, void *stream);
/* gradient of the K poses from the ray gradients of such a window (autograd of src/common.py:74-88; local BA,
 * src/Mapper.py:417-419,441-453): d_c2w + k * out_stride holds rows 0..2 of pose k's gradient, row-major (12 floats;
 * out_stride = 12 for 3x4 poses, 16 for 4x4 ones whose last row the caller zero-fills). */
int nsr_pose_grad(const int64_t *indices, int32_t K, int64_t n, int32_t H0, int32_t H1, int32_t W0, int32_t W1,
                  float fx, float fy, float cx, float cy, const float *d_rays_o, const float *d_rays_d,
                  float *d_c2w, int32_t out_stride, void *stream);

/* --- the per-iteration grid update of Mapper.optimize_map, fused ---------------------------------
 * Replaces, for one feature grid, `val[mask] = val_grad` (src/Mapper.py:394-401), the Adam step on the masked leaf
 * (:368-379,504, torch.optim.Adam defaults) and the write-back `val[mask] = val_grad.detach()` (:511-519) by one in-place
 * pass over the grid: for every voxel whose mask byte is non-zero (mask == NULL: every voxel) and each of its 32 channels
 *     m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= step_size * m / (sqrt(v)/bias2_sqrt + eps)
 * with step_size = lr/(1-b1^t) and bias2_sqrt = sqrt(1-b2^t) evaluated by the caller in double precision, exactly the two
 * host scalars torch.optim.Adam forms (t = number of steps in which this grid received a gradient).
 * p, g, m, v: [Z][Y][X][32] fp32 (channels-last, like every grid of this ABI); voxel_mask: [Z][Y][X] uint8.
 * lr == 0 still updates the moments, exactly like torch.optim.Adam. */
int nsr_masked_adam(float *p, const float *g, float *m, float *v, const uint8_t *voxel_mask, int64_t n_voxels,
                    float step_size, float beta1, float beta2, float eps, float bias2_sqrt, void *stream);

/* The same for up to 4 grids in ONE launch pair with the step counts kept on the device, so that a whole mapping iteration
 * can be captured in a hipGraph (no host scalar changes between replays): steps[i] (device int32, one per grid) is
 * incremented, step_size = lr / (1 - b1^t) and bias2_sqrt = sqrt(1 - b2^t) are formed on the device in fp64, then every
 * grid is updated like nsr_masked_adam does.  zero_grad != 0 also clears the gradient of the voxels it read (so that a
 * persistent, accumulated-into gradient buffer needs no separate fill).  scratch: 8 device floats. */
typedef struct nsr_adam_grid {
    float *p;
    float *g;
    float *m;
    float *v;
    const uint8_t *voxel_mask;
    int64_t n_voxels;
    int32_t *step;            /* device counter of this grid */
    float lr;
    int32_t pad_;
} nsr_adam_grid;
int nsr_masked_adam_multi(const nsr_adam_grid *grids, int32_t n_grids, double beta1, double beta2, double eps,
                          int32_t zero_grad, float *scratch, void *stream);   /* (betas as doubles since ABI 7: the bias corrections
                          1 - beta^t are formed from them in fp64, like torch's python scalars) */

/* The dense rest of the callers' optimiser -- torch.optim.Adam over the decoder parameters and the camera tensors
 * (src/Mapper.py:368-387,504; src/Tracker.py:214-222,127) -- for up to 4 flat fp32 spans (a decoder's parameter blob, an [n,7] pose
 * tensor) in ONE launch pair with the step counts on the device: the same single-tensor Adam arithmetic as nsr_masked_adam_multi
 * (lerp / addcmul / addcdiv order, bias corrections formed on the device in fp64; lr == 0 still updates the moments), every element of
 * every span.  torch's capturable Adam takes ~10 launches per step for the same; together with nsr_masked_adam_multi a whole optimiser
 * step of a mapping iteration is four launches.  zero_grad != 0 clears the gradient it read.  scratch: 8 device floats. */
typedef struct nsr_adam_span {
    float *p;
    float *g;
    float *m;
    float *v;
    int64_t n;
    int32_t *step;            /* device counter of this span */
    float lr;
    int32_t pad_;
} nsr_adam_span;
int nsr_flat_adam(const nsr_adam_span *spans, int32_t n_spans, double beta1, double beta2, double eps, int32_t zero_grad, float *scratch,
                  void *stream);     /* betas as doubles: 1 - beta is formed in fp64 and then rounded, like torch's `value=1 - beta2` */

/* --- packing for the one-collective gradient exchange -------------------------------------------------------
 * Gathers (unpack = 0) the listed voxel rows (32 floats each, rows[] = voxel indices in [Z][Y][X] raster order) of up to 4
 * channels-last grid-gradient tensors and up to 4 flat spans into `packed` (rows of grid 0, grid 1, ..., then the spans), or
 * scatters `packed` back (unpack = 1).  The caller all-reduces `packed` in between (torch.distributed / RCCL): the library
 * itself stays free of communication.  Replaces the nsr_comm_* / nsr_reduce_grid_grads entry points sketched in SURVEY §8(b). */
typedef struct nsr_rows {
    float *grid;
    const int64_t *rows;
    int64_t n_rows;
} nsr_rows;
typedef struct nsr_span {
    float *ptr;
    int64_t n;
} nsr_span;
int nsr_pack_rows(const nsr_rows *grids, int32_t n_grids, const nsr_span *spans, int32_t n_spans, float *packed,
                  int32_t unpack, void *stream);

/* The tracker's loss on rendered outputs -- src/Tracker.py:108-124 (Tracker.optimize_cam_in_batch): with
 * tmp = |gt_depth - depth| / sqrt(var + 1e-10) (fp64, `var` detached), mask = keep & (gt_depth > 0) and, when
 * handle_dynamic, & (tmp < 10 * median(tmp over the kept rays)) (torch.median: the lower middle element; NaN if any
 * element is NaN),
 *     *loss += sum_mask tmp  [+ w_color * sum_mask |gt_color - rgb|   when use_color]
 * and dl_depth [n] / dl_rgb [n][3] receive d loss / d depth and d loss / d rgb -- what autograd would hand to the backward
 * of render_batch_ray (feed them to nsr_render_bwd as d_depth / d_rgb).  `keep` (or NULL) is the bounding-box pre-filter
 * of :92-104 as a byte mask (nsr_aabb_keep / nsr_get_samples_window): the reference compacts the batch instead, so its
 * median runs over exactly the kept rays.  One launch, no host synchronisation, any n. */
int nsr_tracking_loss(int64_t n_rays, const float *gt_depth, const float *gt_color, const uint8_t *keep,
                      const double *depth, const double *var, const float *rgb,
                      int32_t handle_dynamic, int32_t use_color, float w_color,
                      double *loss, double *dl_depth, float *dl_rgb, void *stream);

/* get_camera_from_tensor / quad2rotation -- src/common.py:137-176: n camera tensors [quaternion (w,x,y,z) | translation]
 * (7 floats each) -> n 3x4 matrices [R | T] in `rt` (d_rt == NULL), or -- d_rt != NULL -- the backward: d_cam [n][7] from
 * d_rt [n][3][4].  The pose parametrisation of the tracker and of local BA (Tracker.py:87, Mapper.py:447-451). */
int nsr_camera_from_tensor(const float *cam, int64_t n, float *rt, const float *d_rt, float *d_cam, void *stream);

/* --- frustum feature selection ---------------------------------------------------------------------
 * Replaces Mapper.get_mask_from_c2w (src/Mapper.py:93-164) for one non-coarse feature grid: every voxel centre (xs[ix],
 * ys[iy], zs[iz]: the per-axis torch.linspace over the scene bound, :111-113, device arrays) is projected with
 * w2c = inv(c2w) (HOST array, 12 floats = rows 0..2; :120-131), its depth is looked up in the current depth image with
 * cv2.remap INTER_LINEAR semantics (:133-140), zero depths are replaced by the maximum remapped depth (:147-148), and the
 * voxel is selected when it projects inside the image with 0 <= -z <= depth + 0.5 (:142-151) or lies within 0.5 m of the
 * camera centre cam_center (HOST array, 3 floats; :155-161).
 * depth: [H][W] fp32 device; voxel_mask: [Z][Y][X] uint8 device (the layout nsr_masked_adam takes; the reference's
 * (X,Y,Z) return value is its transpose, which Mapper.py:318 undoes); workspace: nsr_frustum_workspace_floats(nx*ny*nz)
 * floats of device scratch. */
int64_t nsr_frustum_workspace_floats(int64_t n_voxels);
int nsr_frustum_mask(const float *w2c, const float *cam_center, double fx, double fy, double cx, double cy,
                     int32_t H, int32_t W, const float *depth, const float *xs, const float *ys, const float *zs,
                     int32_t nx, int32_t ny, int32_t nz, float *workspace, uint8_t *voxel_mask, void *stream);

/* --- Overlap keyframe selection --------------------------------------------------------------------------------------------
 * The arithmetic of Mapper.keyframe_selection_overlap (src/Mapper.py:166-228) in one launch: for each of the n_rays drawn pixel
 * indices (flat into the [H][W] frame, device int64; the draw of get_samples, :185-186) the ray is formed as nsr_get_samples
 * forms it (fp32 intrinsics, pose c2w: device, rows 0..2 c2w_stride floats apart); n_samples points per ray at
 * z = near * (1 - t) + far * t, near = depth * 0.8, far = depth + 0.5 (fp32; t_vals: HOST array of n_samples floats, the
 * reference's torch.linspace(0, 1, n_samples) on the CPU, :187-196).  Each point is projected with each keyframe's
 * w2c = inv(est_c2w) rows 0..2 (w2c: [K][12] fp32 device; fp32 sum, x negated, fp64 K, z + 1e-5, uv rounded to fp32, :199-212)
 * and counted when edge < u < W - edge, edge < v < H - edge and z < 0 (:213-217).  counts: [K] int32 device, fully written:
 * counts[k] / (n_rays * n_samples) is the reference's percent_inside of keyframe k.  Deterministic; no zero fill needed.
 * 1 <= n_samples <= 64, 1 <= n_rays <= 2^24, 0 <= 2 * edge < min(H, W) (the reference uses edge = 20); K = 0 launches nothing
 * (w2c and counts may then be NULL). */
int nsr_keyframe_overlap(const int64_t *indices, int32_t n_rays, int32_t n_samples, const float *t_vals,
                         int32_t H, int32_t W, double fx, double fy, double cx, double cy, int32_t edge,
                         const float *c2w, int32_t c2w_stride, const float *depth,
                         const float *w2c, int32_t K, int32_t *counts, void *stream);

/* --- SURVEY §8(f) rank 1 (third item): the callers' bounding-box pre-filter without compaction --------------------------
 * Mapper.optimize_map (src/Mapper.py:471-481) and Tracker.optimize_cam_in_batch (src/Tracker.py:95-104) drop, before
 * rendering, every ray whose depth lies beyond the scene bound:  t = min_axis max((lo-o)/d, (hi-o)/d)  (fp64),
 * keep = t >= gt_depth, then index all four ray tensors with the boolean mask (a `nonzero` = a host sync per iteration).
 * nsr_aabb_keep writes the same mask as bytes and, if kept_max != NULL (device float, caller-set to 0), the maximum
 * gt_depth over the KEPT rays -- the batch-global scalar render_batch_ray needs -- so a caller can render the whole batch
 * and weight its loss by the mask instead of compacting.  bound_lo / bound_hi: HOST arrays of 3 doubles. */
int nsr_aabb_keep(const float *rays_o, const float *rays_d, const float *gt_depth, int64_t n,
                  const double *bound_lo, const double *bound_hi, uint8_t *keep, float *kept_max, void *stream);

/* --- Mesh extraction (src/utils/Mesher.py:349-574) ---------------------------------------------------------------------
 * Marching cubes over a dense fp32 lattice vol [nx][ny][nz] (x slowest), welded: one vertex per lattice edge whose end values
 * straddle `level` (a corner is above iff f > level), in lattice-edge-id order 3 * (linear index of the lower end) + axis;
 * the vertex on the edge a -> a + e_axis is origin + (i + t) * spacing (fp64) with t = (level - f_a) / (f_b - f_a) in fp32.
 * Faces index those vertices, in cell order, then in the order of the case table; a cell face is cut by a rule of its own
 * four signs (crack-free); face normals point toward decreasing field.  Bit-identical output run to run.
 *   nsr_mc_workspace_bytes   device scratch for both calls (-1 for a dimension below 2 or more than 2^31 points)
 *   nsr_mc_count             writes counts[0] = n_verts, counts[1] = n_faces (int64, device) and fills the workspace
 *   nsr_mc_emit              after nsr_mc_count on the same workspace: verts [n_verts][3] fp64, faces [n_faces][3] int32;
 *                            fails when n_verts or 3 * n_faces exceeds INT32_MAX.  origin / spacing: HOST arrays of 3. */
int64_t nsr_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int nsr_mc_count(const float *vol, int32_t nx, int32_t ny, int32_t nz, float level, void *workspace, int64_t *counts, void *stream);
int nsr_mc_emit(const float *vol, int32_t nx, int32_t ny, int32_t nz, float level, const double *origin, const double *spacing,
                void *workspace, int64_t n_verts, int64_t n_faces, double *verts, int32_t *faces, void *stream);

/* Seen / forecast / unseen classification of points [n][3] fp32 (Mesher.point_masks, :53-212) against K cameras given as
 * w2c = inv(c2w) computed in fp64 and cast to fp32, rows 0..2 ([K][12] device).  mode 0: get_mask_use_all_frames (frustum
 * and z < 0); 1: keyframes without depth test (projected depth < limit[k] = max(depth_k) * 1.1, [K] device); 2: keyframes
 * with depth test (depth [K][H][W] device sampled as F.grid_sample(bilinear, zeros, align_corners=True); seen within
 * +-2.4; forecast below the maximum sampled depth over the point's chunk of `chunk` points -- the reference's
 * points_batch_size).  out[i]: 0 unseen, 1 seen, 2 forecast.  workspace: nsr_point_masks_workspace_floats floats (mode 2). */
int64_t nsr_point_masks_workspace_floats(int64_t n, int64_t chunk, int32_t K);
int nsr_point_masks(const float *points, int64_t n, int64_t chunk, int32_t mode, int32_t K, const float *w2c, const float *depth,
                    const float *limit, int32_t H, int32_t W, double fx, double fy, double cx, double cy, float *workspace,
                    uint8_t *out, void *stream);

/* Connected components over pairs of elements (faces sharing an edge, trimesh's face_adjacency): nsr_cc_init once, then
 * nsr_cc_round with round = 0, 1, ... until *changed (device) != round + 1 after a round; parent[i] is then the largest
 * element index of i's component.  Indices in `pairs` must be < n < 2^32 - 1. */
int nsr_cc_init(int64_t n, uint32_t *parent, uint32_t *changed, void *stream);
int nsr_cc_round(const int32_t *pairs, int64_t n_pairs, int64_t n, uint32_t *parent, uint32_t *changed, int32_t round, void *stream);
/* area[f] = |(v1 - v0) x (v2 - v0)| / 2 in fp64 */
int nsr_face_areas(const double *verts, const int32_t *faces, int64_t n_faces, double *area, void *stream);
/* out[s] = sum of values[order[j]] for j in [seg[s], seg[s + 1]): keys [n] are the sorted keys (segment s = the run of equal
 * keys starting at seg[s]; seg[n_seg] = n); summed in a fixed order (runs inside tiles of 256 positions, then the tiles in
 * order): deterministic.  partial: [n] doubles of device scratch. */
int nsr_segment_sums(const double *values, const int64_t *order, const int64_t *keys, int64_t n, const int64_t *seg, int64_t n_seg,
                     double *partial, double *out, void *stream);

/* --- Reconstruction evaluation (src/tools/eval_recon.py, src/tools/cull_mesh.py) ------------------------------------------
 * Exact nearest neighbour (the cKDTree queries of eval_recon.py:24-43 and of Open3D's ICP, :45-59).  Points are [n][3], fp32
 * (fp64 = 0) or fp64 (fp64 = 1), computed in fp64: dist = sqrt((dx*dx + dy*dy) + dz*dz), ties -> smallest reference index.
 *   nsr_nn_bounds           bounding box of the reference set into bounds[0..5] (lo xyz, hi xyz); bounds: NSR_NN_BOUNDS_DOUBLES
 *                           doubles of device memory (the rest is per-block scratch)
 *   nsr_nn_plan             HOST: from the box (HOST copy of bounds[0..5]) the grid plan, NSR_NN_PLAN_DOUBLES host doubles;
 *                           fails for n_ref < 1, n_ref >= 2^31 - 1, or non-finite coordinates.  The cell table is O(n_ref).
 *   nsr_nn_workspace_bytes  device workspace of nsr_nn_build / nsr_nn_query for that plan (-1: invalid)
 *   nsr_nn_keys             cell key of every point (queries outside the box are clamped to it); keys [n] int64
 *   nsr_nn_build            after sorting the reference keys (sorted_keys, and `order`: the permutation that sorts them):
 *                           fills the workspace (reference points in key order, fine- and coarse-cell tables)
 *   nsr_nn_query            dist [n] fp64, idx [n] int64, ncand [n] int32 (optional: points examined); qorder [n] (optional):
 *                           the order in which threads take the queries (the queries sorted by their keys).  plan: HOST. */
#define NSR_NN_BOUNDS_DOUBLES (6 * 257)
#define NSR_NN_PLAN_DOUBLES 16
int nsr_nn_bounds(const void *ref, int64_t n_ref, int32_t fp64, double *bounds, void *stream);
int nsr_nn_plan(const double *bounds, int64_t n_ref, double *plan);
int64_t nsr_nn_workspace_bytes(const double *plan, int64_t n_ref);
int nsr_nn_keys(const void *pts, int64_t n, int32_t fp64, const double *plan, int64_t *keys, void *stream);
int nsr_nn_build(const void *ref, int64_t n_ref, int32_t fp64, const double *plan, const int64_t *sorted_keys, const int64_t *order,
                 void *workspace, void *stream);
int nsr_nn_query(const void *query, int64_t n_query, int32_t fp64, const int64_t *qorder, const double *plan, const void *workspace,
                 int64_t n_ref, double *dist, int64_t *idx, int32_t *ncand, void *stream);

/* Area-weighted surface sampling (trimesh.sample.sample_surface, called by eval_recon.py:103,106).  verts [nv][3] fp64,
 * faces [nf][3] int32; areas in fp64 as trimesh's area_faces, their inclusive scan in a fixed order; face = first with
 * cum >= u0 * total; (a, b) -> |(a, b) - 1| when a + b > 1; point = ((v1 - v0) a + (v2 - v0) b) + v0.  uniforms [n][3]
 * (u0, a, b) fp64, or NULL: drawn in the kernel by philox(counter = (point, draw), key = seed), 53 bits each.
 * points [n][3] fp64, face_index [n] int64.  workspace: nsr_sample_workspace_bytes(nf). */
int64_t nsr_sample_workspace_bytes(int64_t nf);
int nsr_sample_surface(const double *verts, int64_t nv, const int32_t *faces, int64_t nf, int64_t n, const double *uniforms,
                       uint64_t seed, void *workspace, double *points, int64_t *face_index, void *stream);

/* Fixed-order fp64 reductions (per-block trees, then the blocks in order: bit-identical run to run).  partial:
 * nsr_recon_partial_doubles(n) doubles of device scratch.
 *   nsr_dist_stats   out[0] = sum of dist, out[1] = number of dist < th (eval_recon.py:24-43: mean, completion ratio)
 *   nsr_icp_stats    over the correspondences with dist < th (idx into tgt [n_tgt][3]; src [n][3]): out[0] count, out[1] sum of
 *                    |s - t|^2, out[2..4] source centroid, out[5..7] target centroid, out[8..16] sum of (t - mu_t)(s - mu_s)^T
 *                    row-major (the point-to-point estimate inside Open3D's registration_icp, eval_recon.py:45-59)
 *   nsr_transform_points  pts [n][3] fp64 <- R pts + t, m: HOST [3][4] row-major [R | t] */
int64_t nsr_recon_partial_doubles(int64_t n);
int nsr_dist_stats(const double *dist, int64_t n, double th, double *partial, double *out, void *stream);
int nsr_icp_stats(const double *src, const double *tgt, const int64_t *idx, const double *dist, int64_t n, int64_t n_tgt, double th,
                  double *partial, double *out, void *stream);
int nsr_transform_points(double *pts, int64_t n, const double *m, void *stream);

/* Frustum culling of mesh vertices over a trajectory (cull_mesh.py:45-75), all K poses in one launch.  verts [n][3] fp32 or fp64
 * (rounded to fp32 as the reference's .float()); w2c [K][12] fp32: rows 0..2 of inv(c2w) as the reference computes it;
 * seen[v] = 1 iff some pose has 0 <= -z, 0 < u < W, 0 < v < H (fp32, the reference's order, z = K[2] . cam + 1e-5);
 * keep[f] = 1 unless none of the face's vertices is seen (faces [nf][3] int32; nf = 0: no faces). */
int nsr_cull_vertices(const void *verts, int64_t n, int32_t fp64, const float *w2c, int32_t K, int32_t H, int32_t W, double fx,
                      double fy, double cx, double cy, const int32_t *faces, int64_t nf, uint8_t *seen, uint8_t *keep, void *stream);

/* --- Point-to-mesh distance (no counterpart in the reference: an opt-in estimator of nice_slam_amd.recon) ----------------
 * The exact distance from every query to a triangle list, the closest point and its face.  verts [nv][3] fp32 (fp64 = 0) or
 * fp64 (fp64 = 1), faces [nf][3] int32 with every index in [0, nv) (a face with an index outside is ignored), queries [n][3]
 * fp32 or fp64; everything is computed in fp64, in the expression order written in nice_slam_amd/csrc/nsr_meshdist.h; a
 * degenerate face counts as its three edges.  dist = sqrt of the smallest per-face squared distance over ALL faces, ties of
 * bit-equal squared distance -> smallest face index.  Coordinates must be finite.  The index is a cell grid over the box of
 * the vertices (nsr_nn_bounds), a face registered in every cell its box overlaps; built without atomics.
 *   nsr_meshdist_plan             HOST: the grid plan for nf faces from the box (HOST copy of bounds[0..5]), NSR_NN_PLAN_DOUBLES
 *                                 host doubles (nsr_nn_plan's layout: nsr_nn_keys gives the queries' cell keys)
 *   nsr_meshdist_count            count [nf] int64: cells the face is registered in; over [nf] int64: 1 for a face that would
 *                                 overlap more than NSR_MESHDIST_CELL_CAP cells (count 0: it goes to the oversize list, which
 *                                 every query tests), so the pair table holds at most NSR_MESHDIST_CELL_CAP * nf entries
 *   nsr_meshdist_fill             count_cum [nf]: the INCLUSIVE scan of count, n_pairs its last entry; keys [n_pairs] int64 and
 *                                 pair_face [n_pairs] int64: every face's (cell key, face) pairs at the face's own offset
 *   nsr_meshdist_workspace_bytes  device workspace of build / query (-1: invalid, or n_pairs >= 2^31 - 1)
 *   nsr_meshdist_build            after sorting the keys (sorted_keys, `order`: the stable permutation that sorts them): fills the
 *                                 workspace; over_cum [nf]: the inclusive scan of over, n_over its last entry
 *   nsr_meshdist_query            dist [n] fp64, face [n] int64, closest [n][3] fp64, ncand [n] int32 (optional: faces examined,
 *                                 repeats counted); qorder [n] (optional): the order in which threads take the queries
 *   nsr_face_normals              normals [nf][3] fp64: (b - a) x (c - a) / its length, the zero vector for a degenerate face
 *   nsr_normal_stats              out[0] = sum of |query_normals[i] . face_normals[face[i]]|, out[1] = number of pairs in which
 *                                 neither normal is the zero vector (the others add nothing); the fixed order of nsr_dist_stats;
 *                                 partial: nsr_recon_partial_doubles(n) doubles of device scratch
 * plan: HOST everywhere. */
#define NSR_MESHDIST_CELL_CAP 32
int nsr_meshdist_plan(const double *bounds, int64_t nf, double *plan);
int nsr_meshdist_count(const void *verts, int64_t nv, int32_t fp64, const int32_t *faces, int64_t nf, const double *plan, int64_t *count,
                       int64_t *over, void *stream);
int nsr_meshdist_fill(const void *verts, int64_t nv, int32_t fp64, const int32_t *faces, int64_t nf, const double *plan,
                      const int64_t *count_cum, int64_t n_pairs, int64_t *keys, int64_t *pair_face, void *stream);
int64_t nsr_meshdist_workspace_bytes(const double *plan, int64_t nf, int64_t n_pairs, int64_t n_over);
int nsr_meshdist_build(const void *verts, int64_t nv, int32_t fp64, const int32_t *faces, int64_t nf, const double *plan,
                       const int64_t *sorted_keys, const int64_t *order, const int64_t *pair_face, int64_t n_pairs, const int64_t *over,
                       const int64_t *over_cum, int64_t n_over, void *workspace, void *stream);
int nsr_meshdist_query(const void *query, int64_t n_query, int32_t fp64, const int64_t *qorder, const double *plan, const void *workspace,
                       int64_t nf, int64_t n_pairs, int64_t n_over, double *dist, int64_t *face, double *closest, int32_t *ncand,
                       void *stream);
int nsr_face_normals(const void *verts, int64_t nv, int32_t fp64, const int32_t *faces, int64_t nf, double *normals, void *stream);
int nsr_normal_stats(const double *query_normals, const double *face_normals, const int64_t *face, int64_t n, int64_t nf, double *partial,
                     double *out, void *stream);

/* --- Mesh bound from keyframes (src/utils/Mesher.py:214-279, get_bound_from_frames) -------------------------------------
 * TSDF fusion restating Open3D's legacy ScalableTSDFVolume (units of 16^3 voxels, depth_sampling_stride 4, depth_scale 1,
 * depth_trunc 1000; the caller passes voxel_length = 4 scale / 512 and sdf_trunc = 0.04 scale), geometry only.  The rules are
 * written out in nice_slam_amd/csrc/nsr_bound.h.  depth [K][H][W] fp32; c2w [K][12] fp64: rows 0..2 of the FLIPPED c2w
 * (columns 1 and 2 negated); w2c [K][12] fp32: rows 0..2 of inv(flipped c2w) taken in fp64.  box: [6] int32 (unit index lo xyz,
 * hi xyz, inclusive): device for nsr_tsdf_unit_box, a HOST copy everywhere else.
 *   nsr_tsdf_unit_box        the box of every unit some frame touches
 *   nsr_tsdf_workspace_bytes device workspace for that box (-1: empty, or more than 2^31 units)
 *   nsr_tsdf_touch_count     dense unit bitmap + its rank into the workspace; n_units [1] int64 (device) out
 *   nsr_tsdf_touch_emit      units [n_units][3] int32 in linear-index order, touch [n_units][(K + 31) / 32] uint32: bit k of
 *                            unit u = frame k touches u
 *   nsr_tsdf_integrate       tsdf, weight [n_units][16][16][16] fp32 (x slowest), frames in order, bit-identical run to run
 *   nsr_tsdf_surface_count   counts [n_units + 1] int64: surface points before each unit; counts[n_units] = the total
 *   nsr_tsdf_surface_emit    points [n_points][3] fp64 (the vertex set of extract_triangle_mesh, fixed order)
 * Hull:
 *   nsr_hull_extremes        ext [26] int64: the extreme point along each direction of {-1, 0, 1}^3 \ 0 (code 0..26 without
 *                            13, x slowest); partial: nsr_hull_partial_doubles() doubles of device scratch
 *   nsr_hull_prefilter       keep [n] uint8 = 0 iff the point is more than `margin` inside every plane (HOST [n_planes][4],
 *                            at most 64): planes of the hull of those extremes
 *   nsr_convex_hull          HOST, all pointers host memory: fp64 quickhull with distance tolerance tol of pts [n][3], scaled
 *                            by bound_scale about the mean of its vertices.  counts [2] = (nv, nf); verts [nv][3] (capacity n),
 *                            vert_index [nv] (the input point of each vertex, ascending), faces [nf][3] int32 outward (capacity
 *                            2 n), planes [nf][4] (unit normal, offset) of the scaled faces
 *   nsr_hull_contains        inside [n] uint8: 1 iff ((nx x + ny y) + nz z) + off <= 0 in fp64 for every plane (device
 *                            [n_planes][4]); pts fp32 (fp64 = 0) or fp64 */
int nsr_tsdf_unit_box(const float *depth, int32_t K, int32_t H, int32_t W, const double *c2w, double fx, double fy, double cx, double cy,
                      double voxel_length, double sdf_trunc, int32_t *box, void *stream);
int64_t nsr_tsdf_workspace_bytes(const int32_t *box);
int nsr_tsdf_touch_count(const float *depth, int32_t K, int32_t H, int32_t W, const double *c2w, double fx, double fy, double cx, double cy,
                         double voxel_length, double sdf_trunc, const int32_t *box, void *workspace, int64_t *n_units, void *stream);
int nsr_tsdf_touch_emit(const float *depth, int32_t K, int32_t H, int32_t W, const double *c2w, double fx, double fy, double cx, double cy,
                        double voxel_length, double sdf_trunc, const int32_t *box, const void *workspace, int64_t n_units, int32_t *units,
                        uint32_t *touch, void *stream);
int nsr_tsdf_integrate(const float *depth, int32_t K, int32_t H, int32_t W, const float *w2c, double fx, double fy, double cx, double cy,
                       double voxel_length, double sdf_trunc, const int32_t *units, const uint32_t *touch, int64_t n_units, float *tsdf,
                       float *weight, void *stream);
int nsr_tsdf_surface_count(const int32_t *box, const void *workspace, const int32_t *units, int64_t n_units, const float *tsdf,
                           const float *weight, int64_t *counts, void *stream);
int nsr_tsdf_surface_emit(const int32_t *box, const void *workspace, const int32_t *units, int64_t n_units, const float *tsdf,
                          const float *weight, double voxel_length, const int64_t *counts, int64_t n_points, double *points, void *stream);
int64_t nsr_hull_partial_doubles(void);
int nsr_hull_extremes(const double *pts, int64_t n, double *partial, int64_t *ext, void *stream);
int nsr_hull_prefilter(const double *pts, int64_t n, const double *planes, int32_t n_planes, double margin, uint8_t *keep, void *stream);
int nsr_convex_hull(const double *pts, int64_t n, double tol, double bound_scale, int64_t *counts, double *verts, int64_t *vert_index,
                    int32_t *faces, double *planes);
int nsr_hull_contains(const void *pts, int64_t n, int32_t fp64, const double *planes, int32_t n_planes, uint8_t *inside, void *stream);

/* --- Depth rasterization and the 2-D depth metric (src/tools/eval_recon.py:131-211, calc_2d_metric and check_proj) ----------
 * A tiled z-buffer rasterizer for triangle meshes; the numerical contract is written out in nice_slam_amd/csrc/nsr_raster.h.
 * verts [n_verts][3] fp32, faces [n_faces][3] int32 (a face with an index outside [0, n_verts) draws nothing), w2c [K][12] fp32:
 * rows 0..2 of inv(c2w) taken in fp64, c2w in the OpenCV convention (x right, y down, z forward).  Intrinsics fx, fy, cx, cy;
 * images H x W, at most 1024 x 1024; 0 < near < far.  Two calls per batch of views:
 *   nsr_raster_workspace_bytes  device workspace of both calls (-1: invalid sizes)
 *   nsr_raster_bin              camera-space vertices, pixel boxes and the per-tile entry counts into the workspace; n_entries
 *                               [1] int64 (device) out: the number of (tile, triangle) entries of all K views
 *   nsr_raster_depth            with bins [n_entries] int32 of device scratch: the entries in (view, tile, triangle) order, then
 *                               depth [K][H][W] fp32 (0 where nothing is drawn).  Bit-identical run to run.
 *   nsr_depth_error                per view k: the mean over n_pixels of |a - b| (fp64, fixed order) into out [K] fp64; partial:
 *                               nsr_depth_error_partial_doubles(K, n_pixels) doubles of device scratch
 *   nsr_view_unseen             check_proj for K candidate poses: sees [K] uint8 = 1 iff some point of pts [n][3] (fp32 / fp64)
 *                               projects into the image; w2c [K][12] fp32: rows 0..2 of inv of the FLIPPED c2w (y, z columns
 *                               negated), as nsr_cull_vertices.
 *   nsr_points_visible          visibility of pts [n][3] (fp32 / fp64) from K views against their depth images (as nsr_raster_depth
 *                               wrote them, same w2c and intrinsics): count [n] int32 += the number of views in which the point
 *                               lies in [near, far], projects to a pixel of the image (nearest centre) and is not behind the
 *                               depth there by more than eps (a pixel reading 0 hides nothing).  The caller zeroes count and
 *                               calls once per batch of views on one stream.  n >= 1, K >= 1, near < far, eps >= 0. */
int64_t nsr_raster_workspace_bytes(int64_t n_verts, int64_t n_faces, int32_t K, int32_t H, int32_t W);
int nsr_raster_bin(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *w2c, int32_t K, int32_t H,
                   int32_t W, double fx, double fy, double cx, double cy, double near, double far, void *workspace, int64_t *n_entries,
                   void *stream);
int nsr_raster_depth(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *w2c, int32_t K, int32_t H,
                     int32_t W, double fx, double fy, double cx, double cy, double near, double far, void *workspace, int32_t *bins,
                     int64_t n_entries, float *depth, void *stream);
int64_t nsr_depth_error_partial_doubles(int32_t K, int64_t n_pixels);
int nsr_depth_error(const float *a, const float *b, int32_t K, int64_t n_pixels, double *partial, double *out, void *stream);
int nsr_view_unseen(const void *pts, int64_t n, int32_t fp64, const float *w2c, int32_t K, int32_t H, int32_t W, double fx, double fy,
                    double cx, double cy, uint8_t *sees, void *stream);
int nsr_points_visible(const void *pts, int64_t n, int32_t fp64, const float *w2c, int32_t K, const float *depth, int32_t H, int32_t W,
                       double fx, double fy, double cx, double cy, double near, double far, double eps, int32_t *count, void *stream);

/* --- Replay view (visualizer.py with src/tools/viz.py: the shaded mesh, camera wireframes and trajectories of a finished run) ---
 * The colour side of the rasterizer; the numerical contract is written out in nice_slam_amd/csrc/nsr_view.h.  Meshes, poses,
 * intrinsics, image limits and near / far as in "Depth rasterization".
 *   nsr_view_workspace_bytes    device workspace of nsr_raster_bin + nsr_view_mesh (nsr_raster_workspace_bytes; -1: invalid sizes)
 *   nsr_view_normals            area-weighted vertex normals: start [n_verts + 1] int64 and incident [n_incident] int32 are the CSR
 *                               list of the faces at each vertex, ascending face id per vertex (device); sums [n_verts][3] fp64 out
 *                               (may be null): the summed face cross products; normals [n_verts][3] fp32 out: the sums normalised,
 *                               a zero sum stays zero.
 *   nsr_view_mesh               after nsr_raster_bin on the same arguments and workspace, in the place of nsr_raster_depth: bins
 *                               [n_entries] int32 of device scratch; normals [n_verts][3] fp32; colors [n_verts][3] uint8 or null
 *                               (0.8 grey); cull: NSR_CULL_NONE, NSR_CULL_BACK (drop the faces whose normal (V1 - V0) x (V2 - V0)
 *                               points away from the camera) or NSR_CULL_FRONT (drop the others).  Out: depth [K][H][W] fp32 (with
 *                               NSR_CULL_NONE what nsr_raster_depth writes, bit for bit), face [K][H][W] int32 (the smallest id
 *                               among the faces at the winning depth, -1: background), rgb [K][H][W][3] uint8 (headlight shading,
 *                               white background).
 *   nsr_view_points             B frames of square points over a base layer: frame b draws pts / colors [offsets[b] ..
 *                               offsets[b + 1]) (offsets [B + 1] int64, device; n: the length of pts / colors) with w2c [b] over
 *                               base_rgb / base_depth [b] (base_per_frame != 0) or [0] (shared) into rgb [b]; a point pixel is
 *                               drawn iff the base depth there is 0 or the point is not behind it; the nearest point wins, then
 *                               the smallest index.  owner [B][H][W] int32 out (may be null): the index in its frame of the
 *                               point drawn, -1 where the base shows.  1 <= size <= 64, B <= 65535.
 * All bit-identical run to run. */
enum { NSR_CULL_NONE = 0, NSR_CULL_BACK = 1, NSR_CULL_FRONT = 2 };
int64_t nsr_view_workspace_bytes(int64_t n_verts, int64_t n_faces, int32_t K, int32_t H, int32_t W);
int nsr_view_normals(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const int64_t *start,
                     const int32_t *incident, int64_t n_incident, double *sums, float *normals, void *stream);
int nsr_view_mesh(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const float *w2c, int32_t K, int32_t H,
                  int32_t W, double fx, double fy, double cx, double cy, double near, double far, void *workspace, int32_t *bins,
                  int64_t n_entries, const float *normals, const uint8_t *colors, int32_t cull, float *depth, int32_t *face,
                  uint8_t *rgb, void *stream);
int nsr_view_points(const float *pts, const uint8_t *colors, int64_t n, const int64_t *offsets, const float *w2c, int32_t B, int32_t H,
                    int32_t W, double fx, double fy, double cx, double cy, double near, double far, int32_t size,
                    const uint8_t *base_rgb, const float *base_depth, int32_t base_per_frame, uint8_t *rgb, int32_t *owner, void *stream);

/* --- Rendering evaluation (src/utils/Visualizer.py:53-65, with PSNR / SSIM / depth L1 of the re-rendered frames) ------------
 * One launch pair evaluates B frame pairs; the numerical contract is written out in nice_slam_amd/csrc/nsr_imgmetrics.h.
 * color / gt_color [B][H][W][3] fp32 (rendered / input), depth / gt_depth [B][H][W] fp32; a pixel is valid iff its input depth
 * is not 0.  H, W >= 11 (one 11 x 11 SSIM window), B <= 65535; B = 0 succeeds and launches nothing.
 *   nsr_image_metrics_workspace_bytes  device workspace of the call (-1: invalid sizes)
 *   nsr_image_metrics                  result [B][8] fp64 per frame:
 *                                        [0] sum over pixels and channels of (clip(color) - clip(gt_color))^2, clip to [0, 1]
 *                                        [1] the number of pixels H W        (PSNR = -10 log10([0] / (3 [1])), data range 1)
 *                                        [2], [3] the same sum and count over the valid pixels
 *                                        [4] SSIM (Gaussian 11 x 11, sigma 1.5, windows inside the image, mean over windows and
 *                                            channels, clipped colours, not masked)
 *                                        [5] sum of |gt_depth - depth| over the valid pixels (count: [3]; metric 100 [5] / [3] cm)
 *                                        [6] the maximum of gt_depth        [7] 0
 *                                      depth_residual [B][H][W], color_residual [B][H][W][3] (either may be null): |gt - rendered|
 *                                      of the depth and of the unclipped colour, 0 where the pixel is not valid.
 *                                      Fixed-order fp64 sums, no atomics: bit-identical run to run and independent of a
 *                                      frame's place in the batch. */
int64_t nsr_image_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W);
int nsr_image_metrics(const float *color, const float *gt_color, const float *depth, const float *gt_depth, int32_t B, int32_t H, int32_t W,
                      double *result, float *depth_residual, float *color_residual, void *workspace, int64_t workspace_bytes, void *stream);

/* --- Rendering figures (src/utils/Visualizer.py:24-107: the sheet the tracker and the mapper save while they run) -------------
 * B frame pairs in, B sheets of bytes out; the numerical contract is written out in nice_slam_amd/csrc/nsr_figure.h.
 * color / gt_color [B][H][W][3] fp32 (rendered / input), depth / gt_depth [B][H][W] fp32; H, W in [1, 32768], stride in
 * [1, 32768], margin and gap in [0, 32768], B <= 65535; B = 0 succeeds and launches nothing.
 *   nsr_figure_sheet_size   SH = 2 margin + 2 h + gap, SW = 2 margin + 3 w + 2 gap with h = ceil(H / stride), w = ceil(W / stride);
 *                           3 SH SW must stay below 2^31.
 *   nsr_figure_sheet        sheet u8 [B][SH][SW][3], 4-byte aligned: panel (r, c) at row margin + r (h + gap), column margin + c (w + gap)
 *                           shows every stride-th pixel of, in row 0, gt_depth, depth and |gt_depth - depth| through matplotlib's
 *                           Normalize(0, vmax) and plasma map (a NaN is white), in row 1 gt_color, color and |gt_color - color| as
 *                           (uint8)(clip(v, 0, 1) 255); the residuals are 0 where gt_depth is 0; everything else is 255.  vmax is
 *                           the frame's largest gt_depth over all pixels (nsr_image_metrics' [6]); vmax_out [B] fp32 (may be null)
 *                           receives it.  The sheet's memory holds intermediate values until the call's last launch has run.
 *   nsr_depth_colorize      the colour map alone: rgb u8 [B][H][W][3], 4-byte aligned, of depth with vmax [B] fp32 (device), or,
 *                           vmax null, with each image's own maximum.
 * No atomics: bit-identical run to run and independent of a frame's place in the batch. */
int nsr_figure_sheet_size(int32_t H, int32_t W, int32_t stride, int32_t margin, int32_t gap, int32_t *SH, int32_t *SW);
int nsr_figure_sheet(const float *color, const float *gt_color, const float *depth, const float *gt_depth, int32_t B, int32_t H, int32_t W,
                     int32_t stride, int32_t margin, int32_t gap, float *vmax_out, uint8_t *sheet, void *stream);
int nsr_depth_colorize(const float *depth, int32_t B, int32_t H, int32_t W, const float *vmax, uint8_t *rgb, void *stream);

/* --- JPEG encoding (baseline sequential DCT, 8 bit, three components, JFIF YCbCr) ----------------------------------------------
 * n images that are on the device in, their entropy-coded segments out: what stands between a JPEG file's SOS header and its EOI.
 * The caller writes the markers around them (nice_slam_amd/jpeg.py); the numerical contract -- integers end to end -- is written
 * out in nice_slam_amd/csrc/nsr_jpeg.h.  images u8 [n][H][W][3] RGB; H, W in [1, 65535]; n <= 65535, n = 0 succeeds and launches
 * nothing; subsampling 0 (4:4:4, MCU 8 x 8) or 2 (4:2:0, MCU 16 x 16), the codes of PIL's JpegImagePlugin.get_sampling; quality in
 * [1, 100]: T.81's tables K.1 / K.2 scaled by the IJG rule; the Huffman tables are K.3 - K.6; the restart interval is one MCU row
 * (DRI = ceil(W / MCU side)), RSTm stands behind every interval but a frame's last.
 *   nsr_jpeg_size     the bytes of workspace and of output that nsr_jpeg_encode needs for such a batch: the worst case of any
 *                     content (a block of 63 AC codes of 26 bits and a DC code of 20, every byte stuffed), nothing is sized by
 *                     the images.
 *   nsr_jpeg_encode   out (out_bytes >= the size query's) receives frame k's segment at [offsets[k], offsets[k + 1]), offsets int64
 *                     [n + 1] on the device, offsets[0] = 0; no byte of out at or behind offsets[n] is written.  workspace: 16-byte
 *                     aligned, workspace_bytes >= the size query's.
 * No atomics on global memory, every sum and scan in a fixed order: the same images give the same bytes, whatever else is in the
 * batch. */
int nsr_jpeg_size(int32_t n, int32_t H, int32_t W, int32_t subsampling, int64_t *workspace_bytes, int64_t *out_bytes);
int nsr_jpeg_encode(const uint8_t *images, int32_t n, int32_t H, int32_t W, int32_t quality, int32_t subsampling, void *workspace,
                    int64_t workspace_bytes, uint8_t *out, int64_t out_bytes, int64_t *offsets, void *stream);

/* --- JPEG decoding (baseline sequential DCT, 8 bit, Huffman coded; one or three components) ------------------------------------
 * The bytes of n JPEG files that are on the device in, out u8 [n][H][W][3] RGB: the pixels libjpeg-turbo's default decoder gives
 * (islow IDCT, fancy upsampling), bit for bit.  The caller walks the markers (nice_slam_amd/jpeg.py) and describes every file by
 * one nsr_jpegdec_frame in device memory (8-byte aligned): its tables, and its entropy-coded segment as a byte range of `files`.
 * The numerical contract is written out in nice_slam_amd/csrc/nsr_jpegdec.h.  All frames of a call share H, W in [1, 65535] and
 * sampling (NSR_JPEG_444 / 422 / 420: three components, luma 1x1 / 2x1 / 2x2 over chroma 1x1, PIL's get_sampling codes;
 * NSR_JPEG_GREY: one component); n <= 65535, n = 0 succeeds and launches nothing.  subsequence_bytes: the piece of a restart
 * interval's stuffed stream that one lane decodes, a multiple of 4 in [16, 1024] (128 is the default of the callers); the result
 * does not depend on it.  max_scan_bytes: the longest entropy-coded segment of the batch, at most 2^28.
 *   nsr_jpegdec_size     the bytes of workspace nsr_jpegdec_decode needs; nothing is sized by what the files hold.
 *   nsr_jpegdec_decode   workspace 16-byte aligned, workspace_bytes >= the size query's.  status int32 [n] on the device: 0, or
 *                        bits 1 an invalid Huffman code, 2 a coefficient index past 63, 4 a block count other than the frame
 *                        header's, 8 restart markers missing or out of sequence; such a frame's pixels are unspecified, the
 *                        other frames of the batch are not affected.  Every stream fetch stays inside [scan_begin, scan_end).
 * No atomics on global memory, every scan in a fixed order: the same bytes give the same pixels, whatever else is in the batch. */
enum { NSR_JPEG_444 = 0, NSR_JPEG_422 = 1, NSR_JPEG_420 = 2, NSR_JPEG_GREY = 3 };
typedef struct nsr_jpegdec_frame {
    int64_t scan_begin, scan_end;       /* the entropy-coded segment: bytes [scan_begin, scan_end) of `files` */
    int32_t restart_interval;           /* DRI, in MCUs; 0: none */
    int32_t reserved;
    uint8_t dc_table[4], ac_table[4];   /* per component (Y, Cb, Cr): its Huffman tables, 0..3 */
    uint8_t quant[3][64];               /* per component: its quantisation table in zig-zag order, as DQT holds it */
    uint8_t huff_bits[8][16];           /* DC tables 0..3, then AC tables 0..3: the number of codes of each length 1..16 */
    uint8_t huff_vals[8][256];          /* their symbols in code order */
} nsr_jpegdec_frame;
int nsr_jpegdec_size(int32_t n, int32_t H, int32_t W, int32_t sampling, int64_t max_scan_bytes, int32_t subsequence_bytes,
                     int64_t *workspace_bytes);
int nsr_jpegdec_decode(const uint8_t *files, const nsr_jpegdec_frame *descriptors, int32_t n, int32_t H, int32_t W, int32_t sampling,
                       int32_t subsequence_bytes, void *workspace, int64_t workspace_bytes, uint8_t *out, int32_t *status, void *stream);

/* --- PNG decoding (8-bit and 16-bit grey, 8-bit RGB and RGBA; non-interlaced) ----------------------------------------------------
 * The compressed bytes of n PNG files that are on the device in, their pixels out: what Pillow returns for the file, bit for bit.
 * The caller walks the chunks and checks their CRCs (nice_slam_amd/png.py) and describes every file by one nsr_png_frame in device
 * memory (8-byte aligned): its zlib stream -- the IDAT payloads, concatenated -- as a byte range of `streams`.  The device inflates
 * (RFC 1950 / 1951 as zlib reads them: stored, fixed and dynamic blocks, a 32 KiB window), un-filters (None, Sub, Up, Average,
 * Paeth) and orders the bytes; the contract is written out in nice_slam_amd/csrc/nsr_png.h.  All frames of a call share H, W in
 * [1, 32768] and kind; n <= 65535, n = 0 succeeds and launches nothing.  out per kind and out_channels:
 *   NSR_PNG_GREY8    1: u8 [n][H][W]; 3: u8 [n][H][W][3], the sample three times
 *   NSR_PNG_GREY16   1: uint16 [n][H][W], host-endian
 *   NSR_PNG_RGB8     3: u8 [n][H][W][3]
 *   NSR_PNG_RGBA8    4: u8 [n][H][W][4]; 3: u8 [n][H][W][3], alpha dropped
 *   nsr_png_size     the bytes of workspace nsr_png_decode needs (the filtered scanlines); nothing is sized by what the files hold.
 *   nsr_png_decode   workspace 16-byte aligned, workspace_bytes >= the size query's.  status int32 [n] on the device: 0, or bits
 *                    1 a zlib header, block type or stored-length error, 2 an invalid code set or code, 4 a distance before the
 *                    start of the output, 8 a stream that ends early or holds more than H (1 + stride) bytes, 16 a filter type
 *                    above 4; such a frame's pixels are unspecified, the other frames of the batch are not affected.  Every
 *                    stream fetch stays inside [stream_begin, stream_end), every store inside the frame's own pixels and its own
 *                    slice of the workspace.  The stream's trailing Adler-32 is neither verified nor required, and
 *                    distances up to 32768 are taken whatever window the zlib header declares (nsr_png.h).
 * No atomics on global memory, a fixed order: the same bytes give the same pixels, whatever else is in the batch. */
enum { NSR_PNG_GREY8 = 0, NSR_PNG_GREY16 = 1, NSR_PNG_RGB8 = 2, NSR_PNG_RGBA8 = 3 };
typedef struct nsr_png_frame {
    int64_t stream_begin, stream_end;   /* the zlib stream: bytes [stream_begin, stream_end) of `streams` */
} nsr_png_frame;
int nsr_png_size(int32_t n, int32_t H, int32_t W, int32_t kind, int64_t *workspace_bytes);
int nsr_png_decode(const uint8_t *streams, const nsr_png_frame *descriptors, int32_t n, int32_t H, int32_t W, int32_t kind,
                   int32_t out_channels, void *workspace, int64_t workspace_bytes, void *out, int32_t *status, void *stream);

/* --- Frame preparation (src/utils/datasets.py:77-113, BaseDataset.__getitem__ after the files are decoded) ---------------------
 * The raw bytes of B frames of one geometry in, the tensors the tracker and the mapper read out: undistortion of the colour image
 * (its own launch, only with distortion coefficients), then ONE launch for the channel order, / 255, the resize of the colour
 * image to the depth image's size, the depth scale, the crop_size resize, crop_edge and the cast.  The numerical contract is
 * written out in nice_slam_amd/csrc/nsr_frame.h.
 *   color_raw u8 [B][color_h][color_w][3], channels BGR (color_bgr = 1: cv2.imread) or RGB (0: PIL)
 *   depth_raw [B][depth_h][depth_w], uint16 (depth_type NSR_DEPTH_U16) or fp32 (NSR_DEPTH_F32)
 *   color fp32 [B][H][W][3] RGB, depth fp32 [B][H][W] = ((float)raw / (float)png_depth_scale) * (float)scale, where
 *   (Hs, Ws) = (crop_h, crop_w) if both are > 0 (both 0: (depth_h, depth_w)) and H = Hs - 2 crop_edge, W = Ws - 2 crop_edge.
 * Every size is in [1, 32768], 0 <= 2 crop_edge < min(Hs, Ws), png_depth_scale is positive and finite as a float; with
 * has_distortion, fx and fy are not 0 and dist = [k1, k2, p1, p2, k3] (the intrinsics are those of the RAW colour image, read
 * only then).  B = 0 succeeds and launches nothing.
 *   nsr_frame_out_size         H, W of the description
 *   nsr_frame_workspace_bytes  device workspace of nsr_frame_prepare: 3 B color_h color_w with distortion, else 0 (-1: invalid)
 *   nsr_frame_prepare          workspace may be null when none is needed.  No atomics, nothing synchronises; a frame's result
 *                              does not depend on its place in the batch. */
enum { NSR_DEPTH_U16 = 0, NSR_DEPTH_F32 = 1 };
typedef struct nsr_frame_desc {
    int32_t color_h, color_w, depth_h, depth_w;
    int32_t depth_type, color_bgr;
    int32_t crop_h, crop_w, crop_edge, has_distortion;
    double fx, fy, cx, cy;
    double dist[5];
    double png_depth_scale, scale;
} nsr_frame_desc;
int nsr_frame_out_size(const nsr_frame_desc *desc, int32_t *H, int32_t *W);
int64_t nsr_frame_workspace_bytes(const nsr_frame_desc *desc, int32_t B);
int nsr_frame_prepare(const void *color_raw, const void *depth_raw, const nsr_frame_desc *desc, int32_t B, float *color, float *depth,
                      void *workspace, int64_t workspace_bytes, void *stream);

/* --- Pose algebra (the run's trajectory and keyframe poses stay on the device) ------------------------------------------------
 * Four launches of one small block each; fp32 in, fp64 arithmetic, one rounding to fp32 at the store; plain stores, nothing
 * synchronises, safe to capture.  The numerical contract is written out in nice_slam_amd/csrc/nsr_pose.h.  Frame and row
 * indices are read from device memory and checked against the table's length: an index outside it writes nothing.
 *   nsr_tensor_from_camera  get_tensor_from_camera (src/common.py:179-201): n poses, rows of row_floats = 12 (3x4) or 16 (4x4)
 *                           floats -> cam [n][7] = [w, x, y, z | tx, ty, tz]; Shepperd's four branches, then normalised.
 *                           n = 0 succeeds and launches nothing.
 *   nsr_pose_predict        the tracker's initial pose (src/Tracker.py:192-201) of frame i = idx[0] (device int64, 1 <= i <
 *                           n_frames) from traj [n_frames][4][4]: with const_speed and i >= 2,
 *                           traj[i-1] inverse(traj[i-2]) traj[i-1] (general 4x4 inverse, Gauss-Jordan with partial pivoting),
 *                           else traj[i-1].  Its 7-vector goes to cam [7] and that 7-vector's pose to traj[i].
 *   nsr_pose_commit         the tracker's choice (src/Tracker.py:224,245-247) over hist [n_iters][8] = loss | cam: from 1e10, a
 *                           row is taken only when its loss is strictly smaller (the first of equal minima; never a NaN).  The
 *                           taken row's pose (quad2rotation, src/common.py:137-160, bottom row 0 0 0 1) goes to traj[idx[0]]
 *                           and the row to best [8] (may be null).  No row taken: nothing is written, traj[idx[0]] keeps
 *                           what nsr_pose_predict wrote.
 *   nsr_pose_store          the bundle-adjustment write-back (src/Mapper.py:527-541): dst[index[i]] = pose of cams[i], i < m;
 *                           index is device int64 [m], dst [n_dst][4][4].  m = 0 succeeds and launches nothing. */
int nsr_tensor_from_camera(const float *rt, int64_t n, int32_t row_floats, float *cam, void *stream);
int nsr_pose_predict(float *traj, int64_t n_frames, const int64_t *idx, int32_t const_speed, float *cam, void *stream);
int nsr_pose_commit(const float *hist, int32_t n_iters, float *traj, int64_t n_frames, const int64_t *idx, float *best, void *stream);
int nsr_pose_store(const float *cams, int32_t m, const int64_t *index, float *dst, int64_t n_dst, void *stream);

/* --- Trajectory evaluation (src/tools/eval_ate.py: the absolute trajectory error of a run and its figure) ----------------------
 * est / gt [n_frames][4][4] fp32 (a checkpoint's estimate_c2w_list / gt_c2w_list), last [B] device int64: problem b evaluates the
 * frames 0..last[b] (the checkpoint's idx, eval_ate.py:291 and convert_poses' range(0, N + 1)).  n_frames in [1, 2^24], scale
 * positive and finite.  The numerical contract is written out in nice_slam_amd/csrc/nsr_trajeval.h.
 *   nsr_ate_eval   B <= 2^20 problems in one launch, one block each; B = 0 succeeds and launches nothing.  A frame is used iff its
 *                  gt pose is finite (eval_ate.py:247-252); positions are (double)(t / scale) with the division in fp32 (:253,
 *                  :146-148); Horn's alignment of the estimate to the ground truth in fp64 (align, :44-78); the statistics of
 *                  the error (:215-223).  rec [B][32] fp64 per problem:
 *                    [0] compared pose pairs   [1] dropped gt frames   [2] non-finite est poses among the used frames
 *                    [3] rmse  [4] mean  [5] median (numpy's)  [6] population std  [7] min  [8] max
 *                    [9..17] rot row-major   [18..20] trans   (aligned = rot est + trans)
 *                    [21] xmin  [22] xmax  [23] ymin  [24] ymax of the gt positions and the aligned est positions
 *                    [25] flags: 1 fewer than two pairs, 2 last[b] outside [0, n_frames), 4 a non-finite est pose
 *                    [26..31] 0
 *                  [3..24] are NaN with no pair, with flag 2 (then [0..2] are 0 and nothing else is written) and with flag 4.
 *                  err (may be null) [B][n_frames] fp64: the errors of the used frames in their order in err[b][0 .. pairs);
 *                  the rest of the row is left as it was.  No global atomics, fixed-order sums: bit-identical run to run and
 *                  independent of the other problems.  Nothing synchronises, safe to capture.
 *   nsr_ate_plot   eval_ate_plot.png (:196-204, :213) of ONE problem: last and rec point at that problem's entry and record in
 *                  device memory.  image u8 [H][W][3] (the reference's figure: H 432, W 576): white, the axes box
 *                  [0.125 W, 0.9 W] x [0.11 H, 0.88 H] and the gt trajectory's x-y projection in black, the aligned estimate in
 *                  blue (0, 0, 255) on top; limits = the record's widened by 5 % of the range; hard-edged lines of 1.875 px
 *                  (1.5 pt at 90 dpi), the box 1 px.  Title, legend, ticks and labels are not drawn. */
int nsr_ate_eval(const float *est, const float *gt, int64_t n_frames, const int64_t *last, int32_t B, float scale, double *rec, double *err,
                 void *stream);
int nsr_ate_plot(const float *est, const float *gt, int64_t n_frames, const int64_t *last, float scale, const double *rec, int32_t H, int32_t W,
                 uint8_t *image, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSR_H_ */
