/* gsr.h -- C ABI of libgsr_hip.so, the MI355X (gfx950) Gaussian-splatting rasterizer.
 *
 * This is the drop-in boundary for the reference's native extension
 * `diff_gaussian_rasterization._C` (reference paths relative to
 * /root/reference/gaussiansplatting/submodules/diff-gaussian-rasterization):
 *
 *   _C.rasterize_gaussians           ext.cpp:16, rasterize_points.cu:35-95
 *       -> gsr_preprocess + gsr_bin + gsr_blend_forward
 *   _C.rasterize_gaussians_backward  ext.cpp:17, rasterize_points.cu:97-157
 *       -> gsr_backward
 *   _C.mark_visible                  ext.cpp:18, rasterize_points.cu:159-175
 *       -> gsr_mark_visible
 *   _C.apply_weights                 ext.cpp:19, rasterize_points.cu:177-234
 *       -> gsr_preprocess + gsr_bin + gsr_trace_weights
 *
 * Rules of the boundary
 *   - plain C: pointers, sizes, scalars; no torch / pybind types.
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`.
 *   - the library never allocates device memory: the caller (torch) owns every
 *     output and scratch buffer; sizes come from gsr_scratch_sizes().  Scratch
 *     buffers are opaque bytes that the caller keeps alive between forward and
 *     backward (the reference's geomBuffer / binningBuffer / imgBuffer,
 *     rasterize_points.cu:64-69, diff_gaussian_rasterization/__init__.py:122-133).
 *   - scratch buffers (geom / binning / image) must be 256-byte aligned (torch's allocations are): their sections are
 *     read with 16-byte vector loads.  A misaligned one is rejected with GSR_ERR_BAD_ARGUMENT.
 *   - `stream` is a hipStream_t (passed as void*); all work is enqueued on it.
 *     The library is re-entrant and keeps no BEHAVIOUR state (the switches that can change a result travel with every
 *     call as `flags`); the only thing it owns is a small pool of 8 KiB pinned host buffers, one checked out per host
 *     thread and device, through which gsr_preprocess receives its counts (the device writes them, the host polls).
 *   - tuning / experiment knobs are environment variables read ONCE per process, none of which changes any result
 *     (launch geometry of the persistent blend kernels, work-list ordering, GSR_BIN_LEGACY=1,
 *     which sends every image down the tile-pair sort that otherwise only images beyond 131 072 tiles take, and
 *     GSR_SORT_THREADS=256|1024, which gives every radix sort the block width that otherwise its size decides, and
 *     GSR_GROUP_CHUNK=64|128|256|512, the same for the chunk length of the grouped binning); they are
 *     listed in DESIGN.md section 3.3 and are not part of this ABI.
 *   - an absent optional input is a NULL pointer (the reference uses empty
 *     tensors for the same purpose, diff_gaussian_rasterization/__init__.py:285-295).
 *   - return value: GSR_OK (0) or a negative gsr_status; never exit()/abort().
 *   - all floating point is IEEE binary32; images are CHW; matrices are the
 *     16-float row-major tensors holding the TRANSPOSED 4x4 matrices exactly as
 *     the reference passes them.
 */
#ifndef GSR_H_INCLUDED
#define GSR_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Everything declared here has default visibility; the library itself is compiled with -fvisibility=hidden, so these
 * entry points are ALL it exports (tests/test_cpu_abi.py checks both directions). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* 4 (round 5): adds gsr_near_workspace_size / gsr_near_points (round 4 had left the number at 3), the scratch layouts
 * changed again (sizes come from gsr_scratch_sizes: rebuild nothing, re-query), images of more than GSR_MAX_TILES tiles
 * are refused by the backward entry points instead of being walked wrongly. */
/* 5 (round 6): adds gsr_arrays_equal; the blend backward accumulates into ONE table of 64-byte rows (`acc`, GSR_ACC_*)
 * instead of four arrays, and gsr_preprocess_backward* copies dL_dmeans2D / dL_dopacity (/ dL_dcolors) out of it: the
 * signatures of gsr_backward, gsr_blend_backward, gsr_preprocess_backward{,_rgb,_rows}, gsr_view_message_plan_blend and
 * gsr_debug_blend_backward_profile changed. */
/* 6 (round 6): adds gsr_preprocess_begin / gsr_preprocess_end (nothing else changed).  Later, purely additive (the number
 * stays): GSR_FLAG_DEPTH_GRAD, the GSR_ACC_DEPTH column, gsr_blend_backward_depth and gsr_backward_depth -- every earlier
 * entry point keeps its signature and its behaviour.  Then, likewise additive: GSR_FLAG_ANTIALIAS and
 * gsr_preprocess_backward_rows_flags.  Then, likewise additive: GSR_FLAG_ABS_GRAD, the GSR_ACC_ABS2D columns and
 * gsr_abs_grad_take.  Then, likewise additive: gsr_alpha_image and gsr_blend_backward_alpha (no new flag bit).  Then,
 * likewise additive: gsr_loss_workspace_size, gsr_photometric_loss_forward and gsr_photometric_loss_backward (the fused
 * L1 + SSIM loss; nothing of the rasterizer changed).  Then, likewise additive: gsr_densify_stats,
 * gsr_densify_workspace_size, gsr_densify_select, gsr_densify_plans, gsr_densify_split_xyz and gsr_densify_keep (the
 * densification policy; nothing existing changed).  Then, likewise additive: gsr_pose_workspace_size and gsr_pose_backward
 * (the camera gradient; no new flag bit, nothing existing changed).  Then, likewise additive:
 * GSR_MAX_FEATURE_CHANNELS, gsr_blend_forward_features and gsr_blend_backward_features (the feature image; no new flag bit).
 * Then, likewise additive: gsr_mcmc_noise, gsr_mcmc_workspace_size, gsr_mcmc_sample, gsr_mcmc_relocation_values and
 * gsr_mcmc_scatter (the 3DGS-MCMC strategy; no new flag bit, nothing existing changed).  Then, likewise additive: the six
 * gsr_bilagrid_* entry points (the bilateral-grid slice and its TV regulariser; nothing existing changed).  Then, likewise
 * additive: gsr_sh_rotation and gsr_transform_rows (similarity transforms of Gaussians; nothing existing changed).  Then,
 * likewise additive: gsr_gaussian_normals_forward / _backward, gsr_depth_normals_forward / _backward,
 * gsr_normal_loss_workspace_size and gsr_normal_loss_forward / _backward (surface normals; nothing existing changed).
 * Then, likewise additive: gsr_blend_forward_distortion and gsr_blend_backward_distortion (the depth-distortion image; no
 * new flag bit, nothing existing changed).  Then, likewise additive: GSR_FILTER3D_CAMERA_DOUBLES, gsr_filter3d_workspace_size,
 * gsr_filter3d_sweep and gsr_filter3d_apply_forward / _backward (Mip-Splatting's 3D filter; nothing existing changed).
 * Then, likewise additive: gsr_tsdf_integrate, gsr_tsdf_mesh_workspace_size, gsr_tsdf_mesh_count and gsr_tsdf_mesh_emit (TSDF
 * fusion and mesh extraction; nothing existing changed). */
#define GSR_ABI_VERSION 6
/* The blend backward's accumulator table: GSR_ACC_ROW floats (one 64-byte line) per Gaussian, 64-byte aligned.  Columns:
 *   [GSR_ACC_MEAN2D] .x [+1] .y of dL_dmean2D      (backward.cu:545-546)
 *   [GSR_ACC_OPACITY] dL_dopacity                  (backward.cu:554)
 *   [GSR_ACC_CONIC] .x [+1] .y [+3] .w of dL_dconic (backward.cu:549-551; the reference's float4 layout, .z unused)
 *   [GSR_ACC_COLOR .. +2] dL_dcolor                (backward.cu:523)
 *   [GSR_ACC_DEPTH] dL_ddepth, the gradient of the Gaussian's view-space depth: sum over pixels of alpha T dL_dout_depth
 *       (written by gsr_blend_backward_depth only; no reference counterpart)
 *   [GSR_ACC_ABS2D] .x [+1] .y of the ABSOLUTE screen-space gradient: the sums over pixels of the absolute values of the
 *       per-pixel terms of dL_dmean2D (written under GSR_FLAG_ABS_GRAD only, taken out again by gsr_abs_grad_take; no
 *       reference counterpart)
 * every other column stays zero.  Why one row: float atomics execute at the memory side on this chip and cost per REQUEST;
 * the lanes of a wave instruction that fall into one 64-byte line travel as one request, so the (up to nine) adds of a
 * (tile, Gaussian) pair leave as one instead of nine (tools/microbench/atomic_merge.hip: 8.8x). */
#define GSR_ACC_ROW 16
#define GSR_ACC_MEAN2D 0
#define GSR_ACC_OPACITY 3
#define GSR_ACC_CONIC 4
#define GSR_ACC_COLOR 8
#define GSR_ACC_DEPTH 11
#define GSR_ACC_ABS2D 12
/* Largest image the blend BACKWARD accepts, in 16 x 16 tiles (its work items carry the tile id in 20 bits). */
#define GSR_MAX_TILES (1 << 20)

typedef enum gsr_status {
  GSR_OK = 0,
  GSR_ERR_BAD_ARGUMENT = -1,   /* NULL where a pointer is required, negative sizes, ... */
  GSR_ERR_BAD_CHANNELS = -2,   /* apply_weights with C outside {1,2,3} (reference: exit(-1), apply_weights.cu:377-380) */
  GSR_ERR_TOO_MANY = -3,       /* num_rendered does not fit the 31-bit index space */
  GSR_ERR_HIP = -4             /* a HIP runtime call failed; see gsr_last_hip_error() */
} gsr_status;

/* Version of this ABI (== GSR_ABI_VERSION of the header the library was built from). */
int gsr_abi_version(void);
/* Static description of a status code. */
const char* gsr_status_string(int status);
/* hipError_t of the most recent failing HIP call on the calling thread (0 if none). */
int gsr_last_hip_error(void);

/* Byte sizes of the three opaque scratch buffers for P Gaussians, R rendered
 * instances, G group instances (both returned by gsr_preprocess) and a W x H image.  Pass R = G = 0 before they are
 * known (sizes[1] is then 0).
 * sizes[0] = geometry (per Gaussian), sizes[1] = binning (per instance),
 * sizes[2] = image (per pixel / tile).  sizes[2] with the real R may be smaller than with R = 0 (the forward's checkpoint
 * pool -- 64 KB per tile, 128 MB at most -- is only needed for views with long lists): a caller that allocates the image
 * scratch after gsr_preprocess saves it, one that sized it with R = 0 beforehand is always large enough.
 * REUSE: the entry points cannot see how large a scratch buffer is.  An image scratch that is kept and reused for later
 * views (or for a view rendered under the GSR_CK_CHUNKS knob) MUST have been sized with R = 0: one sized with a short-list
 * R lacks the pool, and a later view with long lists would have its forward write checkpoints behind the buffer's end.
 * (The Python binding allocates the image scratch per view, with that view's R.)
 * Replaces required<GeometryState/BinningState/ImageState>() (rasterizer_impl.h:63-72). */
int gsr_scratch_sizes(int P, int64_t R, int64_t G, int W, int H, size_t sizes[3]);

/* Per-call behaviour flags (ABI 2; ABI 1 had a process-wide gsr_set_option instead).  The library keeps no option
 * state: every entry point below that takes `flags` receives them with the call, and the calls that belong to one view
 * (gsr_preprocess ... gsr_backward / gsr_trace_weights) must be given the same value.  0 reproduces the reference's
 * internal state bit for bit.
 *   GSR_FLAG_TILE_BOUNDS_ALPHA  (read by gsr_preprocess) a Gaussian is binned only into the tiles its alpha >= 1/255
 *                        level set can reach (bounding box of that ellipse with conservative margins, intersected with
 *                        the reference's square of side 2 ceil(3 sigma_max), auxiliary.h:46-56, forward.cu:226-230).
 *                        Every dropped (tile, Gaussian) instance would have been skipped at each pixel by
 *                        forward.cu:340-344, so images, depths, radii, traced weights and gradients are unchanged --
 *                        but num_rendered, the instance lists in the binning scratch and n_contrib differ from the
 *                        reference's.
 *   GSR_FLAG_CLEAR_GRADS (read by gsr_blend_backward / gsr_backward) the accumulator table `acc`
 *       need not be zero on entry: the call clears it before it accumulates (inside the launch that builds the backward's
 *       work list, while that one workgroup runs: 14 us instead of 8 + 9 at 10^6 Gaussians, and one launch less);
 *   GSR_FLAG_FORWARD_ONLY (read by gsr_preprocess) no gsr_preprocess_backward / gsr_backward will be called on the geometry
 *       state this call leaves: the 48 bytes per Gaussian only the backward reads (the colour's derivative by the view
 *       direction) are neither computed nor written.  A backward on such a state would read uninitialised memory; it is
 *       refused with GSR_ERR_BAD_ARGUMENT where the library can tell: when the flag is passed on to gsr_blend_backward /
 *       gsr_backward, and when `geom` is the buffer the most recent gsr_preprocess on it left forward-only.  That second
 *       check is BEST EFFORT by construction: a host-side table of 1 024 hashed slots keyed by the `geom` pointer, no device
 *       read -- a note can be evicted by a gsr_preprocess on another buffer that hashes to its slot, and a state copied to
 *       another buffer is not recognised; do not rely on it to catch the misuse.  The Python
 *       binding sets the flag exactly for renders none of whose inputs requires a gradient;
 *   GSR_FLAG_FAST_EXP    (read by the blend / trace entry points) exp(power) is evaluated with the hardware's
 *                        v_exp_f32 (2^x, 1 ulp) on power * log2(e) instead of the exactly specified polynomial
 *                        gsr_expf.  Colours / depths / gradients stay within the 1e-5 parity
 *                        bar, but a pixel whose alpha or transmittance sits within a rounding of a threshold
 *                        (1/255, 1e-4) may take the other branch than the CPU oracle, so n_contrib / final_T are no
 *                        longer bit-identical to it (they are not bit-identical to the reference's libm build either).
 *   GSR_FLAG_ACC_SELF_CLEAN (ABI 5; read by gsr_backward / gsr_preprocess_backward / _rgb) the accumulator table `acc` is one the caller KEEPS between
 *       backwards: it is all zero on entry (the caller's promise -- hipMemset it once) and all zero again when the call has
 *       run: K8+K9, which reads every row anyway, writes zeros over the rows K7 touched (one Gaussian in ten on the
 *       benchmark view: 6 MB instead of a 64 MB clear in front of every backward).  Not combined with GSR_FLAG_CLEAR_GRADS
 *       (which it makes unnecessary).  With the two halves called separately: gsr_blend_backward WITHOUT GSR_FLAG_CLEAR_GRADS
 *       on the zero table, then gsr_preprocess_backward (or _rgb) with this flag.  Nothing else may read `acc` while K8+K9
 *       runs (the exchange plans its messages from K7's `touched` mask, not from the table);
 *   GSR_FLAG_SHARED_SIMDS (ABI 4; read by the blend / trace entry points) the caller overlaps this view's kernels with
 *                        another view's on a second stream: the persistent blend kernels are launched with 2 waves per
 *                        SIMD instead of 4, which leaves wave slots and registers for the other stream's kernels (a rank
 *                        that renders several views of a batch: -15 % per view, profiles/r04_c_pipelining.md).  Never
 *                        changes a result.  The environment knob GSR_BLEND_WAVES_PER_SIMD, where set, takes precedence.
 *   GSR_FLAG_DEPTH_GRAD  (read by gsr_preprocess_backward / _rgb; accepted by gsr_blend_backward_depth / gsr_backward_depth,
 *                        which imply it) the backward also differentiates the depth image out_depth = sum_i d_i alpha_i T_i
 *                        (background 0; d_i = view-space z): K7 adds sum alpha T dL_dout_depth into GSR_ACC_DEPTH and folds
 *                        d_i dL_dout_depth into dL/dalpha, K8+K9 adds dL_ddepth * (view[2], view[6], view[10]) to
 *                        dL_dmeans3D.  The reference has no such gradient.  Only the backward entry points above accept
 *                        this bit; the forward / trace entry points, gsr_blend_backward and gsr_backward refuse it (a caller
 *                        keeps it to itself until the backward).
 *   GSR_FLAG_ANTIALIAS   (read by gsr_preprocess / gsr_preprocess_begin and by every K8+K9 entry point: gsr_preprocess_backward,
 *                        _rgb, _rows_flags, gsr_backward, gsr_backward_depth; accepted and ignored by gsr_blend_forward, _aux,
 *                        gsr_blend_backward, gsr_blend_backward_depth and gsr_trace_weights) opacity-compensated 2D filter,
 *                        as the antialiased modes of current 3DGS rasterizers: with Sigma the 2D covariance BEFORE the
 *                        0.3 px^2 dilation, r = det(Sigma) / det(Sigma + 0.3 I) and h = sqrt(max(2.5e-5, r)), the Gaussian
 *                        is blended with opacity * h (rec0.w of the geometry state) instead of opacity; conic, radius,
 *                        means2D, depth and colour are unchanged.  A sub-pixel Gaussian then keeps its integrated weight
 *                        instead of spreading its full opacity over the dilated footprint.  The backward differentiates h
 *                        (dL_dopacity = h dL/d(opacity h), plus the share of r in the covariance gradients).  The reference
 *                        has no such mode.  The calls of one view must all receive the bit or none of them.
 *   GSR_FLAG_ABS_GRAD    (read by gsr_blend_backward and gsr_blend_backward_depth, and by nothing else) K7 also accumulates
 *                        the absolute screen-space gradient ("absgrad", the densification statistic of AbsGS): for every
 *                        Gaussian the sums over the pixels p that blend it of |t_x(p)| and |t_y(p)|, t(p) the term pixel p
 *                        adds into dL_dmean2D (backward.cu:545-546, with the 0.5 W / 0.5 H factors; under
 *                        gsr_blend_backward_depth with the depth image's share of dL/dalpha in it), into the columns
 *                        GSR_ACC_ABS2D, + 1 of the accumulator row.  Hence >= |dL_dmean2D| per component, equal where a
 *                        Gaussian's terms share a sign.  gsr_abs_grad_take, called between the two halves, moves the sums
 *                        out and leaves the columns zero; every other column, and with it every other gradient, is what it
 *                        is without the flag.  The forward / trace entry points, gsr_backward and gsr_backward_depth (which
 *                        have no output for it) and the K8+K9 entry points refuse the bit: like GSR_FLAG_DEPTH_GRAD it is
 *                        a backward-only bit a caller keeps to itself until gsr_blend_backward[_depth].
 * Unknown bits are rejected with GSR_ERR_BAD_ARGUMENT. */
#define GSR_FLAG_TILE_BOUNDS_ALPHA 1u
#define GSR_FLAG_FAST_EXP 2u
#define GSR_FLAG_CLEAR_GRADS 4u
#define GSR_FLAG_FORWARD_ONLY 8u
#define GSR_FLAG_SHARED_SIMDS 16u
#define GSR_FLAG_ACC_SELF_CLEAN 32u
#define GSR_FLAG_DEPTH_GRAD 64u
#define GSR_FLAG_ANTIALIAS 1024u
#define GSR_FLAG_ALL (127u | GSR_FLAG_ANTIALIAS)
#define GSR_FLAG_ABS_GRAD 4096u
/* every bit the library knows: GSR_FLAG_ALL is what the view-wide entry points take, GSR_FLAG_ABS_GRAD only the blend backwards */
#define GSR_FLAG_KNOWN (GSR_FLAG_ALL | GSR_FLAG_ABS_GRAD)

/* Number of sort-key bits, 32 + getHigherMsb(tiles) (rasterizer_impl.cu:36-49, 253). */
int gsr_sort_key_bits(int W, int H);

/* K1 + K2: per-Gaussian preprocessing (SH -> RGB, 3D -> 2D covariance, conic,
 * radius, tile rectangle), the depth ordering of the Gaussians (first half of K4, see gsr_bin) and the
 * prefix sums the emission in that order needs; then the ONE
 * blocking device->host readback of the path: counts_host[0] = num_rendered, the total number
 * of (Gaussian, tile) instances, counts_host[1] = the number of (Gaussian, 8x8-tile group) instances gsr_bin works on
 * (0 for images that take the tile-pair sort).  Both size the binning scratch.  Reference: FORWARD::preprocess +
 * InclusiveSum + cudaMemcpy, rasterizer_impl.cu:217-239 (and :381-403 for apply_weights).
 * The host normally waits ~80 us for the counts, spinning on a pinned word the device writes; if nothing arrives within
 * 5 ms (earlier work queued on the stream, or a failed launch) the call blocks in hipStreamSynchronize instead and
 * reports what that returns.  `prefiltered` is accepted for signature compatibility and has no effect (the reference
 * uses it only to trap the device when a point it was promised to be visible is culled, auxiliary.h:156-160).
 *
 *   P, D, M          #Gaussians, active SH degree (0..3), SH coefficients per Gaussian (0 if shs == NULL)
 *   means3D (P,3); scales (P,3)|NULL; rotations (P,4)|NULL; opacities (P); shs (P,M,3)|NULL;
 *   cov3D_precomp (P,6)|NULL; colors_precomp (P,3)|NULL  (exactly one of shs/colors, one of scales+rot/cov3D,
 *   unless skip_color != 0, in which case neither colour source is read: the apply_weights path)
 *   viewmatrix, projmatrix (16 floats each); campos (3)
 *   radii (P) int32 out; geom: scratch, sizes[0] bytes. */
int gsr_preprocess(void* stream, int P, int D, int M, const float* means3D, const float* scales,
                   float scale_modifier, const float* rotations, const float* opacities, const float* shs,
                   const float* cov3D_precomp, const float* colors_precomp, const float* viewmatrix,
                   const float* projmatrix, const float* campos, int W, int H, float tan_fovx, float tan_fovy,
                   int prefiltered, int skip_color, unsigned flags, int32_t* radii, void* geom,
                   int64_t counts_host[2]);

/* gsr_preprocess in two halves (ABI 6), for a caller that keeps several views in flight: _begin checks the arguments,
 * enqueues K1 and the depth-sort passes that do not depend on the counts, and returns AT ONCE with a ticket; _end (same
 * stream, same P / W / H / geom; any host thread) waits for that view's counts exactly as gsr_preprocess does, enqueues the
 * rest of the depth ordering and fills counts_host.  gsr_preprocess(...) == _begin(...) followed by _end(...): same
 * kernels, same results.  Between the two calls the launch thread may enqueue other views' work -- a rank that renders a
 * batch of views issues view v + 1's _begin before view v's backward and never waits for a readback at all
 * (gaussianeditor_amd/multiview.py; the reference's loop over batch["camera"], threestudio/systems/GassuianEditor.py:
 * 165-207, blocks in cudaMemcpy once per view).  A ticket is spent by _end whatever _end returns; one that is never
 * passed to _end leaks one 64-byte pinned slot.  P == 0 is refused (GSR_ERR_BAD_ARGUMENT): nothing to wait for. */
int gsr_preprocess_begin(void* stream, int P, int D, int M, const float* means3D, const float* scales,
                         float scale_modifier, const float* rotations, const float* opacities, const float* shs,
                         const float* cov3D_precomp, const float* colors_precomp, const float* viewmatrix,
                         const float* projmatrix, const float* campos, int W, int H, float tan_fovx, float tan_fovy,
                         int prefiltered, int skip_color, unsigned flags, int32_t* radii, void* geom, void** ticket);
int gsr_preprocess_end(void* stream, int P, int W, int H, void* geom, void* ticket, int64_t counts_host[2]);

/* Are n <= 8 pairs of device arrays identical bit for bit?  a[i] / b[i]: device pointers (4-byte aligned; a pair with
 * a[i] == b[i] or bytes[i] == 0 is equal without being read), bytes[i]: their size, a multiple of 4.  One compare launch
 * over all pairs (16-byte loads where both sides are 16-byte aligned) plus a one-thread launch that publishes the answer
 * into the calling thread's pinned slot; like gsr_preprocess the call BLOCKS until the answer is there (it polls; ~10 us
 * + 64 MB per 12 us).  *equal_host = 1 (all pairs equal) or 0.
 * No reference counterpart: the Python layer uses it to PROVE that a second render() of a view -- the reference renders
 * every training view and GUI frame twice, with override_color the second time (threestudio/systems/GassuianEditor.py:
 * 166-191, webui.py:693-713) -- got the opacities / scales / rotations of the first (fresh activation tensors each time),
 * before it reuses the first render's preprocessing, sort and tile lists ("view reuse"). */
int gsr_arrays_equal(void* stream, int n, const void* const* a, const void* const* b, const size_t* bytes, int* equal_host);

/* K3 + K4 + K5: the per-tile instance lists (the reference's point_list) and their [begin,end) ranges, in exactly the
 * order of the reference's stable sort on the low gsr_sort_key_bits() bits of (tile << 32 | depth bits): the Gaussians
 * were depth-ordered by gsr_preprocess; here one (group, Gaussian) pair per 8x8-tile group a Gaussian reaches is emitted
 * in that order, stably sorted by group in one radix pass, and expanded group by group into the tiles' lists
 * (gsr_binning.hip).  R and G are the two counts gsr_preprocess returned.
 * Reference: duplicateWithKeys + cub::DeviceRadixSort::SortPairs + identifyTileRanges,
 * rasterizer_impl.cu:248-271.  `binning` holds sizes[1] bytes for this (R, G). */
int gsr_bin(void* stream, int P, int64_t R, int64_t G, int W, int H, const void* geom, void* binning, void* image);

/* K6: per-tile front-to-back alpha compositing.  Reference: FORWARD::render,
 * forward.cu:261-409.  out_color (3,H,W), out_depth (1,H,W) are fully written
 * (background where nothing is blended); final_T / n_contrib go to `image`. */
int gsr_blend_forward(void* stream, int P, int64_t R, int W, int H, const float* bg, const void* geom,
                      const void* binning, void* image, float* out_color, float* out_depth, unsigned flags);

/* Auxiliary forward render of the SAME view with other per-Gaussian colours: blends
 * `colors` (P,3) through the geometry / binning state an earlier gsr_preprocess + gsr_bin left in the scratch buffers,
 * i.e. K6 only.  GaussianEditor renders every training view and every GUI frame twice, the second time with
 * `override_color` = the semantic mask (threestudio/systems/GassuianEditor.py:166-191, webui.py:693-713); K1-K5 of that
 * second render are identical to the first one's.  The image equals what gsr_preprocess(colors_precomp = colors) ...
 * gsr_blend_forward would produce.  final_T / n_contrib in `image` are NOT touched, so the backward of the main render
 * is unaffected; no backward exists for the auxiliary image.  out_depth may be NULL. */
int gsr_blend_forward_aux(void* stream, int P, int64_t R, int W, int H, const float* bg, const void* geom,
                          const void* binning, void* image, const float* colors, float* out_color, float* out_depth,
                          unsigned flags);

/* K7 + K8 + K9: the whole backward.  Reference: Rasterizer::backward,
 * rasterizer_impl.cu:289-341 (BACKWARD::render then BACKWARD::preprocess).
 *   dL_dpix (3,H,W) in.
 *   acc (P, GSR_ACC_ROW) workspace: the accumulator table K7 adds into with atomics and K8+K9 reads.  MUST be zero on entry
 *       (or is cleared by the call: GSR_FLAG_CLEAR_GRADS), 64-byte aligned, and MUST live in ordinary (coarse-grained)
 *       device memory -- hipMalloc, torch's caching allocator --, not in fine-grained / host-coherent allocations
 *       (hipMallocManaged, hipHostMalloc, hipExtMallocWithFlags(... hipDeviceMallocFinegrained)): the library is built with
 *       -munsafe-fp-atomics, i.e. its float adds are the hardware's global_atomic_add_f32, which is only defined on
 *       coarse-grained memory (on fine-grained memory the adds are silently lost).  The same holds for `weights` / `cnt` of
 *       gsr_trace_weights.
 *   Fully written by the library (no need to zero): dL_dmeans2D (P,3) [z = 0], dL_dopacity (P), dL_dcolors (P,3) [may be
 *       NULL: only a caller with precomputed colours needs it], dL_dmeans3D (P,3), dL_dcov3D (P,6) [may be NULL when
 *       cov3D_precomp is NULL: it is the gradient of that input; 24 B per Gaussian nobody reads otherwise],
 *       dL_dsh (P,M,3) [NULL if shs == NULL], dL_dscales (P,3) and dL_drots (P,4) [NULL if scales == NULL].
 *   (The reference zero-fills all nine of its outputs, rasterize_points.cu:120-128, and accumulates into four of them.) */
int gsr_backward(void* stream, int P, int D, int M, int64_t R, int W, int H, const float* bg, const float* means3D,
                 const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                 const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int32_t* radii,
                 const void* geom, const void* binning, const void* image, const float* dL_dpix, float* acc,
                 float* dL_dmeans2D, float* dL_dopacity, float* dL_dcolors, float* dL_dmeans3D,
                 float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drots, unsigned flags);

/* The two halves of gsr_backward as separate entry points (same argument meaning), so a caller
 * can time or overlap them: K7 = BACKWARD::render (backward.cu:399-557), K8+K9 = BACKWARD::preprocess
 * (backward.cu:559-622).  gsr_backward == gsr_blend_backward followed by gsr_preprocess_backward.
 * After gsr_blend_backward alone `acc` holds the sums in the GSR_ACC_* columns; gsr_preprocess_backward reads them and
 * writes dL_dmeans2D / dL_dopacity (/ dL_dcolors) next to its own outputs. */
/* `touched` (P bytes rounded up to a multiple of 16, 16-byte aligned, device; may be NULL): cleared by the call, then 1 for
 * every Gaussian whose accumulator row K7 adds to -- the row mask of the multi-GPU exchange (gsr_view_message_plan_blend)
 * without a pass over the 64 P bytes of the table. */
int gsr_blend_backward(void* stream, int P, int64_t R, int W, int H, const float* bg, const void* geom,
                       const void* binning, const void* image, const float* dL_dpix, float* acc, uint8_t* touched,
                       unsigned flags);
int gsr_preprocess_backward(void* stream, int P, int D, int M, int W, int H, const float* means3D, const float* shs,
                            const float* scales, float scale_modifier, const float* rotations,
                            const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                            const float* campos, float tan_fovx, float tan_fovy, const int32_t* radii,
                            const void* geom, float* acc, float* dL_dmeans2D, float* dL_dopacity,
                            float* dL_dcolors, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                            float* dL_dscales, float* dL_drots,
                            unsigned flags /* 0 | GSR_FLAG_ACC_SELF_CLEAN | GSR_FLAG_DEPTH_GRAD | GSR_FLAG_ANTIALIAS */);

/* Depth gradients (opt-in, GSR_FLAG_DEPTH_GRAD): gsr_blend_backward / gsr_backward with one more input,
 *   dL_ddepth (1,H,W): the gradient of out_depth of gsr_blend_forward.
 * gsr_blend_backward_depth also writes GSR_ACC_DEPTH of `acc`; then gsr_preprocess_backward(_rgb) with GSR_FLAG_DEPTH_GRAD
 * reads it (without the flag the column is ignored, and with GSR_FLAG_ACC_SELF_CLEAN not cleaned: pass the flag).
 * gsr_backward_depth == gsr_blend_backward_depth followed by gsr_preprocess_backward(flags | GSR_FLAG_DEPTH_GRAD).  The
 * work list of these backwards has no list segments (the forward's checkpoints hold no depth): views with long lists take
 * longer than gsr_blend_backward.  flags: as gsr_blend_backward / gsr_backward, plus GSR_FLAG_DEPTH_GRAD (optional). */
int gsr_blend_backward_depth(void* stream, int P, int64_t R, int W, int H, const float* bg, const void* geom,
                             const void* binning, const void* image, const float* dL_dpix, const float* dL_ddepth, float* acc,
                             uint8_t* touched, unsigned flags);
int gsr_backward_depth(void* stream, int P, int D, int M, int64_t R, int W, int H, const float* bg, const float* means3D,
                       const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                       const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                       const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int32_t* radii,
                       const void* geom, const void* binning, const void* image, const float* dL_dpix,
                       const float* dL_ddepth, float* acc, float* dL_dmeans2D, float* dL_dopacity, float* dL_dcolors,
                       float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drots,
                       unsigned flags);

/* Absolute screen-space gradients (opt-in, GSR_FLAG_ABS_GRAD): after gsr_blend_backward[_depth] with the flag and BEFORE the
 * K8+K9 entry point of the view, on the same stream.  One thread per Gaussian g: where touched[g] != 0 (touched == NULL:
 * everywhere) absgrad[g] = (acc[g][GSR_ACC_ABS2D], acc[g][GSR_ACC_ABS2D + 1], 0) and the two columns are put back to zero;
 * elsewhere absgrad[g] = (0, 0, 0) and the row is not read.  absgrad (P,3) is fully written.  `touched` is the row mask the
 * blend backward of this view wrote (a row it did not mark holds zeros in these columns).  Afterwards the table is what a
 * backward without the flag leaves, so K8+K9 -- whichever entry point, GSR_FLAG_ACC_SELF_CLEAN included -- runs unchanged.
 * acc: 64-byte aligned, as for gsr_blend_backward.  P == 0 is an empty call. */
int gsr_abs_grad_take(void* stream, int P, float* acc, const uint8_t* touched, float* absgrad);

/* Camera gradient (opt-in; no flag bit: the call says what is asked): the raw partial derivatives of the loss with respect
 * to the view's three camera tensors, each in the tensor's own layout.  Called after the blend backward of the view (and
 * after gsr_abs_grad_take, if that is called) and BEFORE its K8+K9 entry point, on the same stream: it reads the
 * accumulator rows, which K8+K9 may clean, and changes nothing in them -- the K8+K9 call that follows runs unchanged.
 *   pose_grad[0..15]   dL/dviewmatrix (4,4): the view matrix enters through the view-space mean (which feeds the Jacobian
 *                      J), through its rotation block in T = W J and, under GSR_FLAG_DEPTH_GRAD, through the depth; only
 *                      [:, :3] can be non-zero, column 3 is written as exact zeros
 *   pose_grad[16..31]  dL/dprojmatrix (4,4): enters through p_hom = (mean, 1) projmatrix and ndc = p_hom.xy / (p_hom.w +
 *                      1e-7); columns 0, 1 and 3 can be non-zero, column 2 is written as exact zeros
 *   pose_grad[32..34]  dL/dcampos (3): enters through the view direction of the SH colour only -- minus the sum over the
 *                      Gaussians of the dnormvdv term K8+K9 adds to dL_dmeans3D; exact zeros with M == 0
 * Conventions: those of K8+K9 (the reference's analytic backward) -- off-cone tx / ty are constants, the alpha clamp is
 * straight-through, under GSR_FLAG_ANTIALIAS the opacity factor is differentiated through the covariance.  A caller composes
 * the three with whatever built the tensors (full_proj = view @ projection, campos = inverse(view)[3, :3]).
 * Only Gaussians with radii > 0 and a row that is not zero contribute.  No float atomics: per-block partial sums in
 * `workspace`, added in a fixed order in double -- the same accumulator table gives the same 35 floats, bit for bit.
 *   M          SH coefficients per Gaussian the view's forward was given, 0 = it was given colors_precomp (campos may
 *              then be NULL and is not read)
 *   geom       the geometry state of the view's gsr_preprocess; with M > 0 one left by GSR_FLAG_FORWARD_ONLY is refused
 *              (GSR_ERR_BAD_ARGUMENT), as K8+K9 refuses it
 *   acc        the table the blend backward of the view added into, 64-byte aligned; read only
 *   workspace  gsr_pose_workspace_size(P) bytes, 16-byte aligned, the caller's; contents on entry are irrelevant
 *   flags      0 | GSR_FLAG_DEPTH_GRAD (the blend backward was given dL_ddepth: column GSR_ACC_DEPTH is read)
 *              | GSR_FLAG_ANTIALIAS (the view's flag); any other bit is GSR_ERR_BAD_ARGUMENT
 * All 35 floats are written whatever is visible; P == 0 writes 35 zeros.  Arguments are checked before any device work. */
int gsr_pose_workspace_size(int P, size_t* bytes);
int gsr_pose_backward(void* stream, int P, int D, int M, int W, int H, const float* means3D, const float* scales,
                      float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                      const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int32_t* radii,
                      const void* geom, const float* acc, void* workspace, float* pose_grad, unsigned flags);

/* Alpha image (accumulated opacity, opt-in; no flag bit: the pointers say what is asked).
 * gsr_alpha_image: out_alpha (1,H,W) = 1 - final_T of the image state a gsr_blend_forward left (every forward that is not
 * an auxiliary render writes final_T, GSR_FLAG_FORWARD_ONLY included), i.e. A = 1 - prod_i (1 - alpha_i) over the entries
 * the pixel blended.  One small kernel on `stream`, after the forward; the state is only read, so an auxiliary render of
 * the same view, or a later caller that kept the state, gets the same image.  image: as gsr_blend_forward received it.
 * gsr_blend_backward_alpha: gsr_blend_backward with two more inputs behind dL_dpix,
 *   dL_ddepth (1,H,W) | NULL: as gsr_blend_backward_depth (given, GSR_ACC_DEPTH is written and the work list has no list
 *                     segments; NULL, the call keeps them -- the alpha image needs nothing the checkpoints do not hold);
 *   dL_dalpha (1,H,W), required: the gradient of out_alpha.  dA/dalpha_i = final_T / (1 - alpha_i) for every blended entry,
 *                     so it enters K7 as bg . dL_dpix - dL_dalpha in the place of the background term and reaches every
 *                     gradient through dL/dalpha_i (the GSR_FLAG_ABS_GRAD sums included); no new accumulator column, and
 *                     the K8+K9 entry point of the view runs as it would without it (with GSR_FLAG_DEPTH_GRAD iff
 *                     dL_ddepth was given).
 * flags: as gsr_blend_backward_depth (GSR_FLAG_ABS_GRAD included); GSR_FLAG_DEPTH_GRAD only with a non-NULL dL_ddepth.
 * P == 0 / R == 0: as gsr_blend_backward (nothing is launched but the clears it documents).  There is no fused
 * gsr_backward_alpha: call the halves. */
int gsr_alpha_image(void* stream, int W, int H, const void* image, float* out_alpha);
int gsr_blend_backward_alpha(void* stream, int P, int64_t R, int W, int H, const float* bg, const void* geom,
                             const void* binning, const void* image, const float* dL_dpix, const float* dL_ddepth,
                             const float* dL_dalpha, float* acc, uint8_t* touched, unsigned flags);

/* Feature image (opt-in; no flag bit: the call says what is asked): per-Gaussian feature vectors of C channels, the N-D
 * `colors` of current 3DGS rasterizers, alpha-composited through the geometry / binning state an earlier gsr_preprocess +
 * gsr_bin left, with the alpha of gsr_blend_forward under the view's flags.  1 <= C <= GSR_MAX_FEATURE_CHANNELS; the
 * channels are walked in blocks of 16 (the last one may be partial): alpha and T of a (pixel, entry) pair are evaluated once
 * per block.  The reference has no such image.
 * gsr_blend_forward_features: features (P,C) row-major -> out_features (C,H,W) = sum_i f_ic alpha_i T_i, fully written
 *   (exact zeros where nothing is blended: the background is zero; a caller composites its own with gsr_alpha_image).
 *   Channel c equals, as floats, channel c % 3 of gsr_blend_forward_aux with colors = features[:, 3 (c / 3) : + 3] (zero
 *   padded) and bg = 0.  Like that render it leaves final_T / n_contrib in `image` untouched.  P == 0 or R == 0: zeros.
 * gsr_blend_backward_features: dL_dfeature_image (C,H,W) in.  Walks the first n_contrib entries of every pixel back to
 *   front from final_T and ADDS
 *     - the geometry share of the feature image's gradient into the columns GSR_ACC_MEAN2D, GSR_ACC_OPACITY, GSR_ACC_CONIC
 *       of `acc`, the accumulator table the view's colour backward adds into, in that backward's conventions
 *       (GSR_ACC_COLOR, GSR_ACC_DEPTH and GSR_ACC_ABS2D are not written);
 *     - dL/df into dL_dfeatures (P,C), which the caller zeroes (coarse-grained memory, as `acc`); rows of Gaussians no
 *       pixel blends stay untouched.
 *   Called AFTER the blend half of the view's colour backward (gsr_blend_backward[_depth|_alpha], which is what clears a
 *   table that is not kept), after gsr_abs_grad_take if that is called, and BEFORE gsr_pose_backward and the view's K8+K9
 *   entry point, on the same stream: the camera gradient and every geometry gradient then hold the feature image's share.
 *   It only adds to rows of Gaussians in a tile list (radii > 0), so K8+K9 with GSR_FLAG_ACC_SELF_CLEAN leaves the table
 *   zero as it does without it.  It uses no checkpoints and its work list holds no list segments (the checkpoints hold no
 *   features): views with long lists take longer than gsr_blend_backward, as with gsr_blend_backward_depth.  The absolute
 *   sums of GSR_FLAG_ABS_GRAD do not hold the feature image's share.  P == 0 or R == 0: nothing is launched.
 * flags: 0 | GSR_FLAG_FAST_EXP | GSR_FLAG_ANTIALIAS | GSR_FLAG_TILE_BOUNDS_ALPHA | GSR_FLAG_SHARED_SIMDS, the view's (the last
 *   three change nothing here: what is blended is already the effective opacity of the lists as they are); any other bit is
 *   GSR_ERR_BAD_ARGUMENT.  Arguments are checked before any device work: a NULL pointer, C outside 1 .. 256 and an `acc`
 *   that is not 64-byte aligned are GSR_ERR_BAD_ARGUMENT. */
#define GSR_MAX_FEATURE_CHANNELS 256
int gsr_blend_forward_features(void* stream, int P, int64_t R, int W, int H, int C, const void* geom, const void* binning,
                               void* image, const float* features, float* out_features, unsigned flags);
int gsr_blend_backward_features(void* stream, int P, int64_t R, int W, int H, int C, const void* geom, const void* binning,
                                const void* image, const float* features, const float* dL_dfeature_image,
                                float* acc, float* dL_dfeatures, unsigned flags);

/* Depth-distortion image (opt-in; no flag bit: the call says what is asked): the regulariser of Mip-NeRF 360 / 2DGS, through
 * the geometry / binning state an earlier gsr_preprocess + gsr_bin left, with the alpha of gsr_blend_forward under the view's
 * flags.  The entries of a pixel are exactly the ones the colour image blends (the first n_contrib list entries: the same
 * alpha, 0.99 clamp, power > 0 and alpha < 1/255 skips, and the T < 1e-4 stop).  With w_i = alpha_i T_i and m_i the depth of
 * entry i,
 *     D = 1/2 sum_{i != j} w_i w_j (m_i - m_j)^2 = A M2 - M1^2,   A = sum w, M1 = sum w m, M2 = sum w m^2
 *       = 2DGS's running sum  sum_i w_i (m_i^2 A_{i-1} + M2_{i-1} - 2 m_i M1_{i-1}).
 * Depth of an entry: z_i, the view-space depth of the geometry state (what the depth image blends).  near = far = 0: m = z.
 * Finite 0 < near < far: 2DGS's mapping m = far (z - near) / ((far - near) z).
 * Shift: D does not change under m -> m - m0.  The moments are accumulated, in float32, of the SHIFTED depth m', with z0 the
 * z of the pixel's first blended entry:  linear m'_i = z_i - z0, mu_i = dm/dz = 1;  mapped m'_i = kappa (z_i - z0) / (z0 z_i),
 * mu_i = kappa / z_i^2, kappa = far near / (far - near) -- formed from the difference of the z's, never from two mapped
 * values.  Without the shift A M2 - M1^2 cancels where the term is meant to work, on thin surfaces far from the camera.
 * gsr_blend_forward_distortion: out_distortion (H,W) = A M2' - M1'^2, fully written; a pixel with no entry or one entry
 *   gets exactly 0.  moments (H,W) float4, 16-byte aligned, = (z0, A, M1', M2') per pixel for the backward, or NULL (a
 *   forward without a backward).  final_T / n_contrib in `image` are left untouched.  P == 0 or R == 0: zeros.
 * gsr_blend_backward_distortion: dL_ddistortion (H,W) in, gD.  From the pixel's totals alone,
 *     dD/dw_k = m'_k^2 A + M2' - 2 m'_k M1' =: c_k,   dD/dm_k = 2 w_k (m'_k A - M1'),   no term reaches z0;
 *     dL/dalpha_k = T_k (gD c_k - rec_k): the colour backward's recurrence with the scalar gD c_k in the place of the
 *     collapsed colour, background 0.
 *   Walks the first n_contrib entries of every pixel back to front from final_T and ADDS the geometry share into the columns
 *   GSR_ACC_MEAN2D, GSR_ACC_OPACITY, GSR_ACC_CONIC of `acc` in the colour backward's conventions, and dL/dz_k = sum over
 *   pixels of gD 2 w_k (m'_k A - M1') mu_k into GSR_ACC_DEPTH (GSR_ACC_COLOR and GSR_ACC_ABS2D are not written).  Called
 *   AFTER the blend half of the view's colour backward, gsr_abs_grad_take and gsr_blend_backward_features where those are
 *   called, and BEFORE gsr_pose_backward and the view's K8+K9 entry point, on the same stream; both must then be given
 *   GSR_FLAG_DEPTH_GRAD, which is what carries the GSR_ACC_DEPTH column on (and, with GSR_FLAG_ACC_SELF_CLEAN, zeroes it).
 *   No checkpoints, no list segments, as gsr_blend_backward_features.  The absolute sums of GSR_FLAG_ABS_GRAD do not hold
 *   the distortion image's share.  P == 0 or R == 0: nothing is launched.
 * flags: as the feature entry points (0 | GSR_FLAG_FAST_EXP | GSR_FLAG_ANTIALIAS | GSR_FLAG_TILE_BOUNDS_ALPHA |
 *   GSR_FLAG_SHARED_SIMDS); any other bit is GSR_ERR_BAD_ARGUMENT.  Arguments are checked before any device work: a NULL
 *   pointer where one is required, a (near, far) that is neither (0, 0) nor finite with 0 < near < far, a `moments` that is
 *   not 16-byte aligned and an `acc` that is not 64-byte aligned are GSR_ERR_BAD_ARGUMENT. */
int gsr_blend_forward_distortion(void* stream, int P, int64_t R, int W, int H, const void* geom, const void* binning,
                                 void* image, float near, float far, float* out_distortion, float* moments, unsigned flags);
int gsr_blend_backward_distortion(void* stream, int P, int64_t R, int W, int H, const void* geom, const void* binning,
                                  const void* image, float near, float far, const float* moments,
                                  const float* dL_ddistortion, float* acc, unsigned flags);

/* Multi-GPU exchange support (gaussianeditor_amd/multiview.py).  Per view the SH gradient is
 * rank one, dL_dsh[k] = c_k(dir) * dL_dRGB with dir = normalize(mean - campos) (backward.cu:44-98), so ranks exchange
 * the 3-float colour gradient per Gaussian and view instead of the 3M-float SH gradient:
 *   gsr_preprocess_backward_rgb = gsr_preprocess_backward, but instead of dL_dsh it writes dL_drgb (P,3): dL_dcolors
 *       with the channels the forward clamped at 0 zeroed (zeros for Gaussians the view does not see);
 *   gsr_sh_grad_compose rebuilds dL_dsh (P,M,3) = sum over v = 0..num_views-1 (ascending, binary32) of
 *       c_k(dir_v) * dL_drgb[v] from campos (num_views,3) and dL_drgb (num_views,P,3), all device arrays: bit for bit
 *       what accumulating the views' gsr_preprocess_backward outputs one after the other gives. */
int gsr_preprocess_backward_rgb(void* stream, int P, int D, int M, int W, int H, const float* means3D, const float* shs,
                                const float* scales, float scale_modifier, const float* rotations,
                                const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                const float* campos, float tan_fovx, float tan_fovy, const int32_t* radii,
                                const void* geom, float* acc, float* dL_dmeans2D, float* dL_dopacity,
                                float* dL_dmeans3D, float* dL_dcov3D, float* dL_drgb,
                                float* dL_dscales, float* dL_drots,
                                unsigned flags /* 0 | GSR_FLAG_ACC_SELF_CLEAN | GSR_FLAG_DEPTH_GRAD | GSR_FLAG_ANTIALIAS */);

/* The same kernel for gradient arrays the caller keeps ACROSS calls (a training loop's gradient bucket).  A view leaves
 * nine Gaussians of ten with all-zero gradients (culled, or blended by no pixel), and rewriting those zeros is most of
 * this kernel's traffic (248 B per Gaussian at M = 16).  row_state (P bytes, device) travels with the arrays
 * dL_dmeans2D, dL_dopacity, dL_dcolors (if given), dL_dmeans3D, dL_dsh or dL_drgb (exactly one of the two, the other NULL),
 * dL_dscales, dL_drots:
 *   row_state[g] != 0  the rows of g may hold anything: they are written (values, or zeros) -- initialise to 1;
 *   row_state[g] == 0  the rows of g hold the zeros this function wrote before: if g's gradients are zero again, nothing
 *                      is written.
 * On return row_state[g] = 1 iff g's accumulator row (`acc`) had a non-zero entry.  After the call every row holds what gsr_preprocess_backward(_rgb) would have written, for finite
 * parameters (all-zero accumulator rows give all-zero gradients; with a non-finite parameter that kernel computes 0 x inf
 * on every call, this one only when it writes the row).  Whoever else writes to these arrays must set row_state to 1 for
 * the rows it touched.  dL_dcov3D is written for every Gaussian. */
int gsr_preprocess_backward_rows(void* stream, int P, int D, int M, int W, int H, const float* means3D, const float* shs,
                                 const float* scales, float scale_modifier, const float* rotations,
                                 const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                 const float* campos, float tan_fovx, float tan_fovy, const int32_t* radii,
                                 const void* geom, const float* acc, float* dL_dmeans2D, float* dL_dopacity,
                                 float* dL_dcolors, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                                 float* dL_drgb, float* dL_dscales, float* dL_drots, uint8_t* row_state);
/* gsr_preprocess_backward_rows with flags: 0 (== gsr_preprocess_backward_rows) or GSR_FLAG_ANTIALIAS, for a view whose
 * gsr_preprocess ran with that flag; other bits are rejected with GSR_ERR_BAD_ARGUMENT. */
int gsr_preprocess_backward_rows_flags(void* stream, int P, int D, int M, int W, int H, const float* means3D, const float* shs,
                                       const float* scales, float scale_modifier, const float* rotations,
                                       const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                       const float* campos, float tan_fovx, float tan_fovy, const int32_t* radii,
                                       const void* geom, const float* acc, float* dL_dmeans2D, float* dL_dopacity,
                                       float* dL_dcolors, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh,
                                       float* dL_drgb, float* dL_dscales, float* dL_drots, uint8_t* row_state, unsigned flags);
int gsr_sh_grad_compose(void* stream, int P, int D, int M, int num_views, const float* means3D, const float* campos,
                        const float* dL_drgb, float* dL_dsh);

/* K10: present[i] = (view-space z of point i) > 0.2.  Reference: checkFrustum,
 * rasterizer_impl.cu:53-63, 128-133.  `present` is one byte per Gaussian (torch.bool). */
int gsr_mark_visible(void* stream, int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present);

/* K12: semantic tracing -- every pixel scatters its C mask values to every Gaussian
 * it would blend.  weights (P,C) float and cnt (P) int32 are accumulated IN PLACE.
 * Reference: APPLY_WEIGHTS::render, apply_weights.cu:239-381.  Unlike the reference,
 * image_weights is only read for pixels inside the image (hazard a). */
int gsr_trace_weights(void* stream, int P, int64_t R, int W, int H, int C, const void* geom, const void* binning,
                      const void* image, const float* image_weights, float* weights, int32_t* cnt, unsigned flags);

/* Contribution statistics and the pick buffer of a binned view (no reference counterpart): K12's walk -- the cull, the skip
 * rules (power > 0, alpha < 1/255) and the termination (T (1 - alpha) < 1e-4 ends the pixel before the entry counts) of
 * gsr_blend_forward and gsr_trace_weights -- keeping the blending weight w = alpha T of every (pixel, Gaussian) the pixel
 * blends, the quantity the forward composites with.  One launch on the state gsr_bin left, which is only read.
 *   stats (P, 3 + C) int64, accumulated IN PLACE (the caller zeroes a fresh table), row g:
 *     [0]     total_q        sum over the pixels that blend g of q(w), q(x) = (uint32) trunc(x * 2^32): units of 2^-32
 *                            (w <= 0.99, so q fits 32 bits)
 *     [1]     top_count      number of pixels whose top contributor (below) is g
 *     [2]     max_bits       the largest w of g over all pixels, as the binary32 bit pattern zero-extended (w > 0: the
 *                            integer order of the patterns is the order of the floats)
 *     [3 + c] weighted_q[c]  sum of q(w * m_c), m_c = min(max(image_weights[c][pixel], 0), 1) with NaN -> 0, the product
 *                            one binary32 multiply rounded to nearest
 *   image_weights (C,H,W) float32, C in {0,1,2,3}: NULL if and only if C == 0; only read for pixels inside the image.
 *   top_id (H,W) int32 and top_weight (H,W) float32, each optional (NULL) and FULLY written: the largest w over the entries
 *     the pixel blends and that entry's Gaussian index; among equal weights the front-most entry of the tile's list wins;
 *     -1 and 0 for a pixel that blends nothing (the pixels of empty tiles and of a view with R == 0 included).
 * Every accumulation into `stats` is integer -- 64-bit adds, and a max for column 2; no float atomics --: two calls commute,
 * and a call's result is the same bits on every launch grid, with every cut of the quadrants and in every arrival order.
 * Rows no pixel hits are not touched; with R == 0 `stats` is not touched at all.
 * Overflow: a Gaussian gains at most H * W * 2^32 per view in a sum column -- 2^53 at 1920 x 1080 -- of the 2^63 an int64
 * holds, i.e. no column can overflow within 2^10 views at that size even for a Gaussian that fills every pixel of every view
 * with w near 1 (the weights of a pixel sum to at most 1: all rows TOGETHER gain at most H * W * 2^32 per view).
 * `flags`: the view flags gsr_trace_weights accepts.  Errors, before the device is touched: C outside {0,1,2,3} ->
 * GSR_ERR_BAD_CHANNELS; unknown flags, NULL stats (or one not 8-byte aligned) or image, NULL image_weights with C > 0 or
 * non-NULL with C == 0, negative sizes, NULL geom / binning with R > 0 -> GSR_ERR_BAD_ARGUMENT. */
int gsr_trace_contributions(void* stream, int P, int64_t R, int W, int H, int C, const void* geom, const void* binning,
                            const void* image, const float* image_weights, int64_t* stats, int32_t* top_id, float* top_weight,
                            unsigned flags);

/* ---- the simple-knn submodule -------------------------------------------------
 * mean_dist2[i] = mean of the squared distances from point i to its 3 nearest other points (exact), i.e.
 * `simple_knn._C.distCUDA2(points)` (gaussiansplatting/submodules/simple-knn/spatial.cu:15-25, simple_knn.cu:185-221),
 * used by GaussianModel.create_from_pcd (gaussiansplatting/scene/gaussian_model.py:288-291).
 * points (P,3) f32, mean_dist2 (P) f32, workspace: gsr_knn_workspace_size(P) bytes of device scratch. */
int gsr_knn_workspace_size(int P, size_t* bytes);
int gsr_knn_mean_dist2(void* stream, int P, const float* points, void* workspace, float* mean_dist2);

/* The Delete path's neighbour query: near[q] = 1 iff some reference point lies within dist_thresh of query point q.
 * Replaces the CPU KD-tree call inside GaussianModel.get_near_gaussians_by_mask
 * (gaussiansplatting/scene/gaussian_model.py:865-898: K_nearest_neighbors(object_xyz, 1, query=..., return_dist=True)
 * of gaussiansplatting/knn.py, a scipy.spatial.KDTree, followed by `nn_dist <= dist_thresh`).  The compared value is
 * the reference's: the Euclidean distance of the float64-widened coordinates, rounded to float32 once.
 * ref_points (n_ref,3) f32, query_points (n_query,3) f32, near (n_query) u8, nn_dist (n_query) f32 | NULL: the 1-NN
 * distance where it is <= dist_thresh * (1 + 1e-4), +inf where no reference point lies that close (the mask never needs
 * more; NULL lets a query stop at its first hit).  workspace: gsr_near_workspace_size(n_ref) bytes of device scratch.
 * n_query == 0 is a no-op; n_ref == 0 clears `near` (and fills nn_dist with +inf). */
int gsr_near_workspace_size(int n_ref, size_t* bytes);
int gsr_near_points(void* stream, int n_ref, const float* ref_points, int n_query, const float* query_points,
                    float dist_thresh, void* workspace, uint8_t* near, float* nn_dist);

/* ---- fused, row-masked Adam step over all parameter groups in one launch ----
 * Replaces, per training step, torch.optim.Adam.step() over the six groups of GaussianModel.training_setup
 * (gaussiansplatting/scene/gaussian_model.py:336-380; lr per group, betas (0.9, 0.999), eps 1e-15, no weight decay, no
 * amsgrad), the gradient-mask hooks of apply_grad_mask (:841-856) and, optionally, the gradient of anchor_loss
 * (:152-184).  Arithmetic = torch/optim/adam.py::_single_tensor_adam in binary32 (see gsr_optim.hip).
 * Every tensor is a dense float32 device array; `numel` need not be a multiple of the row length.
 *   row_len      floats per Gaussian in this tensor (3, 45, 1, 3, 4, ...): element e belongs to row e / row_len
 *   masked       != 0: the gradient of rows with row_mask[row] == 0 is replaced by 0 (the moments still decay and the
 *                parameter still moves, exactly as with the reference's hooks)
 *   anchor       NULL, or a snapshot of the parameter: anchor_scale * row_weight[row] * (param - anchor) is added to
 *                the gradient first (anchor_scale = lambda * 2 / N of the reference's mean-reduced MSE term)
 *   lr           this group's learning rate for this step
 * step = the step count AFTER this update (1 for the first), shared by all tensors; row_mask (P bytes, 0/1) and
 * row_weight (P floats) are device pointers or NULL.  At most 8 tensors per call. */
typedef struct gsr_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  const float* anchor;
  int64_t numel;
  int32_t row_len;
  int32_t masked;
  double lr;           /* doubles where torch holds Python floats: the derived scalars are rounded to binary32 once */
  float anchor_scale;
} gsr_adam_tensor;
int gsr_adam_step(void* stream, int num_tensors, const gsr_adam_tensor* tensors, int64_t step, double beta1, double beta2,
                  double eps, const uint8_t* row_mask, const float* row_weight);
/* The same step for gradients of which only some rows were written: grad_valid (one byte per row of every tensor, device;
 * NULL = gsr_adam_step) marks them, the gradient of a row with grad_valid[row] == 0 is taken as zeros WITHOUT being read
 * (what gsr_view_messages_accumulate_rows leaves: the sums of the rows some view touched, and their mask).  Everything
 * else -- anchors, row_mask, the decay of the moments of every row -- is unchanged, so the result equals gsr_adam_step on
 * the same gradients with the invalid rows zero-filled, bit for bit. */
int gsr_adam_step_rows(void* stream, int num_tensors, const gsr_adam_tensor* tensors, int64_t step, double beta1, double beta2,
                       double eps, const uint8_t* row_mask, const float* row_weight, const uint8_t* grad_valid);

/* ---- multi-GPU exchange in "touched rows" form (new; SURVEY.md section 8(e), gaussianeditor_amd/multiview.py) ----
 * A view only produces gradients for the Gaussians it blends.  Instead of all-reducing dense (P, 14 + 3M) buffers a
 * rank packs the rows that are not entirely zero into a MESSAGE, the ranks all-gather the messages, and each rank adds
 * them per Gaussian, view 0 first: the operations and the order of one process accumulating the views one after the
 * other, bit for bit and identical on every replica (a ring all-reduce guarantees no order).
 * Message layout, 32-bit words, nb = ceil(P / 1024):
 *   [0..2] camera centre  [3] count (int32)  [4 .. 4+nb) touched rows before row block b
 *   then idx (cap x int32, ascending), means3D (cap x 3), scales (cap x 3), rotations (cap x 4), means2D (cap x 3),
 *   opacities (cap), rgb (cap x 3: the clamp-masked colour gradient gsr_preprocess_backward_rgb emits); rows >= count
 *   are padding.  All ranks use one `cap` >= every rank's count (they exchange the counts first).
 *   gsr_view_message_words        number of words of a message;
 *   gsr_view_message_plan         marks the touched rows of this view's gradients (mask: P bytes of scratch; workspace:
 *                                 gsr_compact_workspace_size(P) bytes) and returns their number in *count_host
 *                                 (one blocking readback).  With count_host == NULL nothing is read back and the call
 *                                 does not block: the count is then the uint64 at the start of `workspace`, in
 *                                 stream order (multiview.py all-gathers it from there: one host sync for all ranks'
 *                                 counts instead of two);
 *   gsr_view_message_plan_blend   the same plan from what gsr_blend_backward ALONE leaves behind -- the `touched` mask it
 *                                 writes next to its accumulator table (which then IS the plan's mask): a Gaussian no pixel
 *                                 blended has an all-zero row in the table and a 0 there, and gsr_preprocess_backward turns all-zero rows into
 *                                 all-zero gradients, so this mask is a superset of gsr_view_message_plan's (a row it
 *                                 adds carries zeros: the sums do not change).  It never blocks; the count is the uint64 at
 *                                 the start of `workspace`.  Purpose: the ranks can exchange their counts and the host can
 *                                 size the messages WHILE gsr_preprocess_backward (K8+K9, ~100 us) still runs, so the one
 *                                 host synchronisation of the exchange costs the GPU nothing;
 *   gsr_view_message_pack         writes the message (same mask / workspace).  If the view has more touched rows than
 *                                 `cap`, only the first `cap` are written (no overrun) while the header keeps the true
 *                                 count: such a message must not be accumulated -- a sender that sized its messages
 *                                 before the counts were known (multiview.py speculates on the previous steps' counts)
 *                                 sends it again with a sufficient cap;
 *   gsr_view_messages_accumulate  num_views messages, `stride_words` apart, -> the dense sums in `out` (every row of
 *                                 every array is written: Gaussians no view touched get zeros); out->sh, if not NULL,
 *                                 is rebuilt from the colour gradients exactly as gsr_sh_grad_compose does (means3D,
 *                                 active degree D, M coefficients).
 * local->sh is ignored by plan / pack. */
typedef struct gsr_dense_grads {
  float* means3D;   /* (P,3) */
  float* scales;    /* (P,3) */
  float* rotations; /* (P,4) */
  float* means2D;   /* (P,3) */
  float* opacities; /* (P,1) */
  float* sh;        /* (P,M,3) or NULL */
} gsr_dense_grads;
int gsr_view_message_words(int64_t P, int64_t cap, int64_t* words);
int gsr_view_message_plan(void* stream, int64_t P, const gsr_dense_grads* local, const float* rgb, uint8_t* mask,
                          void* workspace, int64_t* count_host);
int gsr_view_message_plan_blend(void* stream, int64_t P, const uint8_t* touched, void* workspace);
int gsr_view_message_pack(void* stream, int64_t P, const gsr_dense_grads* local, const float* rgb, const float* campos,
                          const uint8_t* mask, void* workspace, int64_t cap, float* message);
int gsr_view_messages_accumulate(void* stream, int64_t P, int D, int M, int num_views, const float* messages,
                                 int64_t stride_words, int64_t cap, const float* means3D, const gsr_dense_grads* out);
/* The same sums, written only where a view sent a row: row_valid (P bytes, device; NULL = gsr_view_messages_accumulate)
 * receives 1 for the Gaussians some view touched and 0 for the others, whose rows of `out` are NOT written (they keep their
 * previous contents).  The consumer treats those rows as zero gradients: gsr_adam_step_rows with grad_valid = row_valid takes
 * an invalid row's gradient as zeros WITHOUT reading it and still decays that row's moments, bit for bit what gsr_adam_step
 * does on zero-filled gradients.  (NOT gsr_adam_step's `row_mask`: a masked row keeps its moments from decaying, which is the
 * reference's apply_grad_mask semantics, not a zero gradient.)  A view touches ~10 % of the benchmark scene, so with 2 / 8
 * views 81 / 43 % of the 248 B per Gaussian are neither written here nor read there. */
int gsr_view_messages_accumulate_rows(void* stream, int64_t P, int D, int M, int num_views, const float* messages,
                                      int64_t stride_words, int64_t cap, const float* means3D, const gsr_dense_grads* out,
                                      uint8_t* row_valid);

/* ---- prune = stable compaction of the rows of many tensors by one mask ----
 * Replaces the per-tensor boolean-mask indexing of GaussianModel.prune_points / _prune_optimizer
 * (gaussiansplatting/scene/gaussian_model.py:568-609: parameters, Adam moments, bookkeeping tensors).
 *   gsr_compact_plan   scans keep (P bytes, 0/1, device) into `workspace` (gsr_compact_workspace_size(P) bytes of device
 *                      scratch) and returns the number of surviving rows in *kept_host (one blocking readback: the
 *                      caller sizes the outputs with it);
 *   gsr_compact_apply  one launch: for every tensor copies the surviving rows, in their original order, from src
 *                      (P rows of row_bytes) to dst (kept rows) -- what `tensor[mask]` returns.  At most 32 tensors per
 *                      call; src and dst must not overlap. */
typedef struct gsr_compact_tensor {
  const void* src;
  void* dst;
  int64_t row_bytes;
} gsr_compact_tensor;
int gsr_compact_workspace_size(int64_t P, size_t* bytes);
int gsr_compact_plan(void* stream, int64_t P, const uint8_t* keep, void* workspace, int64_t* kept_host);
int gsr_compact_apply(void* stream, int64_t P, const uint8_t* keep, void* workspace, int num_tensors,
                      const gsr_compact_tensor* tensors);

/* ---- SURVEY.md section 8(f) rank 4, second half: densification = rows APPENDED to many tensors in one launch ----
 * Replaces cat_tensors_to_optimizer (gaussiansplatting/scene/gaussian_model.py:609-641), which per parameter group runs
 * torch.cat on the parameter and on its two Adam moments (the moments extended by torch.zeros_like): 18 cats + 12 fills
 * per densification step (densify_and_clone :730-766 and densify_and_split :673-728 both end in it through
 * densification_postfix :643-671).  For every tensor: dst (P + n rows) = src (P rows) followed by ext (n rows), or by n
 * zero rows when ext == NULL -- what torch.cat((src, ext)) / torch.cat((src, zeros_like(ext))) return, bit for bit.
 * The caller allocates dst; src / ext / dst must not overlap; at most 32 tensors per call.  Which rows are appended (the
 * clone mask, the split samples) stays with the caller: a clone's ext is gsr_compact_apply's output for that mask. */
typedef struct gsr_append_tensor {
  const void* src;   /* P rows */
  const void* ext;   /* n rows, or NULL for zeros */
  void* dst;         /* P + n rows */
  int64_t row_bytes;
} gsr_append_tensor;
int gsr_append_rows(void* stream, int64_t P, int64_t n, int num_tensors, const gsr_append_tensor* tensors);

/* ---- the densification POLICY: statistics, selection, split positions, prune mask ----
 * The tensor surgery above moves rows; these entry points decide WHICH rows, as the reference's torch lines do, bit for bit
 * where stated: all float arithmetic is single binary32 operations in the order written here, no float atomics (the same
 * bits on every run), no device allocation, P == 0 is an empty call, arguments are checked before the device is touched.
 *
 * gsr_densify_stats: the per-step statistics of on_before_optimizer_step (threestudio/systems/GassuianEditor.py:251-281)
 * with add_densification_stats (gaussiansplatting/scene/gaussian_model.py:811-815) in ONE launch, no readback, never
 * blocking.  grads / radii: HOST arrays of num_views (1..8) device pointers, the views' screen-space gradients (P,3) f32
 * (viewspace_points.grad or .absgrad) and radii (P) i32.  Per row: r = max over the views of radii; r <= 0: the row is not
 * in update_filter, nothing of it is read or written (a NaN in its gradient never enters); otherwise
 * gx = ((0 + g[0].x) + g[1].x) + ..., gy likewise (:254-261), xyz_gradient_accum += sqrtf(gx*gx + gy*gy), denom += 1,
 * max_radii2D = fmaxf(max_radii2D, (float)r) (:271-273).  All three (P) f32, updated in place.  P <= 2^31 - 1. */
int gsr_densify_stats(void* stream, int64_t P, int num_views, const float* const* grads, const int32_t* const* radii,
                      float* xyz_gradient_accum, float* denom, float* max_radii2D);

/* gsr_densify_select: the decision of densify_and_prune (:771-777), densify_and_clone (:732-739) and densify_and_split
 * (:676-683) on the P original rows; P <= 2^24 (torch.quantile's own limit; the rank is computed in binary32).
 *   g = accum / denom, NaN -> 0, mask == 0 -> 0                                                     (:771-773)
 *   max_densify_percent < 1: nnz = #{g != 0}; q = 1 - (double)nnz * max_densify_percent / (double)P, rounded to binary32;
 *     rank = q * (float)(P-1), lo = floor(rank), w = rank - lo; a, b = the lo-th and min(lo+1, P-1)-th smallest g;
 *     threshold = fmaf(w, b - a, a) for w < 0.5, else fmaf(w - 1, b - a, b) (torch.quantile, 'linear'); g < threshold -> 0
 *     (:774-777).  a and b come from a radix select over the order-preserving integer image of g: four histogram passes,
 *     state on the device, no sort.  Otherwise no threshold is applied and 0 is reported.
 *   t_dense = (float)(percent_dense * extent);  hot = g >= (float)max_grad   (a float32 tensor against a Python number)
 *   clone_sel = hot && max(scaling) <= t_dense;  split_sel = hot && max(scaling) > t_dense       (P) u8 each, 0 / 1
 * The rows the clone step appends carry a padded gradient of 0 (:676-677) and are never split, so both masks are decided
 * here.  scaling (P,3) f32 is the ACTIVATED scaling (get_scaling); mask (P) u8.  max_grad <= 0 is refused (it would select
 * unmasked rows, which the reference asserts against, :756-758), as is max_densify_percent < 0.
 * workspace: gsr_densify_workspace_size(P) bytes of device scratch, 8-byte aligned.  *result_host is read back once, the
 * only host synchronisation of the call (as gsr_compact_plan's count).  Afterwards the workspace holds a gsr_compact_plan
 * of clone_sel and one of split_sel: gsr_densify_plans (host only, no device access) returns their addresses, usable as
 * gsr_compact_apply's `workspace` with the respective mask and as gsr_densify_split_xyz's `split_plan`. */
typedef struct gsr_densify_result {
  int64_t nonzero;   /* #{g != 0} before the threshold */
  int64_t n_clone;
  int64_t n_split;
  float threshold;   /* 0 when max_densify_percent >= 1 */
} gsr_densify_result;
int gsr_densify_workspace_size(int64_t P, size_t* bytes);
int gsr_densify_select(void* stream, int64_t P, const float* accum, const float* denom, const uint8_t* mask,
                       const float* scaling, double max_grad, double max_densify_percent, double percent_dense, double extent,
                       void* workspace, uint8_t* clone_sel, uint8_t* split_sel, gsr_densify_result* result_host);
int gsr_densify_plans(void* workspace, int64_t P, void** clone_plan, void** split_plan);

/* gsr_densify_split_xyz: the positions of densify_and_split's children (:685-691).  xyz (P,3), activated scaling (P,3),
 * raw rotation (P,4) (_rotation, not normalised), split_sel (P) u8 with its plan (gsr_densify_plans, or a gsr_compact_plan
 * of split_sel), n_split = its number of set rows, N copies (1..8; the reference: 2), noise (N*n_split,3) f32 standard
 * normal numbers drawn by the caller.  The child of the r-th selected parent (ascending row), copy c, is row c*n_split + r
 * of new_xyz (N*n_split,3) -- .repeat(N,1) order:
 *   sample = noise * scaling;  n = sqrtf(((r0*r0 + r1*r1) + r2*r2) + r3*r3), q = rot / n;  R = build_rotation(q) exactly as
 *   gaussiansplatting/utils/general_utils.py:78-99 writes its nine entries;
 *   new_xyz_i = ((R_i0*sample_0 + R_i1*sample_1) + R_i2*sample_2) + xyz_i.
 * The children's scaling stays with the caller (a division by a Python scalar and a log that must be torch's own).
 * P < 2^32 - 1024 (gsr_compact_plan's limit) and 0 <= n_split <= P; n_split == 0 is an empty call. */
int gsr_densify_split_xyz(void* stream, int64_t P, const float* xyz, const float* scaling, const float* rotation,
                          const uint8_t* split_sel, const void* split_plan, int64_t n_split, int N, const float* noise,
                          float* new_xyz);

/* gsr_densify_keep: the prune mask of densify_and_prune (:787-794) joined with the removal of the split parents
 * (:720-727), as a KEEP mask over the P rows after the append:
 *   keep = !(drop && drop[i]) && !((opacity < (float)min_opacity || (max_radii2D && max_radii2D[i] > (float)max_screen_size)
 *                                   || max(scaling) > (float)(0.1 * extent)) && mask)
 * opacity (P) and scaling (P,3) f32 ACTIVATED, mask (P) u8, drop (P) u8 or NULL, max_radii2D (P) f32 or NULL, keep (P) u8.
 * P <= 2^31 - 1. */
int gsr_densify_keep(void* stream, int64_t P, const float* opacity, const float* scaling, const float* max_radii2D,
                     const uint8_t* mask, const uint8_t* drop, double min_opacity, double max_screen_size, double extent,
                     uint8_t* keep);

/* ---- the 3DGS-MCMC strategy (Kheradmand et al. 2024): noise, draws, relocation values, scatter ----
 * No entry point allocates; each checks its arguments before it touches the device (NULL pointers, negative sizes, a
 * misaligned workspace or tensor: GSR_ERR_BAD_ARGUMENT); P == 0 or n == 0 is a valid empty call.  Integer atomics only:
 * every output is the same bits on every run.  P <= 2^31 - 1 (row numbers are int32).
 *
 * gsr_mcmc_noise: the positional noise of one training step, in place, one launch, no workspace, no readback.  xyz (P,3),
 * scaling_raw (P,3), rotation_raw (P,4; 16-byte aligned), opacity_raw (P) the RAW parameters, noise (P,3) standard normal
 * numbers drawn by the caller, mask (P) u8 or NULL.  Per row with mask != 0, in binary64 from the binary32 inputs, every
 * operator one IEEE operation, rounded once at the store:
 *   o = 1 / (1 + exp(-opacity_raw));  s = exp(scaling_raw);  n = sqrt(((r0*r0 + r1*r1) + r2*r2) + r3*r3), q = rot / n;
 *   R = build_rotation(q) as gsr_densify_split_xyz writes its nine entries;  g = 1 / (1 + exp(k * (o - (1 - x0))));
 *   v = (noise * g) * scaler;  w_c = (s_c*s_c) * ((R_0c*v_0 + R_1c*v_1) + R_2c*v_2)   [= diag(s^2) R^T v];
 *   xyz_a = (float)(xyz_a + ((R_a0*w_0 + R_a1*w_1) + R_a2*w_2))                        [= xyz + R diag(s^2) R^T v].
 * Rows with mask == 0 are neither read nor written. */
int gsr_mcmc_noise(void* stream, int64_t P, float* xyz, const float* scaling_raw, const float* rotation_raw,
                   const float* opacity_raw, const float* noise, const uint8_t* mask, double k, double x0, double scaler);

/* gsr_mcmc_sample: classification and the opacity-weighted draws.  opacity (P) f32 ACTIVATED, mask (P) u8 or NULL (all
 * rows), u (n) f32 in [0,1) drawn by the caller (torch.rand: multiples of 2^-24).
 *   dead_j = mask_j && opacity_j <= (float)min_opacity;  alive_j = mask_j && opacity_j > (float)min_opacity  (a NaN is
 *   neither);  k_j = (uint32)(opacity_j * 2^23) truncated (at most 2^23) for alive rows, 0 otherwise;  S_j = the inclusive
 *   64-bit prefix sum of k, total = S_{P-1}.
 *   draw r < n_draws: m = (uint64)(u_r * 2^24) (at most 2^24 - 1; a NaN or negative u draws as 0),
 *   t = (m * total) >> 24 from the full 128-bit product, src_r = the smallest j with S_j > t.
 * n_draws = n, or with draws_from_dead != 0 min(n_dead, n) (relocation: one draw per dead row, decided on the device).
 * Outputs: dead_sel (P) u8; dead_idx (P) i32, its first n_dead entries the dead rows ascending (the rest untouched);
 * src (n) i32, -1 for r >= n_draws or when total == 0; count (P) i32 = draws of row j; ratio (n) i32 =
 * min(count[src_r] + 1, 51), 0 where src_r == -1.  workspace: gsr_mcmc_workspace_size(P) bytes of device scratch, 8-byte
 * aligned.  *record_host is read back once, the only host synchronisation of the call; total == 0 with draws requested
 * shows there (every src is -1). */
typedef struct gsr_mcmc_record {
  int64_t n_dead;
  int64_t n_alive;
  int64_t n_draws;
  uint64_t total;
} gsr_mcmc_record;
int gsr_mcmc_workspace_size(int64_t P, size_t* bytes);
int gsr_mcmc_sample(void* stream, int64_t P, int64_t n, const float* opacity, const uint8_t* mask, double min_opacity,
                    const float* u, int draws_from_dead, void* workspace, uint8_t* dead_sel, int32_t* dead_idx, int32_t* src,
                    int32_t* count, int32_t* ratio, gsr_mcmc_record* record_host);

/* gsr_mcmc_relocation_values: for draw r with source s = src_r and N = ratio_r (clamped to 1..51), in binary64 from the
 * binary32 inputs, rounded at the stores:
 *   o = min(opacity_s, 1 - 2^-24);  o' = 1 - pow(1 - o, 1 / N);
 *   denom = sum_{i=1..N} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1)   (added in this order; the power by repeated
 *   products; term = (C * power) / sqrt(k+1));  f = o / denom;  o' clamped to [(float)min_opacity, 1 - 2^-23];
 *   new_opacity_raw_r = log(o' / (1 - o'));  new_scaling_raw_r,c = log(exp(scaling_raw_s,c) * f).
 * opacity (P) ACTIVATED, scaling_raw (P,3) RAW; outputs (n) and (n,3), zeros where src_r is not a row.  Only inputs are
 * read and only draw-indexed outputs written: the outputs may not alias the inputs. */
int gsr_mcmc_relocation_values(void* stream, int64_t P, int64_t n, const int32_t* src, const int32_t* ratio,
                               const float* opacity, const float* scaling_raw, double min_opacity, float* new_opacity_raw,
                               float* new_scaling_raw);

/* gsr_mcmc_scatter: the row writes of relocation and growth for up to 32 tensors, one launch per role in use.  Draw r has the source
 * row s = src_r of `base` (P rows) and the destination row d = dst_idx_r (dst_idx != NULL) or r of `dst` (dst_rows rows;
 * relocation: dst == base, dst_idx = the dead rows; growth: dst = the rows to append, dst_idx = NULL).
 *   GSR_MCMC_COPY   dst[d] = base[s]
 *   GSR_MCMC_VALUE  dst[d] = base[s] = values[r]        (values: (n) rows of row_bytes)
 *   GSR_MCMC_ZERO   base[s] = 0                          (dst unused)
 * Draws with src_r outside [0, P) write nothing, a d outside [0, dst_rows) no destination row.  The caller guarantees what
 * gsr_mcmc_sample's outputs have: no source row is a destination row, and the draws of one source carry equal values.
 * row_bytes a multiple of 4 up to 2^20, pointers 4-byte aligned. */
#define GSR_MCMC_COPY 0
#define GSR_MCMC_VALUE 1
#define GSR_MCMC_ZERO 2
typedef struct gsr_mcmc_tensor {
  void* base;
  void* dst;
  const void* values;
  int64_t row_bytes;
  int32_t role;
} gsr_mcmc_tensor;
int gsr_mcmc_scatter(void* stream, int64_t P, int64_t n, const int32_t* src, const int32_t* dst_idx, int64_t dst_rows,
                     int num_tensors, const gsr_mcmc_tensor* tensors);

/* ---- similarity transforms of Gaussians, with the rotation of the SH coefficients ----
 * The editing operation "move what was selected": T: x -> s R x + t, R a proper rotation, s > 0 uniform.  Per selected row,
 * in binary64 from the binary32 inputs, rounded once at the store:
 *   xyz (P,3):             xyz' = s R^ xyz + t
 *   rotation (P,4) w,x,y,z RAW: q' = q_R (x) q, the Hamilton product; the raw norm is kept (the activation normalises)
 *   scaling (P,3) RAW:     sigma' = log(exp(sigma) s + scale_eps)
 *   sh_rest (P,rest,3), rest = 3, 8 or 15 (SH degree 1, 2, 3 without the DC term): for each band l and each channel
 *                          c' = D^l c, D^l the (2l+1) x (2l+1) matrix with sum_m c'_m Y_m(R^ d) = sum_m c_m Y_m(d) for every
 *                          unit d, Y the real basis of the rasterizer (its order and signs).  Band 0 is invariant.
 * q_R is the unit quaternion of rot (row-major, x' = rot x) by Shepperd's method in binary64, w >= 0, and R^ = matrix(q_R)
 * is what all four use: an exactly orthonormal rotation even where rot was rounded to binary32.  rot is refused
 * (GSR_ERR_BAD_ARGUMENT) unless it is a proper rotation: the largest absolute row sum of rot^T rot - I at most 1e-4 and a
 * positive determinant -- no reflections, no non-uniform scale.
 * gsr_sh_rotation: host only, no device.  out[83] = D1 (9) | D2 (25) | D3 (49), row-major, of R^.  The identity gives
 *   exactly the identity.
 * gsr_transform_rows: in place, one launch, no workspace, no host synchronisation, any stream.  rot, trans and the numbers
 *   are read before the call returns (they travel as kernel arguments: no host-to-device copy).  Any of the four tensors
 *   may be NULL = untouched; 4-byte alignment is all they need (views at any float offset).  mask (P) u8 or NULL (all rows):
 *   a row whose mask is 0 is NEVER stored to, not even with its own value.  No atomics: the same bits on every run.
 *   P == 0 returns GSR_OK.  GSR_ERR_BAD_ARGUMENT, before the device is touched: all four tensors NULL, rest outside
 *   {0, 3, 8, 15}, sh_rest with rest == 0, rot not a proper rotation, scale <= 0, scale_eps < 0, a number that is not
 *   finite, a misaligned pointer.  A failed launch is GSR_ERR_HIP and gsr_last_hip_error() is not updated. */
int gsr_sh_rotation(const double rot[9], double out[83]);
int gsr_transform_rows(void* stream, int64_t P, int rest, float* xyz, float* rotation, float* scaling, float* sh_rest,
                       const uint8_t* mask, const double rot[9], const double trans[3], double scale, double scale_eps);

/* ---- surface normals: per Gaussian, from the depth image, and the loss that ties them together ----
 * Conventions.  viewmatrix: the 16 floats the rasterizer takes (the transposed view matrix V, row 3 the translation): the
 * view-space point is p_c = p_w V[:3,:3] + V[3,:3], axes as COLMAP (z forward), and the depth of a Gaussian is p_c.z.
 * Pixel (x, y) (column, row; integers) lies on the ray r(x,y) = ((x - cx) / fx, (y - cy) / fy, 1); what ndc2Pix implies is
 * fx = W / (2 tanfovx), fy = H / (2 tanfovy), cx = (W - 1) / 2, cy = (H - 1) / 2.  Every normal is in camera space and
 * points towards the camera (n . p_c < 0).  Inputs and outputs are binary32, the arithmetic is binary64, rounded once at
 * the store; no atomics, every sum in a fixed order: the same bits on every run and on every stream.
 *
 * (a) The normal of a Gaussian.  rotations (P,4) w,x,y,z RAW, scales (P,3), means3D (P,3), out (P,3):
 *   q^ = q / |q|;  k = argmin_j scales[j], on a tie the lowest index;  n_w = column k of R(q^), R as the reference's
 *   build_rotation;  n_c = n_w V[:3,:3];  s = -1 if n_c . p_c > 0 else +1;  out = s n_c.
 *   The backward, from dL_dout (P,3), writes dL_drotations (P,4): through column k and through the normalisation, so it is
 *   orthogonal to q; k and s are recomputed from the inputs (no saved state).  scales, means3D and the camera get no
 *   gradient: the output is piecewise constant in them.  A precomputed covariance is not supported.
 *
 * (b) The normal of the depth image.  depth (1,H,W); alpha (1,H,W) or NULL; out (3,H,W), planar.
 *   z = depth / max(alpha, 1e-8) with alpha (depth is then the unnormalised sum of z w), z = depth without;
 *   p(x,y) = z(x,y) r(x,y);  c = (p(x,y+1) - p(x,y-1)) x (p(x+1,y) - p(x-1,y));  n = c / |c|
 *   (central differences; with this operand order the camera-facing normal, exact on a plane under perspective).
 *   out is exactly (0,0,0) at an invalid pixel: one on the image border, one whose centre or any of whose four taps has
 *   alpha <= alpha_min (with alpha) or z <= 0, or one with |c|^2 < 1e-30.  The normal depends on the four taps, not on the
 *   centre.  The backward, from dL_dout (3,H,W), writes dL_ddepth and dL_dalpha (1,H,W) (through z only; the validity mask
 *   carries no gradient): each depth pixel gathers the terms of the up to four normals around it.  Either may be NULL: it
 *   is then not computed (both NULL: nothing is launched); dL_dalpha without alpha is refused.
 *
 * (c) The consistency loss.  normals N (3,H,W): the alpha-composited normal image (|N| <= A); depth, alpha (1,H,W) as in
 *   (b), alpha required: it is also the weight A.
 *   loss = 1 / (H W) sum over the valid pixels of (A - <N, n_d>),  n_d of (b), never written to memory.
 *   Every term is >= 0 and equals A (1 - <N / A, n_d>).  The normalisation is H W, not the number of valid pixels: the loss
 *   does not jump when a pixel changes validity.  out_loss: one device float.  workspace: gsr_normal_loss_workspace_size
 *   bytes of device scratch, 8-byte aligned (one partial sum per tile, added in ascending order).
 *   The backward reads dL_dloss, ONE device float (the host neither waits nor reads anything back), and writes
 *   dL_dnormals (3,H,W) = -dL_dloss / (H W) n_d at valid pixels, 0 elsewhere, and dL_ddepth, dL_dalpha (1,H,W) through n_d;
 *   the explicit A term gives no gradient (a constant weight).  Any of the three may be NULL: it is then not computed.
 *
 * All seven: the caller owns every buffer and every output element is written (no pre-zeroing); the caller's stream, no
 * host synchronisation.  P == 0 and images without interior pixels (H < 3 or W < 3) are valid: outputs fully written, zeros.
 * GSR_ERR_BAD_ARGUMENT, before the device is touched: P < 0 or > 2^31 - 1, H or W < 1, H W > 2^31 - 1, H > 524 280, fx or fy
 * not finite and positive, cx, cy or alpha_min not finite, a required pointer NULL (P > 0 for (a)), a pointer of (a) that is
 * not 4-byte aligned, a misaligned workspace.  A failed launch is GSR_ERR_HIP and gsr_last_hip_error() is not updated. */
int gsr_gaussian_normals_forward(void* stream, int64_t P, const float* rotations, const float* scales, const float* means3D,
                                 const float* viewmatrix, float* out);
int gsr_gaussian_normals_backward(void* stream, int64_t P, const float* rotations, const float* scales, const float* means3D,
                                  const float* viewmatrix, const float* dL_dout, float* dL_drotations);
int gsr_depth_normals_forward(void* stream, int H, int W, double fx, double fy, double cx, double cy, double alpha_min,
                              const float* depth, const float* alpha, float* out);
int gsr_depth_normals_backward(void* stream, int H, int W, double fx, double fy, double cx, double cy, double alpha_min,
                               const float* depth, const float* alpha, const float* dL_dout, float* dL_ddepth, float* dL_dalpha);
int gsr_normal_loss_workspace_size(int H, int W, size_t* bytes);
int gsr_normal_loss_forward(void* stream, int H, int W, double fx, double fy, double cx, double cy, double alpha_min,
                            const float* normals, const float* depth, const float* alpha, void* workspace, float* out_loss);
int gsr_normal_loss_backward(void* stream, int H, int W, double fx, double fy, double cx, double cy, double alpha_min,
                             const float* normals, const float* depth, const float* alpha, const float* dL_dloss,
                             float* dL_dnormals, float* dL_ddepth, float* dL_dalpha);

/* ---- Mip-Splatting's 3D smoothing filter: the camera sweep and the fused apply ----
 * What a scene trained with Mip-Splatting (compute_3D_filter, get_scaling_with_3D_filter, get_opacity_with_3D_filter) needs
 * next to the 2D filter of GSR_FLAG_ANTIALIAS: a per-Gaussian filter size from the training cameras, folded into scales and
 * opacity in front of every render.
 *
 * (a) The sweep.  means3D (P,3) f32; cameras: V records of GSR_FILTER3D_CAMERA_DOUBLES binary64 ON THE DEVICE, 8-byte
 *   aligned, packed once by the caller.  With M = the camera's transposed view matrix (the 16 floats the rasterizer takes, row 3
 *   the translation), W, H its image size and fx = W / (2 tan(FoVx / 2)), fy = H / (2 tan(FoVy / 2)) its focal lengths in
 *   pixels, a record is
 *     [3 r + k] = (double)M[r][k], r = 0..3, k = 0..2 | [12] fx | [13] fy | [14] 0.5 W | [15] 0.5 H |
 *     [16] -0.15 W | [17] 1.15 W | [18] -0.15 H | [19] 1.15 H            (each product one binary64 multiplication).
 *   All arithmetic is binary64 on the binary32 inputs, one IEEE operation per operator, in exactly this order.  For the row
 *   (x, y, z) and every camera:
 *     p_k = ((x M[0][k] + y M[1][k]) + z M[2][k]) + M[3][k], k = 0, 1, 2;   zc = p_2;   zz = max(zc, 0.001);
 *     u = (p_0 / zz) fx + 0.5 W;   v = (p_1 / zz) fy + 0.5 H;
 *     the camera sees the row if zc > (double)0.2f (the rasterizer's near plane) and -0.15 W <= u <= 1.15 W and
 *     -0.15 H <= v <= 1.15 H (bounds inclusive);  then d = min(d, zc).
 *   valid (P) u8: 1 where at least one camera saw the row.  A row no camera saw takes d = the largest d of the seen rows;
 *   when no row at all was seen every row takes d = 100000 (Mip-Splatting raises there; nothing here waits for the device
 *   in order to raise).  filter_3D (P,1) f32 = (float)((d / f_max) coef): the caller passes f_max = the largest fx of ALL
 *   cameras, whether they saw anything or not, and coef = sqrt(0.2).
 *   One launch sweeps all cameras, a second small one fills in the unseen rows; the host reads nothing back.  workspace:
 *   gsr_filter3d_workspace_size bytes of device scratch, 8-byte aligned, zeroed by the call itself (one 64-bit word: the
 *   maximum, by an integer atomic max on the bits of the positive double -- independent of the order; no float atomics).
 *
 * (b) The apply.  scales (P,3), opacity (P,1), filter_3D (P,1) -> scales_eff (P,3), opacity_eff (P,1).  from_raw = 0: the
 *   inputs are the activated values s, o;  from_raw = 1: they are the raw parameters and s = exp(raw), o = 1 / (1 + exp(-raw)).
 *   With f = filter_3D of the row and e_k = s_k^2 + f^2:
 *     s_eff_k = sqrt(e_k);   coef = sqrt((s_0^2 / e_0) (s_1^2 / e_1) (s_2^2 / e_2));   o_eff = o coef.
 *   At f = 0 coef is exactly 1 and s_eff = s.  The backward, from dL_dscales_eff (P,3) and dL_dopacity_eff (P,1) (either may
 *   be NULL = zero), writes
 *     dL_ds_k = dL_ds_eff_k s_k / s_eff_k + dL_do_eff o_eff f^2 / (s_k e_k);   dL_do = dL_do_eff coef
 *   (no 0 / 0 at f = 0: the cross term is then exactly 0), with from_raw = 1 multiplied by s_k and o (1 - o): the gradient
 *   of the raw parameters.  Either output may be NULL: it is then not computed (both NULL: nothing is launched).  filter_3D
 *   gets no gradient.  Everything is recomputed from the inputs (no saved state).  Scales must be positive.
 *
 * All four: binary32 in and out, binary64 inside, rounded once at the store; the caller owns every buffer and every output
 * element is written; the caller's stream, no host synchronisation; the same bits on every run.  P == 0 returns GSR_OK
 * without a launch.  GSR_ERR_BAD_ARGUMENT, before the device is touched: P < 0 or > 2^31 - 1, V <= 0, f_max not finite and
 * positive, coef not finite, from_raw outside {0, 1}, a required pointer NULL (P > 0; cameras always), a float pointer that
 * is not 4-byte aligned, cameras or workspace not 8-byte aligned.  A failed launch is GSR_ERR_HIP and gsr_last_hip_error()
 * is not updated. */
#define GSR_FILTER3D_CAMERA_DOUBLES 20
int gsr_filter3d_workspace_size(int64_t P, size_t* bytes);
int gsr_filter3d_sweep(void* stream, int64_t P, int V, const float* means3D, const double* cameras, double f_max, double coef,
                       void* workspace, float* filter_3D, uint8_t* valid);
int gsr_filter3d_apply_forward(void* stream, int64_t P, int from_raw, const float* scales, const float* opacity,
                               const float* filter_3D, float* scales_eff, float* opacity_eff);
int gsr_filter3d_apply_backward(void* stream, int64_t P, int from_raw, const float* scales, const float* opacity,
                                const float* filter_3D, const float* dL_dscales_eff, const float* dL_dopacity_eff,
                                float* dL_dscales, float* dL_dopacity);

/* ---- TSDF fusion of rendered depth and mesh extraction by marching tetrahedra ----
 * A dense truncated-signed-distance volume on a lattice of nx x ny x nz points, fused from depth images, and the mesh of
 * its zero level.  Lattice point (i, j, k) sits at origin + voxel_size (i, j, k); its linear index is n = (i ny + j) nz + k
 * (k fastest).  tsdf (nx,ny,nz) f32 (a fresh volume holds 1), weight (nx,ny,nz) f32 (a fresh volume holds 0), optionally
 * vol_color (3,nx,ny,nz) f32; the caller owns and initialises them.
 *
 * (a) gsr_tsdf_integrate fuses V views, IN ORDER, in one launch: depth (V,1,H,W) f32, alpha (V,1,H,W) f32 | NULL, color
 *   (V,3,H,W) f32 | NULL (given exactly when vol_color is), cameras: V records of GSR_FILTER3D_CAMERA_DOUBLES binary64 on the
 *   device, the layout of gsr_filter3d_sweep, of which [0..11] (the view rows M) and [12] fx, [13] fy are read; the image
 *   size is the W, H of the call.  Projection and comparisons are binary64 on the binary32 inputs, the running average is
 *   binary32; one IEEE operation per operator in exactly this order.  With cx = ((double)W - 1) 0.5, cy = ((double)H - 1) 0.5
 *   (the rasterizer's pixel centres, ndc2Pix) and the point x_c = (double)origin_c + (double)voxel_size (double)index_c,
 *   per lattice point and per view:
 *     1. p_k = ((x M[0][k] + y M[1][k]) + z M[2][k]) + M[3][k], k = 0, 1, 2;  zc = p_2;  skip unless zc > (double)0.2f;
 *     2. u = (p_0 / zc) fx + cx;  v = (p_1 / zc) fy + cy;
 *     3. iu = floor(u + 0.5), iv = floor(v + 0.5);  skip unless 0 <= iu < W and 0 <= iv < H;
 *     4. d = depth[iv][iu];  with alpha: a = alpha[iv][iu], skip if (double)a < alpha_min, else d = d / a (binary32);
 *        skip unless d > 0;
 *     5. sdf = (double)d - zc;  skip if sdf < -trunc;  obs = (float)min(sdf / trunc, 1);
 *     6. w1 = w + 1;  tsdf = (tsdf w + obs) / w1, and color_c = (color_c w + pixel_c) / w1 for the three channels;
 *        if max_weight > 0: w1 = min(w1, max_weight);  w = w1                                   (all binary32).
 *   A lattice point's state stays in registers over all V views and is stored once, so a call with V views gives the bits of
 *   V calls with one view each.  No atomics; the same bits on every run.
 *   GSR_ERR_BAD_ARGUMENT, before the device is touched: an extent < 1, nx ny nz > 2^31 - 1, V < 1, W or H < 1, V H W >
 *   2^31 - 1, voxel_size, trunc or alpha_min not finite and positive, max_weight negative or not finite, origin not finite,
 *   a required pointer NULL, color given without vol_color or the reverse, a float pointer not 4-byte aligned, cameras not
 *   8-byte aligned.
 *
 * (b) Mesh extraction, marching tetrahedra on the same lattice.  A point is inside iff tsdf < 0 and observed iff weight > 0.
 *   Cube (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, is cut into the six Kuhn tetrahedra, one per axis permutation in the
 *   order xyz, xzy, yxz, yzx, zxy, zyx:  v0 = the corner, v1 = v0 + e_pi1, v2 = v1 + e_pi2, v3 = corner + (1,1,1) ("path
 *   order").  A tetrahedron emits nothing unless all four points are observed.  One point a inside (or, mirrored, one
 *   outside), the others b < c < d in path order: the triangle over the edges (a,b), (a,c), (a,d).  Two inside a < b, two
 *   outside c < d: the quad q0 = (a,c), q1 = (a,d), q2 = (b,d), q3 = (b,c) as the triangles (q0,q1,q2), (q0,q2,q3).  Where the
 *   6 x 16 orientation table (tetrahedron, case; built at compile time in integers from the edge midpoints, never from the
 *   values) says so, a triangle (A,B,C) is emitted as (A,C,B): every normal points to the outside (positive) half.
 *   A vertex lives on a lattice edge from a lower point in one of the 7 directions d, kinds 0..6 = 100, 010, 001, 110, 101,
 *   011, 111 (as dx dy dz), with key 7 n(lower) + kind.  With f0, f1 the values at the lower and the upper point, in binary32:
 *     t = f0 / (f0 - f1);  position_c = origin_c + voxel_size ((float)lower_c + t d_c);  color_c = c0 + t (c1 - c0).
 *   Vertex ids are the ranks of the used keys in ascending order; faces are ordered by (n of the cube's corner, tetrahedron,
 *   triangle); every vertex is referenced by a face.
 *   gsr_tsdf_mesh_count marks the used edges, counts the faces per cube, scans, and returns counts_host[0] = vertices,
 *   counts_host[1] = faces after ONE host synchronisation of `stream` (the caller sizes the outputs by them).
 *   gsr_tsdf_mesh_emit, with the SAME workspace untouched in between and the same volume, fills vertices (n_vertices,3) f32,
 *   colors (n_vertices,3) f32 | NULL (needs vol_color) and faces (n_faces,3) i32; no host synchronisation.  With both counts
 *   0 nothing is launched and the pointers may be NULL.  workspace: gsr_tsdf_mesh_workspace_size bytes, 256-byte aligned.
 *   Integer atomics only (an OR of marks: independent of the order); the same bits on every run.
 *   GSR_ERR_TOO_MANY: 7 nx ny nz >= 2^31 (the keys are 31-bit) or more than 2^31 - 1 faces.  GSR_ERR_BAD_ARGUMENT, before the
 *   device is touched: an extent < 1, a required pointer NULL, a misaligned pointer, voxel_size or origin not finite,
 *   negative counts.
 * A failed launch is GSR_ERR_HIP and gsr_last_hip_error() is not updated. */
int gsr_tsdf_integrate(void* stream, int nx, int ny, int nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                       int V, int H, int W, const float* depth, const float* alpha, const float* color, const double* cameras,
                       double trunc, double alpha_min, float max_weight, float* tsdf, float* weight, float* vol_color);
int gsr_tsdf_mesh_workspace_size(int nx, int ny, int nz, size_t* bytes);
int gsr_tsdf_mesh_count(void* stream, int nx, int ny, int nz, const float* tsdf, const float* weight, void* workspace,
                        int64_t* counts_host);
int gsr_tsdf_mesh_emit(void* stream, int nx, int ny, int nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                       const float* tsdf, const float* weight, const float* vol_color, const void* workspace,
                       int64_t n_vertices, int64_t n_faces, float* vertices, float* colors, int32_t* faces);

/* ---- the training loss: fused L1 + SSIM of two images, and its gradient ----
 * Replaces l1_loss / ssim of gaussiansplatting/utils/loss_utils.py:17-63 and the loss line of the reference's trainers,
 * (1 - lambda) * l1_loss + lambda * (1 - ssim) (gaussiansplatting/train.py:89, train_from_mesh.py:136): five grouped
 * 11 x 11 conv2d calls, some fifteen elementwise kernels, and autograd's backward through all of them.
 *   loss = w_l1 * L1 + w_ssim * SSIM + c,   L1 = mean |img - gt|,   SSIM = mean of the SSIM map
 * over `planes` (= batch x channels) planes of H x W pixels, N = planes * H * W values in all; the SSIM window is the
 * reference's: 11 taps, sigma 1.5, normalised, zero padding of 5.  (1 - lambda, -lambda, lambda) gives the trainers' loss,
 * (0, 1, 0) ssim(), (1, 0, 0) l1_loss().  With w_ssim == 0 the SSIM is NOT evaluated: no convolution work, `maps` is neither
 * written nor read, out3[2] is NaN.
 *   img, gt (planes,H,W) f32 in; workspace: gsr_loss_workspace_size bytes of device scratch, 8-byte aligned (two partial
 *       sums per 16 x 64 tile, added in a fixed order: no float atomics, the same bits on every run);
 *   out3: three device floats, (loss, L1, SSIM);
 *   maps (3,planes,H,W) f32: three per-pixel derivative maps the forward writes for the backward, NULL when no backward
 *       follows (the metric path: 12 N bytes less traffic).  The backward requires them (NULL: GSR_ERR_BAD_ARGUMENT; with
 *       w_ssim == 0 any non-NULL pointer, e.g. img, serves);
 *   dL_dloss: ONE device float, the upstream gradient, read by the kernel (the host neither waits nor reads anything back);
 *   dL_dimg (planes,H,W) f32 out, fully written: dL_dloss * d loss / d img, with sign(0) = 0 in the L1 term.  gt gets no
 *       gradient.
 * img / gt / w_l1 / w_ssim of the backward are those of the forward that wrote `maps`.  At most 2^24 - 1 tiles of 16 x 64
 * pixels (more: GSR_ERR_BAD_ARGUMENT).  A failed launch is reported as GSR_ERR_HIP, but gsr_last_hip_error() is NOT updated
 * by these three entry points (it may hold an earlier call's code): rely on the return value alone. */
int gsr_loss_workspace_size(int planes, int H, int W, size_t* bytes);
int gsr_photometric_loss_forward(void* stream, int planes, int H, int W, const float* img, const float* gt, float w_l1,
                                 float w_ssim, float c, float* maps, void* workspace, float* out3);
int gsr_photometric_loss_backward(void* stream, int planes, int H, int W, const float* img, const float* gt,
                                  const float* maps, float w_l1, float w_ssim, const float* dL_dloss, float* dL_dimg);

/* ---- per-image appearance compensation: the bilateral-grid slice and its TV regulariser ----
 * What 3DGS trainers put between the render and the loss for real captures (gsplat: use_bilateral_grid, "slice" and
 * total_variation_loss): a small learnable grid of 3 x 4 affine colour transforms per training image.
 *   grids (N,12,GZ,GY,GX) f32, grids[n][k][z][y][x], k = 4 c + m: row c, column m of a row-major 3 x 4 matrix (gsplat's layout);
 *   img, out, dL_dout, dL_dimg (B,3,H,W) f32, planar;  idx (B) int64 ON THE DEVICE: image b uses grids[idx[b]].  The kernels
 *       read it (the host neither waits nor reads anything back) and CLAMP it to [0, N - 1]: an index out of range selects
 *       the nearest valid grid and nothing outside `grids` is read or written.
 * Slice, for the pixel in row i, column j with colour (r, g, b):
 *   u = (j + 0.5) / W, v = (i + 0.5) / H, gray = 0.299 r + 0.587 g + 0.114 b,
 *   gx = u (GX - 1), gy = v (GY - 1), gz = clamp(gray, 0, 1) (GZ - 1);  x0 = min(floor(gx), GX - 2), fx = gx - x0, same for y, z;
 *   A[k] = the trilinear interpolation of grids[idx[b]][k] at (gz, gy, gx) (grid_sample with align_corners = True and border
 *   padding);  out_c = A[4c] r + A[4c+1] g + A[4c+2] b + A[4c+3].
 * Backward, from dL_dout: dL_dgrids (N,12,GZ,GY,GX), dense and FULLY written -- grids no image selected get exact zeros, a
 * grid selected by several images the sum over them --; dL_dimg_m = sum_c dL_dout_c A[4c+m] + (0.299, 0.587, 0.114)_m
 * (GZ - 1) sum_k dA[k]/dgz dL/dA[k], the second (guidance) term only where 0 < gray < 1.  Either output may be NULL: it is
 * then not computed (both NULL: nothing is launched).
 * TV: tv = (1 / N) sum over d in {z, y, x} of sum (forward difference along d)^2 / count_d, count_d = the differenced
 * elements of ONE grid (12 (GZ - 1) GY GX for z); out1: one device float.  Its backward writes dL_dtv * d tv / d grids;
 * dL_dtv is ONE device float read by the kernel.
 * 2 <= GX, GY <= 32, 2 <= GZ <= 16, N, B, H, W >= 1, H W < 2^31 - 2^17 (else GSR_ERR_BAD_ARGUMENT).  workspace:
 * gsr_bilagrid_workspace_size (the slice backward; needed only with dL_dgrids) or gsr_bilagrid_tv_workspace_size (the TV
 * forward) bytes of device scratch, 8-byte aligned.  Coordinates, weights and sums are binary64, there are no atomics and
 * every sum has a fixed order: all four results are the same bits on every run.  As with the loss, a failed launch is
 * GSR_ERR_HIP and gsr_last_hip_error() is not updated. */
int gsr_bilagrid_workspace_size(int B, int H, int W, int GX, int GY, int GZ, size_t* bytes);
int gsr_bilagrid_slice_forward(void* stream, int B, int H, int W, int N, int GX, int GY, int GZ, const float* grids,
                               const int64_t* idx, const float* img, float* out);
int gsr_bilagrid_slice_backward(void* stream, int B, int H, int W, int N, int GX, int GY, int GZ, const float* grids,
                                const int64_t* idx, const float* img, const float* dL_dout, void* workspace, float* dL_dimg,
                                float* dL_dgrids);
int gsr_bilagrid_tv_workspace_size(int N, int GX, int GY, int GZ, size_t* bytes);
int gsr_bilagrid_tv_forward(void* stream, int N, int GX, int GY, int GZ, const float* grids, void* workspace, float* out1);
int gsr_bilagrid_tv_backward(void* stream, int N, int GX, int GY, int GZ, const float* grids, const float* dL_dtv,
                             float* dL_dgrids);

/* ---- introspection used by the parity tests (not needed by the drop-in) ----
 * Copy internal per-Gaussian / per-instance / per-pixel state out of the opaque
 * scratch buffers into caller-provided DEVICE arrays (any may be NULL):
 *   means2D (P,2) f32, depths (P) f32, rgb (P,3) f32, conic_opacity (P,4) f32,
 *   tiles_touched (P) u32, clamped (P,3) u8;
 *   keys (R) u64 sorted, point_list (R) u32 sorted; ranges (T,2) u32; final_T (N) f32; n_contrib (N) u32.
 * The 3D covariance (reference: geomState.cov3D, rasterizer_impl.cu:225) is not kept in `geom`: forward and backward
 * both compute it from scales / rotations with the same operations.  gsr_debug_cov3d evaluates that function for all
 * P Gaussians into cov3D (P,6). */
int gsr_debug_export_geom(void* stream, int P, const void* geom, float* means2D, float* depths, float* rgb,
                          float* conic_opacity, uint32_t* tiles_touched, uint8_t* clamped);
int gsr_debug_cov3d(void* stream, int P, const float* scales, float scale_modifier, const float* rotations, float* cov3D);
int gsr_debug_export_binning(void* stream, int P, int64_t R, int W, int H, const void* geom, const void* binning,
                             uint64_t* keys, uint32_t* point_list);
int gsr_debug_export_image(void* stream, int W, int H, const void* image, uint32_t* ranges, float* final_T,
                           uint32_t* n_contrib);

/* Performance introspection (tools/wave_profile.py): run K6 with per-wave instrumentation.  One record
 * of 8 x u64 per launched workgroup: {s_memtime at start, at end, XCC_ID<<32 | HW_ID,
 * items<<32 | entries evaluated, cycles chunk start -> survivors staged, cycles in the group loops, chunks walked,
 * cycles chunk start -> cull ballot}; records of workgroups that exit before doing any work stay zero.  *n_records_host = number of workgroups (call with max_records = 0
 * to query; returns GSR_ERR_BAD_ARGUMENT in that case after setting it). */
/* The same for K7: one record of 8 x u64 per 4-wave workgroup: {start, end, XCC_ID<<32 | HW_ID, tiles<<32 | forward work
 * estimate of those tiles, longest tile (ticks), first tile (ticks), 0, 0}.  Arguments as gsr_blend_backward. */
int gsr_debug_blend_backward_profile(void* stream, int P, int64_t R, int W, int H, const float* bg, const void* geom,
                                     const void* binning, const void* image, const float* dL_dpix, float* acc,
                                     uint64_t* records, int64_t max_records, int64_t* n_records_host);
int gsr_debug_blend_forward_profile(void* stream, int P, int64_t R, int W, int H, const float* bg, const void* geom,
                                    const void* binning, void* image, float* out_color, float* out_depth,
                                    uint64_t* records, int64_t max_records, int64_t* n_records_host);

/* Which kernel did a backward run, and on what work?  Host-side bookkeeping for the tests: nothing is launched.
 * gsr_debug_blend_backward_launches: counts[32] (HOST) receives how often this process has launched K7 so far, per
 * instantiation, at index FAST | SEG << 1 | DEPTH << 2 | ABS << 3 | ALPHA << 4 -- FAST: GSR_FLAG_FAST_EXP; SEG: the work
 * list MAY hold list-segment items (the view's forward left checkpoints, GSR_BWD_SEG > 0 and there is no depth gradient;
 * whether a tile is then cut depends on its work: gsr_debug_blend_backward_items says); DEPTH: gsr_blend_backward_depth / _alpha with
 * dL_ddepth (excludes SEG: those eight indices stay 0); ABS: GSR_FLAG_ABS_GRAD; ALPHA: gsr_blend_backward_alpha.  Counted
 * where the instantiation is chosen, with relaxed atomics (renders may run from several host threads).
 * gsr_debug_blend_backward_items: counts[2] (HOST) receives {items, list-segment items among them} of the work list the
 * LATEST blend backward of the view with image state `image` (W x H) built.  Copies the list to the host and waits for
 * `stream`; GSR_ERR_BAD_ARGUMENT for NULL / non-positive arguments or a state whose item count exceeds the list's room
 * (no blend backward has run on it). */
int gsr_debug_blend_backward_launches(uint64_t* counts);
int gsr_debug_blend_backward_items(void* stream, int W, int H, const void* image, int64_t* counts);

/* Which radix scatter did the binning run?  Host-side bookkeeping for the tests: nothing is launched.
 * gsr_debug_sort_launches: counts[24] (HOST) receives how often this process has launched the stable scatter kernels of
 * gsr_binning.hip so far, per instantiation.  TH is the block width of the sort: 1024 for sorts of up to 1024 blocks of
 * 4096 keys, 256 beyond, or what GSR_SORT_THREADS says for every sort of the process (depth order, group instances, tile
 * pairs, gsr_knn's and gsr_near's Morton codes).
 *    0 ..  7  sort_scatter_kernel<IOTA, K, TH>      IOTA | (K is uint32_t) << 1 | (TH == 1024) << 2
 *             (the tile-pair sort, 16- or 32-bit tile ids, IOTA never; the depth order of the pair-sort path and the
 *              Morton sort: K = uint32_t, IOTA in their first pass.  IOTA with 16-bit keys is never launched: 1 and 5 stay 0)
 *    8 .. 15  depth_scatter_kernel<LAST, IOTA, TH>  LAST | IOTA << 1 | (TH == 1024) << 2
 *             (the grouped path's depth order: three or four passes, so LAST & IOTA is never launched: 11 and 15 stay 0)
 *   16 .. 19  group_scatter_kernel<BITS, TH>        (BITS == 11) | (TH == 1024) << 1
 *   20        launches of sort_scan_kernel whose rows exceed one round of its block (more than 2048 blocks, i.e. more than
 *             8 388 608 keys): the rounds behind the first start from a carry
 *   21 .. 23  zero
 * Counted where the instantiation is chosen, with relaxed atomics (renders may run from several host threads).
 * GSR_ERR_BAD_ARGUMENT for NULL. */
int gsr_debug_sort_launches(uint64_t* counts);

/* Which chunk kernel did the grouped binning run?  Host-side bookkeeping for the tests: nothing is launched.
 * gsr_debug_group_launches: counts[16] (HOST) receives how often this process has launched group_chunk_kernel<SCATTER, NB>
 * of gsr_binning.hip so far.  NB = chunk length / 64: 1, 2, 4 or 8 by the number of group instances G of the view, or what
 * GSR_GROUP_CHUNK=64|128|256|512 says for every view of the process.  Index:
 *    log2(NB) | SCATTER << 2 | (LDS stage of 2048 entries) << 3
 *    0 ..  3  the count pass (no stage: the stage bit is 0, so 8 .. 11 stay 0)
 *    4 ..  7  the append pass with a stage of 1024 entries: (R / G + 1) * chunk length <= 820.  R >= G, so a chunk of 512
 *             never has it: 7 stays 0
 *   12 .. 15  the append pass with a stage of 2048 entries
 * Counted where the instantiation is chosen, with relaxed atomics (renders may run from several host threads).
 * GSR_ERR_BAD_ARGUMENT for NULL. */
int gsr_debug_group_launches(uint64_t* counts);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GSR_H_INCLUDED */
