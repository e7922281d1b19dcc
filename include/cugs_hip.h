/* cugs_hip.h — C ABI of libcugs_hip.so: the MI355X-native differentiable Gaussian-splat
 * rasterizer + fused Adam, as a drop-in for the hot path of
 * Artemarius/cuda-gaussian-splatting (namespace cugs).
 *
 * Conventions:
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless its name
 *     ends in _host; arrays use the reference's layouts and dtypes (fp32 / int32, row-major);
 *   - the callee allocates nothing: outputs and scratch are caller-owned; outputs the
 *     reference zero-fills (torch::zeros) are fully written by the kernels;
 *   - every function is stream-ordered on `stream` (a hipStream_t passed as void*; NULL =
 *     the null stream), re-entrant, and keeps no global state;
 *   - return value: 0 on success, a positive hipError_t from the HIP runtime, or a negative
 *     CUGS_E* argument error.  Nothing throws or aborts across this boundary; the adapter
 *     turns non-zero into std::runtime_error the way CUDA_CHECK does (utils/cuda_utils.cuh:12-20);
 *   - only launch errors are reported (no device sync), as in the reference
 *     (projection.cu:267); cugs_sort_count_pairs is the one blocking call (sorting.cu:146).
 *
 * Citations are file:line in the reference's src/ tree.
 */
#ifndef CUGS_HIP_H
#define CUGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUGS_TILE 16                 /* rasterizer/sorting.hpp:16 kTileSize */
#define CUGS_PACKED_STRIDE 12        /* floats per packed projected-Gaussian record */
#define CUGS_GRAD_STRIDE 16          /* floats per packed 2-D gradient accumulator row */

#define CUGS_EINVAL (-1)             /* bad size / degree / null pointer */
#define CUGS_EALIGN (-2)             /* a buffer that must be 16-byte aligned is not */
#define CUGS_EOVERFLOW (-3)          /* pair count does not fit int32 (the reference's index type) */
#define CUGS_EWORKSPACE (-4)         /* workspace too small for (n, total_pairs) */

/* POD camera: what the adapter derives from cugs::CameraInfo (core/types.hpp:78-109).
 * view = row-major 4x4 world-to-camera, the float[16] built at projection.cu:228-233;
 * cam_center = -R^T t (types.hpp:98-100), the 3 floats uploaded at projection.cu:273-275. */
typedef struct cugs_camera {
    float view[16];
    float fx, fy, cx, cy;
    int32_t width, height;
    float cam_center[3];
    float reserved;
} cugs_camera;

const char* cugs_version(void);
/* Message for a return code of this library (hipGetErrorString for positive codes). */
const char* cugs_error_string(int code);

/* ---- a3+a4: project_gaussians (projection.cu:195-289) -------------------------------
 * One launch: k_project_gaussians (projection.cu:55-189) + view directions
 * (projection.cu:273-280) + k_evaluate_sh (core/sh.cu:19-79) + clamp_min(0) (projection.cu:284).
 * positions [n,3], rotations [n,4] (wxyz), scales [n,3] (log), opacities [n] (logit),
 * sh_coeffs [n,3,num_coeffs]; active_degree in 0..3 with (active_degree+1)^2 <= num_coeffs.
 * Outputs: means_2d [n,2], depths [n], cov_2d_inv [n,3], radii [n] i32, tiles_touched [n] i32,
 * opacities_act [n], rgb [n,3] (clamped).  `packed` ([n,CUGS_PACKED_STRIDE] floats, 16-byte
 * aligned) is optional scratch consumed by cugs_rasterize_*; pass NULL to skip it.
 * `colour_gate` ([n] bytes, optional): bit ch = the SH backward's ReLU gate of channel ch, i.e. the sign test of
 * the colour AS THE BACKWARD RECOMPUTES IT (sh_backward.cu:92-99), made here while the coefficients are on
 * chip; cugs_project_backward takes it instead of re-reading them.  rgb > 0 is not that test: forward (sh.cu:44-77)
 * and backward round differently, and within an ulp of zero they disagree. */
int cugs_project_forward(int64_t n, int num_coeffs, int active_degree,
                         const float* positions, const float* rotations, const float* scales,
                         const float* opacities, const float* sh_coeffs,
                         const cugs_camera* camera_host, float scale_modifier,
                         float* means_2d, float* depths, float* cov_2d_inv, int32_t* radii,
                         int32_t* tiles_touched, float* opacities_act, float* rgb,
                         float* packed, uint8_t* colour_gate, void* stream);

/* cugs_project_forward that ALSO leaves the sort's per-Gaussian inputs - the depth key and the tile rectangle
 * sort_gaussians derives from depths / means_2d / radii / tiles_touched first thing (sorting.cu:37-60, :115-131) -
 * in `sort_workspace` (the N-level buffer, cugs_sort_workspace_bytes(n)), while they are in registers.  Not in the
 * reference, whose render() (rasterizer.cpp:58-75) hands the arrays from one stage to the next; this is what a
 * render() built on this library calls, followed by cugs_sort_pairs_predicted_keyed on the same stream with the same
 * workspace and camera size.  All outputs of cugs_project_forward are written as well, bit for bit.
 * CONTRACT: a keyed projection must be consumed by a NARROW sort of the same workspace (cugs_sort_pairs_predicted_keyed
 * / _keyed_ordered; cugs_sort_count_pairs and cugs_sort_pairs_predicted consume it too).  A view with a pair-emitting
 * splat outside the narrow depth range raises the workspace's range flag here, and only a narrow sort reads and
 * re-arms it: the *_wide entry points rebuild their keys from the arrays and neither read nor clear it.  Followed by a
 * *_wide sort instead, the flag stays up and the NEXT narrow sort of that workspace reports -1 for a view that is in
 * range (results stay correct - the caller re-sorts on the general route - but a host that keeps a sticky "wide" bit
 * then spends another hold on the slow route).  A host that knows its next sort is a *_wide one calls
 * cugs_project_forward instead (render() does: key the sort iff the stream is not in its wide-depth hold). */
int cugs_project_forward_keyed(int64_t n, int num_coeffs, int active_degree,
                               const float* positions, const float* rotations, const float* scales,
                               const float* opacities, const float* sh_coeffs,
                               const cugs_camera* camera_host, float scale_modifier,
                               float* means_2d, float* depths, float* cov_2d_inv, int32_t* radii,
                               int32_t* tiles_touched, float* opacities_act, float* rgb,
                               float* packed, uint8_t* colour_gate, void* sort_workspace,
                               size_t sort_workspace_bytes, void* stream);

/* ---- a4: evaluate_sh_cuda (core/sh.cu:81-123), output NOT clamped ------------------- */
int cugs_evaluate_sh(int degree, int64_t n, int num_coeffs, const float* sh_coeffs,
                     const float* directions, float* out_rgb, void* stream);

/* ---- a9: evaluate_sh_backward_cuda (core/sh_backward.cu:114-156) -------------------- */
int cugs_evaluate_sh_backward(int degree, int64_t n, int num_coeffs, const float* sh_coeffs,
                              const float* directions, const float* dL_dcolor,
                              float* dL_dsh, void* stream);

/* The projection in TWO launches, for a caller that overlaps the colour half with the sort (render() does: the sort
 * needs depths / means / radii / tile counts only, while 81 % of the projection's reads - the SH rows - feed nothing
 * before the forward blend).  Same device functions as cugs_project_forward: every output bit-identical.
 *   cugs_project_forward_geometry  k_project_gaussians' half (projection.cu:55-189): 44 B/Gaussian in; means_2d, depths,
 *                                  cov_2d_inv, radii, tiles_touched, opacities_act, words 0..7 of each packed record
 *                                  and - when sort_workspace is given - the sort's keys, exactly as
 *                                  cugs_project_forward_keyed leaves them.  sort_workspace may be NULL.
 *   cugs_project_forward_colour    directions + k_evaluate_sh + clamp (projection.cu:273-284): rgb, colour_gate (may be
 *                                  NULL) and words 8..11 of each packed record (packed may be NULL).
 * The two may run concurrently on different streams (they write disjoint bytes); the blend kernels need both. */
int cugs_project_forward_geometry(int64_t n, const float* positions, const float* rotations, const float* scales,
                                  const float* opacities, const cugs_camera* camera_host, float scale_modifier,
                                  float* means_2d, float* depths, float* cov_2d_inv, int32_t* radii,
                                  int32_t* tiles_touched, float* opacities_act, float* packed, void* sort_workspace,
                                  size_t sort_workspace_bytes, void* stream);
int cugs_project_forward_colour(int64_t n, int num_coeffs, int active_degree, const float* positions,
                                const float* sh_coeffs, const cugs_camera* camera_host, float* rgb, float* packed,
                                uint8_t* colour_gate, void* stream);

/* Fills `packed` from the reference-layout projection outputs, for callers that did not get
 * it from cugs_project_forward (e.g. tests that drive rasterize_forward directly). */
int cugs_pack_projected(int64_t n, const float* means_2d, const float* cov_2d_inv,
                        const float* rgb, const float* opacities_act, float* packed,
                        void* stream);

/* ---- a5: sort_gaussians (sorting.cu:115-227) ----------------------------------------
 * Replaces the cumsum + .item() (sorting.cu:145-146), k_fill_sort_pairs (:30-72),
 * cub::DeviceRadixSort::SortPairs (:191-210; contract: ascending, stable, full 64-bit key)
 * and k_compute_tile_ranges (:82-109).  The two workspace queries replace CUB's two-call
 * temp-storage idiom (:191-198): `workspace` (N-level, cugs_sort_workspace_bytes(n)) carries
 * state from cugs_sort_count_pairs to cugs_sort_pairs and must be the same buffer in both calls,
 * with the same per-Gaussian inputs; `pair_workspace` (cugs_sort_pair_workspace_bytes(P)) can
 * only be sized after the count.  Size of the N-level buffer: ~59 bytes per Gaussian + 0.2 MB, and - up to 2 M
 * Gaussians - 40 KB per 4096 Gaussians more for the table of the keyed route's pair binning (69 MB in all at 1 M).
 * The first 256 bytes of the N-level buffer are control words that carry over from one launch to the next (the range
 * flag above among them): they must be ZERO when a newly allocated buffer is first used - garbage there reads as "a
 * depth outside the narrow range" (a spurious -1 / a spurious repeat on the general route).  The library re-arms them
 * itself from then on; the rest of the buffer, and the pair-level buffer, need no initialisation. */
size_t cugs_sort_workspace_bytes(int64_t n);
size_t cugs_sort_pair_workspace_bytes(int64_t total_pairs);

/* total_pairs = sum(tiles_touched).  BLOCKS until the value is on the host (the reference's one
 * forced sync) - after having queued all the work that does not depend on it (depth ordering of
 * the Gaussians), so the device is busy while the host waits. */
int cugs_sort_count_pairs(int64_t n, const float* means_2d, const float* depths,
                          const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                          void* workspace, size_t workspace_bytes, int64_t* total_pairs_host,
                          void* stream);

/* keys_sorted [P] u64 (tile_id<<32 | depth bits; may be NULL), values_sorted [P] i32,
 * tile_ranges [tiles,2] i32 ({0,0} for untouched tiles, sorting.cu:216). */
int cugs_sort_pairs(int64_t n, int64_t total_pairs, const float* means_2d, const float* depths,
                    const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                    void* workspace, size_t workspace_bytes, void* pair_workspace,
                    size_t pair_workspace_bytes, uint64_t* keys_sorted, int32_t* values_sorted,
                    int32_t* tile_ranges, void* stream);

/* The whole sort (cugs_sort_count_pairs + cugs_sort_pairs) WITHOUT the host round trip: the caller predicts
 * the pair count (`capacity`: e.g. the previous frame's count plus a margin) and sizes pair_workspace
 * (cugs_sort_pair_workspace_bytes(capacity)), keys_sorted and values_sorted for it; the pair-level kernels take
 * the live count from device memory.  The total is copied to *total_pairs_host asynchronously (pinned host
 * memory recommended); once the stream has completed, the outputs are valid iff
 * 0 <= *total_pairs_host <= capacity.  Otherwise: a count above the capacity -> call cugs_sort_pairs with the now
 * known count (the N-level workspace still holds the depth order); -1 -> some splat's depth lies outside
 * [0.2, ~13 000), the range the three-pass depth ordering of this entry point covers: call cugs_sort_count_pairs
 * (which then takes the general route) and cugs_sort_pairs.  Never blocks. */
int cugs_sort_pairs_predicted(int64_t n, int64_t capacity, const float* means_2d, const float* depths,
                              const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                              void* workspace, size_t workspace_bytes, void* pair_workspace,
                              size_t pair_workspace_bytes, uint64_t* keys_sorted, int32_t* values_sorted,
                              int32_t* tile_ranges, int64_t* total_pairs_host, void* stream);

/* cugs_sort_pairs_predicted on a `workspace` that cugs_project_forward_keyed filled for these arrays (same n, same
 * width x height) on this stream since the last sort that used it: the per-Gaussian key / rectangle launch is
 * skipped (one kernel and 40 MB per million Gaussians).  Outputs and validity rule are those of
 * cugs_sort_pairs_predicted.  BOTH fallbacks (a count above the capacity, or -1) are cugs_sort_count_pairs followed by
 * cugs_sort_pairs, which rebuild everything from the arrays: on images of up to 10 240 tiles and up to 2 M Gaussians this
 * entry point bins the pairs straight into their tiles' lists (no pair-level radix passes, csrc/sort_bin.h k_bin_*) and
 * does not leave in `workspace` what cugs_sort_pairs alone continues from.  On either miss every tile range is {0,0}:
 * a blend queued behind the sort before the host has looked at the count then does nothing (the index buffer is
 * unwritten).  pair_workspace is not touched on that route (it may still be sized as for cugs_sort_pairs_predicted). */
int cugs_sort_pairs_predicted_keyed(int64_t n, int64_t capacity, const float* means_2d, const float* depths,
                                    const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                                    void* workspace, size_t workspace_bytes, void* pair_workspace,
                                    size_t pair_workspace_bytes, uint64_t* keys_sorted, int32_t* values_sorted,
                                    int32_t* tile_ranges, int64_t* total_pairs_host, void* stream);

/* cugs_sort_pairs_predicted_keyed that also leaves in tile_order[tiles][4] (16-byte aligned) the tiles ordered by the
 * length of their lists, longest first (to 6 %; empty tiles last), as records {tile, first pair, one past the last pair,
 * 0} - what the blends hand their workgroups out by when given as `tile_order` in their options (tile and
 * range in one load).  Not in the reference; what a render() built on this library calls: on views whose splats
 * cluster (every real capture) the blend kernels run a quarter shorter, on uniform ones the same.
 * Whenever the call leaves valid tile ranges it leaves a valid order (every tile once, with its range), misses included. */
int cugs_sort_pairs_predicted_keyed_ordered(int64_t n, int64_t capacity, const float* means_2d, const float* depths,
                                            const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                                            void* workspace, size_t workspace_bytes, void* pair_workspace,
                                            size_t pair_workspace_bytes, uint64_t* keys_sorted, int32_t* values_sorted,
                                            int32_t* tile_ranges, int64_t* total_pairs_host, uint32_t* tile_order,
                                            void* stream);

/* The same order from any valid tile_ranges (e.g. after cugs_sort_pairs): one small launch. */
int cugs_tile_order(int width, int height, const int32_t* tile_ranges, uint32_t* tile_order, void* stream);

/* The same two entry points on the GENERAL depth route (four 8-bit passes over the raw depth bits: any positive
 * depth), for a caller that already knows the view leaves the three-pass range - an earlier sort of it reported -1.
 * cugs_sort_count_pairs tries the three-pass route first and repeats on the general one; a host that renders such a
 * view every frame (a scene in millimetres, a far backdrop) would pay that twice per frame, and
 * cugs_sort_pairs_predicted would report -1 every time.  Outputs and every other rule are unchanged; the predicted
 * variant never reports -1.  The host keeps the "this view is wide" bit (render() does: sticky per stream, re-probed
 * every 256 sorts). */
int cugs_sort_count_pairs_wide(int64_t n, const float* means_2d, const float* depths,
                               const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                               void* workspace, size_t workspace_bytes, int64_t* total_pairs_host,
                               void* stream);
int cugs_sort_pairs_predicted_wide(int64_t n, int64_t capacity, const float* means_2d, const float* depths,
                                   const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                                   void* workspace, size_t workspace_bytes, void* pair_workspace,
                                   size_t pair_workspace_bytes, uint64_t* keys_sorted, int32_t* values_sorted,
                                   int32_t* tile_ranges, int64_t* total_pairs_host, void* stream);

/* ---- a6: rasterize_forward (forward.cu:180-240, kernel :48-174) ---------------------
 * out_color [H,W,3], out_final_T [H,W], out_n_contrib [H,W] i32.  `packed` may be NULL
 * (records are then gathered from the four reference-layout arrays). */
int cugs_rasterize_forward(int width, int height, const float background_host[3],
                           const int32_t* tile_ranges, const int32_t* gaussian_indices,
                           const float* means_2d, const float* cov_2d_inv, const float* rgb,
                           const float* opacities_act, const float* packed,
                           float* out_color, float* out_final_T, int32_t* out_n_contrib,
                           void* stream);

/* What the forward blend can do beyond the reference (none of it is in the reference).  Every field may be NULL / 0. */
typedef struct cugs_blend_forward_opts {
    /* In passing, a zero-fill of `zero_buf` (zero_bytes: multiple of 16, buffer 16-byte aligned): the blend kernel is
     * bound by instruction issue and leaves HBM idle, so the [n, CUGS_GRAD_STRIDE] accumulator the backward needs is
     * cleared here for free instead of by a fill in front of the backward blend (then set
     * cugs_blend_backward_opts::prezeroed).  An empty image still clears it. */
    void* zero_buf;
    size_t zero_bytes;
    /* The workgroups take their tile AND its range from the records tile_order[0 .. tiles)[4], 16-byte aligned
     * (cugs_tile_order / cugs_sort_pairs_predicted_keyed_ordered; NULL: the spatial order and tile_ranges).  Any order
     * of the tiles is a correct one: the outputs do not depend on it, bit for bit; the records must agree with
     * tile_ranges. */
    const uint32_t* tile_order;
    /* The accumulated DEPTH MAP out_depth [H,W], written when either of the two is given:
     * out_depth[px] = sum_i z_i alpha_i T_i over the same contributors, in the same front-to-back order and with the
     * same decisions as the colour channels, z_i = depths[i] of cugs_project_forward (the camera-space t.z), bit for
     * bit; each step is fmaf(alpha_i T_i, z_i, acc) and the background does not enter.  The result equals, bit for bit,
     * the red channel of this blend with rgb := (z, z, z) and background 0.  color, final_T and n_contrib are those of
     * the blend without it, bit for bit.  The alpha (coverage) map is 1 - final_T; it needs no output.
     * depths [n] is then required whenever gaussian_indices is given; out_depth whenever the image is not empty. */
    const float* depths;
    float* out_depth;
} cugs_blend_forward_opts;

/* cugs_rasterize_forward with options (NULL: all off, i.e. cugs_rasterize_forward itself). */
int cugs_rasterize_forward_opts(int width, int height, const float background_host[3],
                                const int32_t* tile_ranges, const int32_t* gaussian_indices,
                                const float* means_2d, const float* cov_2d_inv, const float* rgb,
                                const float* opacities_act, const float* packed,
                                float* out_color, float* out_final_T, int32_t* out_n_contrib,
                                const cugs_blend_forward_opts* opts, void* stream);

/* ---- per-Gaussian contribution scores (not in the reference) ---------
 * The forward blend's walk without its colour: for every Gaussian g, statistics of its blend weight w = alpha * T over
 * the pixels of this view, with the forward's decisions and the forward's w, bit for bit.  They are ADDED to row g of
 * `scores`, a table [n,4] of 32-bit words, 16-byte aligned:
 *   word 0  float   sum of w                       (float atomic adds: the last bits depend on their order)
 *   word 1  float   largest w on any pixel         (exact: an unsigned atomic max on the bits, w >= 0)
 *   word 2  uint32  number of pixels with w > 0    (exact; wraps at 2^32)
 *   word 3  padding, never written
 * The table is never cleared by the call: zero it once, then score V views with V calls - the sums and counts add up,
 * the maximum is the maximum over the views.  A zeroed table is the identity of all three.
 * Inputs as for cugs_rasterize_forward (no colour is read: there is no rgb, and of `packed` only the first 32 bytes of
 * a record); tile_order as cugs_blend_forward_opts::tile_order (NULL: the spatial order).  gaussian_indices and the
 * per-Gaussian sources may be NULL when every tile range is empty.
 * CUGS_EINVAL for a negative size, a NULL `scores` with n > 0, gaussian_indices without a source (packed, or the three
 * arrays), a NULL tile_ranges when something would be launched; CUGS_EALIGN for packed, tile_order or scores not
 * 16-byte aligned; all before anything is queued.  n == 0 or an empty image: 0, nothing is launched.  Stream-ordered,
 * no host sync, no workspace. */
int cugs_blend_scores(int width, int height, const int32_t* tile_ranges, const int32_t* gaussian_indices,
                      const float* means_2d, const float* cov_2d_inv, const float* opacities_act,
                      const float* packed, const void* tile_order, int n, void* scores, void* stream);

/* ---- pixel maps lifted onto Gaussians (not in the reference) ----------
 * The weighted form of cugs_blend_scores: for every Gaussian g and channel c < channels (1..4),
 *   S[g,c] = sum over the pixels p of this view of w_g(p) * M_c(p),
 * with the forward's decisions and the forward's w = alpha * T, bit for bit.  Exactly one of the two maps is given:
 *   maps    [height,width,channels] float32, channel-last (the layout of the colour image); no alignment required
 *   labels  [height,width] int32: M_c(p) = 1 where labels[p] == label_base + c, else 0 - a label outside the window
 *           label_base .. label_base + channels - 1, negatives included, contributes nothing
 * The sums are ADDED (float atomic adds: the last bits depend on their order) to words 0..channels-1 of row g of
 * `table`, [n,4] float32, 16-byte aligned; words channels..3 are never written and the table is never cleared by the
 * call: a zeroed table is the identity, V views are V calls.  A pixel's map value reaches only the Gaussians with
 * w > 0 at that pixel - a NaN or Inf in the map goes to those rows and to no other.
 * Other inputs as for cugs_blend_scores.  CUGS_EINVAL for a negative size, channels outside 1..4, both or neither of
 * maps and labels when something would be launched, a NULL `table` with n > 0, gaussian_indices without a source, a
 * NULL tile_ranges when something would be launched; then CUGS_EALIGN for packed, tile_order or table not 16-byte
 * aligned; all before anything is queued.  n == 0 or an empty image: 0, nothing is launched.  Stream-ordered, no host
 * sync, no workspace. */
int cugs_blend_lift(int width, int height, const int32_t* tile_ranges, const int32_t* gaussian_indices,
                    const float* means_2d, const float* cov_2d_inv, const float* opacities_act,
                    const float* packed, const void* tile_order, int n,
                    const float* maps, const int32_t* labels, int channels, int label_base,
                    void* table, void* stream);

/* ---- a7: rasterize_backward (backward.cu:239-306, kernel :31-233) -------------------
 * grad_accum: [n,CUGS_GRAD_STRIDE] floats, 64-byte aligned scratch (zeroed by the callee).  A row is
 *   {dL_drgb[3], dL_dopacity_act, M1x, M1y, M2xx, M2xy, M2yy, dL_dz, abs_x, abs_y, 0...}
 * Word 9, dL_dz, is the gradient of the depth map with respect to the Gaussian's camera-space depth z (= depths[i]):
 * written on the depth route of cugs_blend_backward_opts only, 0 otherwise.  cugs_project_backward and its fused
 * variants add it to dL/dt.z (t = W p + t_cam), i.e. dL_dpositions += dL_dz * W[2,:], for radii > 0 - a zero word
 * changes no bit.
 * Words 10 and 11, abs_x and abs_y, are the ABSOLUTE 2-D mean gradients (AbsGrad): the per-pixel summands of
 * dL_dmeans_2d with fabs around each, abs_x = sum_p |dL/dpower (a dx + b dy)|, abs_y = sum_p |dL/dpower (b dx + c dy)|:
 * written with cugs_blend_backward_opts::abs_grad only, 0 otherwise.  They are final, and no other entry point reads
 * them but cugs_densify_accumulate_strided when it is pointed at them.
 * Words 4..8 are NOT gradients: they are the MOMENTS of dL/dpower over the pixel offsets d = pixel centre - mean,
 *   M1 = sum dL/dpower * (dx, dy),   M2 = sum dL/dpower * (dx^2, dx dy, dy^2),
 * from which the reference's two tensors follow by a per-Gaussian linear map with Sigma'^-1 = (a, b, c)
 * (backward.cu:200-213):   dL_dmeans_2d   = (a M1x + b M1y,  b M1x + c M1y)
 *                          dL_dcov_2d_inv = (-M2xx / 2,  -M2xy,  -M2yy / 2)      [Q3: [1] is the combined off-diagonal]
 * A C caller that wants gradients must either pass the four reference-layout outputs below (the callee applies the
 * map: dL_drgb [n,3], dL_dopacity_act [n], dL_dmeans_2d [n,2], dL_dcov_2d_inv [n,3]; all four or none), or hand the
 * rows to cugs_project_backward / cugs_project_backward_adam, which apply it themselves.  Words 0..3 are final. */
int cugs_rasterize_backward(int width, int height, const float background_host[3],
                            const int32_t* tile_ranges, const int32_t* gaussian_indices,
                            const float* means_2d, const float* cov_2d_inv, const float* rgb,
                            const float* opacities_act, const float* packed,
                            const float* dL_dcolor, const float* final_T,
                            const int32_t* n_contrib, int64_t n, float* grad_accum,
                            float* dL_drgb, float* dL_dopacity_act, float* dL_dmeans_2d,
                            float* dL_dcov_2d_inv, void* stream);

/* What the backward blend can do beyond the reference (none of it is in the reference).  Every field may be NULL / 0;
 * every output that no option touches is the same, up to the order of the atomic adds. */
typedef struct cugs_blend_backward_opts {
    /* != 0: grad_accum is ALREADY all zeros (cleared by cugs_blend_forward_opts::zero_buf since its last use): skips
     * the fill. */
    int prezeroed;
    /* != 0: also accumulates the ABSOLUTE 2-D mean gradients (AbsGS / `absgrad`) into words 10 and 11
     * of each row (layout above): for every contribution the backward blend evaluates, after the gates Q1-Q3 and the
     * clamp gate, the summand of dL_dmeans_2d with fabs around each component.  Both are >= 0, and 0 for a Gaussian
     * without a contribution.  On the depth route dL/dpower includes the depth and alpha map terms. */
    int abs_grad;
    /* The workgroups are handed out in the order of the records tile_order[0 .. tiles)[4], 16-byte aligned (NULL: the
     * spatial order).  The sums are the same up to the order of the atomic adds. */
    const uint32_t* tile_order;
    /* The DEPTH ROUTE, taken when any of these three is given: the gradients of the DEPTH MAP and the ALPHA MAP
     * (cugs_blend_forward_opts::out_depth).  dL_ddepth_map [H,W] and dL_dalpha [H,W] (alpha = 1 -
     * final_T) may each be NULL (zero).  Through the blend they add to dL_dopacity_act and to the moments (words 3..8);
     * through z they give dL_dz in word 9 of the row.  Colour gradients (words 0..2) are those of dL_dcolor alone.
     * depths [n] (those of the forward) is then required whenever gaussian_indices is given. */
    const float* depths;
    const float* dL_ddepth_map;
    const float* dL_dalpha;
    /* dL_ddepths [n] receives word 9: required exactly when the four reference-layout outputs are given on the depth
     * route, and never off it.  dL_dmeans_2d_abs [n,2] receives words 10 and 11: required exactly when the four are
     * given with abs_grad.  (CUGS_EINVAL otherwise, before anything is queued.) */
    float* dL_ddepths;
    float* dL_dmeans_2d_abs;
} cugs_blend_backward_opts;

/* cugs_rasterize_backward with options (NULL: all off, i.e. cugs_rasterize_backward itself). */
int cugs_rasterize_backward_opts(int width, int height, const float background_host[3],
                                 const int32_t* tile_ranges, const int32_t* gaussian_indices,
                                 const float* means_2d, const float* cov_2d_inv, const float* rgb,
                                 const float* opacities_act, const float* packed,
                                 const float* dL_dcolor, const float* final_T,
                                 const int32_t* n_contrib, int64_t n, float* grad_accum,
                                 float* dL_drgb, float* dL_dopacity_act, float* dL_dmeans_2d,
                                 float* dL_dcov_2d_inv, const cugs_blend_backward_opts* opts, void* stream);

/* ---- a8+a9: project_backward (projection_backward.cu:253-344, kernel :26-247) -------
 * One launch: k_project_backward + directions + k_evaluate_sh_backward.  The incoming 2-D
 * gradients come either from grad_accum (the MOMENT rows cugs_rasterize_backward leaves - layout there; the
 * kernel turns words 4..8 into dL_dmeans_2d / dL_dcov_2d_inv with the Sigma'^-1 it recomputes; preferred) or,
 * when grad_accum is NULL, from the four reference-layout arrays (which hold gradients, not moments).
 * colour_gate ([n] bytes from cugs_project_forward of the same model, camera and degree) supplies the ReLU gate (sh_backward.cu:92-100); when NULL the gate is
 * recomputed from sh_coeffs as the reference does - the same bits, 12 num_coeffs more bytes read per
 * Gaussian.  dL_dmeans_2d_out ([n,2], may be NULL)
 * receives BackwardOutput::dL_dmeans_2d (rasterizer.cpp:184) when grad_accum is used.
 * dL_dsh_coeffs may be NULL when dL_drgb_gated_out ([n,3]: dL_drgb with the ReLU gate applied) is
 * given instead: the data-parallel exchange (cugs_sh_backward_views) rebuilds the SH gradient from it.
 * Both NULL: geometry gradients only (the caller took the colour half with cugs_gated_colour_grad). */
int cugs_project_backward(int64_t n, int num_coeffs, int active_degree,
                          const float* positions, const float* rotations, const float* scales,
                          const float* opacities, const float* sh_coeffs, const int32_t* radii,
                          const uint8_t* colour_gate, const cugs_camera* camera_host,
                          float scale_modifier, const float* grad_accum,
                          const float* dL_dmeans_2d, const float* dL_dcov_2d_inv,
                          const float* dL_drgb, const float* dL_dopacity_act,
                          float* dL_dpositions, float* dL_drotations, float* dL_dscales,
                          float* dL_dopacities, float* dL_dsh_coeffs, float* dL_dmeans_2d_out,
                          float* dL_drgb_gated_out, void* stream);

/* ---- a8+a9+a11 in one launch (single-GPU training; trainer.cpp:228-242 calls render_backward, then
 * FusedAdam::apply_gradients + step): the projection/SH backward applies k_fused_adam's update
 * (fused_adam.cu:44-76) to each Gaussian's own parameters as soon as its gradients exist, so the five gradient
 * tensors (236 B/Gaussian at degree 3) are neither written nor read back by an optimizer launch.  Same
 * arithmetic in the same order as cugs_project_backward followed by cugs_fused_adam_groups: identical bits.
 * The parameters are updated IN PLACE; the 2-D gradients come from grad_accum, the ReLU gate from colour_gate
 * (both required).  adam_host: moments and learning rates in ParamGroup order {positions, sh_coeffs,
 * opacities, scales, rotations} (lr_schedule.hpp:23-29), bc1/bc2 from cugs_adam_bias_correction.  Not for
 * data-parallel training: there the gradients must be exchanged between backward and optimizer. */
typedef struct cugs_adam_fused {
    float* m[5];
    float* v[5];
    float lr[5];
    float beta1, beta2, eps, bc1, bc2;
} cugs_adam_fused;
int cugs_project_backward_adam(int64_t n, int num_coeffs, int active_degree, float* positions,
                               float* rotations, float* scales, float* opacities, float* sh_coeffs,
                               const int32_t* radii, const uint8_t* colour_gate,
                               const cugs_camera* camera_host, float scale_modifier,
                               const float* grad_accum, const cugs_adam_fused* adam_host,
                               float* dL_dmeans_2d_out, void* stream);

/* ---- data-parallel extension (no counterpart in the single-GPU reference) ----------
 * dL_dsh[i] = sum over views v of gated_rgb_views[v][i] (x) Y(normalize(positions[i] - centre_v)),
 * accumulated in view order.  gated_rgb_views: [num_views][n][3] (the all-gather of every rank's
 * dL_drgb_gated_out); cam_centers_host: [num_views][3]; num_views <= 16.  Equals the sum of the
 * per-view evaluate_sh_backward_cuda results (sh_backward.cu:29-112) without moving them. */
int cugs_sh_backward_views(int degree, int64_t n, int num_coeffs, const float* positions,
                           int num_views, const float* gated_rgb_views,
                           const float* cam_centers_host, float* dL_dsh, void* stream);

/* dL_drgb_gated_out[i][ch] = grad_accum[i][ch] * (bit ch of colour_gate[i]) - the [n,3] tensor
 * cugs_project_backward writes to its dL_drgb_gated_out, made from the backward blend's accumulator alone
 * (sh_backward.cu:92-100 applied to the blend's dL_drgb): the data-parallel exchange starts the all-gather of
 * these 12 B/Gaussian before the projection backward runs and lets it travel underneath. */
int cugs_gated_colour_grad(int64_t n, const float* grad_accum, const uint8_t* colour_gate,
                           float* dL_drgb_gated_out, void* stream);

/* ---- a11: FusedAdam (optimizer/fused_adam.cu:44-76,140-219) -------------------------
 * bc1 = 1/(1-beta1^t), bc2 = 1/(1-beta2^t) computed in double on the host, then float
 * (fused_adam.cu:145-148,161-162). */
void cugs_adam_bias_correction(float beta1, float beta2, int step, float* bc1_host,
                               float* bc2_host);

/* One parameter tensor (k_fused_adam, fused_adam.cu:44-76): in-place on param, m, v. */
int cugs_fused_adam(float* param, const float* grad, float* m, float* v, int64_t n, float lr,
                    float beta1, float beta2, float eps, float bc1, float bc2, void* stream);

typedef struct cugs_adam_group {
    float* param;
    const float* grad;     /* NULL: group skipped (fused_adam.cu:156 "if (!grads_[i].defined())") */
    float* m;
    float* v;
    int64_t n;
    float lr;
    float reserved;
} cugs_adam_group;

/* All parameter groups in ONE launch (the reference launches one kernel per group,
 * fused_adam.cu:155-163).  ngroups <= 8. */
int cugs_fused_adam_groups(const cugs_adam_group* groups_host, int ngroups, float beta1,
                           float beta2, float eps, float bc1, float bc2, void* stream);

/* ---- sparse Adam (not in the reference): step only the rows a view sees -------------------------
 * cugs_fused_adam_groups_rows: cugs_fused_adam_groups restricted to the rows with radii[row] > 0 (radii: DEVICE int32
 * [n_rows], cugs_project_forward's, of the view just rendered; a visible row whose gradient is zero is still stepped).
 * Group k holds n_rows rows of row_elems_host[k] floats (3, 3 num_coeffs, 1, 3, 4 for the five model tensors).
 *   visible row:    exactly cugs_fused_adam_groups' update - the same arithmetic in the same order, with the bc1 / bc2
 *                   given (the optimizer's GLOBAL step count; Inria's sparse_adam and gsplat's SelectiveAdam apply no
 *                   bias correction at all), so all rows visible = cugs_fused_adam_groups, bit for bit;
 *   invisible row:  param, m and v keep their bits; nothing of the row is read or written, except that a 16-byte piece
 *                   shared with a visible row is loaded and stored whole with the invisible elements unchanged.
 * Hence for any mask: result = where(visible row, cugs_fused_adam_groups' result, value before), bit for bit.
 * One launch; a group with grad == NULL is skipped.  CUGS_EINVAL: ngroups > 8, a group with row_elems <= 0 or
 * n != row_elems * n_rows, radii == NULL with n_rows > 0; n_rows == 0 returns 0 and queues nothing.
 * The fused step under the same rule: cugs_projection_opts.sparse (cugs_project_backward_adam_opts, further down). */
int cugs_fused_adam_groups_rows(const cugs_adam_group* groups_host, int ngroups, const int32_t* row_elems_host,
                                const int32_t* radii, int64_t n_rows, float beta1, float beta2, float eps,
                                float bc1, float bc2, void* stream);

/* ---- N1: combined_loss + dL/dcolor (training/loss.cpp:88-140, trainer.cpp:214-217) ----
 * L = (1-lambda) mean|x-y| + lambda (1 - mean SSIM), SSIM with a window_size x window_size sigma-1.5
 * Gaussian window (odd, 3..15; the reference default is 11), zero padding, C1 = 1e-4, C2 = 9e-4.
 * rendered, target: [H,W,3].  loss_out: DEVICE float[4] = {loss, L1, mean SSIM, 1 - mean SSIM} (no host
 * sync).  ssim_map ([H,W], mean over channels = ssim(), loss.cpp:93) and dL_dcolor ([H,W,3] = d loss /
 * d rendered, what autograd returns at trainer.cpp:217) are optional.  workspace: cugs_loss_workspace_bytes. */
size_t cugs_loss_workspace_bytes(int width, int height);
int cugs_combined_loss(int width, int height, const float* rendered, const float* target, float lambda,
                       int window_size, void* workspace, size_t workspace_bytes, float* loss_out,
                       float* ssim_map, float* dL_dcolor, void* stream);

/* ---- Per-view exposure compensation and pixel masks in the fused loss (not in the reference) ----
 * The same loss of x'(p) = m(p) (A c(p) + b) against y'(p) = m(p) y(p): c = rendered, y = target, E = [A | b] a
 * row-major 3x4 matrix, m a per-pixel weight.  Both means stay over all 3 H W elements whatever the mask, and the SSIM
 * window's zero padding applies to x' and y' (a pixel outside the image is 0, not b).  With g = dL/dx':
 *   dL_dcolor(p) = m(p) A^T g(p),   dL_dexposure[4 i + j] = sum_p m(p) g_i(p) c_j(p)  (j = 3: sum_p m(p) g_i(p)),
 * the twelve sums in fp64 in a fixed order (per-tile partials, then one workgroup): the same bits from run to run, no
 * float atomics, no host sync.  No gradient flows to the mask or the target.  ssim_map is the map of (x', y').
 * Every field may be NULL; opts == NULL or all NULL runs the kernels of cugs_combined_loss and gives its bits.
 * CUGS_EINVAL for dL_dexposure without exposure or without dL_dcolor; otherwise the checks of cugs_combined_loss
 * against cugs_loss_opts_workspace_bytes (CUGS_EWORKSPACE for a short workspace), all before anything is queued. */
typedef struct cugs_loss_opts {
    const float* exposure;      /* DEVICE float[12], row-major [A | b]; NULL: identity */
    const float* mask;          /* DEVICE float[H*W]; NULL: all ones */
    float*       dL_dexposure;  /* DEVICE float[12]; needs exposure and dL_dcolor */
    float*       corrected;     /* DEVICE float[H*W*3], x' */
} cugs_loss_opts;
size_t cugs_loss_opts_workspace_bytes(int width, int height);
int cugs_combined_loss_opts(int width, int height, const float* rendered, const float* target, float lambda,
                            int window_size, const cugs_loss_opts* opts, void* workspace, size_t workspace_bytes,
                            float* loss_out, float* ssim_map, float* dL_dcolor, void* stream);

/* ---- Depth supervision: fused expected-depth L1 loss with a scale/shift fit (not in the reference) ----
 * depth_map D, alpha A (cugs_blend_forward_opts::out_depth and the alpha of the blend), target t: DEVICE float[H*W].
 * x = D / A in depth space, A / D in inverse space (against an inverse-depth or disparity target).  A pixel is VALID iff
 * A > min_alpha, weight > 0, 0 < t < +inf (a NaN target is invalid) and, in inverse space, D > 0.
 * The target is aligned as t' = s t + b (two roundings), (s, b) = (1, 0), `scale_shift`, or - fit - the weighted least
 * squares min sum_valid w (s t + b - x)^2, solved on the device in fp64 from the sums w, w t, w x, w t^2, w t x (terms
 * formed in double); accepted with >= 2 valid pixels and Sw Stt - St^2 > 1e-12 Sw Stt, else (1, 0) and fit_ok = 0.
 * (s, b) is a CONSTANT in the gradient (a fit under no_grad): no term for ds/dx or db/dx.
 *   r = x - t',  gx = (w sgn(r)) * (1.0f / (float)(H W)),  loss = (float)(sum_valid (double)(w |r|) / (H W)):
 *   the mean is over ALL pixels whatever the mask - an invalid pixel counts as a perfect one.
 *   depth space:   dL/dD = gx / A,          dL/dA = -((gx x) / A)
 *   inverse space: dL/dD = -((gx x) / D),   dL/dA = gx / D
 * At an invalid pixel both gradients and `expected` are 0; nothing there is NaN or inf.
 * loss_out: DEVICE float[8] = {loss, s, b, sum of valid w, valid count, fit_ok, 0, 0} (the count is a float, exact
 * below 2^24 pixels; fit_ok is 1 when nothing was fitted).  dL_ddepth_map and dL_dalpha ([H*W]) may each be NULL.
 * Two launches without a fit, four with one; fp64 partials per workgroup reduced in a fixed order: the same bits from
 * run to run, no float atomics, no host sync, no allocation.  16-byte accesses where every map is 16-byte aligned.
 * All checks before anything is queued, in this order: CUGS_EINVAL for a non-positive size, a NULL depth_map, alpha,
 * target, opts, workspace or loss_out, a min_alpha that is not positive and finite, fit together with scale_shift;
 * CUGS_EWORKSPACE for a workspace shorter than cugs_depth_loss_workspace_bytes (0 for a negative size, a multiple of
 * 256); CUGS_EOVERFLOW for H W > 2^31 - 1. */
typedef struct cugs_depth_loss_opts {
    const float* weight;       /* DEVICE float[H*W]; NULL: all ones */
    const float* scale_shift;  /* DEVICE float[2] = (s, b); NULL: (1, 0) unless fit */
    int          fit;          /* 1: fit (s, b) on the device; CUGS_EINVAL together with scale_shift */
    int          inverse;      /* 0: D/A against depth; 1: A/D against inverse depth */
    float        min_alpha;    /* > 0 and finite, else CUGS_EINVAL */
    float*       expected;     /* optional DEVICE float[H*W]: x, 0 where invalid */
} cugs_depth_loss_opts;
size_t cugs_depth_loss_workspace_bytes(int width, int height);
int cugs_depth_loss(int width, int height, const float* depth_map, const float* alpha, const float* target,
                    const cugs_depth_loss_opts* opts, void* workspace, size_t workspace_bytes,
                    float* loss_out /* DEVICE float[8] */, float* dL_ddepth_map, float* dL_dalpha, void* stream);

/* ---- Normal supervision from the rendered depth: fused depth-to-normal loss (not in the reference) ----
 * depth_map D, alpha A: DEVICE float[H*W] as above; target t: DEVICE float[3*H*W] (planes x, y, z: a normal prior in
 * camera axes x right, y down, z forward, of any length), or NULL for the normal map alone.  Pinhole fx, fy, cx, cy;
 * pixel centres at u + 0.5, v + 0.5.  The fp32 operation order (every step one correctly rounded operation):
 *   depth-valid: A > min_alpha;  d = D / A there, 0 elsewhere
 *   ax(u) = (((float)u + 0.5f) - cx) / fx,  ay(v) likewise;  P = (ax d, ay d, d)
 *   Px = P(u+1, v) - P(u-1, v),  Py = P(u, v+1) - P(u, v-1),  n = Py x Px (towards the camera: n_z < 0 on a visible
 *   surface, the 2DGS depth_to_normal),  nn = (n_x^2 + n_y^2) + n_z^2,  rl = 1.0f / sqrtf(nn),  n^ = n rl
 *   normal-valid: not on the image border, the pixel and its four neighbours depth-valid, 0 < nn < inf; n^ = 0 elsewhere
 *   tt = (t_x^2 + t_y^2) + t_z^2,  t^ = t (1.0f / sqrtf(tt))
 *   loss-valid: normal-valid, weight > 0, 0 < tt < inf (a zero or non-finite prior vector marks "no data")
 *   l = w (cos_weight (1 - ((n^_x t^_x + n^_y t^_y) + n^_z t^_z)) + l1_weight ((|e_x| + |e_y|) + |e_z|)),  e = n^ - t^
 *   loss = (float)(sum_loss-valid (double)l / (H W)): the mean is over ALL pixels, as in cugs_depth_loss.
 * Backward, the masks held constant:  b = (w (1.0f / (float)(H W))) (l1_weight sgn(e) - cos_weight t^),
 *   c = (b - n^ ((n^_x b_x + n^_y b_y) + n^_z b_z)) rl,  gPx = c x Py,  gPy = Px x c  (0 where not loss-valid), then the
 *   GATHER  gP(u,v) = ((gPx(u-1,v) - gPx(u+1,v)) + gPy(u,v-1)) - gPy(u,v+1),  g_d = (gP_x ax + gP_y ay) + gP_z,
 *   dL/dD = g_d / A,  dL/dA = -((g_d d) / A);  both +0 where none of the four neighbours is loss-valid.
 * loss_out: DEVICE float[8] = {loss, sum of loss-valid w, loss-valid count, 0, 0, 0, 0, 0}; all 0 without a target.
 * dL_ddepth_map and dL_dalpha ([H*W]) may each be NULL.  Two launches (the fused forward + backward over 64x16 tiles, one
 * workgroup of fixed-order fp64 sums); no atomics, no host sync, no allocation, the same bits from run to run, and a
 * pixel's result does not depend on the tiling.  4-byte accesses only: no alignment beyond float's is asked for.
 * All checks before anything is queued, in this order: CUGS_EINVAL for a non-positive size, a NULL depth_map, alpha,
 * opts, workspace or loss_out, a min_alpha that is not positive and finite, fx or fy not positive and finite, cx or cy
 * not finite, a loss weight that is negative or not finite, both loss weights 0 with a target, and without a target a
 * NULL normals_out or a non-NULL weight, dL_ddepth_map or dL_dalpha; CUGS_EWORKSPACE for a workspace shorter than
 * cugs_normal_loss_workspace_bytes (0 for a negative size, a multiple of 256: 24 bytes per tile); CUGS_EOVERFLOW for
 * H W > 2^31 - 1. */
typedef struct cugs_normal_loss_opts {
    const float* weight;       /* DEVICE float[H*W]; NULL: all ones */
    float*       normals_out;  /* optional DEVICE float[3*H*W]: n^, 0 where not normal-valid */
    float        cos_weight;   /* >= 0 and finite */
    float        l1_weight;    /* >= 0 and finite; not both 0 with a target */
    float        min_alpha;    /* > 0 and finite, else CUGS_EINVAL */
} cugs_normal_loss_opts;
size_t cugs_normal_loss_workspace_bytes(int width, int height);
int cugs_normal_loss(int width, int height, float fx, float fy, float cx, float cy, const float* depth_map,
                     const float* alpha, const float* target /* nullable */, const cugs_normal_loss_opts* opts,
                     void* workspace, size_t workspace_bytes, float* loss_out /* DEVICE float[8] */,
                     float* dL_ddepth_map, float* dL_dalpha, void* stream);

/* ---- Bilateral-grid colour correction: fused slice, backward and TV loss (not in the reference) ----
 * grid G: DEVICE float[12, L, GY, GX], coefficient k = 4 i + j = row i, column j of a 3x4 transform [A | b]; the identity
 * grid holds [I | 0] at every vertex; 2 <= L, GY, GX <= 64.  rendered c, corrected, dL_dcorrected g, dL_drendered:
 * DEVICE float[H, W, 3].  The fp32 operation order (every step one correctly rounded operation), for pixel (x, y):
 *   sx = (float)(GX-1) / (float)(W-1), 0 when W = 1 (sy likewise; formed once on the host)
 *   fx = (float)x * sx;  x0 = min((int)fx, GX-2);  tx = fx - (float)x0            (y likewise)
 *   luma = (0.299f r + 0.587f g) + 0.114f b;  zs = luma * (float)(L-1);  fz = min(max(zs, 0), (float)(L-1))
 *   z0 = min((int)fz, L-2);  tz = fz - (float)z0;  inside = 0 <= zs <= L-1
 *   lerp(a, b, t) = a + t * (b - a); per coefficient k, a.. = G[k] at level z0, b.. at z0+1 (rows y0, y0+1; columns x0, x0+1):
 *     p0 = lerp(lerp(a00, a01, tx), lerp(a10, a11, tx), ty);  p1 likewise from b..;  D_k = p1 - p0;  E_k = p0 + tz * D_k
 *   corrected_i = ((E[4i] r + E[4i+1] g) + E[4i+2] b) + E[4i+3]
 * i.e. trilinear weights wx wy wz, w = t or 1 - t, on the eight corners: grid_sample(bilinear, align_corners, border) at
 * (x / (W-1), y / (H-1), luma) followed by the affine apply.  Backward:
 *   q_i = ((D[4i] r + D[4i+1] g) + D[4i+2] b) + D[4i+3];  s = inside ? ((g_0 q_0 + g_1 q_1) + g_2 q_2) * (float)(L-1) : 0
 *   dL_drendered_j = ((E[j] g_0 + E[4+j] g_1) + E[8+j] g_2) + s * lw_j,  lw = (0.299f, 0.587f, 0.114f)
 *   dL_dgrid[k, z, y, x] = sum_p w(p; z, y, x) g_i(p) [c(p), 1]_j,  w = {1-ty, ty} {1-tx, tx} {1-tz at z0, tz at z0+1}
 * The term s lw is the gradient through the luminance guidance; it is 0 where the clamp is active.  The lerp form makes a
 * lattice that is constant over a pixel's corners exact, so the identity grid returns rendered, and dL_drendered = g, bit
 * for bit (a -0.0 input comes back +0.0).  dL_dgrid is WRITTEN, not accumulated: per-workgroup fp32 partials over the
 * xy-cells of the lattice (a fixed tree), combined per element in fp64 in a fixed order - no float atomics, no host sync,
 * no allocation, the same bits from run to run.  Either of dL_drendered, dL_dgrid may be NULL (both: nothing is queued).
 * cugs_bilagrid_workspace_bytes = round256(4 * 48 * L * (GX-1)(GY-1) * Q), Q = ceil(pixels of the largest xy-cell / 1024)
 * (the [cell][chunk][z][corner][12] partials; 0 for a bad size or lattice); needed only with dL_dgrid.
 * cugs_bilagrid_tv: tv = sum over the axes z, y, x of mean((G[.., i+1, ..] - G[.., i, ..])^2), each mean over the
 * 12 (n_axis - 1) (other two extents) differences of that axis; differences, squares and sums in fp64; tv_out (DEVICE
 * float[1]) gets the UNWEIGHTED tv, dL_dgrid gets weight * dtv/dG (accumulate != 0: that is added to what it holds, one
 * fp32 add per element - so it can follow cugs_bilagrid_slice_backward on the same buffer).  One launch, one workgroup.
 * Either output may be NULL, not both.
 * All checks before anything is queued, in this order.  slice / slice_backward: CUGS_EINVAL for a non-positive size, NULL
 * dims, an extent outside [2, 64], a NULL grid, rendered, corrected / dL_dcorrected, dL_dgrid without workspace;
 * CUGS_EWORKSPACE for dL_dgrid with a short workspace; CUGS_EOVERFLOW for H W > 2^31 - 1.  tv: CUGS_EINVAL for NULL dims,
 * an extent outside [2, 64], a NULL grid, or both outputs NULL. */
typedef struct cugs_bilagrid_dims {
    int32_t l, gy, gx;      /* vertices along luminance, y, x: each in [2, 64] */
} cugs_bilagrid_dims;
size_t cugs_bilagrid_workspace_bytes(int width, int height, const cugs_bilagrid_dims* dims);
int cugs_bilagrid_slice(int width, int height, const cugs_bilagrid_dims* dims, const float* grid, const float* rendered,
                        float* corrected, void* stream);
int cugs_bilagrid_slice_backward(int width, int height, const cugs_bilagrid_dims* dims, const float* grid,
                                 const float* rendered, const float* dL_dcorrected, void* workspace,
                                 size_t workspace_bytes, float* dL_drendered, float* dL_dgrid, void* stream);
int cugs_bilagrid_tv(const cugs_bilagrid_dims* dims, const float* grid, float weight, float* tv_out /* DEVICE float[1] */,
                     float* dL_dgrid, int accumulate, void* stream);

/* ---- Evaluation metrics of one view (training/metrics.cpp:21-46: compute_psnr, compute_ssim) ---------------
 * rendered: [H,W,3] float.  The target is EITHER target_f32 ([H,W,3] float) OR target_u8 ([H,W,3] uint8, a cached
 * view at the camera's size, expanded in registers as (float)b * (1.0f / 255.0f): the bits of cugs_image_to_float
 * at equal size followed by the float path); exactly one is non-null.
 * metrics_out: DEVICE float[4] = {MSE, mean SSIM, mean |x-y|, max |x-y|} (no host sync, no allocation; two
 * launches, no per-pixel output).  MSE = (float)(sum of (double)d*(double)d / (3 H W)), d = x - y in float; PSNR is
 * the host's 10 log10(1 / MSE) (metrics.cpp:27-34).  Mean SSIM and the L1 mean are, bit for bit, loss_out[2] and
 * loss_out[1] of cugs_combined_loss on the same float inputs and window (same per-pixel arithmetic, same
 * fixed-order fp64 reduction); window_size odd, 3..15, the reference's is 11.  A NaN input gives NaN results.
 * CUGS_EINVAL for a negative size, an even or out-of-range window, both or neither target, a null pointer or a
 * workspace shorter than cugs_eval_workspace_bytes with pixels to process; width * height == 0 queues nothing. */
size_t cugs_eval_workspace_bytes(int width, int height);
int cugs_eval_metrics(int width, int height, const float* rendered, const float* target_f32,
                      const uint8_t* target_u8, int window_size, void* workspace, size_t workspace_bytes,
                      float* metrics_out, void* stream);

/* ---- N2: adaptive density control (optimizer/densification.cpp) ------------------------------
 * cugs_densify_accumulate: DensificationController::accumulate_gradients (densification.cpp:59-88), one
 *   launch, no host sync: for radii > 0, grad_accum += ||dL_dmeans_2d||_2 and grad_count += 1; for every
 *   Gaussian max_radii_2d = max(max_radii_2d, radii).  All three accumulators are float [n].
 * cugs_densify_accumulate_strided: the same, bit for bit, reading Gaussian i's gradient at
 *   dL_dmeans_2d[i * row_stride_floats + {0, 1}] (row_stride_floats >= 2, CUGS_EINVAL otherwise; even and the base
 *   8-byte aligned, CUGS_EALIGN otherwise): pointed at word 10 of the rows cugs_blend_backward_opts::abs_grad leaves,
 *   with stride CUGS_GRAD_STRIDE, it accumulates the AbsGrad norm with no intermediate tensor.
 * cugs_densify_classify: compute_clone_mask / compute_split_mask / compute_keep_mask (:351-442) as one
 *   byte per Gaussian: bit 0 clone candidate, bit 1 split candidate, bit 2 keep.  The thresholds are the
 *   reference's float products (size = percent_dense * scene_extent, ws = 0.1f * scene_extent);
 *   apply_size_pruning = (opacity_reset_every > 0 && step > opacity_reset_every); max_screen_size <= 0
 *   disables the screen-size test.  avg_grad (nullable) receives grad_accum / max(grad_count, 1), the key
 *   of the reference's max_gaussians top-k (:127-134).
 * cugs_densify_plan: counts and orders the result of densify() (:116-325) for FINAL flags (bit 0 clone,
 *   bit 1 split, bit 2 keep; the caller has applied any budget).  counts_host = {kept originals, clones,
 *   splits, n_out = kept + clones + 2 * splits}; an original is kept iff bit 2 is set and bit 1 is not.
 *   Blocks on a 32-byte read-back (the reference's sum().item() calls, :118,179).
 * cugs_densify_apply: writes each array of the new model, n_out rows in the reference's final order
 *   [kept originals | clones | first children | second children], each group in ascending parent index.
 *   Modes: COPY (new rows copy the parent: sh, opacities, rotations), POSITIONS (children:
 *   parent + noise[which][parent] * exp(scale - log 1.6), :253-262; noise is [2, n, 3] standard normal
 *   supplied by the caller in place of the reference's torch::randn_like), SCALES (children: scale -
 *   log 1.6), STATE (optimizer moments: survivors keep theirs, new rows are zero - the reference rebuilds
 *   its optimizer instead, trainer.cpp:267-304).  `scales` is the OLD scales array [n, 3].
 */
enum { CUGS_DENSIFY_COPY = 0, CUGS_DENSIFY_POSITIONS = 1, CUGS_DENSIFY_SCALES = 2, CUGS_DENSIFY_STATE = 3 };
typedef struct cugs_densify_array {
    const float* src;     /* [n, row_floats] device */
    float* dst;           /* [n_out, row_floats] device */
    int32_t row_floats;
    int32_t mode;         /* CUGS_DENSIFY_* */
} cugs_densify_array;
int cugs_densify_accumulate(int64_t n, const float* dL_dmeans_2d, const int32_t* radii, float* grad_accum,
                            float* grad_count, float* max_radii_2d, void* stream);
int cugs_densify_accumulate_strided(int64_t n, const float* dL_dmeans_2d, int64_t row_stride_floats,
                                    const int32_t* radii, float* grad_accum, float* grad_count, float* max_radii_2d,
                                    void* stream);
int cugs_densify_classify(int64_t n, const float* grad_accum, const float* grad_count, const float* max_radii_2d,
                          const float* scales, const float* opacities, float grad_threshold, float size_threshold,
                          float opacity_threshold, int apply_size_pruning, float max_screen_size,
                          float ws_threshold, uint8_t* flags, float* avg_grad, void* stream);
size_t cugs_densify_workspace_bytes(int64_t n);
int cugs_densify_plan(int64_t n, const uint8_t* flags, void* workspace, size_t workspace_bytes,
                      int64_t counts_host[4], void* stream);
int cugs_densify_apply(int64_t n, int64_t n_out, const void* workspace, size_t workspace_bytes, const float* noise,
                       const float* scales, const cugs_densify_array* arrays_host, int num_arrays, void* stream);

/* ---- N3: Gaussian-model PLY records (utils/ply_io.cpp:98-196, 258-351) -------------------------
 * The vertex record of the reference's checkpoint format, assembled / taken apart on the device:
 *   x y z | nx ny nz (zero) | f_dc_0..2 | f_rest_0..3(C-1)-1 (f_rest_{(k-1)*3+ch} = sh[ch][k]) | opacity |
 *   scale_0..2 | rot_0..3                                         = 14 + 3C floats (62 at SH degree 3),
 * optionally followed by the Adam first and second moments in the same order without the normals (2 x (11 + 3C)
 * floats): what a resumable checkpoint needs and the reference does not store.
 * params / m / v: five device pointers each in ParamGroup order {positions, sh_coeffs, opacities, scales,
 * rotations}; m and v both NULL = no optimizer state.
 * cugs_ply_pack:   vertices [n, cugs_ply_vertex_floats(C, state)] <- the tensors.
 * cugs_ply_unpack: the tensors <- vertices [n, num_props] as read from a file whose properties may be in any
 *   order or include others: col_of[c] (device, 11 + 3C entries, x3 with state) is the file column of canonical
 *   model float c (the record order above without the normals; then m, then v), looked up by NAME on the host.
 */
int cugs_ply_vertex_floats(int num_coeffs, int with_state);
int cugs_ply_pack(int64_t n, int num_coeffs, const float* const params[5], const float* const m[5],
                  const float* const v[5], float* vertices, void* stream);
int cugs_ply_unpack(int64_t n, int num_coeffs, int num_props, const float* vertices, const int32_t* col_of,
                    float* const params[5], float* const m[5], float* const v[5], void* stream);

/* ---- N4: training target from a cached 8-bit view (data/image_io.cpp:35-39, 47-100) -------------
 * dst [dst_height, dst_width, 3] float <- src [src_height, src_width, 3] uint8 (device, decoded once by the
 * caller): value * (1/255), and - when the sizes differ - the reference's resize_image (pixel-centre bilinear,
 * clamped edges, same fp32 operation order), i.e. the tensor trainer.cpp:186-198 builds on the CPU and uploads
 * every iteration, bit for bit. */
int cugs_image_to_float(int src_width, int src_height, const uint8_t* src_rgb8, int dst_width, int dst_height,
                        float* dst, void* stream);

/* ---- N5: MCMC densification (optimizer/mcmc_densification.cpp) ---------------------------------
 * Random draws come from a counter-based Philox4x32-10: key (seed_lo, seed_hi), counter (index_lo, index_hi,
 * stream_id, step).  One call per index gives four words; u = ((x >> 8) + 1) * 2^-24 in (0, 1]; Box-Muller on
 * (u0, u1) and (u2, u3), the first three normals used.  Streams: NOISE (index = Gaussian), JITTER (index =
 * relocated row), SAMPLE (index = ordinal of the relocation; r64 = w1 << 32 | w0).  They replace randn_like /
 * multinomial (:60-138, :158), whose draws cannot be reproduced; the same (seed, step) gives the same bits on
 * every replica and every route.
 * cugs_mcmc_random_bits: out[4 j + w] = word w of the draw for index first_index + j (pins the generator).
 * cugs_mcmc_regularization: compute_regularization (:167-186) without autograd or a host sync:
 *   out_o[i] = base_o[i] + ((lambda_o / N) * (1 - y)) * y, y = sigmoid(opacities[i])      [N, 1]
 *   out_s[i] = base_s[i] + (lambda_s / (3N)) * exp(scales[i])                             [N, 3]
 *   base NULL = write the regulariser gradient alone; base == out adds in place; outs NULL = value only.
 *   value_out (device float, may be NULL) = lambda_o mean(y) + lambda_s mean(exp s), a fixed-order two-level
 *   reduction (double partials) through a small workspace (below).
 * cugs_mcmc_inject_noise: inject_noise (:144-161): positions += ((lr * exp(s)) * gate) * n,
 *   gate = sigmoid(-gate_k * (sigmoid(opa) - gate_t)); n = noise [N, 3] when given, else stream NOISE.
 * cugs_mcmc_relocate: relocate (:56-138) in place, N constant.  Dead = sigmoid(opa) < dead_threshold;
 *   M = min(num_dead, (int)(relocate_cap * (float)N)); the first M dead rows in index order are relocated
 *   (none when num_dead or num_alive is 0).  Sources are drawn with replacement over the alive rows weighted by
 *   w_i = rintf(y_i * 2^24) (uint64 inclusive scan cdf; x = mulhi64(r64, total); the first i with cdf[i] > x).
 *   Per relocated row: rotation and SH copied; pos = src_pos + (n * scene_extent) * 0.01f (stream JITTER);
 *   scale = src_scale - logf(10); opacity = logf(0.01f / 0.99f).  m / v (host arrays of five device pointers in
 *   ParamGroup order, both NULL = untouched, as the reference, trainer.cpp:265): the relocated rows' Adam moments
 *   are zeroed.  stats (device int32[2]) = {num_dead, num_relocated}; src_out (device int32 [N], may be NULL):
 *   source row of the j-th relocated row, j < num_relocated.  No host sync.  Workspace:
 *   cugs_mcmc_relocate_workspace_bytes(n).  cugs_mcmc_regularization needs cugs_mcmc_relocate_workspace_bytes(0)
 *   bytes (16 KB of partial sums) whatever n; a relocation workspace serves it too.
 * cugs_mcmc_fused: the same work fused into the optimizer step (cugs_projection_opts.mcmc, further down).
 */
#define CUGS_MCMC_STREAM_NOISE 0u
#define CUGS_MCMC_STREAM_JITTER 1u
#define CUGS_MCMC_STREAM_SAMPLE 2u
typedef struct cugs_mcmc_fused {
    float lambda_opacity;
    float lambda_scale;
    float noise_lr;
    float gate_k;
    float gate_t;
    uint32_t step;
    uint64_t seed;
    const float* noise;    /* [n, 3] explicit standard normals (device), or NULL: the generator */
} cugs_mcmc_fused;
int cugs_mcmc_random_bits(uint64_t seed, uint32_t stream_id, uint32_t step, uint64_t first_index, int64_t count,
                          uint32_t* out, void* stream);
int cugs_mcmc_regularization(int64_t n, const float* opacities, const float* scales, float lambda_opacity,
                             float lambda_scale, const float* base_dL_dopacities, const float* base_dL_dscales,
                             float* dL_dopacities, float* dL_dscales, float* value_out, void* workspace,
                             size_t workspace_bytes, void* stream);
int cugs_mcmc_inject_noise(int64_t n, float* positions, const float* scales, const float* opacities, float noise_lr,
                           float gate_k, float gate_t, const float* noise, uint64_t seed, uint32_t step, void* stream);
size_t cugs_mcmc_relocate_workspace_bytes(int64_t n);
int cugs_mcmc_relocate(int64_t n, int num_coeffs, float* positions, float* rotations, float* scales, float* opacities,
                       float* sh_coeffs, float dead_threshold, float relocate_cap, float scene_extent, uint64_t seed,
                       uint32_t step, float* const m[5], float* const v[5], void* workspace, size_t workspace_bytes,
                       int32_t* stats, int32_t* src_out, void* stream);

/* ---- the camera gradient's block (not in the reference): see cugs_projection_opts.pose ----
 * dL_dview: device float[16] in the layout of cugs_camera.view, row 3 written 0.  rows: optional device [n,12], each
 * Gaussian's dL/dW (row-major) then dL/dtvec; NULL in production.  workspace: cugs_pose_grad_workspace_bytes(n)
 * device bytes, 16-byte aligned. */
typedef struct cugs_pose_grad {
    float* dL_dview;
    float* rows;
    void* workspace;
    size_t workspace_bytes;
} cugs_pose_grad;
size_t cugs_pose_grad_workspace_bytes(int64_t n);

/* ---- the projection backward with options ----------------------------------------------------------------------
 * cugs_project_backward_opts / cugs_project_backward_adam_opts: cugs_project_backward / cugs_project_backward_adam
 * (further up; the same arguments, checks and results) with one block of options in front of `stream`.  opts == NULL or
 * an all-zero block: exactly those two, which are this call with NULL.  A non-NULL block pointer switches its option on.
 * In this order, before anything is queued:
 *   1. the request: CUGS_EINVAL for mcmc or sparse on cugs_project_backward_opts, and for mcmc together with sparse;
 *   2. the checks of the entry point without options;
 *   3. with pose: CUGS_EINVAL for a NULL dL_dview and, for n > 0, a NULL workspace, CUGS_EWORKSPACE for one that is
 *      too small, CUGS_EALIGN for a misaligned one;
 *   4. n == 0: nothing is queued but, with pose, the 16 zeros of dL_dview;
 *   5. with mcmc: CUGS_EOVERFLOW for 3 n > INT32_MAX. */
typedef struct cugs_projection_opts {
    /* Fused entry only.  The per-iteration MCMC work of N5 rides in the launch, bit for bit the sequence regulariser
     * (add) -> Adam step -> inject_noise: the regulariser gradient joins the opacity and scale gradients of every
     * Gaussian, and the noise (from the updated opacity and scales) the updated position. */
    const cugs_mcmc_fused* mcmc;
    /* Either entry.  Every output the call has without it, bit for bit, plus dL/dview, the gradient with respect to
     * cugs_camera.view: t = W p + tvec with W = view[0..2][0..2], tvec[r] = view[r*4+3].  Per live Gaussian with
     * radii > 0 and an invertible Sigma': dL/dtvec = dt (the gradient of its camera-space position, depth-map word
     * included) and dL/dW = dt (x) p + J^T K (K = dL/d(J W)); every other Gaussian adds 0.  The SH view direction is
     * held constant (as dL_dpositions holds it).  The workgroup partials are summed in fp64 in a fixed order by two
     * more launches on `stream` and rounded once: the same bits from run to run, no host sync. */
    const cugs_pose_grad* pose;
    /* Fused entry only, non-zero = on; not together with mcmc, whose regulariser and noise act on every Gaussian.
     * Sparse Adam (the block beside cugs_fused_adam_groups_rows above) with the `radii` the call is
     * given anyway: a Gaussian with radii <= 0 is not read (no gradient row, no geometry, none of its parameter and
     * moment words), dL_dmeans_2d_out gets (0, 0) for it and dL_dview nothing from it, as on the dense route; every
     * visible Gaussian is stepped exactly as the dense route steps it, bit for bit. */
    int sparse;
} cugs_projection_opts;
int cugs_project_backward_opts(int64_t n, int num_coeffs, int active_degree,
                               const float* positions, const float* rotations, const float* scales,
                               const float* opacities, const float* sh_coeffs, const int32_t* radii,
                               const uint8_t* colour_gate, const cugs_camera* camera_host,
                               float scale_modifier, const float* grad_accum,
                               const float* dL_dmeans_2d, const float* dL_dcov_2d_inv,
                               const float* dL_drgb, const float* dL_dopacity_act,
                               float* dL_dpositions, float* dL_drotations, float* dL_dscales,
                               float* dL_dopacities, float* dL_dsh_coeffs, float* dL_dmeans_2d_out,
                               float* dL_drgb_gated_out, const cugs_projection_opts* opts, void* stream);
int cugs_project_backward_adam_opts(int64_t n, int num_coeffs, int active_degree, float* positions,
                                    float* rotations, float* scales, float* opacities, float* sh_coeffs,
                                    const int32_t* radii, const uint8_t* colour_gate,
                                    const cugs_camera* camera_host, float scale_modifier,
                                    const float* grad_accum, const cugs_adam_fused* adam_host,
                                    float* dL_dmeans_2d_out, const cugs_projection_opts* opts, void* stream);

/* ---- init_gaussians_from_sparse (core/gaussian_init.cpp:25-152) on the device ----------------------------------
 * The reference turns a point cloud into a model on the CPU: positions copied, the DC coefficient from the colour
 * (:111-119), opacity logit of 0.1 (:125-126), identity rotations (:129-130) and isotropic scales log(max(m, 1e-7))
 * (:132-144), m_i = mean distance from point i to its k nearest OTHER points, by a brute-force search on one thread
 * (compute_knn_mean_distances, :25-68).  Here the search is exact on the device:
 *   d^2 = (dx*dx + dy*dy) + dz*dz, dx = p_j.x - p_i.x, one fp32 rounding per operation (:48-51); the point itself is
 *   excluded by index, so a duplicate is a neighbour at distance 0 (:54); k is clamped to n - 1 (:36);
 *   m_i = (sum of sqrt(d^2) over the k smallest d^2, added in ASCENDING order) / float(k) (:59-64, whose order
 *   nth_element leaves open); n == 1: m = 1 (:29-33).
 * cugs_knn_mean_distances writes mean_dist [n] in the input order of the points.  `route`:
 *   CUGS_KNN_EXHAUSTIVE  every query against every point; needs no workspace (NULL, 0 allowed);
 *   CUGS_KNN_TREE        Morton order, buckets of 32, a tree of boxes walked per query; same bits as the exhaustive route;
 *   CUGS_KNN_AUTO        exhaustive for small clouds, the tree from the size DESIGN.md 4.15 records.
 * TREE and AUTO need cugs_knn_workspace_bytes(n, k) bytes of scratch (monotone in n; 0 for invalid arguments).
 * k in 1..16, 0 <= n <= 2^30, non-null positions / mean_dist when n > 0, a known route: CUGS_EINVAL otherwise;
 * CUGS_EWORKSPACE for a short workspace, before anything is queued; n == 0 queues nothing.  Stream-ordered, no host
 * read-back, nothing allocated, no float atomics: the same bits from run to run.
 * cugs_init_from_points: one launch that writes the five model arrays (positions [n,3], sh_coeffs [n,3,num_coeffs],
 * opacities [n,1], rotations [n,4], scales [n,3]) from positions [n,3], colors [n,3] uint8 and mean_dist [n];
 * num_coeffs in {1, 4, 9, 16}. */
#define CUGS_KNN_AUTO 0
#define CUGS_KNN_EXHAUSTIVE 1
#define CUGS_KNN_TREE 2
size_t cugs_knn_workspace_bytes(int64_t n, int k);
int cugs_knn_mean_distances(int64_t n, int k, const float* positions, float* mean_dist, void* workspace,
                            size_t workspace_bytes, int route, void* stream);
int cugs_init_from_points(int64_t n, int num_coeffs, const float* positions, const uint8_t* colors,
                          const float* mean_dist, float* out_positions, float* out_sh, float* out_opacities,
                          float* out_rotations, float* out_scales, void* stream);

/* ---- Mesh export: TSDF fusion of rendered depth and surface-net extraction (not in the reference) ----
 * The volume: a dense box of nx x ny x nz voxels, x fastest; origin = the world position of the centre of voxel (0,0,0);
 * one DEVICE array of float planes [P, nz, ny, nx]: plane 0 the tsdf in units of trunc (initially 1), plane 1 the weight
 * (initially 0), and with color != 0 planes 2-4 r, g, b (initially 0); P = 5 with colour, 2 without.
 *
 * cugs_tsdf_integrate fuses num_views (1..16) views in ONE pass over the volume: each voxel is loaded once, updated by
 * the views in the order given and stored once if any view touched it; a voxel no view touches moves no volume bytes;
 * 16 views in one call leave the bits of 16 calls of one view.  A view: its camera (row-major view matrix v0..v11,
 * pinhole, image size W x H), depth_map D and alpha A (DEVICE float[H*W], the maps render() returns), optional color
 * (DEVICE float[H,W,3]) and optional per-pixel weight (DEVICE float[H*W]).  The fp32 rule per voxel (ix, iy, iz) and
 * view, every step one correctly rounded operation:
 *   1. px = ox + (float)ix * vs,  py, pz likewise
 *   2. xc = ((v0 px + v1 py) + v2 pz) + v3,  yc from v4..v7, zc from v8..v11;  skip unless zc > min_depth
 *   3. u = (fx xc) / zc + cx,  v = (fy yc) / zc + cy;  iu = floorf(u), iv = floorf(v) (pixel i covers [i, i+1));
 *      skip unless 0 <= iu < W and 0 <= iv < H, tested on the floored FLOATS
 *   4. pix = iv W + iu;  A = alpha[pix];  skip unless A > min_alpha;  d = D[pix] / A
 *   5. w = weight[pix], or 1 without a weight map;  skip unless w > 0 (NaN skips)
 *   6. sdf = d - zc;  skip unless sdf >= -trunc (a NaN depth skips);  tn = fminf(sdf / trunc, 1)
 *   7. Wn = Wo + w;  T = (Wo To + w tn) / Wn;  each colour plane likewise from color[3 pix + ch];  W = fminf(Wn, max_weight)
 * Every decision comes before the load that depends on it; no index is formed from a value that failed its test.
 * 16-byte accesses (four x-neighbours per plane) where planes is 16-byte aligned and nx % 4 == 0, 4-byte accesses
 * otherwise: the same bits either way.  One launch, the view table as a kernel argument; no atomics, no host sync, no
 * allocation.  All checks before anything is queued, in this order: CUGS_EINVAL for a NULL vol, views or opts, a
 * non-positive nx, ny or nz, num_views outside 1..16, NULL planes, voxel_size or trunc not positive and finite,
 * min_depth, min_alpha or max_weight not positive and finite, then per view in order: fx or fy not positive and finite,
 * a non-positive image size, a NULL depth_map or alpha, colour planes and no color; CUGS_EOVERFLOW for
 * nx ny nz > 2^31 - 1.
 *
 * Surface nets.  A corner is valid where weight > min_weight and inside where tsdf < 0.  Cell (cx, cy, cz),
 * 0 <= c < n - 1, is active when all eight corners are valid and their signs differ.  Corner k of a cell is the voxel
 * (cx + (k & 1), cy + ((k >> 1) & 1), cz + (k >> 2)).
 *   Vertices: one per active cell, in ascending cell index (x fastest).  Over the cell's twelve edges (a, b) in the fixed
 *   order - the four along x (a = 0, 2, 4, 6), the four along y (a = 0, 1, 4, 5), the four along z (a = 0, 1, 2, 3),
 *   b = a + (1 << axis) - whose ends differ in sign: t = fa / (fa - fb), the crossing = corner a's local coordinates with
 *   t on the edge's axis; m = (the crossings added in that order, per component) / (float)count;
 *   vertex = origin + ((float)c + m) * vs.  Colours: ca + t (cb - ca) per channel, added and divided the same way.
 *   Faces: the lattice edge from voxel (x, y, z) to its +axis neighbour belongs to cell (x, y, z).  With the other two
 *   axes (b, c) = (axis + 1, axis + 2) mod 3, the four cells around it are at offsets (-1,-1), (0,-1), (0,0), (-1,0) on
 *   (b, c): q0..q3, counter-clockwise seen from +axis.  If the ends differ in sign and all four cells exist and are
 *   active, the edge gives the triangles (q0,q1,q2), (q0,q2,q3) when the edge runs from negative to positive tsdf and
 *   (q3,q2,q1), (q3,q1,q0) otherwise: the normal points from negative to positive tsdf, out of the surface.  Faces come
 *   in ascending order of the owning cell, within a cell the edges along x, y, z, within an edge the two triangles;
 *   int32 [F,3] of vertex indices.
 * cugs_mesh_workspace_bytes: scratch for a volume (6 bytes per cell rounded up to chunks of 1024 cells, 8 bytes per
 * chunk, 16 per 256 chunks; a multiple of 256; 0 for a non-positive size or nx ny nz > 2^31 - 1).
 * cugs_mesh_plan classifies and scans (four launches) and blocks on one 16-byte read-back: counts_host = {vertices,
 * faces}.  A volume without cells (an axis of one voxel) plans {0, 0} with nothing queued.
 * cugs_mesh_emit writes vertices [V,3], optional colors [V,3] (colour planes needed) and faces [F,3] for the counts and
 * the workspace of the plan (two launches; zero counts queue nothing); it never writes past V or F rows.
 * Integer scans only, no float atomics: the same bytes from run to run.
 * Checks, before anything is queued, in this order: CUGS_EINVAL for a NULL vol, non-positive nx, ny or nz, NULL planes,
 * voxel_size or trunc not positive and finite, a NULL workspace, then (plan) a min_weight that is negative or not finite
 * or a NULL counts_host, (emit) a negative count, a NULL vertices with V > 0 or faces with F > 0, colors without colour
 * planes; CUGS_EOVERFLOW for nx ny nz > 2^31 - 1; CUGS_EWORKSPACE for a short workspace; CUGS_EALIGN for a workspace
 * that is not 16-byte aligned; (emit) CUGS_EINVAL for counts no plan of this volume can give (V > cells, F > 6 cells). */
typedef struct cugs_tsdf_volume {
    float*  planes;         /* DEVICE float[P, nz, ny, nx] */
    int32_t nx, ny, nz;
    int32_t color;          /* 0: P = 2;  otherwise P = 5 */
    float   origin[3];
    float   voxel_size;     /* > 0 and finite */
    float   trunc;          /* > 0 and finite */
} cugs_tsdf_volume;
typedef struct cugs_tsdf_view {
    cugs_camera  camera;
    const float* depth_map; /* DEVICE float[H*W] */
    const float* alpha;     /* DEVICE float[H*W] */
    const float* color;     /* DEVICE float[H,W,3]; needed with colour planes, ignored without */
    const float* weight;    /* DEVICE float[H*W]; NULL: all ones */
} cugs_tsdf_view;
typedef struct cugs_tsdf_opts {
    float min_depth;        /* > 0 and finite */
    float min_alpha;        /* > 0 and finite */
    float max_weight;       /* > 0 and finite */
} cugs_tsdf_opts;
int cugs_tsdf_integrate(const cugs_tsdf_volume* vol, const cugs_tsdf_view* views, int num_views,
                        const cugs_tsdf_opts* opts, void* stream);
size_t cugs_mesh_workspace_bytes(int nx, int ny, int nz);
int cugs_mesh_plan(const cugs_tsdf_volume* vol, float min_weight, void* workspace, size_t workspace_bytes,
                   int64_t* counts_host /* HOST int64[2] */, void* stream);
int cugs_mesh_emit(const cugs_tsdf_volume* vol, void* workspace, size_t workspace_bytes, int64_t num_vertices,
                   int64_t num_faces, float* vertices, float* colors /* nullable */, int32_t* faces, void* stream);

/* ---- similarity transform of a model (not in the reference) ---------------------------------------
 * x' = s R x + t with R a proper rotation and s > 0.  On a Gaussian: positions' = s R p + t; scales' = scales + log s
 * (log-scales); rotations' = q_R (x) q, the Hamilton product in wxyz order with q left raw, so |q'| = |q|; opacities
 * unchanged; per channel and band l = 1..degree, sh[l^2 .. (l+1)^2)' = D_l(R) sh[l^2 .. (l+1)^2), the DC term unchanged.
 * D_l is the rotation of band l in the real basis the projection evaluates (Y1 = -k y, Y2 = k z, Y3 = -k x, ...):
 * Y_l(R d) = D_l Y_l(d), hence sum_k c'_k Y_k(R d) = sum_k c_k Y_k(d).  A camera (Rc, tc) that moves along,
 * Rc' = Rc R^T, tc' = s tc - Rc R^T t, sees camera-space coordinates scaled by s: the same image, the depth map times s.
 *
 * cugs_similarity_init (host only, no device work): CUGS_EINVAL for a NULL argument, a non-finite input, scale <= 0,
 * max |R^T R - I| > 1e-4 or det R < 0 (no reflections).  Otherwise R is first replaced by the nearest rotation, in fp64,
 * and every field below derives from that rotation in fp64 and is rounded to fp32 once.  For a signed permutation matrix
 * every D_l is an exact signed permutation; for the identity every matrix is exactly I and q = (1, 0, 0, 0).
 *
 * cugs_transform_gaussians: one launch, in place, no workspace, no host sync.  positions [n,3], rotations [n,4],
 * scales [n,3], sh [n,3,sh_coeffs] with sh_coeffs in {1, 4, 9, 16}; pointers need dword alignment only (16-byte accesses
 * are used where the pointer and sh_coeffs allow them: the same bits either way).  `mask` (n bytes, nullable): a row
 * whose byte is 0 is neither read nor written.  zero_rows_host / zero_row_floats_host: HOST arrays of num_zero
 * (0..CUGS_TRANSFORM_MAX_ZERO) DEVICE arrays [n, zero_row_floats[k]] whose rows are set to 0.0f for exactly the rows
 * transformed (an optimizer's moments).  Arithmetic, each product and each sum rounded to fp32 on its own:
 *   positions   acc = m[3i] x; acc = acc + m[3i+1] y; acc = acc + m[3i+2] z; out_i = acc + t[i]
 *   scales      out = scale + log_scale                         (skipped with CUGS_SIMILARITY_SCALE_IS_ONE: bits kept)
 *   rotations   a = q_R, b = q:  w' = aw bw - ax bx - ay by - az bz;  x' = aw bx + ax bw + ay bz - az by;
 *               y' = aw by - ax bz + ay bw + az bx;  z' = aw bz + ax by - ay bx + az bw, each summed left to right
 *   sh          out_i = D[i][0] c_0, then + D[i][j] c_j for j ascending
 * With CUGS_SIMILARITY_ROTATION_IS_IDENTITY rotations and sh are not touched; with both flags and t = 0 nothing but the
 * zero_rows is.  Checks, before anything is queued, in this order: CUGS_EINVAL for n < 0, another sh_coeffs, a NULL xf,
 * num_zero out of range or without its arrays, a non-positive zero_row_floats, a NULL tensor or zero row array with n > 0;
 * CUGS_EALIGN for a pointer that is not dword aligned; n = 0 then succeeds with nothing queued. */
#define CUGS_SIMILARITY_ROTATION_IS_IDENTITY 1u
#define CUGS_SIMILARITY_SCALE_IS_ONE 2u
#define CUGS_TRANSFORM_MAX_ZERO 8
typedef struct CugsSimilarity {
    float    m[9];          /* s R, row-major */
    float    t[3];
    float    log_scale;     /* log s */
    float    q[4];          /* unit quaternion of R, wxyz, w >= 0 */
    float    d1[9];         /* D_1, row-major */
    float    d2[25];        /* D_2 */
    float    d3[49];        /* D_3 */
    uint32_t flags;         /* CUGS_SIMILARITY_* */
} CugsSimilarity;
int cugs_similarity_init(CugsSimilarity* out, const double rotation[9], const double translation[3], double scale);
int cugs_transform_gaussians(int64_t n, int sh_coeffs, float* positions, float* rotations, float* scales, float* sh,
                             const uint8_t* mask /* nullable */, float* const* zero_rows_host,
                             const int* zero_row_floats_host, int num_zero, const CugsSimilarity* xf_host, void* stream);

/* ---- vector quantisation: nearest-code assignment and a deterministic Lloyd update (not in the reference; DESIGN.md
 * 4.27) ----------------------------------------------------------------------------------------------------------------
 * x [n, d] fp32 with a row stride of ldx >= d floats, codebook [k, d] fp32 contiguous, 1 <= d <= 48, 1 <= k <= 65536,
 * 0 <= n <= 2^31 - 1.  cugs_vq_workspace_bytes(k, d): scratch for either call (the int64 sums, 0.5 |c|^2 and the
 * codebook repacked for the matrix pipe; a multiple of 256, monotone in k and in d, 0 for a k or d outside the limits).
 *
 * cugs_vq_assign (two launches, a third with dist; no host sync):
 *   dot(i,j)   acc = 0; for t = 0..d-1 ascending: acc = fmaf(x[i,t], c[j,t], acc)
 *              (computed by v_mfma_f32_32x32x2_f32, which is that chain bit for bit; d is padded with zeros to an even
 *              length, and fmaf(0, 0, acc) changes no comparison)
 *   h[j]       0.5f * (acc = 0; acc = fmaf(c[j,t], c[j,t], acc), t ascending)
 *   score(i,j) h[j] - dot(i,j), one fp32 subtraction
 *   assign[i]  the j of the smallest score, the lowest j among equal scores: a strict < against a running best that
 *              starts at (+inf, 0), pairs (score, index) merged lexicographically wherever partial results meet.  A row
 *              whose scores are all NaN (a NaN in the row) therefore gets 0.
 *   dist[i]    (nullable) acc = 0; for t ascending: df = x[i,t] - c[a,t]; acc = acc + df * df, for the winner a; the
 *              subtraction, the product and the sum each rounded to fp32 on its own.
 *
 * cugs_vq_update (three launches, no host sync): with F = frac_bits (0..62) and w_i = 1 where weights is NULL,
 *   num[j,t] = sum over i with assign[i] = j of (int64) rint((double) w_i * (double) x[i,t] * 2^F)
 *   den[j]   = sum over the same i of (int64) rint((double) w_i * 2^F)
 *   codebook[j,t] = (float) ((double) num[j,t] / (double) den[j]) where den[j] > 0; a code with den[j] <= 0 (no member,
 *   or members of weight 0 only) keeps its bits: it is not re-seeded.  counts [k] int32 (nullable) receives the number of
 *   rows assigned to each code, whatever their weight.  A row whose assign is outside [0, k) is skipped - neither it nor
 *   anything through it is touched; -1 is the mark for "leave this row out".  The sums are two's complement integers
 *   added by 64-bit integer atomics, so the result does not depend on the order of the additions: the same bytes from
 *   run to run.  The call clears the sums it uses itself.  The caller guarantees n max|w x| 2^F < 2^62 and
 *   n max w 2^F < 2^62 (no overflow of a sum), and finite non-negative weights.
 *
 * Checks, before anything is queued, in this order: CUGS_EINVAL for n, d, k, ldx or frac_bits outside the limits above,
 * or with n > 0 a NULL x, codebook, assign or workspace; CUGS_EWORKSPACE for workspace_bytes below
 * cugs_vq_workspace_bytes(k, d); CUGS_EALIGN for a pointer that is not dword aligned or a workspace that is not 8-byte
 * aligned; n = 0 then returns 0 with nothing queued. */
size_t cugs_vq_workspace_bytes(int k, int d);
int cugs_vq_assign(int64_t n, int d, int k, const float* x, int64_t ldx, const float* codebook, int32_t* assign,
                   float* dist /* nullable */, void* workspace, size_t workspace_bytes, void* stream);
int cugs_vq_update(int64_t n, int d, int k, const float* x, int64_t ldx, const float* weights /* nullable */,
                   const int32_t* assign, int frac_bits, float* codebook /* in, out */, int32_t* counts /* nullable */,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- environment-map background: octahedral sky, fused composite and gradients (not in the reference) --
 * The Gaussians are rendered on background 0, so the blend leaves color = C; the final image is I = C + T B(p), B the
 * bilinear sample of one octahedral map E [3, R, R] fp32 (R a power of two, 4..2048) in the direction of pixel p's ray,
 * or a caller's background image [H, W, 3].  color, image, sample, dL_dimage, background: [H, W, 3]; final_T, dL_dalpha:
 * [H, W].  Every step is one correctly rounded fp32 operation (fmaf where written); tests/envmap_ref.py mirrors it bit for
 * bit.  For pixel (u, v):
 *   1. ax = (((float) u + 0.5f) - cx) / fx,  ay = (((float) v + 0.5f) - cy) / fy        (the blend's pixel centre)
 *   2. d_k = fmaf(m[3k], ax, fmaf(m[3k+1], ay, m[3k+2])), k = 0..2: m = O R^T, rows of the map's axes in camera
 *      coordinates.  cugs_envmap_view_init forms it in fp64 from the camera's world-to-camera rotation R and the
 *      orientation O (world to map axes, row-major, NULL = identity): m[3i+j] = (float) ((O[i][0] R[j][0] + O[i][1] R[j][1])
 *      + O[i][2] R[j][2]), one rounding to fp32.
 *   3. s = (|d0| + |d1|) + |d2|;  n = d / s (three divisions).  If n2 < 0: x = (1 - |n1|) sgn(n0), y = (1 - |n0|) sgn(n1),
 *      sgn(t) = t >= 0 ? 1 : -1; otherwise x = n0, y = n1.  (s not in (0, inf): x = y = 0.)
 *   4. h = 0.5f R;  sx = fmaf(x, h, h - 0.5f), i0 = floorf(sx) held to [-1, R - 1], a = sx - (float) i0;  sy, j0, b
 *      likewise from y.  Taps (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1): E00, E01, E10, E11.
 *   5. a tap outside [0, R) is folded by the octahedral rule:  i < 0: (i, j) = (-1 - i, R - 1 - j);  i >= R: (2R - 1 - i,
 *      R - 1 - j);  then j < 0: (i, j) = (R - 1 - i, -1 - j);  j >= R: (R - 1 - i, 2R - 1 - j).  Texel (i, j) of channel c
 *      is E[(c R + j) R + i].
 *   6. top = fmaf(a, E01 - E00, E00), bot = fmaf(a, E11 - E10, E10), B_c = fmaf(b, bot - top, top)
 *   7. I_c = fmaf(T, B_c, C_c)
 * Backward, g = dL_dimage:
 *   dL_dalpha = -fmaf(g2, B2, fmaf(g1, B1, g0 * B0))
 *   dL_dbackground_c = T * g_c                                                             (the image route)
 *   dL_denv: tap k of channel c receives the share  w_k * (T * g_c),  w00 = (1 - a) * (1 - b), w01 = a * (1 - b),
 *   w10 = (1 - a) * b, w11 = a * b, as the integer rint((double) share * 2^F) added by 64-bit integer atomics, and
 *   dL_denv = (float) ((double) sum * 2^-F): the same bytes from run to run.  With 2^e the smallest power of two >=
 *   grad_bound and 2^q the smallest power of two > 4 H W, F = 61 - q - e (cugs_envmap_frac_bits).  A share beyond
 *   +-2^e is clamped to it (a NaN share counts 0) and sets *clamped (device int32, written every call) to 1.
 *
 * cugs_envmap_workspace_bytes(R): the int64 table of the map gradient; 0 for a bad R.
 * cugs_envmap_composite: exactly one of env and background.  image needs color and final_T; sample (env route only,
 * nullable) receives B itself; at least one of image and sample.
 * cugs_envmap_composite_backward: exactly one of env and background; dL_dalpha, dL_denv (env route; needs workspace and
 * clamped) and dL_dbackground (image route) are each nullable.  Three launches with dL_denv, one without; no host sync.
 * Checks, before anything is queued, in this order: CUGS_EINVAL (NULL view or required pointer, width or height <= 0,
 * on the env route R not a power of two in [4, 2048] or fx, fy not positive and finite or cx, cy, m not finite,
 * grad_bound not in [2^-60, 2^24]); CUGS_EOVERFLOW for H W > 2^31 - 1; CUGS_EWORKSPACE; CUGS_EALIGN for a pointer that
 * is not dword aligned or a workspace that is not 8-byte aligned. */
typedef struct cugs_envmap_view {
    float m[9];
    float fx, fy, cx, cy;
    int32_t width, height, resolution;     /* resolution is not read on the image route */
} cugs_envmap_view;
int cugs_envmap_view_init(cugs_envmap_view* out, const cugs_camera* camera, const double* orientation /* [9], nullable */,
                          int resolution);
size_t cugs_envmap_workspace_bytes(int resolution);
int cugs_envmap_frac_bits(int width, int height, float grad_bound);      /* F, or a negative error code */
int cugs_envmap_composite(const cugs_envmap_view* view, const float* env, const float* background, const float* color,
                          const float* final_T, float* image /* nullable */, float* sample /* nullable */, void* stream);
int cugs_envmap_composite_backward(const cugs_envmap_view* view, const float* env, const float* background,
                                   const float* dL_dimage, const float* final_T, float grad_bound, void* workspace,
                                   size_t workspace_bytes, float* dL_dalpha, float* dL_denv, float* dL_dbackground,
                                   int32_t* clamped, void* stream);

/* Device properties the host side needs without linking the HIP runtime itself. */
int cugs_device_count(int* count_host);

#ifdef __cplusplus
}
#endif
#endif /* CUGS_HIP_H */
