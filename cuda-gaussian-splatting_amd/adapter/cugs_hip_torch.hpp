// cugs_hip_torch.hpp — libtorch layer over the C ABI (include/cugs_hip.h).
//
// C++ host side of the drop-in: the reference's stage functions and render()/render_backward()
// with torch::Tensor arguments and results (same names, shapes, dtypes and zero/empty-case
// behaviour as namespace cugs), the camera as the POD `cugs_camera`.  It depends on libtorch
// only; `reference_glue.hpp` adds the few lines that map cugs::CameraInfo / cugs::GaussianModel
// (Eigen + the reference's headers) onto it.  Errors: non-zero C-ABI codes become
// std::runtime_error like CUDA_CHECK (utils/cuda_utils.cuh:12-20); argument checks are TORCH_CHECK.
#pragma once

#include <torch/torch.h>

#include <atomic>
#include <memory>

#include <array>
#include <string>
#include <vector>

#include "../../include/cugs_hip.h"
#include "eval_results.hpp"

namespace cugs_hip {

struct ProjectionOutput {          // rasterizer/projection.hpp
    torch::Tensor means_2d, depths, cov_2d_inv, radii, tiles_touched, rgb, opacities_act;
    torch::Tensor packed;          // [N,12] scratch for the blend kernels (not in the reference)
    torch::Tensor colour_gate;     // [N] uint8: ReLU gate bits of the SH backward (cugs_hip.h; not in the reference)
};
struct SortingOutput {             // rasterizer/sorting.hpp:18-24
    torch::Tensor gaussian_keys_sorted, gaussian_values_sorted, tile_ranges;
    int total_pairs = 0;
    torch::Tensor tile_order;      // [tiles,4] int32, optional (not in the reference): {tile, first, end, 0}, longest list first (cugs_tile_order)
};
struct ForwardOutput {
    torch::Tensor color, final_T, n_contrib;
    torch::Tensor depth_map;       // [H,W] with rasterize_forward(..., depths) (not in the reference)
};
struct RasterizeBackwardOutput {
    torch::Tensor dL_drgb, dL_dopacity_act, dL_dmeans_2d, dL_dcov_2d_inv;
    torch::Tensor grad_accum;      // [N,16] packed rows (not in the reference)
    torch::Tensor dL_ddepths;      // [N] dL/dz of the depth map (rasterize_backward(..., depths, ...), unpacked)
    torch::Tensor dL_dmeans_2d_abs;   // [N,2] AbsGrad sums (want_abs_grad): own tensor unpacked, else grad_accum[:, 10:12]
};
struct ProjectionBackwardOutput { torch::Tensor dL_dpositions, dL_drotations, dL_dscales, dL_dopacities, dL_dsh_coeffs; };

struct ModelTensors {              // the five tensors of cugs::GaussianModel (core/gaussian.hpp:34-40)
    torch::Tensor positions, sh_coeffs, opacities, rotations, scales;
};
struct RenderSettings { float background[3] = {0.f, 0.f, 0.f}; int active_sh_degree = 3; float scale_modifier = 1.f; };
struct RenderOutput {              // rasterizer/rasterizer.hpp:27-46
    torch::Tensor color, final_T, n_contrib, means_2d, depths, cov_2d_inv, radii, rgb, opacities_act,
        gaussian_indices, tile_ranges;
    torch::Tensor packed;
    torch::Tensor colour_gate;     // from the projection; undefined = render_backward recomputes the gate from the coefficients
    // [N, 16] accumulator of the blend backward, already cleared by the forward blend (which leaves HBM idle); handed
    // to ONE render_backward, which takes it out of the struct (hence mutable).  COPIES of a RenderOutput share the
    // buffer; `accum_used` (shared by the copies) makes "one" hold across them: the second backward - through whichever
    // copy - finds the flag set and fills a fresh accumulator instead of adding onto the first one's rows.
    mutable torch::Tensor zeroed_accum;
    std::shared_ptr<std::atomic<bool>> accum_used;
    torch::Tensor tile_order;      // [tiles,4] int32: the order the blend kernels' workgroups take the tiles in (undefined: spatial)
    // render(..., want_depth_map = true) (not in the reference): [H,W] sum_i z_i alpha_i T_i, background 0.
    // The alpha (coverage) map is 1 - final_T; depth_map / alpha is the normalised depth.
    torch::Tensor depth_map;
};
// dL_dviewmat (not in the reference): [4,4] dL/d(world-to-camera matrix), render_backward(...,
// want_camera_grad = true) only, undefined otherwise.
// dL_dmeans_2d_abs (not in the reference): [N,2] absolute 2-D mean gradients (AbsGrad),
// render_backward(..., want_abs_grad = true) only, undefined otherwise: a view of words 10, 11 of the blend's accumulator
// rows (row stride 16, no copy), which it keeps alive; DensificationController::accumulate_gradients reads it in place.
struct BackwardOutput {
    torch::Tensor dL_dpositions, dL_drotations, dL_dscales, dL_dopacities, dL_dsh_coeffs, dL_dmeans_2d;
    torch::Tensor dL_dviewmat;
    torch::Tensor dL_dmeans_2d_abs;
};

ProjectionOutput project_gaussians(const torch::Tensor& positions, const torch::Tensor& rotations,
                                   const torch::Tensor& scales, const torch::Tensor& opacities,
                                   const torch::Tensor& sh_coeffs, const cugs_camera& camera,
                                   int active_sh_degree, float scale_modifier = 1.0f);
SortingOutput sort_gaussians(const torch::Tensor& means_2d, const torch::Tensor& depths, const torch::Tensor& radii,
                             const torch::Tensor& tiles_touched, int img_w, int img_h);
ForwardOutput rasterize_forward(const torch::Tensor& means_2d, const torch::Tensor& cov_2d_inv,
                                const torch::Tensor& rgb, const torch::Tensor& opacities,
                                const torch::Tensor& tile_ranges, const torch::Tensor& gaussian_indices,
                                int img_w, int img_h, const float background[3],
                                const torch::Tensor& packed = {}, const torch::Tensor& zero_buf = {},
                                const torch::Tensor& tile_order = {}, const torch::Tensor& depths = {});
// the tiles ordered by the length of their lists, longest first, from any valid tile_ranges (cugs_tile_order)
torch::Tensor tile_order_of(const torch::Tensor& tile_ranges, int img_w, int img_h);
RasterizeBackwardOutput rasterize_backward(const torch::Tensor& dL_dcolor, const torch::Tensor& means_2d,
                                           const torch::Tensor& cov_2d_inv, const torch::Tensor& rgb,
                                           const torch::Tensor& opacities, const torch::Tensor& tile_ranges,
                                           const torch::Tensor& gaussian_indices, const torch::Tensor& final_T,
                                           const torch::Tensor& n_contrib, int img_w, int img_h,
                                           const float background[3], int n_gaussians,
                                           const torch::Tensor& packed = {}, bool unpack = true,
                                           const torch::Tensor& zeroed_accum = {}, const torch::Tensor& tile_order = {},
                                           const torch::Tensor& depths = {}, const torch::Tensor& dL_ddepth_map = {},
                                           const torch::Tensor& dL_dalpha = {}, bool want_abs_grad = false);
ProjectionBackwardOutput project_backward(const torch::Tensor& dL_dmeans_2d, const torch::Tensor& dL_dcov_2d_inv,
                                          const torch::Tensor& dL_drgb, const torch::Tensor& dL_dopacity_act,
                                          const torch::Tensor& positions, const torch::Tensor& rotations,
                                          const torch::Tensor& scales, const torch::Tensor& opacities,
                                          const torch::Tensor& sh_coeffs, const torch::Tensor& radii,
                                          const cugs_camera& camera, int active_sh_degree,
                                          float scale_modifier = 1.0f);
torch::Tensor evaluate_sh_cuda(int degree, const torch::Tensor& sh_coeffs, const torch::Tensor& directions);
torch::Tensor evaluate_sh_backward_cuda(int degree, const torch::Tensor& sh_coeffs, const torch::Tensor& directions,
                                        const torch::Tensor& dL_dcolor);

// `for_backward` = false (evaluation, viewer; not in the reference): no accumulator is prepared for a backward pass.
// `want_depth_map` (not in the reference): also RenderOutput::depth_map (cugs_blend_forward_opts::out_depth); the colour
// outputs are unchanged, bit for bit.
RenderOutput render(const ModelTensors& model, const cugs_camera& camera, const RenderSettings& settings,
                    bool for_backward = true, bool want_depth_map = false);
class FusedAdam;
struct Similarity;
class MCMCController;
// `fused` (optional, not in the reference; single-GPU training): the projection backward applies the optimizer step to
// the model in place (cugs_project_backward_adam_opts) and the five parameter gradients are never materialised (undefined
// in the result; dL_dmeans_2d is returned) - bit for bit render_backward + apply_gradients + step.
BackwardOutput render_backward(const torch::Tensor& dL_dcolor, const RenderOutput& render_out,
                               const ModelTensors& model, const cugs_camera& camera, const RenderSettings& settings,
                               FusedAdam* fused = nullptr, const MCMCController* mcmc = nullptr, int step = 0,
                               const torch::Tensor& dL_ddepth_map = {}, const torch::Tensor& dL_dalpha = {},
                               bool want_camera_grad = false, bool want_abs_grad = false, bool sparse_adam = false);
// `sparse_adam` (with `fused` only, never with `mcmc`; not in the reference): the fused step touches only
// the Gaussians this view sees, render_out.radii > 0 (cugs_projection_opts.sparse, with or without the camera gradient) - bit for bit
// render_backward + apply_gradients + step(render_out.radii); every other Gaussian keeps parameters and moments and is
// not read at all.
// `mcmc` (with `fused` only): the regulariser gradient and the position noise of iteration `step` ride in
// the same launch (cugs_projection_opts.mcmc) - bit for bit render_backward, + compute_regularization's
// gradients, apply_gradients, step, inject_noise(model, step).
// `dL_ddepth_map`, `dL_dalpha` ([H,W] each, optional, not in the reference): the gradients of RenderOutput::depth_map
// (needs render(..., want_depth_map = true)) and of the alpha map 1 - final_T, on every route above.
// `want_camera_grad` (not in the reference): BackwardOutput::dL_dviewmat, the gradient with respect to
// camera.view (row 3 zero; the SH view direction held constant), on every route above, with no host sync; every other
// output is unchanged, bit for bit.
// `want_abs_grad` (not in the reference): BackwardOutput::dL_dmeans_2d_abs, the AbsGrad densification
// signal, from the backward blend (cugs_blend_backward_opts::abs_grad), on every route above; every other output is the same
// up to the order of the blend's atomic adds.

// training/loss.hpp:21-52 + the autograd step of trainer.cpp:214-217 in two launches.
// Scalars are 0-dim device tensors, as in the reference.
struct LossAndGrad { torch::Tensor loss, l1, ssim_mean, dL_dcolor; };
LossAndGrad combined_loss_and_grad(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_ = 0.2f,
                                   bool want_grad = true);
torch::Tensor combined_loss(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_ = 0.2f);
torch::Tensor ssim(const torch::Tensor& rendered, const torch::Tensor& target, int window_size = 11);

// Not in the reference: the same loss of x' = mask * (A rendered + b) against y' = mask * target, inside
// the same two launches.  `exposure`: float32 [3,4] = [A | b], contiguous, on the images' device (undefined: identity);
// `mask`: float32 [H,W] (undefined: all ones).  Both means stay over all 3 H W elements.  dL_dcolor = mask A^T dL/dx'
// (with want_grad), dL_dexposure [3,4] (with want_grad and an exposure; twelve fixed-order fp64 sums, the same bits
// from run to run), corrected = x' (with want_corrected); no gradient to the mask or the target, no host sync.
// With neither exposure nor mask nor want_corrected: combined_loss_and_grad, bit for bit.
struct ExposureLoss { torch::Tensor loss, dL_dcolor, dL_dexposure, l1, ssim_mean, corrected; };
ExposureLoss combined_loss_exposure(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_ = 0.2f,
                                    const torch::Tensor& exposure = {}, const torch::Tensor& mask = {},
                                    bool want_grad = true, bool want_corrected = false, int window_size = 11);

// Not in the reference: depth supervision on render()'s depth and alpha maps.  The L1 loss of the
// expected depth x = depth_map / alpha (`inverse`: alpha / depth_map, against an inverse-depth prior) against
// s * target + b, all maps float32 [H,W] on one device; `weight` undefined: all ones.  A pixel counts iff alpha >
// min_alpha, weight > 0, 0 < target < inf and (inverse) depth_map > 0; elsewhere the gradients and `expected` are 0; the
// mean is over all H W pixels.  `align`: undefined for (1, 0), or a float32 [2] device tensor (s, b); `fit`: the weighted
// least squares of the target to x, solved on the device in fp64 (fit_ok = 0 and (1, 0) when it is degenerate) - not
// together with `align`.  (s, b) is a constant in the gradient.  Two launches (four with a fit), no host sync, the same
// bits from run to run; the scalars are 0-dim device tensors, scale_shift a [2] view.  The gradients feed
// render_backward's dL_ddepth_map and dL_dalpha.
struct DepthLoss { torch::Tensor loss, dL_ddepth_map, dL_dalpha, scale_shift, valid_weight, valid_count, fit_ok, expected; };
DepthLoss depth_loss(const torch::Tensor& depth_map, const torch::Tensor& alpha, const torch::Tensor& target,
                     const torch::Tensor& weight = {}, bool inverse = false, const torch::Tensor& align = {},
                     bool fit = false, float min_alpha = 1e-3f, bool want_grad = true, bool want_expected = false);

// Not in the reference: normal supervision from render()'s depth and alpha maps.  The surface normal of
// the expected depth depth_map / alpha (back-projected through the pinhole fx, fy, cx, cy; central differences; n = Py x
// Px normalised - the 2DGS depth_to_normal, camera axes x right, y down, z forward, pointing at the camera) against a
// normal prior `target` float32 [3,H,W] (normalised in the kernel): the mean over all H W pixels of weight *
// (cos_weight (1 - n.t) + l1_weight |n - t|_1) over the pixels that count - not on the image border, alpha > min_alpha
// there and at the four neighbours, a normal and a prior vector of finite non-zero length, weight > 0 (`weight`
// undefined: all ones).  The masks are constants in the gradient; the gradients feed render_backward's dL_ddepth_map and
// dL_dalpha.  `target` undefined: the normal map alone (want_normals must be set; loss 0, no gradients).  Two launches, no
// host sync, the same bits from run to run and whatever the tiling; the scalars are 0-dim device tensors.
struct NormalLoss { torch::Tensor loss, dL_ddepth_map, dL_dalpha, valid_weight, valid_count, normals; };
NormalLoss normal_loss(const torch::Tensor& depth_map, const torch::Tensor& alpha, float fx, float fy, float cx, float cy,
                       const torch::Tensor& target = {}, const torch::Tensor& weight = {}, float cos_weight = 1.0f,
                       float l1_weight = 0.0f, float min_alpha = 1e-3f, bool want_grad = true, bool want_normals = false);
torch::Tensor depth_to_normals(const torch::Tensor& depth_map, const torch::Tensor& alpha, float fx, float fy, float cx,
                               float cy, float min_alpha = 1e-3f);

// Not in the reference: mesh export.  A dense truncated signed distance volume over torch::Tensor -
// planes float32 [P, nz, ny, nx] (tsdf in units of trunc, weight, and with colour r, g, b; P = 5 or 2), voxel (0,0,0)
// centred on `origin` - fused from render()'s depth and alpha maps by tsdf_integrate (up to 16 views per pass over the
// volume, the views in the order given, the same bits however they are batched) and turned into a surface-net mesh by
// mesh_extract (vertices float32 [V,3], faces int32 [F,3] with normals towards free space, colours float32 [V,3] or
// undefined; one host sync for the two counts).  The rules are in include/cugs_hip.h.
struct TsdfVolume {
    torch::Tensor planes;
    float origin[3] = {0.0f, 0.0f, 0.0f};
    float voxel_size = 0.0f, trunc = 0.0f, max_weight = 64.0f, min_depth = 0.05f;
    bool has_color() const { return planes.size(0) == 5; }
};
TsdfVolume make_tsdf_volume(const float origin[3], int nx, int ny, int nz, float voxel_size, float trunc, bool color,
                            const torch::Device& device, float max_weight = 64.0f, float min_depth = 0.05f);
struct TsdfViewInput {
    cugs_camera camera;
    torch::Tensor depth_map, alpha;     // float32 [H,W]
    torch::Tensor color;                // float32 [H,W,3]; needed by a volume with colour
    torch::Tensor weight;               // float32 [H,W]; undefined: all ones
};
void tsdf_integrate(TsdfVolume& volume, const std::vector<TsdfViewInput>& views, float min_alpha = 0.5f);
struct Mesh { torch::Tensor vertices, faces, colors; };
Mesh mesh_extract(const TsdfVolume& volume, float min_weight = 0.0f);

// Not in the reference: per-view bilateral-grid colour correction.  grid: float32 [12, L, GY, GX],
// contiguous, each extent in [2, 64], coefficient 4 i + j = row i, column j of [A | b]; images float32 [H,W,3] on the
// grid's device.  bilagrid_slice: corrected = A(p) rendered(p) + b(p), the transform sampled trilinearly at
// (x / (W-1), y / (H-1), luma) - grid_sample(bilinear, align_corners, border) + the affine apply in one launch; the
// identity grid returns rendered bit for bit.  bilagrid_slice_backward: dL_drendered (with the gradient through the
// luminance guidance) and dL_dgrid (written, not accumulated; fixed-order sums, no float atomics, the same bits from
// run to run), each only when asked for.  bilagrid_tv: tv = the UNWEIGHTED total variation (0-dim), dL_dgrid = weight *
// dtv/dgrid, ADDED to the tensor given (bilagrid_slice_backward's) or written to a new one.  No host sync anywhere.
// The loop: render -> bilagrid_slice -> combined_loss_and_grad(corrected, target) -> bilagrid_slice_backward ->
// render_backward(dL_drendered); held-out views are evaluated without a grid.
struct BilagridGrad { torch::Tensor dL_drendered, dL_dgrid; };
struct BilagridTV { torch::Tensor tv, dL_dgrid; };
torch::Tensor bilagrid_slice(const torch::Tensor& grid, const torch::Tensor& rendered);
BilagridGrad bilagrid_slice_backward(const torch::Tensor& grid, const torch::Tensor& rendered,
                                     const torch::Tensor& dL_dcorrected, bool want_grid_grad = true,
                                     bool want_image_grad = true);
BilagridTV bilagrid_tv(const torch::Tensor& grid, float weight = 1.0f, const torch::Tensor& dL_dgrid = {});

// Not in the reference: an environment-map background.  The model is rendered on background 0 (the
// blend leaves color = C); composite_environment adds the sky behind it, image = fmaf(final_T, B, color) with B the
// bilinear sample of one octahedral map [3, R, R] (R a power of two in [4, 2048]; the centre is the map frame's +z, the
// corners its -z) in the direction of each pixel's ray - one launch, a uniform map of colour c giving render(background
// = c) bit for bit.  composite_environment_backward: dL_dalpha = -sum_c g_c B_c for render_backward (with dL_dimage as
// its dL_dcolor), dL_denv summed in 64-bit fixed point through integer atomics (the same bytes from run to run, no host
// sync) and `clamped`, a 0-dim int32 device word set when a share T g_c w_k exceeded grad_bound (rounded up to a power
// of two; it fixes the scale, cugs_envmap_frac_bits).  composite_background / _backward do the same for a caller's
// background image [H,W,3]: dL_dbackground = T g.  The composites refuse a RenderSettings whose background is not 0.
// The step: render_with_environment -> loss and g -> composite_environment_backward -> render_backward(g, ...,
// dL_dalpha) and env.step(dL_denv, lr).
class EnvironmentMap {
public:
    // `orientation`: row-major 3x3, world axes to map axes (nullptr: identity); init_color fills the map
    EnvironmentMap(int resolution, const torch::Device& device, const float init_color[3] = nullptr,
                   const double* orientation = nullptr);
    torch::Tensor& texture() { return texture_; }
    const torch::Tensor& texture() const { return texture_; }
    int resolution() const { return static_cast<int>(texture_.size(1)); }
    const std::array<double, 9>& orientation() const { return orientation_; }
    cugs_envmap_view view(const cugs_camera& camera) const;             // M = orientation R^T rounded once, intrinsics, sizes
    torch::Tensor sample(const cugs_camera& camera) const;              // B [H,W,3]
    void step(const torch::Tensor& dL_denv, float lr);                  // one fused Adam update (AdamHyper's defaults), moments inside
private:
    torch::Tensor texture_, m_, v_;
    std::array<double, 9> orientation_;
    int step_count_ = 0;
};
struct EnvGrad { torch::Tensor dL_dalpha, dL_denv, clamped; };
struct BackgroundGrad { torch::Tensor dL_dalpha, dL_dbackground; };
struct EnvRender { torch::Tensor image; RenderOutput render_out; };
torch::Tensor composite_environment(const RenderOutput& render_out, const cugs_camera& camera, const EnvironmentMap& env,
                                    const RenderSettings* settings = nullptr);
EnvGrad composite_environment_backward(const torch::Tensor& dL_dimage, const RenderOutput& render_out,
                                       const cugs_camera& camera, const EnvironmentMap& env, float grad_bound = 1.0f,
                                       bool want_env_grad = true, const RenderSettings* settings = nullptr);
torch::Tensor composite_background(const torch::Tensor& color, const torch::Tensor& final_T, const torch::Tensor& background);
BackgroundGrad composite_background_backward(const torch::Tensor& dL_dimage, const torch::Tensor& final_T,
                                             const torch::Tensor& background, bool want_background_grad = true);
EnvRender render_with_environment(const ModelTensors& model, const cugs_camera& camera, const RenderSettings& settings,
                                  const EnvironmentMap& env, bool for_backward = true, bool want_depth_map = false);

// optimizer/fused_adam.hpp:29-106 on raw tensors (group order: positions, sh, opacities, scales, rotations)
struct AdamHyper { float beta1 = 0.9f, beta2 = 0.999f, eps = 1e-15f; };
class FusedAdam {
public:
    FusedAdam(std::array<torch::Tensor, 5> params, std::array<float, 5> lrs, AdamHyper h = {});
    void apply_gradients(const BackwardOutput& grads);
    void zero_grad();
    void set_lr(int group, float lr) { lrs_[group] = lr; }
    float get_lr(int group) const { return lrs_[group]; }
    void step();
    // Sparse Adam (not in the reference): `visible` is RenderOutput::radii of the view just rendered
    // (int32 [N]) or a bool [N] mask; only the rows with radii > 0 are stepped, exactly as step() would step them (bias
    // corrections from the global step count, which advances by one whatever the mask); the others keep parameters and
    // moments bit for bit and are neither read nor written (cugs_fused_adam_groups_rows).
    void step(const torch::Tensor& visible);
    // The optimizer half of cugs_project_backward_adam_opts: counts the step, returns moments / learning rates / bias
    // corrections for the launch that updates the parameters in place (they must be contiguous float32).
    cugs_adam_fused begin_fused_step();
    const std::array<torch::Tensor, 5>& params() const { return params_; }
    const std::array<torch::Tensor, 5>& exp_avg() const { return m_; }          // first / second moments, group order
    const std::array<torch::Tensor, 5>& exp_avg_sq() const { return v_; }
private:
    friend class DensificationController;      // carries m_/v_ through clone/split/prune
    friend class MCMCController;               // zeroes the relocated rows' moments
    friend int64_t prune_gaussians(ModelTensors&, const torch::Tensor&, FusedAdam*);   // carries m_/v_ through the prune
    friend void transform_gaussians(ModelTensors&, const Similarity&, const torch::Tensor&, FusedAdam*);   // zeroes moments
    friend int64_t merge_gaussians(ModelTensors&, const ModelTensors&, FusedAdam*);                                // extends m_/v_
    friend bool write_gaussian_ply(const std::string&, const ModelTensors&, const FusedAdam*);
    friend ModelTensors read_gaussian_ply(const std::string&, const torch::Device&, FusedAdam*);
    void step_groups(const torch::Tensor* rows);     // rows: int32 [N] radii of the sparse step, or nullptr
    std::array<torch::Tensor, 5> params_, m_, v_, grads_;
    std::array<float, 5> lrs_;
    AdamHyper h_;
    int step_count_ = 0;
};

// optimizer/densification.hpp:23-168 over csrc/densify.hip.  Same schedule, thresholds and
// result order as the reference; the split noise is an argument ([2, N, 3] standard normal, drawn from the
// device generator when undefined) and the VRAM guards are not mirrored.
struct DensificationConfig {
    int densify_from = 500, densify_until = 15000, densify_every = 100, opacity_reset_every = 3000;
    float grad_threshold = 0.0002f, opacity_threshold = 0.005f, percent_dense = 0.01f;
    int max_screen_size = 20, max_gaussians = 0;
};
struct DensificationStats { int num_cloned = 0, num_split = 0, num_pruned = 0, num_before = 0, num_after = 0; };
class DensificationController {
public:
    DensificationController(const DensificationConfig& config, float scene_extent)
        : config_(config), scene_extent_(scene_extent) {}
    void accumulate_gradients(const torch::Tensor& dL_dmeans_2d, const torch::Tensor& radii);
    bool should_densify(int step) const;
    bool should_reset_opacity(int step) const;
    // `optimizer` (optional): its parameter tensors are re-pointed at the new model and its moments carried over
    // (survivors keep theirs, new Gaussians start at zero) instead of the reference's optimizer rebuild.
    DensificationStats densify(ModelTensors& model, int step, const torch::Tensor& noise = {},
                               FusedAdam* optimizer = nullptr);
    void reset_opacity(ModelTensors& model);
    const torch::Tensor& grad_accum() const { return grad_accum_; }     // [N] sum of the gradient norms since the last densify
private:
    void reset_accumulators(int64_t n, const torch::Device& device);
    DensificationConfig config_;
    float scene_extent_;
    torch::Tensor grad_accum_, grad_count_, max_radii_2d_;
};

// optimizer/mcmc_densification.hpp:27-170 over csrc/mcmc.hip.  Same schedule and statistics as the
// reference; the random draws come from the counter-based generator keyed by (seed, step) (cugs_hip.h N5 block), the
// sampling weights are quantised to 2^-24, and the VRAM guard is not mirrored.  N never changes.
struct MCMCConfig {
    int relocate_from = 500, relocate_until = 15000, relocate_every = 100;
    float dead_opacity_threshold = 0.005f, relocate_cap = 0.05f;
    float noise_lr_init = 5e5f, noise_lr_final = 1e3f;
    int noise_lr_max_steps = 30000;
    float noise_gate_k = 100.0f, noise_gate_t = 0.995f;
    float lambda_opacity = 0.01f, lambda_scale = 0.01f;
    uint64_t seed = 0;                                     // not in the reference: the generator's key
};
struct MCMCStats { int num_relocated = 0, num_dead = 0, num_total = 0; bool skipped_vram = false; };
class MCMCController {
public:
    MCMCController(const MCMCConfig& config, float scene_extent) : config_(config), scene_extent_(scene_extent) {}
    bool should_relocate(int step) const;
    float noise_lr(int step) const;
    // in place, N constant; one 8-byte read-back.  `optimizer` (optional): the relocated rows' moments are zeroed.
    // `sources_out` (optional, int32 [N] device): the source row of the j-th relocated row.
    MCMCStats relocate(ModelTensors& model, int step, FusedAdam* optimizer = nullptr,
                       const torch::Tensor& sources_out = {});
    // `noise` (optional, [N, 3] standard normals): replaces the generator's draw
    void inject_noise(ModelTensors& model, int step, const torch::Tensor& noise = {}) const;
    // the value as a 0-dim device tensor (no host sync; the reference returns reg_loss.item())
    torch::Tensor compute_regularization(const ModelTensors& model, torch::Tensor& reg_dL_dopacities,
                                         torch::Tensor& reg_dL_dscales) const;
    // the fused route's arguments (render_backward(..., &adam, &mcmc, step))
    cugs_mcmc_fused fused_args(int step, const torch::Tensor& noise = {}) const;
    const MCMCConfig& config() const { return config_; }
private:
    MCMCConfig config_;
    float scene_extent_;
};

// the float [height, width, 3] training target from a device-resident uint8 [h, w, 3] view - x 1/255
// and, if the sizes differ, the reference's resize_image (data/image_io.cpp:35-39, 47-100), bit for bit what
// trainer.cpp:186-198 builds on the CPU and uploads.
torch::Tensor image_to_float(const torch::Tensor& view_u8, int width, int height);

// training/metrics.hpp:22-76 over csrc/metrics.hip.  ImageMetrics / EvalResults: eval_results.hpp.
// eval_metrics: device float[4] = {MSE, mean SSIM, L1 mean, max |rendered - target|}, two launches, no host sync;
//   `target` is float32 [H,W,3] or the uint8 [H,W,3] of a cached view (expanded in registers); `out` (optional): a
//   contiguous float32 [4] on the same device to write into - row v of a [V,4] table.  Mean SSIM and the L1 mean are
//   the bits of combined_loss_and_grad's ssim_mean and l1.
// compute_psnr / compute_ssim: the reference's scalars (metrics.cpp:21-46; one blocking 16-byte read-back each).
// evaluate: metrics.cpp:93-163 for `cameras[v]` against `targets[v]` (device tensors: uint8 [h,w,3], resized to the
//   camera as the reference does when the sizes differ, or float32 [H,W,3]); every view is queued, then ONE
//   device-to-host copy of the [V,4] table.  `names` (optional) fills ImageMetrics::image_name.
torch::Tensor eval_metrics(const torch::Tensor& rendered, const torch::Tensor& target, const torch::Tensor& out = {},
                           int window_size = 11);
float psnr_from_mse(float mse);
float compute_psnr(const torch::Tensor& rendered, const torch::Tensor& target);
float compute_ssim(const torch::Tensor& rendered, const torch::Tensor& target);
EvalResults evaluate(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                     const std::vector<torch::Tensor>& targets, const RenderSettings& settings,
                     const std::vector<std::string>& names = {});

// utils/ply_io.hpp:53-64 over csrc/ply.hip: the reference's binary PLY layout, records packed and
// unpacked on the device.  `optimizer` (optional): the Adam moments and step count ride along as extra properties
// m_*, v_* and a header comment (the reference's reader skips both); read_gaussian_ply restores them into
// `optimizer` when the file has them.  Errors as in the reference: write returns false, read throws.
bool write_gaussian_ply(const std::string& path, const ModelTensors& model, const FusedAdam* optimizer = nullptr);
ModelTensors read_gaussian_ply(const std::string& path, const torch::Device& device = torch::kCPU,
                               FusedAdam* optimizer = nullptr);

// core/gaussian_init.hpp over csrc/knn.hip: a model from a point cloud, on the device.
// positions [n, 3] float32, colors [n, 3] uint8, on any device (moved to `device`, which must be a HIP device; the
// default takes the positions' device, or the current HIP device if they are on the CPU).  Rows keep the input order.
// knn_mean_distances: compute_knn_mean_distances (gaussian_init.cpp:25-68), exact; k is clamped to n - 1.
// `route`: CUGS_KNN_AUTO / CUGS_KNN_EXHAUSTIVE / CUGS_KNN_TREE - the same bits on each.
torch::Tensor knn_mean_distances(const torch::Tensor& positions, int k_neighbors = 3, int route = CUGS_KNN_AUTO,
                                 c10::optional<torch::Device> device = c10::nullopt);
ModelTensors init_gaussians_from_sparse(const torch::Tensor& positions, const torch::Tensor& colors, int sh_degree = 3,
                                        int k_neighbors = 3, int route = CUGS_KNN_AUTO,
                                        c10::optional<torch::Device> device = c10::nullopt);

// Per-Gaussian contribution scores and score-based pruning (not in the reference).  The table is
// [N,4] 32-bit words {sum of w, max of w, pixel count (uint32), padding} of the blend weight w = alpha T, zeroed at
// construction and ADDED to by every launch (cugs_blend_scores): sums and counts add up over the views, the maximum is
// the maximum over the views.
struct ContributionScores {
    ContributionScores(int64_t n, const torch::Device& device);
    torch::Tensor table;                                   // [N,4] int32 words
    int num_views = 0;
    int64_t n() const { return table.size(0); }
    torch::Tensor weight_sum() const;                      // [N] float32, a view of word 0
    torch::Tensor weight_max() const;                      // [N] float32, a view of word 1
    torch::Tensor pixel_count() const;                     // [N] int64, read from the uint32 word 2
    void reset();
};
// One launch from an existing RenderOutput (its tile_ranges, gaussian_indices, packed records and tile_order); needs no
// for_backward state.
void accumulate_contribution_scores(ContributionScores& scores, const RenderOutput& render_out, const cugs_camera& camera);
// Offline, over many views, with no colour blend: per view the projection at SH degree 0, the plain sort and the score
// launch (one host sync per view: the sort's pair count).
ContributionScores contribution_scores(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                                       const RenderSettings& settings = {});
// Removes the rows whose entry of `prune_mask` (bool [N] on the model's device) is set, through cugs_densify_plan /
// cugs_densify_apply (flag 4 = keep on the rows that stay): the survivors keep their relative order and their bits.  With `optimizer` its
// parameter tensors are re-pointed at the new model, its moments carried over and its pending gradients cleared.
// Returns the number removed.  Per-Gaussian state held elsewhere is the caller's: a DensificationController's
// accumulators (the next accumulate_gradients or densify resizes them) and whatever an MCMCController keeps.
int64_t prune_gaussians(ModelTensors& model, const torch::Tensor& prune_mask, FusedAdam* optimizer = nullptr);
// The mask is weight_max < min_max_weight (when >= 0) and / or everything outside the round(keep_fraction N) largest
// weight_sum (libtorch topk; when >= 0); both given: the union of the two prunes.  A Gaussian with weight_max == 0 is
// always dropped.  Returns the number removed.
int64_t prune_by_scores(ModelTensors& model, const ContributionScores& scores, float min_max_weight = -1.0f,
                        float keep_fraction = -1.0f, FusedAdam* optimizer = nullptr);

// Pixel maps lifted onto Gaussians (not in the reference): S[g,c] = sum_p w_g(p) M_c(p) with the forward's
// blend weight w = alpha T.  The table is [N,4] float32, zeroed at construction; every launch (cugs_blend_lift) ADDS to
// words 0..channels-1 of a row and never writes the others.
struct LiftedMaps {
    LiftedMaps(int64_t n, const torch::Device& device, int channels = 1);
    torch::Tensor table;                                   // [N,4] float32
    int channels;
    int num_views = 0;
    int64_t n() const { return table.size(0); }
    torch::Tensor sums() const;                            // [N,channels] float32, a view of the table
    void reset();
};
// One launch from an existing RenderOutput; needs no for_backward state.  Exactly one of `maps` ([H,W,C] float32, or
// [H,W] for C = 1) and `labels` ([H,W] int32: channel c is the indicator of label_base + c) is defined.
void lift_pixel_maps(LiftedMaps& lifted, const RenderOutput& render_out, const cugs_camera& camera,
                     const torch::Tensor& maps, const torch::Tensor& labels = {}, int label_base = 0);
// Offline, as contribution_scores: per view the projection at SH degree 0, the plain sort and the lift launch of
// maps_per_view[i].  channels <= 0: the first map's (1 for an [H,W] map).
LiftedMaps lift_maps(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                     const std::vector<torch::Tensor>& maps_per_view, const RenderSettings& settings = {}, int channels = 0);
// votes[g,l] = sum over views and pixels of w_g(p) [label(p) == l] for l in 0..num_labels-1 (per view one projection and
// sort, ceil(num_labels / 4) launches); labels[g] = the first maximum of votes[g], -1 where a Gaussian collected no vote.
// Returns {labels [N] int64, votes [N,num_labels] float32}.
std::pair<torch::Tensor, torch::Tensor> vote_labels(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                                                    const std::vector<torch::Tensor>& label_maps, int num_labels,
                                                    const RenderSettings& settings = {});
// [N] float32: per view sum_p w_g(p) err(p) of error_maps[i] ([H,W] float32), the views combined by the maximum
// (max_over_views, the rule of "Revising Densification in Gaussian Splatting") or by addition.
torch::Tensor error_scores(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                           const std::vector<torch::Tensor>& error_maps, const RenderSettings& settings = {},
                           bool max_over_views = true);
// The complement of prune_gaussians: keeps the rows whose entry of `keep_mask` is set.  Returns the number kept.
int64_t select_gaussians(ModelTensors& model, const torch::Tensor& keep_mask, FusedAdam* optimizer = nullptr);

// A model moved by a similarity x' = scale * rotation x + translation (not in the reference): fp64 host
// values, the rotation row-major.  to_abi() is cugs_similarity_init (throws for what is no similarity).
struct Similarity {
    double scale = 1.0;
    std::array<double, 9> rotation = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::array<double, 3> translation = {0, 0, 0};
    Similarity inverse() const;
    Similarity compose(const Similarity& other) const;     // self after other
    std::array<double, 16> matrix() const;                 // row-major [[s R, t], [0, 1]]
    bool is_pure_translation() const;
    CugsSimilarity to_abi() const;
};
// One cugs_transform_gaussians launch on the current stream, in place (contiguous float32 tensors), no host sync:
// positions' = s R p + t, scales' = scales + log s, rotations' = q_R (x) q, every SH band l >= 1 times D_l(R).  `mask`
// (bool [N], optional): only the rows set are touched.  With `optimizer`: a pure translation leaves its moments alone;
// otherwise the moments of the transformed rows of the positions, SH and rotations groups are zeroed in the same launch
// (second moments are not covariant under a rotation - the precedent of densification's new rows and sparse Adam's
// late-seen rows); scales and opacities keep theirs, the step count is unchanged.
void transform_gaussians(ModelTensors& model, const Similarity& sim, const torch::Tensor& mask = {},
                         FusedAdam* optimizer = nullptr);
// Rc' = Rc R^T, tc' = s tc - Rc R^T t, in fp64, stored as float; the camera centre follows.
cugs_camera transform_camera(const cugs_camera& camera, const Similarity& sim);
// Appends the rows of `other` (in order) and replaces the model's tensors; differing SH degrees meet at the higher one,
// zero-padded.  With `optimizer` the old rows keep their moments, the new rows start from zero, pending gradients are
// cleared.  Returns the new N.
int64_t merge_gaussians(ModelTensors& model, const ModelTensors& other, FusedAdam* optimizer = nullptr);

// Vector quantisation of rows of up to 48 floats (not in the reference; the arithmetic is stated in
// cugs_hip.h).  x [n, d] float32 on a CUDA device (a row stride >= d is passed through), codebook [k, d].
// vq_assign: int32 [n], the nearest code of every row, the lowest index among equals, 0 for a row holding a NaN;
// `dist` (optional) receives the squared distance to it, float32 [n].
torch::Tensor vq_assign(const torch::Tensor& x, const torch::Tensor& codebook, torch::Tensor* dist = nullptr);
// The fraction bits of the fixed-point sums for n rows with |x| <= x_max and weights <= w_max: 61 minus the binary
// exponents (frexp) of n and of max(w_max x_max, w_max), at most 62; throws where that is negative or not finite.
int vq_frac_bits(int64_t n, double x_max, double w_max = 1.0);
// Lloyd's k-means: {codebook [k', d], indices int32 [n], counts int32 [k']}, k' = min(k, n).  The first codebook is
// `init` or the rows (j n) // k' of x; `iters` times assign and the deterministic update (weights: float32 [n],
// non-negative, optional), then a last assign; counts is the histogram of the indices.  An empty code keeps its value.
// One host read per call, none per iteration; the same bytes from run to run.  The container and compress_gaussians of
// the Python host have no C++ counterpart yet.
struct VqFit { torch::Tensor codebook, indices, counts; };
VqFit vq_fit(const torch::Tensor& x, int64_t k, int iters = 10, const torch::Tensor& weights = {},
             const torch::Tensor& init = {});

}  // namespace cugs_hip
