// torch_losses.cpp — cugs_hip_torch.hpp: the combined, exposure, depth and normal losses, depth_to_normals and the
// bilateral grid.
#include "torch_glue.hpp"

namespace cugs_hip {

namespace {
void validate_pair(const torch::Tensor& rendered, const torch::Tensor& target) {               // loss.cpp:14-34
    for (const torch::Tensor* img : {&rendered, &target}) {
        TORCH_CHECK(img->dim() == 3, "image must be 3-dimensional [H, W, 3], got ", img->dim(), " dims");
        TORCH_CHECK(img->size(2) == 3, "image must have 3 channels, got ", img->size(2));
        TORCH_CHECK(img->dtype() == torch::kFloat32, "image must be float32, got ", img->dtype());
        TORCH_CHECK(img->is_cuda(), "image must be on a CUDA device");
    }
    TORCH_CHECK(rendered.sizes() == target.sizes(), "rendered and target must have the same shape, got ",
                rendered.sizes(), " vs ", target.sizes());
}
torch::Tensor run_loss(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_, int window_size,
                       torch::Tensor* ssim_map, torch::Tensor* grad) {
    validate_pair(rendered, target);
    TORCH_CHECK(window_size % 2 == 1, "window_size must be odd, got ", window_size);               // loss.cpp:96-97
    TORCH_CHECK(window_size >= 3, "window_size must be >= 3, got ", window_size);
    const int h = static_cast<int>(rendered.size(0)), w = static_cast<int>(rendered.size(1));
    auto r = rendered.contiguous(), t = target.contiguous();
    auto out = torch::empty({4}, fopt(rendered));
    if (ssim_map) *ssim_map = torch::empty({h, w}, fopt(rendered));
    if (grad) *grad = torch::empty({h, w, 3}, fopt(rendered));
    auto ws = workspace(rendered.device(), cugs_loss_workspace_bytes(w, h), 2);
    check(cugs_combined_loss(w, h, ptr<float>(r), ptr<float>(t), lambda_, window_size, ws.data_ptr(), ws.numel(),
                             ptr<float>(out), ssim_map ? ptr<float>(*ssim_map) : nullptr,
                             grad ? ptr<float>(*grad) : nullptr, stream_of(rendered)), "cugs_combined_loss");
    return out;
}
}  // namespace

LossAndGrad combined_loss_and_grad(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_, bool want_grad) {
    LossAndGrad o;
    auto out = run_loss(rendered, target, lambda_, 11, nullptr, want_grad ? &o.dL_dcolor : nullptr);
    o.loss = out[0]; o.l1 = out[1]; o.ssim_mean = out[2];
    return o;
}
torch::Tensor combined_loss(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_) {
    return run_loss(rendered, target, lambda_, 11, nullptr, nullptr)[0];
}
torch::Tensor ssim(const torch::Tensor& rendered, const torch::Tensor& target, int window_size) {
    torch::Tensor map;
    run_loss(rendered, target, 0.2f, window_size, &map, nullptr);
    return map;
}

ExposureLoss combined_loss_exposure(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_,
                                    const torch::Tensor& exposure, const torch::Tensor& mask, bool want_grad,
                                    bool want_corrected, int window_size) {
    validate_pair(rendered, target);
    TORCH_CHECK(window_size % 2 == 1, "window_size must be odd, got ", window_size);
    TORCH_CHECK(window_size >= 3, "window_size must be >= 3, got ", window_size);
    const int h = static_cast<int>(rendered.size(0)), w = static_cast<int>(rendered.size(1));
    if (exposure.defined()) {
        TORCH_CHECK(exposure.dim() == 2 && exposure.size(0) == 3 && exposure.size(1) == 4, "exposure must be [3, 4], got ", exposure.sizes());
        TORCH_CHECK(exposure.dtype() == torch::kFloat32, "exposure must be float32, got ", exposure.dtype());
        TORCH_CHECK(exposure.is_cuda() && exposure.device() == rendered.device(), "exposure must be on the images' CUDA device");
        TORCH_CHECK(exposure.is_contiguous(), "exposure must be contiguous");
    }
    torch::Tensor m;
    if (mask.defined()) {
        TORCH_CHECK(mask.dim() == 2 && mask.size(0) == h && mask.size(1) == w, "mask must be [H, W], got ", mask.sizes());
        TORCH_CHECK(mask.dtype() == torch::kFloat32, "mask must be float32, got ", mask.dtype());
        TORCH_CHECK(mask.is_cuda() && mask.device() == rendered.device(), "mask must be on the images' CUDA device");
        m = mask.contiguous();
    }
    auto r = rendered.contiguous(), t = target.contiguous();
    auto out = torch::empty({4}, fopt(rendered));
    ExposureLoss o;
    if (want_grad) o.dL_dcolor = torch::empty({h, w, 3}, fopt(rendered));
    if (want_grad && exposure.defined()) o.dL_dexposure = torch::empty({3, 4}, fopt(rendered));
    if (want_corrected) o.corrected = torch::empty({h, w, 3}, fopt(rendered));
    cugs_loss_opts opts{};
    opts.exposure = exposure.defined() ? exposure.data_ptr<float>() : nullptr;
    opts.mask = m.defined() ? m.data_ptr<float>() : nullptr;
    opts.dL_dexposure = o.dL_dexposure.defined() ? o.dL_dexposure.data_ptr<float>() : nullptr;
    opts.corrected = o.corrected.defined() ? o.corrected.data_ptr<float>() : nullptr;
    auto ws = workspace(rendered.device(), cugs_loss_opts_workspace_bytes(w, h), 2);
    check(cugs_combined_loss_opts(w, h, ptr<float>(r), ptr<float>(t), lambda_, window_size, &opts, ws.data_ptr(), ws.numel(),
                                  ptr<float>(out), nullptr, want_grad ? o.dL_dcolor.data_ptr<float>() : nullptr,
                                  stream_of(rendered)), "cugs_combined_loss_opts");
    o.loss = out[0]; o.l1 = out[1]; o.ssim_mean = out[2];
    return o;
}

DepthLoss depth_loss(const torch::Tensor& depth_map, const torch::Tensor& alpha, const torch::Tensor& target,
                     const torch::Tensor& weight, bool inverse, const torch::Tensor& align, bool fit, float min_alpha,
                     bool want_grad, bool want_expected) {
    TORCH_CHECK(depth_map.dim() == 2, "depth_map must be 2-dimensional [H, W], got ", depth_map.dim(), " dims");
    TORCH_CHECK(depth_map.dtype() == torch::kFloat32, "depth_map must be float32, got ", depth_map.dtype());
    TORCH_CHECK(depth_map.is_cuda(), "depth_map must be on a CUDA device");
    const int h = static_cast<int>(depth_map.size(0)), w = static_cast<int>(depth_map.size(1));
    auto validate_map = [&](const torch::Tensor& t, const char* name) {
        TORCH_CHECK(t.dim() == 2 && t.size(0) == h && t.size(1) == w, name, " must be [H, W], got ", t.sizes());
        TORCH_CHECK(t.dtype() == torch::kFloat32, name, " must be float32, got ", t.dtype());
        TORCH_CHECK(t.is_cuda() && t.device() == depth_map.device(), name, " must be on the depth map's CUDA device");
    };
    validate_map(alpha, "alpha");
    validate_map(target, "target");
    torch::Tensor wt, ss;
    if (weight.defined()) { validate_map(weight, "weight"); wt = weight.contiguous(); }
    TORCH_CHECK(min_alpha > 0.0f && std::isfinite(min_alpha), "min_alpha must be positive and finite, got ", min_alpha);
    TORCH_CHECK(!(fit && align.defined()), "align must be a fit or a given (s, b), not both");
    if (align.defined()) {
        TORCH_CHECK(align.dim() == 1 && align.size(0) == 2, "align must be [2] = (s, b), got ", align.sizes());
        TORCH_CHECK(align.dtype() == torch::kFloat32, "align must be float32, got ", align.dtype());
        TORCH_CHECK(align.is_cuda() && align.device() == depth_map.device(), "align must be on the depth map's CUDA device");
        ss = align.contiguous();
    }
    auto d = depth_map.contiguous(), a = alpha.contiguous(), t = target.contiguous();
    auto out = torch::empty({8}, fopt(depth_map));
    DepthLoss o;
    if (want_grad) { o.dL_ddepth_map = torch::empty({h, w}, fopt(depth_map)); o.dL_dalpha = torch::empty({h, w}, fopt(depth_map)); }
    if (want_expected) o.expected = torch::empty({h, w}, fopt(depth_map));
    cugs_depth_loss_opts opts{};
    opts.weight = ptr<float>(wt);
    opts.scale_shift = ptr<float>(ss);
    opts.fit = fit ? 1 : 0;
    opts.inverse = inverse ? 1 : 0;
    opts.min_alpha = min_alpha;
    opts.expected = ptr<float>(o.expected);
    auto ws = workspace(depth_map.device(), cugs_depth_loss_workspace_bytes(w, h), 9);
    check(cugs_depth_loss(w, h, ptr<float>(d), ptr<float>(a), ptr<float>(t), &opts, ws.data_ptr(), ws.numel(),
                          ptr<float>(out), ptr<float>(o.dL_ddepth_map), ptr<float>(o.dL_dalpha), stream_of(depth_map)),
          "cugs_depth_loss");
    o.loss = out[0]; o.scale_shift = out.slice(0, 1, 3); o.valid_weight = out[3]; o.valid_count = out[4]; o.fit_ok = out[5];
    return o;
}

NormalLoss normal_loss(const torch::Tensor& depth_map, const torch::Tensor& alpha, float fx, float fy, float cx, float cy,
                       const torch::Tensor& target, const torch::Tensor& weight, float cos_weight, float l1_weight,
                       float min_alpha, bool want_grad, bool want_normals) {
    TORCH_CHECK(depth_map.dim() == 2, "depth_map must be 2-dimensional [H, W], got ", depth_map.dim(), " dims");
    TORCH_CHECK(depth_map.dtype() == torch::kFloat32, "depth_map must be float32, got ", depth_map.dtype());
    TORCH_CHECK(depth_map.is_cuda(), "depth_map must be on a CUDA device");
    const int h = static_cast<int>(depth_map.size(0)), w = static_cast<int>(depth_map.size(1));
    auto validate_map = [&](const torch::Tensor& t, const char* name) {
        TORCH_CHECK(t.dim() == 2 && t.size(0) == h && t.size(1) == w, name, " must be [H, W], got ", t.sizes());
        TORCH_CHECK(t.dtype() == torch::kFloat32, name, " must be float32, got ", t.dtype());
        TORCH_CHECK(t.is_cuda() && t.device() == depth_map.device(), name, " must be on the depth map's CUDA device");
    };
    validate_map(alpha, "alpha");
    TORCH_CHECK(fx > 0.0f && std::isfinite(fx) && fy > 0.0f && std::isfinite(fy), "fx, fy must be positive and finite, got ", fx, ", ", fy);
    TORCH_CHECK(std::isfinite(cx) && std::isfinite(cy), "cx, cy must be finite, got ", cx, ", ", cy);
    TORCH_CHECK(min_alpha > 0.0f && std::isfinite(min_alpha), "min_alpha must be positive and finite, got ", min_alpha);
    TORCH_CHECK(cos_weight >= 0.0f && std::isfinite(cos_weight) && l1_weight >= 0.0f && std::isfinite(l1_weight),
                "cos_weight and l1_weight must be non-negative and finite, got ", cos_weight, ", ", l1_weight);
    torch::Tensor t, wt;
    if (target.defined()) {
        TORCH_CHECK(target.dim() == 3 && target.size(0) == 3 && target.size(1) == h && target.size(2) == w,
                    "target must be [3, H, W], got ", target.sizes());
        TORCH_CHECK(target.dtype() == torch::kFloat32, "target must be float32, got ", target.dtype());
        TORCH_CHECK(target.is_cuda() && target.device() == depth_map.device(), "target must be on the depth map's CUDA device");
        TORCH_CHECK(cos_weight > 0.0f || l1_weight > 0.0f, "cos_weight and l1_weight must not both be 0");
        t = target.contiguous();
    } else {
        TORCH_CHECK(!weight.defined(), "weight needs a target");
        TORCH_CHECK(want_normals, "without a target there is only the normal map: want_normals must be set");
    }
    if (weight.defined()) { validate_map(weight, "weight"); wt = weight.contiguous(); }
    auto d = depth_map.contiguous(), a = alpha.contiguous();
    auto out = torch::empty({8}, fopt(depth_map));
    NormalLoss o;
    if (want_grad && t.defined()) { o.dL_ddepth_map = torch::empty({h, w}, fopt(depth_map)); o.dL_dalpha = torch::empty({h, w}, fopt(depth_map)); }
    if (want_normals) o.normals = torch::empty({3, h, w}, fopt(depth_map));
    cugs_normal_loss_opts opts{};
    opts.weight = ptr<float>(wt);
    opts.normals_out = ptr<float>(o.normals);
    opts.cos_weight = cos_weight;
    opts.l1_weight = l1_weight;
    opts.min_alpha = min_alpha;
    auto ws = workspace(depth_map.device(), cugs_normal_loss_workspace_bytes(w, h), 11);
    check(cugs_normal_loss(w, h, fx, fy, cx, cy, ptr<float>(d), ptr<float>(a), ptr<float>(t), &opts, ws.data_ptr(), ws.numel(),
                           ptr<float>(out), ptr<float>(o.dL_ddepth_map), ptr<float>(o.dL_dalpha), stream_of(depth_map)),
          "cugs_normal_loss");
    o.loss = out[0]; o.valid_weight = out[1]; o.valid_count = out[2];
    return o;
}

torch::Tensor depth_to_normals(const torch::Tensor& depth_map, const torch::Tensor& alpha, float fx, float fy, float cx,
                               float cy, float min_alpha) {
    return normal_loss(depth_map, alpha, fx, fy, cx, cy, {}, {}, 1.0f, 0.0f, min_alpha, false, true).normals;
}

namespace {
void validate_image(const torch::Tensor& img, const char* name) {
    TORCH_CHECK(img.dim() == 3 && img.size(2) == 3, name, " must be [H, W, 3], got ", img.sizes());
    TORCH_CHECK(img.dtype() == torch::kFloat32, name, " must be float32, got ", img.dtype());
    TORCH_CHECK(img.is_cuda(), name, " must be on a CUDA device");
}
cugs_bilagrid_dims validate_grid(const torch::Tensor& grid, const torch::Device* dev) {
    TORCH_CHECK(grid.dim() == 4 && grid.size(0) == 12, "grid must be [12, L, GY, GX], got ", grid.sizes());
    for (int a = 1; a < 4; ++a)
        TORCH_CHECK(grid.size(a) >= 2 && grid.size(a) <= 64, "grid extents L, GY, GX must lie in [2, 64], got ", grid.sizes());
    TORCH_CHECK(grid.dtype() == torch::kFloat32, "grid must be float32, got ", grid.dtype());
    TORCH_CHECK(grid.is_cuda() && (!dev || grid.device() == *dev), "grid must be on the image's CUDA device");
    TORCH_CHECK(grid.is_contiguous(), "grid must be contiguous");
    cugs_bilagrid_dims d;
    d.l = static_cast<int32_t>(grid.size(1)); d.gy = static_cast<int32_t>(grid.size(2)); d.gx = static_cast<int32_t>(grid.size(3));
    return d;
}
}  // namespace

torch::Tensor bilagrid_slice(const torch::Tensor& grid, const torch::Tensor& rendered) {
    validate_image(rendered, "rendered");
    const auto dev = rendered.device();
    const auto dims = validate_grid(grid, &dev);
    auto r = rendered.contiguous();
    auto out = torch::empty_like(r);
    check(cugs_bilagrid_slice(static_cast<int>(r.size(1)), static_cast<int>(r.size(0)), &dims, ptr<float>(grid), ptr<float>(r),
                              ptr<float>(out), stream_of(r)), "cugs_bilagrid_slice");
    return out;
}

BilagridGrad bilagrid_slice_backward(const torch::Tensor& grid, const torch::Tensor& rendered,
                                     const torch::Tensor& dL_dcorrected, bool want_grid_grad, bool want_image_grad) {
    validate_image(rendered, "rendered");
    validate_image(dL_dcorrected, "dL_dcorrected");
    TORCH_CHECK(dL_dcorrected.sizes() == rendered.sizes(), "dL_dcorrected must have rendered's shape ", rendered.sizes(),
                ", got ", dL_dcorrected.sizes());
    TORCH_CHECK(dL_dcorrected.device() == rendered.device(), "dL_dcorrected must be on rendered's CUDA device");
    const auto dev = rendered.device();
    const auto dims = validate_grid(grid, &dev);
    const int h = static_cast<int>(rendered.size(0)), w = static_cast<int>(rendered.size(1));
    auto r = rendered.contiguous(), g = dL_dcorrected.contiguous();
    BilagridGrad o;
    if (want_image_grad) o.dL_drendered = torch::empty_like(r);
    if (want_grid_grad) o.dL_dgrid = torch::empty_like(grid);
    torch::Tensor ws;
    if (want_grid_grad) ws = workspace(dev, cugs_bilagrid_workspace_bytes(w, h, &dims), 10);
    check(cugs_bilagrid_slice_backward(w, h, &dims, ptr<float>(grid), ptr<float>(r), ptr<float>(g),
                                       ws.defined() ? ws.data_ptr() : nullptr, ws.defined() ? static_cast<size_t>(ws.numel()) : 0,
                                       ptr<float>(o.dL_drendered), ptr<float>(o.dL_dgrid), stream_of(r)),
          "cugs_bilagrid_slice_backward");
    return o;
}

BilagridTV bilagrid_tv(const torch::Tensor& grid, float weight, const torch::Tensor& dL_dgrid) {
    const auto dims = validate_grid(grid, nullptr);
    BilagridTV o;
    const bool accumulate = dL_dgrid.defined();
    if (accumulate) {
        TORCH_CHECK(dL_dgrid.sizes() == grid.sizes() && dL_dgrid.dtype() == torch::kFloat32 && dL_dgrid.device() == grid.device() &&
                    dL_dgrid.is_contiguous(), "dL_dgrid must be a contiguous float32 tensor of the grid's shape and device");
        o.dL_dgrid = dL_dgrid;
    } else {
        o.dL_dgrid = torch::empty_like(grid);
    }
    auto tv = torch::empty({1}, fopt(grid));
    check(cugs_bilagrid_tv(&dims, ptr<float>(grid), weight, ptr<float>(tv), ptr<float>(o.dL_dgrid), accumulate ? 1 : 0,
                           stream_of(grid)), "cugs_bilagrid_tv");
    o.tv = tv[0];
    return o;
}

}  // namespace cugs_hip
