// torch_envmap.cpp — cugs_hip_torch.hpp: the environment-map background (EnvironmentMap, the two composites and their
// backwards, render_with_environment).
#include "torch_glue.hpp"

namespace cugs_hip {

namespace {
constexpr int kEnvWorkspace = 12;      // workspace() kind

void validate_image(const torch::Tensor& img, const char* name) {
    TORCH_CHECK(img.dim() == 3 && img.size(2) == 3, name, " must be [H, W, 3], got ", img.sizes());
    TORCH_CHECK(img.dtype() == torch::kFloat32, name, " must be float32, got ", img.dtype());
    TORCH_CHECK(img.is_cuda(), name, " must be on a CUDA device");
}
void validate_pair(const torch::Tensor& img, const torch::Tensor& final_T, const char* name) {
    validate_image(img, name);
    TORCH_CHECK(final_T.defined() && final_T.is_cuda() && final_T.device() == img.device() &&
                final_T.dtype() == torch::kFloat32 && final_T.dim() == 2 && final_T.size(0) == img.size(0) &&
                final_T.size(1) == img.size(1), "final_T must be a float32 [H, W] tensor of ", name, "'s size and device");
}
void validate_texture(const torch::Tensor& tex, const torch::Device* dev) {
    TORCH_CHECK(tex.dim() == 3 && tex.size(0) == 3 && tex.size(1) == tex.size(2), "the environment map must be [3, R, R], got ",
                tex.sizes());
    const int64_t r = tex.size(1);
    TORCH_CHECK(r >= 4 && r <= 2048 && (r & (r - 1)) == 0,
                "the environment map's resolution must be a power of two in [4, 2048], got ", r);
    TORCH_CHECK(tex.dtype() == torch::kFloat32 && tex.is_cuda() && tex.is_contiguous(),
                "the environment map must be a contiguous float32 tensor on a CUDA device");
    TORCH_CHECK(!dev || tex.device() == *dev, "the environment map must be on the image's CUDA device");
}
void require_zero_background(const RenderSettings* settings, const char* what) {
    if (!settings) return;
    TORCH_CHECK(settings->background[0] == 0.0f && settings->background[1] == 0.0f && settings->background[2] == 0.0f, what,
                ": the render must be made on background (0, 0, 0) - the composite adds the background itself");
}
cugs_envmap_view image_view(const torch::Tensor& img) {
    cugs_envmap_view v{};
    v.width = static_cast<int32_t>(img.size(1));
    v.height = static_cast<int32_t>(img.size(0));
    return v;
}
}  // namespace

EnvironmentMap::EnvironmentMap(int resolution, const torch::Device& device, const float init_color[3],
                               const double* orientation) {
    TORCH_CHECK(resolution >= 4 && resolution <= 2048 && (resolution & (resolution - 1)) == 0,
                "the environment map's resolution must be a power of two in [4, 2048], got ", resolution);
    const auto opt = torch::TensorOptions().dtype(torch::kFloat32).device(device);
    texture_ = torch::zeros({3, resolution, resolution}, opt);
    if (init_color)
        for (int c = 0; c < 3; ++c) texture_[c].fill_(init_color[c]);
    m_ = torch::zeros_like(texture_);
    v_ = torch::zeros_like(texture_);
    orientation_ = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (orientation)
        for (int i = 0; i < 9; ++i) {
            TORCH_CHECK(std::isfinite(orientation[i]), "EnvironmentMap: orientation must be a finite 3x3 matrix");
            orientation_[i] = orientation[i];
        }
}

cugs_envmap_view EnvironmentMap::view(const cugs_camera& camera) const {
    validate_texture(texture_, nullptr);
    cugs_envmap_view v{};
    TORCH_CHECK(cugs_envmap_view_init(&v, &camera, orientation_.data(), resolution()) == 0,
                "EnvironmentMap: the camera needs a positive size, finite positive fx, fy and finite cx, cy and rotation");
    return v;
}

torch::Tensor EnvironmentMap::sample(const cugs_camera& camera) const {
    const auto v = view(camera);
    auto out = torch::empty({camera.height, camera.width, 3}, fopt(texture_));
    check(cugs_envmap_composite(&v, ptr<float>(texture_), nullptr, nullptr, nullptr, nullptr, ptr<float>(out),
                                stream_of(texture_)), "cugs_envmap_composite");
    return out;
}

void EnvironmentMap::step(const torch::Tensor& dL_denv, float lr) {
    TORCH_CHECK(dL_denv.defined() && dL_denv.is_cuda() && dL_denv.device() == texture_.device() &&
                dL_denv.dtype() == torch::kFloat32 && dL_denv.sizes() == texture_.sizes(),
                "EnvironmentMap::step: dL_denv must be a float32 tensor of the texture's shape and device");
    auto g = dL_denv.contiguous();
    const AdamHyper h;
    ++step_count_;
    float bc1, bc2;
    cugs_adam_bias_correction(h.beta1, h.beta2, step_count_, &bc1, &bc2);
    cugs_adam_group group{ptr<float>(texture_), ptr<float>(g), ptr<float>(m_), ptr<float>(v_), texture_.numel(), lr, 0.f};
    check(cugs_fused_adam_groups(&group, 1, h.beta1, h.beta2, h.eps, bc1, bc2, stream_of(texture_)), "cugs_fused_adam_groups");
}

torch::Tensor composite_environment(const RenderOutput& render_out, const cugs_camera& camera, const EnvironmentMap& env,
                                    const RenderSettings* settings) {
    require_zero_background(settings, "composite_environment");
    validate_pair(render_out.color, render_out.final_T, "render_out.color");
    TORCH_CHECK(render_out.color.size(0) == camera.height && render_out.color.size(1) == camera.width,
                "render_out was not made with this camera's image size");
    const auto dev = render_out.color.device();
    validate_texture(env.texture(), &dev);
    const auto v = env.view(camera);
    auto c = render_out.color.contiguous(), t = render_out.final_T.contiguous();
    auto out = torch::empty_like(c);
    check(cugs_envmap_composite(&v, ptr<float>(env.texture()), nullptr, ptr<float>(c), ptr<float>(t), ptr<float>(out), nullptr,
                                stream_of(c)), "cugs_envmap_composite");
    return out;
}

EnvGrad composite_environment_backward(const torch::Tensor& dL_dimage, const RenderOutput& render_out,
                                       const cugs_camera& camera, const EnvironmentMap& env, float grad_bound,
                                       bool want_env_grad, const RenderSettings* settings) {
    require_zero_background(settings, "composite_environment_backward");
    TORCH_CHECK(render_out.final_T.defined() && render_out.depths.defined(),
                "composite_environment_backward: this RenderOutput cannot carry dL_dalpha through render_backward - it "
                "needs final_T and the per-Gaussian depths of render()");
    validate_pair(dL_dimage, render_out.final_T, "dL_dimage");
    TORCH_CHECK(dL_dimage.size(0) == camera.height && dL_dimage.size(1) == camera.width,
                "dL_dimage does not have this camera's image size");
    const auto dev = dL_dimage.device();
    validate_texture(env.texture(), &dev);
    const auto v = env.view(camera);
    auto g = dL_dimage.contiguous(), t = render_out.final_T.contiguous();
    EnvGrad o;
    o.dL_dalpha = torch::empty({camera.height, camera.width}, fopt(g));
    torch::Tensor ws;
    if (want_env_grad) {
        TORCH_CHECK(cugs_envmap_frac_bits(camera.width, camera.height, grad_bound) >= 0,
                    "composite_environment_backward: grad_bound must be finite and in [2^-60, 2^24], got ", grad_bound);
        o.dL_denv = torch::empty_like(env.texture());
        o.clamped = torch::empty({}, iopt(g));
        ws = workspace(dev, cugs_envmap_workspace_bytes(env.resolution()), kEnvWorkspace);
    }
    check(cugs_envmap_composite_backward(&v, ptr<float>(env.texture()), nullptr, ptr<float>(g), ptr<float>(t), grad_bound,
                                         ws.defined() ? ws.data_ptr() : nullptr,
                                         ws.defined() ? static_cast<size_t>(ws.numel()) : 0, ptr<float>(o.dL_dalpha),
                                         ptr<float>(o.dL_denv), nullptr, ptr<int32_t>(o.clamped), stream_of(g)),
          "cugs_envmap_composite_backward");
    return o;
}

torch::Tensor composite_background(const torch::Tensor& color, const torch::Tensor& final_T, const torch::Tensor& background) {
    validate_pair(color, final_T, "color");
    validate_image(background, "background");
    TORCH_CHECK(background.sizes() == color.sizes() && background.device() == color.device(),
                "background must have color's shape ", color.sizes(), " and device");
    const auto v = image_view(color);
    auto c = color.contiguous(), t = final_T.contiguous(), b = background.contiguous();
    auto out = torch::empty_like(c);
    check(cugs_envmap_composite(&v, nullptr, ptr<float>(b), ptr<float>(c), ptr<float>(t), ptr<float>(out), nullptr,
                                stream_of(c)), "cugs_envmap_composite");
    return out;
}

BackgroundGrad composite_background_backward(const torch::Tensor& dL_dimage, const torch::Tensor& final_T,
                                             const torch::Tensor& background, bool want_background_grad) {
    validate_pair(dL_dimage, final_T, "dL_dimage");
    validate_image(background, "background");
    TORCH_CHECK(background.sizes() == dL_dimage.sizes() && background.device() == dL_dimage.device(),
                "background must have dL_dimage's shape ", dL_dimage.sizes(), " and device");
    const auto v = image_view(dL_dimage);
    auto g = dL_dimage.contiguous(), t = final_T.contiguous(), b = background.contiguous();
    BackgroundGrad o;
    o.dL_dalpha = torch::empty({g.size(0), g.size(1)}, fopt(g));
    if (want_background_grad) o.dL_dbackground = torch::empty_like(g);
    check(cugs_envmap_composite_backward(&v, nullptr, ptr<float>(b), ptr<float>(g), ptr<float>(t), 1.0f, nullptr, 0,
                                         ptr<float>(o.dL_dalpha), nullptr, ptr<float>(o.dL_dbackground), nullptr, stream_of(g)),
          "cugs_envmap_composite_backward");
    return o;
}

EnvRender render_with_environment(const ModelTensors& model, const cugs_camera& camera, const RenderSettings& settings,
                                  const EnvironmentMap& env, bool for_backward, bool want_depth_map) {
    require_zero_background(&settings, "render_with_environment");
    EnvRender o;
    o.render_out = render(model, camera, settings, for_backward, want_depth_map);
    o.image = composite_environment(o.render_out, camera, env);
    return o;
}

}  // namespace cugs_hip
