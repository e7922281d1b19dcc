// torch_optim.cpp — cugs_hip_torch.hpp: FusedAdam, DensificationController, MCMCController, pruning and selection.
#include "torch_glue.hpp"

namespace cugs_hip {

FusedAdam::FusedAdam(std::array<torch::Tensor, 5> params, std::array<float, 5> lrs, AdamHyper h)
    : params_(std::move(params)), lrs_(lrs), h_(h) {
    for (int i = 0; i < 5; ++i) { m_[i] = torch::zeros_like(params_[i]); v_[i] = torch::zeros_like(params_[i]); }
}
void FusedAdam::apply_gradients(const BackwardOutput& g) {        // references, no copy (fused_adam.cu:113-120)
    grads_ = {g.dL_dpositions, g.dL_dsh_coeffs, g.dL_dopacities, g.dL_dscales, g.dL_drotations};
}
void FusedAdam::zero_grad() { for (auto& g : grads_) g = torch::Tensor(); }
cugs_adam_fused FusedAdam::begin_fused_step() {
    ++step_count_;
    cugs_adam_fused a{};
    cugs_adam_bias_correction(h_.beta1, h_.beta2, step_count_, &a.bc1, &a.bc2);
    for (int i = 0; i < 5; ++i) {
        TORCH_CHECK(params_[i].is_cuda() && params_[i].is_contiguous() && params_[i].scalar_type() == torch::kFloat32 &&
                    m_[i].is_contiguous() && v_[i].is_contiguous(),
                    "FusedAdam: the fused step needs contiguous float32 CUDA parameters and moments");
        a.m[i] = m_[i].data_ptr<float>(); a.v[i] = v_[i].data_ptr<float>(); a.lr[i] = lrs_[i];
    }
    a.beta1 = h_.beta1; a.beta2 = h_.beta2; a.eps = h_.eps;
    zero_grad();
    return a;
}
void FusedAdam::step() { step_groups(nullptr); }
void FusedAdam::step(const torch::Tensor& visible) {
    const int64_t n_rows = params_[0].size(0);
    TORCH_CHECK(visible.defined() && visible.dim() == 1 && visible.size(0) == n_rows,
                "FusedAdam: visible must be a [N] tensor with N = ", n_rows, " (RenderOutput::radii or a bool mask)");
    TORCH_CHECK(visible.is_cuda() && visible.device() == params_[0].device(),
                "FusedAdam: visible must be on the model's CUDA device");
    TORCH_CHECK(visible.scalar_type() == torch::kInt32 || visible.scalar_type() == torch::kBool,
                "FusedAdam: visible must be int32 radii or a bool mask, got ", visible.dtype());
    const torch::Tensor rows = (visible.scalar_type() == torch::kBool ? visible.to(torch::kInt32) : visible).contiguous();
    step_groups(&rows);
}
void FusedAdam::step_groups(const torch::Tensor* rows) {
    ++step_count_;
    float bc1, bc2;
    cugs_adam_bias_correction(h_.beta1, h_.beta2, step_count_, &bc1, &bc2);
    cugs_adam_group groups[5];
    std::array<torch::Tensor, 5> pc, gc, mc, vc;
    void* st = nullptr;
    for (int i = 0; i < 5; ++i) {
        groups[i] = cugs_adam_group{nullptr, nullptr, nullptr, nullptr, 0, lrs_[i], 0.f};
        if (!grads_[i].defined()) continue;                       // fused_adam.cu:156
        TORCH_CHECK(params_[i].is_cuda(), "FusedAdam: param must be on CUDA");
        TORCH_CHECK(grads_[i].is_cuda(), "FusedAdam: grad must be on CUDA");
        TORCH_CHECK(params_[i].numel() == grads_[i].numel(), "FusedAdam: param/grad size mismatch: ", params_[i].numel(),
                    " vs ", grads_[i].numel());
        pc[i] = params_[i].contiguous(); gc[i] = grads_[i].contiguous(); mc[i] = m_[i].contiguous(); vc[i] = v_[i].contiguous();
        groups[i].param = pc[i].data_ptr<float>(); groups[i].grad = gc[i].data_ptr<float>();
        groups[i].m = mc[i].data_ptr<float>(); groups[i].v = vc[i].data_ptr<float>(); groups[i].n = pc[i].numel();
        st = stream_of(params_[i]);
    }
    if (rows) {
        const int64_t n_rows = rows->size(0);
        int32_t row_elems[5];
        for (int i = 0; i < 5; ++i) {                             // floats per row: 3, 3C, 1, 3, 4
            int64_t w = 1;
            for (int64_t d = 1; d < params_[i].dim(); ++d) w *= params_[i].size(d);
            row_elems[i] = static_cast<int32_t>(w);
        }
        check(cugs_fused_adam_groups_rows(groups, 5, row_elems, rows->data_ptr<int32_t>(), n_rows, h_.beta1, h_.beta2,
                                          h_.eps, bc1, bc2, st), "cugs_fused_adam_groups_rows");
    } else {
        check(cugs_fused_adam_groups(groups, 5, h_.beta1, h_.beta2, h_.eps, bc1, bc2, st), "cugs_fused_adam_groups");
    }
    for (int i = 0; i < 5; ++i) {                                 // fused_adam.cu:216-218
        if (!grads_[i].defined()) continue;
        if (!params_[i].is_contiguous()) params_[i].copy_(pc[i]);
        if (!m_[i].is_contiguous()) m_[i].copy_(mc[i]);
        if (!v_[i].is_contiguous()) v_[i].copy_(vc[i]);
    }
}

// ---------------------------------------------------------------------------------------------
// N2: adaptive density control (optimizer/densification.cpp)
// ---------------------------------------------------------------------------------------------
bool DensificationController::should_densify(int step) const {             // densification.cpp:42-46
    return step >= config_.densify_from && step <= config_.densify_until && step % config_.densify_every == 0;
}
bool DensificationController::should_reset_opacity(int step) const {       // :48-52
    return config_.opacity_reset_every > 0 && step >= config_.densify_from && step % config_.opacity_reset_every == 0;
}
void DensificationController::reset_accumulators(int64_t n, const torch::Device& device) {   // :344-349
    auto o = torch::TensorOptions().dtype(torch::kFloat32).device(device);
    grad_accum_ = torch::zeros({n}, o); grad_count_ = torch::zeros({n}, o); max_radii_2d_ = torch::zeros({n}, o);
}
void DensificationController::accumulate_gradients(const torch::Tensor& dL_dmeans_2d, const torch::Tensor& radii) {
    TORCH_CHECK(dL_dmeans_2d.is_cuda() && radii.is_cuda(), "accumulate_gradients: tensors must be on CUDA");
    TORCH_CHECK(dL_dmeans_2d.dim() == 2 && dL_dmeans_2d.size(1) == 2, "dL_dmeans_2d must be [N, 2]");
    const int64_t n = dL_dmeans_2d.size(0);
    TORCH_CHECK(radii.numel() == n, "radii must be [N]");
    if (!grad_accum_.defined() || grad_accum_.size(0) != n) reset_accumulators(n, dL_dmeans_2d.device());
    auto r = radii.contiguous().to(torch::kInt32);
    // a strided [N,2] view (BackwardOutput::dL_dmeans_2d_abs: words 10, 11 of the accumulator rows) is read in place
    const int64_t row = n > 0 ? dL_dmeans_2d.stride(0) : 2;
    if (dL_dmeans_2d.scalar_type() == torch::kFloat32 && !dL_dmeans_2d.is_contiguous() && dL_dmeans_2d.stride(1) == 1 &&
        row >= 2 && row % 2 == 0 && reinterpret_cast<uintptr_t>(dL_dmeans_2d.data_ptr()) % 8 == 0) {
        check(cugs_densify_accumulate_strided(n, dL_dmeans_2d.data_ptr<float>(), row, ptr<int32_t>(r),
                                              ptr<float>(grad_accum_), ptr<float>(grad_count_), ptr<float>(max_radii_2d_),
                                              stream_of(dL_dmeans_2d)), "cugs_densify_accumulate_strided");
        return;
    }
    auto g = dL_dmeans_2d.contiguous().to(torch::kFloat32);
    check(cugs_densify_accumulate(n, ptr<float>(g), ptr<int32_t>(r), ptr<float>(grad_accum_), ptr<float>(grad_count_),
                                  ptr<float>(max_radii_2d_), stream_of(g)), "cugs_densify_accumulate");
}
void DensificationController::reset_opacity(ModelTensors& model) {          // :331-334
    torch::NoGradGuard no_grad;
    model.opacities.fill_(-4.59511985013459f);
}
DensificationStats DensificationController::densify(ModelTensors& model, int step, const torch::Tensor& noise_in,
                                                    FusedAdam* optimizer) {
    torch::NoGradGuard no_grad;
    DensificationStats stats;
    const int64_t n = model.positions.size(0);
    stats.num_before = stats.num_after = static_cast<int>(n);
    if (n == 0) return stats;
    TORCH_CHECK(model.positions.is_cuda(), "densify: model must be on CUDA");
    const auto dev = model.positions.device();
    if (!grad_accum_.defined() || grad_accum_.size(0) != n) reset_accumulators(n, dev);
    void* st = stream_of(model.positions);
    auto scales_c = model.scales.contiguous(), opa_c = model.opacities.contiguous();
    auto flags = torch::empty({n}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
    auto avg = torch::empty({n}, fopt(model.positions));
    const float size_thr = config_.percent_dense * scene_extent_;           // :367, :394
    const float ws_thr = 0.1f * scene_extent_;                              // :436
    const int size_pruning = config_.opacity_reset_every > 0 && step > config_.opacity_reset_every;   // :415-416
    check(cugs_densify_classify(n, ptr<float>(grad_accum_), ptr<float>(grad_count_), ptr<float>(max_radii_2d_),
                                ptr<float>(scales_c), ptr<float>(opa_c), config_.grad_threshold, size_thr,
                                config_.opacity_threshold, size_pruning, static_cast<float>(config_.max_screen_size),
                                ws_thr, flags.data_ptr<uint8_t>(), ptr<float>(avg), st), "cugs_densify_classify");
    if (config_.max_gaussians > 0) {                                        // :121-139, :184-209 (rare path: libtorch topk)
        auto clone = flags.bitwise_and(1).to(torch::kBool);
        int64_t num_clone = clone.sum().item<int64_t>();
        const int64_t budget = config_.max_gaussians - n;
        if (num_clone > budget) {
            auto keep_clone = torch::zeros_like(clone);
            if (budget > 0) keep_clone.index_fill_(0, std::get<1>(avg.masked_fill(~clone, -1.0f).topk(budget)), true);
            clone = keep_clone;
            num_clone = budget > 0 ? budget : 0;
        }
        auto split = flags.bitwise_right_shift(1).bitwise_and(1).to(torch::kBool);
        const int64_t num_split = split.sum().item<int64_t>();
        const int64_t sbudget = (config_.max_gaussians - (n + num_clone)) / 2;
        if (num_split > sbudget) {
            auto keep_split = torch::zeros_like(split);
            if (sbudget > 0) keep_split.index_fill_(0, std::get<1>(avg.masked_fill(~split, -1.0f).topk(sbudget)), true);
            split = keep_split;
        }
        flags = flags.bitwise_and(4).bitwise_or(clone.to(torch::kUInt8)).bitwise_or(split.to(torch::kUInt8).bitwise_left_shift(1)).contiguous();
    }
    auto ws = workspace(dev, cugs_densify_workspace_bytes(n), 3);
    int64_t counts[4];
    check(cugs_densify_plan(n, flags.data_ptr<uint8_t>(), ws.data_ptr(), ws.numel(), counts, st), "cugs_densify_plan");
    const int64_t n_out = counts[3];
    torch::Tensor noise = noise_in.defined() ? noise_in.contiguous().to(torch::kFloat32)
                                             : (counts[2] > 0 ? torch::randn({2, n, 3}, fopt(model.positions))
                                                              : torch::zeros({2, n, 3}, fopt(model.positions)));
    TORCH_CHECK(noise.is_cuda() && noise.dim() == 3 && noise.size(0) == 2 && noise.size(1) == n && noise.size(2) == 3,
                "noise must be [2, N, 3] on CUDA");
    std::vector<torch::Tensor> srcs, dsts;
    std::vector<cugs_densify_array> desc;
    auto add = [&](const torch::Tensor& src, int mode) {
        auto s = src.contiguous();
        auto sizes = s.sizes().vec();
        sizes[0] = n_out;
        auto d = torch::empty(sizes, fopt(model.positions));
        srcs.push_back(s); dsts.push_back(d);
        desc.push_back(cugs_densify_array{s.data_ptr<float>(), d.data_ptr<float>(), static_cast<int32_t>(s.numel() / n), mode});
        return d;
    };
    auto new_pos = add(model.positions, CUGS_DENSIFY_POSITIONS);
    auto new_sh = add(model.sh_coeffs, CUGS_DENSIFY_COPY);
    auto new_opa = add(model.opacities, CUGS_DENSIFY_COPY);
    auto new_rot = add(model.rotations, CUGS_DENSIFY_COPY);
    auto new_scl = add(model.scales, CUGS_DENSIFY_SCALES);
    std::array<torch::Tensor, 5> nm, nv;
    if (optimizer) for (int i = 0; i < 5; ++i) { nm[i] = add(optimizer->m_[i], CUGS_DENSIFY_STATE); nv[i] = add(optimizer->v_[i], CUGS_DENSIFY_STATE); }
    if (n_out > 0)
        check(cugs_densify_apply(n, n_out, ws.data_ptr(), ws.numel(), ptr<float>(noise), ptr<float>(scales_c), desc.data(),
                                 static_cast<int>(desc.size()), st), "cugs_densify_apply");
    model.positions = new_pos; model.sh_coeffs = new_sh; model.opacities = new_opa; model.rotations = new_rot; model.scales = new_scl;
    if (optimizer) {
        optimizer->params_ = {model.positions, model.sh_coeffs, model.opacities, model.scales, model.rotations};
        optimizer->m_ = nm; optimizer->v_ = nv;
        optimizer->zero_grad();
    }
    stats.num_cloned = static_cast<int>(counts[1]);
    stats.num_split = static_cast<int>(counts[2]);
    stats.num_pruned = static_cast<int>(n + counts[1] + 2 * counts[2] - n_out);   // :313-316
    stats.num_after = static_cast<int>(n_out);
    reset_accumulators(n_out, dev);                                               // :321
    return stats;
}

// ---- N5: MCMC densification (optimizer/mcmc_densification.cpp) ----
namespace {
void check_model(const ModelTensors& m, const char* what) {
    for (const torch::Tensor* t : {&m.positions, &m.sh_coeffs, &m.opacities, &m.rotations, &m.scales})
        TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->is_contiguous(), what,
                    ": the model tensors must be contiguous float32 CUDA tensors (updated in place)");
}
}  // namespace

bool MCMCController::should_relocate(int step) const {                                      // :30-34
    return step >= config_.relocate_from && step <= config_.relocate_until && step % config_.relocate_every == 0;
}

float MCMCController::noise_lr(int step) const {                                             // :40-50
    if (step >= config_.noise_lr_max_steps) return config_.noise_lr_final;
    if (step <= 0) return config_.noise_lr_init;
    const float t = static_cast<float>(step) / static_cast<float>(config_.noise_lr_max_steps);
    const float log_ratio = std::log(config_.noise_lr_final / config_.noise_lr_init);
    return config_.noise_lr_init * std::exp(t * log_ratio);
}

MCMCStats MCMCController::relocate(ModelTensors& model, int step, FusedAdam* optimizer, const torch::Tensor& sources_out) {
    MCMCStats stats;
    const int64_t n = model.positions.defined() ? model.positions.size(0) : 0;
    stats.num_total = static_cast<int>(n);
    if (n == 0) return stats;
    check_model(model, "relocate");
    const auto dev = model.positions.device();
    float* m[5];
    float* v[5];
    if (optimizer) {
        TORCH_CHECK(optimizer->params_[0].data_ptr() == model.positions.data_ptr(),
                    "relocate: the optimizer must have been built on this model");
        for (int g = 0; g < 5; ++g) {
            TORCH_CHECK(optimizer->m_[g].is_contiguous() && optimizer->v_[g].is_contiguous(),
                        "relocate: the optimizer moments must be contiguous");
            m[g] = optimizer->m_[g].data_ptr<float>();
            v[g] = optimizer->v_[g].data_ptr<float>();
        }
    }
    if (sources_out.defined())
        TORCH_CHECK(sources_out.is_cuda() && sources_out.scalar_type() == torch::kInt32 && sources_out.numel() >= n &&
                    sources_out.is_contiguous(), "sources_out must be a contiguous int32 CUDA tensor of N");
    auto ws = workspace(dev, cugs_mcmc_relocate_workspace_bytes(n), 5);
    auto out = torch::zeros({2}, iopt(model.positions));
    check(cugs_mcmc_relocate(n, static_cast<int>(model.sh_coeffs.size(2)), ptr<float>(model.positions),
                             ptr<float>(model.rotations), ptr<float>(model.scales), ptr<float>(model.opacities),
                             ptr<float>(model.sh_coeffs), config_.dead_opacity_threshold, config_.relocate_cap,
                             scene_extent_, config_.seed, static_cast<uint32_t>(step), optimizer ? m : nullptr,
                             optimizer ? v : nullptr, ws.data_ptr(), static_cast<size_t>(ws.numel()), ptr<int32_t>(out),
                             sources_out.defined() ? sources_out.data_ptr<int32_t>() : nullptr,
                             stream_of(model.positions)),
          "cugs_mcmc_relocate");
    auto host = out.to(torch::kCPU);
    stats.num_dead = host[0].item<int>();
    stats.num_relocated = host[1].item<int>();
    return stats;
}

void MCMCController::inject_noise(ModelTensors& model, int step, const torch::Tensor& noise_in) const {   // :144-161
    const int64_t n = model.positions.defined() ? model.positions.size(0) : 0;
    if (n == 0) return;
    check_model(model, "inject_noise");
    torch::Tensor noise;
    if (noise_in.defined()) {
        TORCH_CHECK(noise_in.is_cuda() && noise_in.dim() == 2 && noise_in.size(0) == n && noise_in.size(1) == 3,
                    "noise must be [N, 3] on CUDA");
        noise = f32c(noise_in);
    }
    check(cugs_mcmc_inject_noise(n, ptr<float>(model.positions), ptr<float>(model.scales), ptr<float>(model.opacities),
                                 noise_lr(step), config_.noise_gate_k, config_.noise_gate_t,
                                 noise.defined() ? ptr<float>(noise) : nullptr, config_.seed, static_cast<uint32_t>(step),
                                 stream_of(model.positions)),
          "cugs_mcmc_inject_noise");
}

torch::Tensor MCMCController::compute_regularization(const ModelTensors& model, torch::Tensor& reg_dL_dopacities,
                                                     torch::Tensor& reg_dL_dscales) const {     // :167-186
    const int64_t n = model.positions.size(0);
    auto value = torch::zeros({}, fopt(model.positions));
    reg_dL_dopacities = torch::empty({n, 1}, fopt(model.positions));
    reg_dL_dscales = torch::empty({n, 3}, fopt(model.positions));
    if (n == 0) return value;
    auto opa = f32c(model.opacities), scl = f32c(model.scales);
    auto ws = workspace(model.positions.device(), cugs_mcmc_relocate_workspace_bytes(0), 6);
    check(cugs_mcmc_regularization(n, ptr<float>(opa), ptr<float>(scl), config_.lambda_opacity, config_.lambda_scale,
                                   nullptr, nullptr, ptr<float>(reg_dL_dopacities), ptr<float>(reg_dL_dscales),
                                   ptr<float>(value), ws.data_ptr(), static_cast<size_t>(ws.numel()),
                                   stream_of(model.positions)),
          "cugs_mcmc_regularization");
    return value;
}

cugs_mcmc_fused MCMCController::fused_args(int step, const torch::Tensor& noise) const {
    cugs_mcmc_fused a{};
    a.lambda_opacity = config_.lambda_opacity; a.lambda_scale = config_.lambda_scale;
    a.noise_lr = noise_lr(step); a.gate_k = config_.noise_gate_k; a.gate_t = config_.noise_gate_t;
    a.step = static_cast<uint32_t>(step); a.seed = config_.seed;
    a.noise = noise.defined() ? noise.data_ptr<float>() : nullptr;
    return a;
}

int64_t prune_gaussians(ModelTensors& model, const torch::Tensor& prune_mask, FusedAdam* optimizer) {
    torch::NoGradGuard no_grad;
    const int64_t n = model.positions.size(0);
    TORCH_CHECK(model.positions.is_cuda(), "prune_gaussians: model must be on CUDA");
    TORCH_CHECK(prune_mask.defined() && prune_mask.scalar_type() == torch::kBool && prune_mask.dim() == 1 &&
                prune_mask.size(0) == n, "prune_gaussians: prune_mask must be a bool tensor of shape [", n, "]");
    TORCH_CHECK(prune_mask.device() == model.positions.device(), "prune_gaussians: prune_mask must be on the model's device");
    if (n == 0) return 0;
    const auto dev = model.positions.device();
    void* st = stream_of(model.positions);
    auto flags = prune_mask.logical_not().to(torch::kUInt8).bitwise_left_shift(2).contiguous();   // bit 2: keep
    auto ws = workspace(dev, cugs_densify_workspace_bytes(n), 3);
    int64_t counts[4];
    check(cugs_densify_plan(n, flags.data_ptr<uint8_t>(), ws.data_ptr(), ws.numel(), counts, st), "cugs_densify_plan");
    const int64_t n_out = counts[3];
    if (n_out == n) return 0;
    std::vector<torch::Tensor> srcs, dsts;
    std::vector<cugs_densify_array> desc;
    auto add = [&](const torch::Tensor& src, int mode) {
        auto s = src.contiguous();
        auto sizes = s.sizes().vec();
        sizes[0] = n_out;
        auto d = torch::empty(sizes, fopt(model.positions));
        srcs.push_back(s); dsts.push_back(d);
        desc.push_back(cugs_densify_array{s.data_ptr<float>(), d.data_ptr<float>(), static_cast<int32_t>(s.numel() / n), mode});
        return d;
    };
    auto new_pos = add(model.positions, CUGS_DENSIFY_COPY), new_sh = add(model.sh_coeffs, CUGS_DENSIFY_COPY);
    auto new_opa = add(model.opacities, CUGS_DENSIFY_COPY), new_rot = add(model.rotations, CUGS_DENSIFY_COPY);
    auto new_scl = add(model.scales, CUGS_DENSIFY_COPY);
    std::array<torch::Tensor, 5> nm, nv;
    if (optimizer) for (int i = 0; i < 5; ++i) { nm[i] = add(optimizer->m_[i], CUGS_DENSIFY_STATE); nv[i] = add(optimizer->v_[i], CUGS_DENSIFY_STATE); }
    if (n_out > 0)
        check(cugs_densify_apply(n, n_out, ws.data_ptr(), ws.numel(), nullptr, nullptr, desc.data(),
                                 static_cast<int>(desc.size()), st), "cugs_densify_apply");
    model.positions = new_pos; model.sh_coeffs = new_sh; model.opacities = new_opa; model.rotations = new_rot; model.scales = new_scl;
    if (optimizer) {
        optimizer->params_ = {model.positions, model.sh_coeffs, model.opacities, model.scales, model.rotations};
        optimizer->m_ = nm; optimizer->v_ = nv;
        optimizer->zero_grad();
    }
    return n - n_out;
}

int64_t prune_by_scores(ModelTensors& model, const ContributionScores& scores, float min_max_weight, float keep_fraction,
                        FusedAdam* optimizer) {
    const int64_t n = model.positions.size(0);
    TORCH_CHECK(scores.n() == n, "prune_by_scores: the table holds ", scores.n(), " Gaussians, the model ", n);
    TORCH_CHECK(min_max_weight >= 0.0f || keep_fraction >= 0.0f, "prune_by_scores: give min_max_weight, keep_fraction or both");
    if (n == 0) return 0;
    TORCH_CHECK(scores.table.device() == model.positions.device(), "prune_by_scores: the score table is on another device");
    const auto wmax = scores.weight_max();
    auto mask = wmax.eq(0.0f);
    if (min_max_weight >= 0.0f) mask = mask.logical_or(wmax.lt(min_max_weight));
    if (keep_fraction >= 0.0f) {
        TORCH_CHECK(keep_fraction <= 1.0f, "prune_by_scores: keep_fraction must lie in [0, 1]");
        const int64_t keep = std::llround(static_cast<double>(keep_fraction) * static_cast<double>(n));
        auto drop = torch::ones({n}, torch::TensorOptions().dtype(torch::kBool).device(mask.device()));
        if (keep > 0) drop.index_fill_(0, std::get<1>(scores.weight_sum().topk(keep)), false);
        mask = mask.logical_or(drop);
    }
    return prune_gaussians(model, mask, optimizer);
}

int64_t select_gaussians(ModelTensors& model, const torch::Tensor& keep_mask, FusedAdam* optimizer) {
    TORCH_CHECK(keep_mask.defined() && keep_mask.scalar_type() == torch::kBool, "select_gaussians: keep_mask must be a bool tensor");
    prune_gaussians(model, keep_mask.logical_not(), optimizer);
    return model.positions.size(0);
}

}  // namespace cugs_hip
