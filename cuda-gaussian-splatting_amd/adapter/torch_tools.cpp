// torch_tools.cpp — cugs_hip_torch.hpp: TSDF fusion and mesh extraction, contribution scores, lifted pixel maps, the
// similarity transform and vector quantisation.
#include "torch_glue.hpp"

namespace cugs_hip {

TsdfVolume make_tsdf_volume(const float origin[3], int nx, int ny, int nz, float voxel_size, float trunc, bool color,
                            const torch::Device& device, float max_weight, float min_depth) {
    TORCH_CHECK(nx > 0 && ny > 0 && nz > 0, "the voxel counts must be positive, got ", nx, ", ", ny, ", ", nz);
    TORCH_CHECK(static_cast<int64_t>(nx) * ny * nz <= 2147483647ll, "the volume does not fit 2^31 - 1 voxels");
    TORCH_CHECK(device.is_cuda(), "a TsdfVolume lives on a CUDA device");
    TsdfVolume v;
    v.planes = torch::zeros({color ? 5 : 2, nz, ny, nx}, torch::TensorOptions().dtype(torch::kFloat32).device(device));
    v.planes[0].fill_(1.0f);
    for (int k = 0; k < 3; ++k) v.origin[k] = origin[k];
    v.voxel_size = voxel_size; v.trunc = trunc; v.max_weight = max_weight; v.min_depth = min_depth;
    return v;
}

static cugs_tsdf_volume tsdf_abi(const TsdfVolume& volume) {
    const auto& p = volume.planes;
    TORCH_CHECK(p.defined() && p.dim() == 4 && (p.size(0) == 2 || p.size(0) == 5), "planes must be [2 or 5, nz, ny, nx]");
    TORCH_CHECK(p.dtype() == torch::kFloat32 && p.is_cuda() && p.is_contiguous(), "planes must be contiguous float32 on a CUDA device");
    cugs_tsdf_volume v{};
    v.planes = p.data_ptr<float>();
    v.nx = static_cast<int32_t>(p.size(3)); v.ny = static_cast<int32_t>(p.size(2)); v.nz = static_cast<int32_t>(p.size(1));
    v.color = p.size(0) == 5;
    for (int k = 0; k < 3; ++k) v.origin[k] = volume.origin[k];
    v.voxel_size = volume.voxel_size; v.trunc = volume.trunc;
    return v;
}

void tsdf_integrate(TsdfVolume& volume, const std::vector<TsdfViewInput>& views, float min_alpha) {
    const cugs_tsdf_volume vol = tsdf_abi(volume);
    TORCH_CHECK(min_alpha > 0.0f && std::isfinite(min_alpha), "min_alpha must be positive and finite, got ", min_alpha);
    cugs_tsdf_opts opts{};
    opts.min_depth = volume.min_depth; opts.min_alpha = min_alpha; opts.max_weight = volume.max_weight;
    constexpr size_t kMaxViews = 16;
    for (size_t first = 0; first < views.size(); first += kMaxViews) {
        const size_t n = std::min(kMaxViews, views.size() - first);
        std::vector<cugs_tsdf_view> table(n);
        std::vector<torch::Tensor> keep;                     // the contiguous maps, alive until the launch is queued
        for (size_t i = 0; i < n; ++i) {
            const TsdfViewInput& in = views[first + i];
            const int64_t h = in.camera.height, w = in.camera.width;
            auto map = [&](const torch::Tensor& t, const char* name, bool rgb) -> const float* {
                TORCH_CHECK(t.defined() && t.dim() == (rgb ? 3 : 2) && t.size(0) == h && t.size(1) == w && (!rgb || t.size(2) == 3),
                            name, " must be [H, W", rgb ? ", 3" : "", "] of the view's camera, got ", t.sizes());
                TORCH_CHECK(t.dtype() == torch::kFloat32, name, " must be float32, got ", t.dtype());
                TORCH_CHECK(t.is_cuda() && t.device() == volume.planes.device(), name, " must be on the volume's device");
                keep.push_back(t.contiguous());
                return keep.back().data_ptr<float>();
            };
            cugs_tsdf_view& v = table[i];
            v.camera = in.camera;
            v.depth_map = map(in.depth_map, "depth_map", false);
            v.alpha = map(in.alpha, "alpha", false);
            v.color = volume.has_color() ? map(in.color, "color", true) : nullptr;
            v.weight = in.weight.defined() ? map(in.weight, "weight", false) : nullptr;
        }
        check(cugs_tsdf_integrate(&vol, table.data(), static_cast<int>(n), &opts, stream_of(volume.planes)), "cugs_tsdf_integrate");
    }
}

Mesh mesh_extract(const TsdfVolume& volume, float min_weight) {
    const cugs_tsdf_volume vol = tsdf_abi(volume);
    TORCH_CHECK(min_weight >= 0.0f && std::isfinite(min_weight), "min_weight must be non-negative and finite, got ", min_weight);
    const auto dev = volume.planes.device();
    const size_t bytes = std::max<size_t>(cugs_mesh_workspace_bytes(vol.nx, vol.ny, vol.nz), 256);
    auto ws = torch::empty({static_cast<int64_t>(bytes)}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
    int64_t counts[2] = {0, 0};
    check(cugs_mesh_plan(&vol, min_weight, ws.data_ptr(), bytes, counts, stream_of(volume.planes)), "cugs_mesh_plan");
    Mesh m;
    m.vertices = torch::empty({counts[0], 3}, fopt(volume.planes));
    m.faces = torch::empty({counts[1], 3}, torch::TensorOptions().dtype(torch::kInt32).device(dev));
    if (volume.has_color()) m.colors = torch::empty({counts[0], 3}, fopt(volume.planes));
    check(cugs_mesh_emit(&vol, ws.data_ptr(), bytes, counts[0], counts[1], ptr<float>(m.vertices), ptr<float>(m.colors),
                         ptr<int32_t>(m.faces), stream_of(volume.planes)), "cugs_mesh_emit");
    return m;
}

// ---- contribution scores and score-based pruning ----
ContributionScores::ContributionScores(int64_t n, const torch::Device& device)
    : table(torch::zeros({n, 4}, torch::TensorOptions().dtype(torch::kInt32).device(device))) {}
torch::Tensor ContributionScores::weight_sum() const { return table.view(torch::kFloat32).select(1, 0); }
torch::Tensor ContributionScores::weight_max() const { return table.view(torch::kFloat32).select(1, 1); }
torch::Tensor ContributionScores::pixel_count() const {
    return table.select(1, 2).to(torch::kInt64).bitwise_and(static_cast<int64_t>(0xFFFFFFFFll));
}
void ContributionScores::reset() { table.zero_(); num_views = 0; }

namespace {
void launch_scores(ContributionScores& scores, int width, int height, const torch::Tensor& tile_ranges,
                   const torch::Tensor& gaussian_indices, const torch::Tensor& means_2d, const torch::Tensor& cov_2d_inv,
                   const torch::Tensor& opacities_act, const torch::Tensor& packed, const torch::Tensor& tile_order) {
    auto tr = tile_ranges.contiguous(), gi = gaussian_indices.contiguous();
    auto m = means_2d.contiguous(), c = cov_2d_inv.contiguous(), op = opacities_act.contiguous();
    auto pk = packed.defined() ? packed.contiguous() : packed;
    if (tile_order.defined())
        TORCH_CHECK(tile_order.is_contiguous() && tile_order.scalar_type() == torch::kInt32 &&
                    tile_order.numel() == 4 * tr.size(0), "tile_order must be a contiguous [tiles, 4] int32 tensor");
    check(cugs_blend_scores(width, height, ptr<int32_t>(tr), ptr<int32_t>(gi), ptr<float>(m), ptr<float>(c), ptr<float>(op),
                            ptr<float>(pk), order_ptr(tile_order), static_cast<int>(scores.n()),
                            scores.n() > 0 ? scores.table.data_ptr() : nullptr, stream_of(scores.table)),
          "cugs_blend_scores");
    ++scores.num_views;
}
}  // namespace

void accumulate_contribution_scores(ContributionScores& scores, const RenderOutput& out, const cugs_camera& camera) {
    const int64_t n = out.means_2d.size(0);
    TORCH_CHECK(n == scores.n(), "accumulate_contribution_scores: the table holds ", scores.n(), " Gaussians, the render ", n);
    if (n == 0) { ++scores.num_views; return; }
    TORCH_CHECK(out.means_2d.device() == scores.table.device(), "accumulate_contribution_scores: the score table is on another device");
    launch_scores(scores, camera.width, camera.height, out.tile_ranges, out.gaussian_indices, out.means_2d, out.cov_2d_inv,
                  out.opacities_act, out.packed, out.tile_order);
}

ContributionScores contribution_scores(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                                       const RenderSettings& settings) {
    TORCH_CHECK(model.positions.is_cuda(), "GaussianModel must be on CUDA device");
    const int64_t n = model.positions.size(0);
    ContributionScores scores(n, model.positions.device());
    for (const auto& cam : cameras) {
        if (n == 0) { ++scores.num_views; continue; }
        auto proj = project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam,
                                      0, settings.scale_modifier);             // degree 0: the colour is not used
        auto srt = sort_gaussians(proj.means_2d, proj.depths, proj.radii, proj.tiles_touched, cam.width, cam.height);
        launch_scores(scores, cam.width, cam.height, srt.tile_ranges, srt.gaussian_values_sorted, proj.means_2d,
                      proj.cov_2d_inv, proj.opacities_act, proj.packed, {});
    }
    return scores;
}

// ---- pixel maps lifted onto Gaussians ----
LiftedMaps::LiftedMaps(int64_t n, const torch::Device& device, int channels_)
    : table(torch::zeros({n, 4}, torch::TensorOptions().dtype(torch::kFloat32).device(device))), channels(channels_) {
    TORCH_CHECK(channels >= 1 && channels <= 4, "LiftedMaps: channels must be 1..4");
}
torch::Tensor LiftedMaps::sums() const { return table.narrow(1, 0, channels); }
void LiftedMaps::reset() { table.zero_(); num_views = 0; }

namespace {
// the validated, contiguous map of one launch: exactly one of the two comes back defined
std::pair<torch::Tensor, torch::Tensor> lift_map_args(const LiftedMaps& lifted, int width, int height,
                                                      const torch::Tensor& maps, const torch::Tensor& labels,
                                                      const char* what) {
    TORCH_CHECK(maps.defined() != labels.defined(), what, ": give exactly one of maps and labels");
    if (maps.defined()) {
        TORCH_CHECK(maps.device() == lifted.table.device() && maps.scalar_type() == torch::kFloat32, what,
                    ": maps must be a float32 tensor on the table's device");
        const bool ok = (maps.dim() == 3 && maps.size(0) == height && maps.size(1) == width && maps.size(2) == lifted.channels) ||
                        (lifted.channels == 1 && maps.dim() == 2 && maps.size(0) == height && maps.size(1) == width);
        TORCH_CHECK(ok, what, ": maps must be [", height, ", ", width, ", ", lifted.channels, "]");
        return {maps.contiguous(), torch::Tensor()};
    }
    TORCH_CHECK(labels.device() == lifted.table.device() && labels.scalar_type() == torch::kInt32, what,
                ": labels must be an int32 tensor on the table's device");
    TORCH_CHECK(labels.dim() == 2 && labels.size(0) == height && labels.size(1) == width, what, ": labels must be [",
                height, ", ", width, "]");
    return {torch::Tensor(), labels.contiguous()};
}

void launch_lift(LiftedMaps& lifted, int width, int height, const torch::Tensor& tile_ranges,
                 const torch::Tensor& gaussian_indices, const torch::Tensor& means_2d, const torch::Tensor& cov_2d_inv,
                 const torch::Tensor& opacities_act, const torch::Tensor& packed, const torch::Tensor& tile_order,
                 const torch::Tensor& maps, const torch::Tensor& labels, int label_base) {
    auto tr = tile_ranges.contiguous(), gi = gaussian_indices.contiguous();
    auto m = means_2d.contiguous(), c = cov_2d_inv.contiguous(), op = opacities_act.contiguous();
    auto pk = packed.defined() ? packed.contiguous() : packed;
    if (tile_order.defined())
        TORCH_CHECK(tile_order.is_contiguous() && tile_order.scalar_type() == torch::kInt32 &&
                    tile_order.numel() == 4 * tr.size(0), "tile_order must be a contiguous [tiles, 4] int32 tensor");
    check(cugs_blend_lift(width, height, ptr<int32_t>(tr), ptr<int32_t>(gi), ptr<float>(m), ptr<float>(c), ptr<float>(op),
                          ptr<float>(pk), order_ptr(tile_order), static_cast<int>(lifted.n()), ptr<float>(maps),
                          ptr<int32_t>(labels), lifted.channels, label_base,
                          lifted.n() > 0 ? lifted.table.data_ptr() : nullptr, stream_of(lifted.table)),
          "cugs_blend_lift");
    ++lifted.num_views;
}

// projection at SH degree 0 (the colour is not used), the plain sort (one host sync) and the lift launch
struct SortedView { ProjectionOutput proj; SortingOutput srt; };
SortedView sorted_view(const ModelTensors& model, const cugs_camera& cam, const RenderSettings& settings) {
    auto proj = project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam,
                                  0, settings.scale_modifier);
    auto srt = sort_gaussians(proj.means_2d, proj.depths, proj.radii, proj.tiles_touched, cam.width, cam.height);
    return {proj, srt};
}
void launch_lift_sorted(LiftedMaps& lifted, const cugs_camera& cam, const SortedView& v, const torch::Tensor& maps,
                        const torch::Tensor& labels, int label_base) {
    launch_lift(lifted, cam.width, cam.height, v.srt.tile_ranges, v.srt.gaussian_values_sorted, v.proj.means_2d,
                v.proj.cov_2d_inv, v.proj.opacities_act, v.proj.packed, {}, maps, labels, label_base);
}
}  // namespace

void lift_pixel_maps(LiftedMaps& lifted, const RenderOutput& out, const cugs_camera& camera, const torch::Tensor& maps,
                     const torch::Tensor& labels, int label_base) {
    const int64_t n = out.means_2d.size(0);
    TORCH_CHECK(n == lifted.n(), "lift_pixel_maps: the table holds ", lifted.n(), " Gaussians, the render ", n);
    auto args = lift_map_args(lifted, camera.width, camera.height, maps, labels, "lift_pixel_maps");
    if (n == 0) { ++lifted.num_views; return; }
    TORCH_CHECK(out.means_2d.device() == lifted.table.device(), "lift_pixel_maps: the table is on another device");
    launch_lift(lifted, camera.width, camera.height, out.tile_ranges, out.gaussian_indices, out.means_2d, out.cov_2d_inv,
                out.opacities_act, out.packed, out.tile_order, args.first, args.second, label_base);
}

LiftedMaps lift_maps(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                     const std::vector<torch::Tensor>& maps_per_view, const RenderSettings& settings, int channels) {
    TORCH_CHECK(model.positions.is_cuda(), "GaussianModel must be on CUDA device");
    TORCH_CHECK(maps_per_view.size() == cameras.size(), "lift_maps: one map per camera");
    if (channels <= 0)
        channels = (maps_per_view.empty() || maps_per_view[0].dim() == 2) ? 1 : static_cast<int>(maps_per_view[0].size(2));
    const int64_t n = model.positions.size(0);
    LiftedMaps lifted(n, model.positions.device(), channels);
    for (size_t i = 0; i < cameras.size(); ++i) {
        const auto& cam = cameras[i];
        auto args = lift_map_args(lifted, cam.width, cam.height, maps_per_view[i], {}, "lift_maps");
        if (n == 0) { ++lifted.num_views; continue; }
        launch_lift_sorted(lifted, cam, sorted_view(model, cam, settings), args.first, {}, 0);
    }
    return lifted;
}

std::pair<torch::Tensor, torch::Tensor> vote_labels(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                                                    const std::vector<torch::Tensor>& label_maps, int num_labels,
                                                    const RenderSettings& settings) {
    TORCH_CHECK(model.positions.is_cuda(), "GaussianModel must be on CUDA device");
    TORCH_CHECK(label_maps.size() == cameras.size(), "vote_labels: one map per camera");
    TORCH_CHECK(num_labels >= 1, "vote_labels: num_labels must be positive");
    const int64_t n = model.positions.size(0);
    std::vector<LiftedMaps> windows;
    for (int base = 0; base < num_labels; base += 4)
        windows.emplace_back(n, model.positions.device(), std::min(4, num_labels - base));
    for (size_t i = 0; i < cameras.size(); ++i) {
        const auto& cam = cameras[i];
        auto args = lift_map_args(windows[0], cam.width, cam.height, {}, label_maps[i], "vote_labels");
        if (n == 0) continue;
        const auto view = sorted_view(model, cam, settings);
        for (size_t k = 0; k < windows.size(); ++k)
            launch_lift_sorted(windows[k], cam, view, {}, args.second, static_cast<int>(4 * k));
    }
    std::vector<torch::Tensor> parts;
    for (const auto& win : windows) parts.push_back(win.sums());
    auto votes = torch::cat(parts, 1);
    auto labels = votes.argmax(1);
    auto top = votes.gather(1, labels.unsqueeze(1)).squeeze(1);
    labels = torch::where(top.gt(0.0f), labels, torch::full_like(labels, -1));
    return {labels, votes};
}

torch::Tensor error_scores(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                           const std::vector<torch::Tensor>& error_maps, const RenderSettings& settings,
                           bool max_over_views) {
    TORCH_CHECK(model.positions.is_cuda(), "GaussianModel must be on CUDA device");
    TORCH_CHECK(error_maps.size() == cameras.size(), "error_scores: one map per camera");
    const int64_t n = model.positions.size(0);
    LiftedMaps scratch(n, model.positions.device(), 1);
    auto out = torch::zeros({n}, fopt(model.positions));
    for (size_t i = 0; i < cameras.size(); ++i) {
        const auto& cam = cameras[i];
        auto args = lift_map_args(scratch, cam.width, cam.height, error_maps[i], {}, "error_scores");
        if (n == 0) continue;
        if (max_over_views) scratch.reset();
        launch_lift_sorted(scratch, cam, sorted_view(model, cam, settings), args.first, {}, 0);
        if (max_over_views) out = torch::maximum(out, scratch.sums().select(1, 0));
    }
    if (!max_over_views) out.copy_(scratch.sums().select(1, 0));
    return out;
}

// ---- a model moved by a similarity ----
Similarity Similarity::inverse() const {
    Similarity o;
    o.scale = 1.0 / scale;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o.rotation[3 * i + j] = rotation[3 * j + i];
    for (int i = 0; i < 3; ++i) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc += o.rotation[3 * i + j] * translation[j];
        o.translation[i] = -acc / scale;
    }
    return o;
}

Similarity Similarity::compose(const Similarity& other) const {
    Similarity o;
    o.scale = scale * other.scale;
    for (int i = 0; i < 3; ++i) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) {
            double r = 0.0;
            for (int k = 0; k < 3; ++k) r += rotation[3 * i + k] * other.rotation[3 * k + j];
            o.rotation[3 * i + j] = r;
            acc += rotation[3 * i + j] * other.translation[j];
        }
        o.translation[i] = scale * acc + translation[i];
    }
    return o;
}

std::array<double, 16> Similarity::matrix() const {
    std::array<double, 16> m{};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m[4 * i + j] = scale * rotation[3 * i + j];
        m[4 * i + 3] = translation[i];
    }
    m[15] = 1.0;
    return m;
}

bool Similarity::is_pure_translation() const {
    for (int i = 0; i < 9; ++i)
        if (rotation[i] != ((i % 4 == 0) ? 1.0 : 0.0)) return false;
    return scale == 1.0;
}

CugsSimilarity Similarity::to_abi() const {
    CugsSimilarity xf;
    TORCH_CHECK(cugs_similarity_init(&xf, rotation.data(), translation.data(), scale) == 0,
                "Similarity: the rotation must be a proper rotation (within 1e-4 of orthogonal, det > 0), the scale "
                "positive and every value finite");
    return xf;
}

void transform_gaussians(ModelTensors& model, const Similarity& sim, const torch::Tensor& mask, FusedAdam* optimizer) {
    const int64_t n = model.positions.size(0);
    TORCH_CHECK(model.positions.is_cuda(), "transform_gaussians: model must be on CUDA");
    const int64_t coeffs = model.sh_coeffs.size(2);
    TORCH_CHECK(coeffs == 1 || coeffs == 4 || coeffs == 9 || coeffs == 16, "transform_gaussians: sh_coeffs has ", coeffs,
                " coefficients, not 1, 4, 9 or 16");
    for (const torch::Tensor* t : {&model.positions, &model.rotations, &model.scales, &model.sh_coeffs})
        TORCH_CHECK(t->scalar_type() == torch::kFloat32 && t->is_contiguous() && t->size(0) == n,
                    "transform_gaussians: the model's tensors must be contiguous float32 [N, ...] (the update is in place)");
    torch::Tensor bytes;
    if (mask.defined()) {
        TORCH_CHECK(mask.scalar_type() == torch::kBool && mask.dim() == 1 && mask.size(0) == n,
                    "transform_gaussians: mask must be a bool tensor of shape [", n, "]");
        TORCH_CHECK(mask.device() == model.positions.device(), "transform_gaussians: mask must be on the model's device");
        bytes = mask.contiguous().view(torch::kUInt8);
    }
    const CugsSimilarity xf = sim.to_abi();
    std::vector<float*> zero;
    std::vector<int> floats;
    if (optimizer && !sim.is_pure_translation() && n > 0)
        for (int g : {0, 1, 4})                                      // positions, SH, rotations
            for (const torch::Tensor* t : {&optimizer->m_[g], &optimizer->v_[g]}) {
                TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->is_contiguous() && t->size(0) == n,
                            "transform_gaussians: the optimizer's moments must be contiguous float32 [N, ...]");
                zero.push_back(t->data_ptr<float>());
                floats.push_back(static_cast<int>(t->numel() / n));
            }
    if (n == 0) return;
    check(cugs_transform_gaussians(n, static_cast<int>(coeffs), ptr<float>(model.positions), ptr<float>(model.rotations),
                                   ptr<float>(model.scales), ptr<float>(model.sh_coeffs), ptr<uint8_t>(bytes), zero.data(),
                                   floats.data(), static_cast<int>(zero.size()), &xf, stream_of(model.positions)),
          "cugs_transform_gaussians");
}

cugs_camera transform_camera(const cugs_camera& camera, const Similarity& sim) {
    cugs_camera out = camera;
    double Rn[9], tn[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) acc += static_cast<double>(camera.view[4 * i + k]) * sim.rotation[3 * j + k];
            Rn[3 * i + j] = acc;                                     // Rc R^T
        }
    for (int i = 0; i < 3; ++i) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc += Rn[3 * i + j] * sim.translation[j];
        tn[i] = sim.scale * static_cast<double>(camera.view[4 * i + 3]) - acc;
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out.view[4 * i + j] = static_cast<float>(Rn[3 * i + j]);
        out.view[4 * i + 3] = static_cast<float>(tn[i]);
    }
    for (int i = 0; i < 3; ++i) {                                    // C = -R^T t of the stored float values
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc += static_cast<double>(out.view[4 * j + i]) * static_cast<double>(out.view[4 * j + 3]);
        out.cam_center[i] = static_cast<float>(-acc);
    }
    return out;
}

int64_t merge_gaussians(ModelTensors& model, const ModelTensors& other, FusedAdam* optimizer) {
    torch::NoGradGuard no_grad;
    TORCH_CHECK(other.positions.device() == model.positions.device(), "merge_gaussians: the models are on different devices");
    const int64_t coeffs = std::max(model.sh_coeffs.size(2), other.sh_coeffs.size(2));
    const int64_t n_new = other.positions.size(0);
    auto pad = [&](const torch::Tensor& t) {
        if (t.size(2) == coeffs) return t;
        auto out = torch::zeros({t.size(0), 3, coeffs}, t.options());
        out.slice(2, 0, t.size(2)).copy_(t);
        return out;
    };
    auto join = [](const torch::Tensor& a, const torch::Tensor& b) { return torch::cat({a, b.to(a.scalar_type())}, 0).contiguous(); };
    model.positions = join(model.positions, other.positions);
    model.sh_coeffs = join(pad(model.sh_coeffs), pad(other.sh_coeffs));
    model.opacities = join(model.opacities, other.opacities);
    model.rotations = join(model.rotations, other.rotations);
    model.scales = join(model.scales, other.scales);
    if (optimizer) {
        optimizer->params_ = {model.positions, model.sh_coeffs, model.opacities, model.scales, model.rotations};
        for (int g = 0; g < 5; ++g)
            for (auto* moments : {&optimizer->m_, &optimizer->v_}) {
                auto old = g == 1 ? pad((*moments)[g]) : (*moments)[g];
                auto sizes = old.sizes().vec();
                sizes[0] = n_new;
                (*moments)[g] = torch::cat({old, torch::zeros(sizes, old.options())}, 0).contiguous();
            }
        optimizer->zero_grad();
    }
    return model.positions.size(0);
}

// ---- vector quantisation ----
namespace {
torch::Tensor vq_rows(const torch::Tensor& x, const char* what) {
    TORCH_CHECK(x.defined() && x.dim() == 2, what, " must be a 2-D tensor");
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kFloat32, what, " must be float32 on a CUDA device");
    TORCH_CHECK(x.size(1) >= 1 && x.size(1) <= 48, what, ": 1 <= d <= 48, got ", x.size(1));
    if (x.size(0) <= 1 || x.stride(1) != 1 || x.stride(0) < x.size(1)) return x.contiguous();
    return x;
}
int64_t vq_ldx(const torch::Tensor& x) { return x.size(0) > 1 ? x.stride(0) : x.size(1); }
torch::Tensor vq_workspace(int64_t k, int64_t d, const torch::Tensor& like) {
    const size_t bytes = cugs_vq_workspace_bytes(static_cast<int>(k), static_cast<int>(d));
    TORCH_CHECK(bytes > 0, "vq: no workspace for k = ", k, ", d = ", d);
    return torch::empty({static_cast<int64_t>(bytes)}, torch::TensorOptions().dtype(torch::kUInt8).device(like.device()));
}
void vq_assign_into(const torch::Tensor& x, const torch::Tensor& codebook, torch::Tensor& assign, torch::Tensor* dist,
                    torch::Tensor& ws) {
    check(cugs_vq_assign(x.size(0), static_cast<int>(x.size(1)), static_cast<int>(codebook.size(0)), ptr<float>(x), vq_ldx(x),
                         ptr<float>(codebook), ptr<int32_t>(assign), dist ? ptr<float>(*dist) : nullptr, ws.data_ptr(),
                         static_cast<size_t>(ws.numel()), stream_of(x)), "cugs_vq_assign");
}
}  // namespace

torch::Tensor vq_assign(const torch::Tensor& x_in, const torch::Tensor& codebook_in, torch::Tensor* dist) {
    torch::NoGradGuard no_grad;
    const auto x = vq_rows(x_in, "x");
    TORCH_CHECK(codebook_in.defined() && codebook_in.dim() == 2 && codebook_in.size(1) == x.size(1), "vq_assign: codebook must be [k, d]");
    TORCH_CHECK(codebook_in.device() == x.device() && codebook_in.scalar_type() == torch::kFloat32,
                "vq_assign: codebook must be float32 on the device of x");
    const int64_t k = codebook_in.size(0), n = x.size(0);
    TORCH_CHECK(k >= 1 && k <= 65536, "vq_assign: 1 <= k <= 65536, got ", k);
    const auto codebook = codebook_in.contiguous();
    auto assign = torch::empty({n}, iopt(x));
    if (dist) *dist = torch::empty({n}, fopt(x));
    if (n > 0) {
        auto ws = vq_workspace(k, x.size(1), x);
        vq_assign_into(x, codebook, assign, dist, ws);
    }
    return assign;
}

int vq_frac_bits(int64_t n, double x_max, double w_max) {
    TORCH_CHECK(std::isfinite(x_max) && std::isfinite(w_max) && w_max >= 0.0,
                "vq_fit: the data and the weights must be finite and the weights non-negative");
    const double big = std::max(w_max * x_max, w_max);
    if (big <= 0.0) return 62;
    int en = 0, eb = 0;
    std::frexp(static_cast<double>(std::max<int64_t>(n, 1)), &en);
    std::frexp(big, &eb);
    const int bits = 61 - en - eb;
    TORCH_CHECK(bits >= 0, "vq_fit: n * max|w x| is too large for 64-bit fixed-point sums");
    return std::min(bits, 62);
}

VqFit vq_fit(const torch::Tensor& x_in, int64_t k, int iters, const torch::Tensor& weights_in, const torch::Tensor& init) {
    torch::NoGradGuard no_grad;
    const auto x = vq_rows(x_in, "x");
    const int64_t n = x.size(0), d = x.size(1);
    TORCH_CHECK(k >= 1 && k <= 65536, "vq_fit: 1 <= k <= 65536, got ", k);
    TORCH_CHECK(iters >= 0, "vq_fit: iters must not be negative");
    const int64_t kk = std::min(k, n);
    torch::Tensor weights;
    if (weights_in.defined()) {
        TORCH_CHECK(weights_in.numel() == n && weights_in.device() == x.device(),
                    "vq_fit: weights must hold one value per row, on the device of x");
        weights = weights_in.reshape({n}).to(torch::kFloat32).contiguous();
    }
    if (n == 0) return {torch::empty({0, d}, fopt(x)), torch::empty({0}, iopt(x)), torch::empty({0}, iopt(x))};
    torch::Tensor codebook;
    if (init.defined()) {
        TORCH_CHECK(init.dim() == 2 && init.size(0) == kk && init.size(1) == d, "vq_fit: init must be [", kk, ", ", d, "]");
        codebook = init.to(x.device(), torch::kFloat32).contiguous().clone();
    } else {
        const auto first = (torch::arange(kk, torch::TensorOptions().dtype(torch::kInt64).device(x.device())) * n).floor_divide(kk);
        codebook = x.index_select(0, first).contiguous();
    }
    std::vector<torch::Tensor> top = {x.abs().max()};
    if (weights.defined()) { top.push_back(weights.max()); top.push_back(weights.min()); }
    const auto host = torch::stack(top).to(torch::kCPU);            // the one host read of a fit
    const float* hv = host.data_ptr<float>();
    TORCH_CHECK(!weights.defined() || hv[2] >= 0.0f, "vq_fit: the weights must be non-negative");
    const int frac_bits = vq_frac_bits(n, hv[0], weights.defined() ? hv[1] : 1.0);
    auto ws = vq_workspace(kk, d, x);
    auto assign = torch::empty({n}, iopt(x));
    for (int it = 0; it < iters; ++it) {
        vq_assign_into(x, codebook, assign, nullptr, ws);
        check(cugs_vq_update(n, static_cast<int>(d), static_cast<int>(kk), ptr<float>(x), vq_ldx(x), ptr<float>(weights),
                             ptr<int32_t>(assign), frac_bits, ptr<float>(codebook), nullptr, ws.data_ptr(),
                             static_cast<size_t>(ws.numel()), stream_of(x)), "cugs_vq_update");
    }
    vq_assign_into(x, codebook, assign, nullptr, ws);
    auto counts = torch::bincount(assign.to(torch::kInt64), {}, kk).to(torch::kInt32);
    return {codebook, assign, counts};
}

}  // namespace cugs_hip
