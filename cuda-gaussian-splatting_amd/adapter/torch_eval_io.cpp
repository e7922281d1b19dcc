// torch_eval_io.cpp — cugs_hip_torch.hpp: image_to_float, the evaluation metrics, PLY checkpoints and the point-cloud
// initialisation.
#include "torch_glue.hpp"

namespace cugs_hip {

// N4: training target from a cached 8-bit view
torch::Tensor image_to_float(const torch::Tensor& view_u8, int width, int height) {
    TORCH_CHECK(view_u8.is_cuda() && view_u8.dtype() == torch::kUInt8 && view_u8.dim() == 3 && view_u8.size(2) == 3,
                "image must be a uint8 [H, W, 3] CUDA tensor");
    if (width <= 0 || height <= 0) throw std::runtime_error("Invalid target dimensions for resize");   // image_io.cpp:48-50
    auto src = view_u8.contiguous();
    auto dst = torch::empty({height, width, 3}, torch::TensorOptions().dtype(torch::kFloat32).device(src.device()));
    check(cugs_image_to_float(static_cast<int>(src.size(1)), static_cast<int>(src.size(0)), src.data_ptr<uint8_t>(), width,
                              height, dst.data_ptr<float>(), stream_of(src)), "cugs_image_to_float");
    return dst;
}

// ---------------------------------------------------------------------------------------------
// Evaluation metrics (training/metrics.cpp)
// ---------------------------------------------------------------------------------------------
namespace {
torch::Tensor run_eval(const torch::Tensor& rendered, const torch::Tensor& target, const torch::Tensor& out_in,
                       int window_size, const char* who) {
    TORCH_CHECK(rendered.sizes() == target.sizes(), who, ": rendered and target must have same shape");   // metrics.cpp:22-25
    TORCH_CHECK(rendered.dim() == 3 && rendered.size(2) == 3, who, ": expected [H, W, 3] tensors");
    TORCH_CHECK(rendered.dtype() == torch::kFloat32, who, ": rendered must be float32, got ", rendered.dtype());
    TORCH_CHECK(target.dtype() == torch::kFloat32 || target.dtype() == torch::kUInt8, who,
                ": target must be float32 or uint8, got ", target.dtype());
    TORCH_CHECK(rendered.is_cuda() && target.is_cuda(), who, ": rendered and target must be on a CUDA device");
    TORCH_CHECK(rendered.device() == target.device(), who, ": rendered and target must be on the same device");
    TORCH_CHECK(window_size % 2 == 1, "window_size must be odd, got ", window_size);
    TORCH_CHECK(window_size >= 3 && window_size <= 15, "window_size must be in 3..15, got ", window_size);
    torch::Tensor out = out_in;
    if (!out.defined()) {
        out = torch::empty({4}, fopt(rendered));
    } else {
        TORCH_CHECK(out.dtype() == torch::kFloat32 && out.device() == rendered.device() && out.numel() == 4 &&
                    out.is_contiguous(), who, ": out must be a contiguous float32 [4] on the images' device");
    }
    const int h = static_cast<int>(rendered.size(0)), w = static_cast<int>(rendered.size(1));
    auto r = rendered.contiguous(), t = target.contiguous();
    const bool f32 = t.dtype() == torch::kFloat32;
    auto ws = workspace(rendered.device(), cugs_eval_workspace_bytes(w, h), 8);
    check(cugs_eval_metrics(w, h, ptr<float>(r), f32 ? ptr<float>(t) : nullptr, f32 ? nullptr : ptr<uint8_t>(t),
                            window_size, ws.data_ptr(), ws.numel(), ptr<float>(out), stream_of(rendered)),
          "cugs_eval_metrics");
    return out;
}
}  // namespace

torch::Tensor eval_metrics(const torch::Tensor& rendered, const torch::Tensor& target, const torch::Tensor& out,
                           int window_size) {
    return run_eval(rendered, target, out, window_size, "eval_metrics");
}
float psnr_from_mse(float mse) {                                  // metrics.cpp:27-34
    if (mse < 1e-10f) return 100.0f;
    return 10.0f * std::log10(1.0f / mse);
}
float compute_psnr(const torch::Tensor& rendered, const torch::Tensor& target) {
    return psnr_from_mse(run_eval(rendered, target, {}, 11, "PSNR").cpu().data_ptr<float>()[0]);
}
float compute_ssim(const torch::Tensor& rendered, const torch::Tensor& target) {
    return run_eval(rendered, target, {}, 11, "SSIM").cpu().data_ptr<float>()[1];
}

EvalResults evaluate(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                     const std::vector<torch::Tensor>& targets, const RenderSettings& settings,
                     const std::vector<std::string>& names) {
    const size_t num_test = cameras.size();
    if (num_test == 0) return {};                                 // metrics.cpp:98-102
    TORCH_CHECK(targets.size() >= num_test, "evaluate: ", num_test, " cameras but ", targets.size(), " targets");
    TORCH_CHECK(names.empty() || names.size() >= num_test, "evaluate: fewer image names than cameras");
    EvalResults results;
    results.num_gaussians = static_cast<int>(model.positions.size(0));
    results.sh_degree = settings.active_sh_degree;
    const auto t_start = std::chrono::steady_clock::now();
    torch::NoGradGuard no_grad;
    auto table = torch::empty({static_cast<int64_t>(num_test), 4}, fopt(model.positions));
    for (size_t v = 0; v < num_test; ++v) {
        const cugs_camera& cam = cameras[v];
        auto color = render(model, cam, settings, /*for_backward=*/false).color;
        torch::Tensor tgt = targets[v];
        if (tgt.dtype() == torch::kUInt8 && tgt.dim() == 3 && (tgt.size(1) != cam.width || tgt.size(0) != cam.height))
            tgt = image_to_float(tgt, cam.width, cam.height);     // the reference's resize, metrics.cpp:121-128
        run_eval(color, tgt, table[static_cast<int64_t>(v)], 11, "evaluate");
    }
    const auto rows = table.cpu();                                // the one read-back
    const float* m = rows.data_ptr<float>();
    float sum_psnr = 0.0f, sum_ssim = 0.0f;
    for (size_t v = 0; v < num_test; ++v) {
        ImageMetrics im;
        if (!names.empty()) im.image_name = names[v];
        im.psnr = psnr_from_mse(m[4 * v]);
        im.ssim = m[4 * v + 1];
        results.per_image.push_back(im);
        sum_psnr += im.psnr;                                      // metrics.cpp:143-151
        sum_ssim += im.ssim;
    }
    results.mean_psnr = sum_psnr / static_cast<float>(num_test);
    results.mean_ssim = sum_ssim / static_cast<float>(num_test);
    results.eval_time_seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - t_start).count();
    return results;
}

// ---------------------------------------------------------------------------------------------
// N3: PLY checkpoints (utils/ply_io.cpp:98-196, 258-351)
// ---------------------------------------------------------------------------------------------
namespace {
std::vector<std::string> ply_model_names(int c) {                 // record order without the normals
    std::vector<std::string> n = {"x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2"};
    for (int i = 0; i < 3 * (c - 1); ++i) n.push_back("f_rest_" + std::to_string(i));
    for (const char* p : {"opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"}) n.push_back(p);
    return n;
}
}  // namespace

bool write_gaussian_ply(const std::string& path, const ModelTensors& model, const FusedAdam* optimizer) {
    const auto& p0 = model.positions;
    if (!p0.defined() || p0.dim() != 2 || p0.size(1) != 3 || !model.sh_coeffs.defined() || model.sh_coeffs.dim() != 3 ||
        model.sh_coeffs.size(0) != p0.size(0) || model.sh_coeffs.size(1) != 3 || model.opacities.numel() != p0.size(0) ||
        model.scales.numel() != 3 * p0.size(0) || model.rotations.numel() != 4 * p0.size(0))
        return false;                                             // ply_io.cpp:100-103 (is_valid)
    const auto dev = p0.is_cuda() ? p0.device() : torch::Device(torch::kCUDA, c10::hip::current_device());
    auto f32 = [&](const torch::Tensor& t) { return t.to(dev).contiguous().to(torch::kFloat32); };
    std::array<torch::Tensor, 5> pr = {f32(model.positions), f32(model.sh_coeffs), f32(model.opacities), f32(model.scales),
                                       f32(model.rotations)}, mm, vv;
    const int64_t n = pr[0].size(0);
    const int c = static_cast<int>(pr[1].size(2));
    const bool state = optimizer != nullptr;
    const float *pp[5], *pm[5], *pv[5];
    for (int i = 0; i < 5; ++i) {
        pp[i] = pr[i].data_ptr<float>();
        if (state) { mm[i] = f32(optimizer->m_[i]); vv[i] = f32(optimizer->v_[i]); pm[i] = mm[i].data_ptr<float>(); pv[i] = vv[i].data_ptr<float>(); }
    }
    const int row = cugs_ply_vertex_floats(c, state ? 1 : 0);
    auto verts = torch::empty({n, row}, fopt(pr[0]));
    check(cugs_ply_pack(n, c, pp, state ? pm : nullptr, state ? pv : nullptr, ptr<float>(verts), stream_of(pr[0])), "cugs_ply_pack");
    auto host = verts.cpu();                                      // one device-to-host copy of the finished records
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    std::string head = "ply\nformat binary_little_endian 1.0\n";
    if (state) head += "comment cugs_adam_step " + std::to_string(optimizer->step_count_) + "\n";
    head += "element vertex " + std::to_string(n) + "\n";
    auto names = ply_model_names(c);
    auto emit = [&](const std::string& prefix, bool normals) {
        for (size_t i = 0; i < names.size(); ++i) {
            head += "property float " + prefix + names[i] + "\n";
            if (normals && i == 2) head += "property float nx\nproperty float ny\nproperty float nz\n";
        }
    };
    emit("", true);
    if (state) { emit("m_", false); emit("v_", false); }
    head += "end_header\n";
    bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
    const size_t bytes = static_cast<size_t>(n) * row * sizeof(float);
    ok = ok && (bytes == 0 || fwrite(host.data_ptr<float>(), 1, bytes, f) == bytes);
    return (fclose(f) == 0) && ok;
}

ModelTensors read_gaussian_ply(const std::string& path, const torch::Device& device, FusedAdam* optimizer) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("Failed to open PLY file: " + path);
    std::string buf;
    {
        char chunk[1 << 16];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.append(chunk, got);
        fclose(f);
    }
    // parse_ply_header (ply_io.cpp:211-250)
    size_t pos = 0;
    std::vector<std::string> lines;
    while (true) {
        const size_t end = buf.find('\n', pos);
        if (end == std::string::npos) throw std::runtime_error("Not a PLY file");
        std::string line = buf.substr(pos, end - pos);
        if (!line.empty() && line.back() == '\r') line.pop_back();
        pos = end + 1;
        lines.push_back(line);
        if (line == "end_header") break;
    }
    if (lines[0].find("ply") == std::string::npos) throw std::runtime_error("Not a PLY file");
    if (lines.size() < 2 || lines[1].find("binary_little_endian") == std::string::npos)
        throw std::runtime_error("Only binary_little_endian PLY is supported");
    int64_t n = 0;
    long step = 0;
    std::vector<std::string> names;
    for (size_t i = 2; i < lines.size(); ++i) {
        char a[64] = {0}, b[64] = {0}, c3[64] = {0};
        const int got = sscanf(lines[i].c_str(), "%63s %63s %63s", a, b, c3);
        if (got >= 3 && std::string(a) == "element" && std::string(b) == "vertex") n = atoll(c3);
        else if (got >= 3 && std::string(a) == "property") names.push_back(c3);
        else if (got == 3 && std::string(a) == "comment" && std::string(b) == "cugs_adam_step") step = atol(c3);
    }
    std::map<std::string, int> index;
    for (size_t i = 0; i < names.size(); ++i) index[names[i]] = static_cast<int>(i);
    int num_rest = 0;
    while (index.count("f_rest_" + std::to_string(num_rest))) ++num_rest;
    const int c = 1 + num_rest / 3;                               // :283
    const bool state = optimizer != nullptr && index.count("m_x") && index.count("v_x");
    auto canon = ply_model_names(c);
    std::vector<int32_t> col_of;
    for (const char* prefix : {"", "m_", "v_"}) {
        if (prefix[0] && !state) break;
        for (auto& nm : canon) {
            auto it = index.find(std::string(prefix) + nm);
            if (it == index.end()) throw std::runtime_error("Missing PLY property: " + std::string(prefix) + nm);
            col_of.push_back(it->second);
        }
    }
    const int num_props = static_cast<int>(names.size());
    if (buf.size() - pos < static_cast<size_t>(n) * num_props * sizeof(float)) throw std::runtime_error("Failed to read PLY binary data");
    const auto work = device.is_cuda() ? device : torch::Device(torch::kCUDA, c10::hip::current_device());
    auto data = torch::from_blob(const_cast<char*>(buf.data() + pos), {n * num_props}, torch::kFloat32).to(work);
    auto cols = torch::from_blob(col_of.data(), {static_cast<int64_t>(col_of.size())}, torch::kInt32).to(work);
    auto o = torch::TensorOptions().dtype(torch::kFloat32).device(work);
    auto mk = [&] { return std::array<torch::Tensor, 5>{torch::empty({n, 3}, o), torch::empty({n, 3, c}, o), torch::empty({n, 1}, o),
                                                        torch::empty({n, 3}, o), torch::empty({n, 4}, o)}; };
    auto pr = mk();
    std::array<torch::Tensor, 5> mm, vv;
    float *pp[5], *pm[5], *pv[5];
    if (state) { mm = mk(); vv = mk(); }
    for (int i = 0; i < 5; ++i) { pp[i] = ptr<float>(pr[i]); if (state) { pm[i] = ptr<float>(mm[i]); pv[i] = ptr<float>(vv[i]); } }
    check(cugs_ply_unpack(n, c, num_props, ptr<float>(data), cols.data_ptr<int32_t>(), pp, state ? pm : nullptr,
                          state ? pv : nullptr, stream_of(data)), "cugs_ply_unpack");
    ModelTensors m{pr[0].to(device), pr[1].to(device), pr[2].to(device), pr[4].to(device), pr[3].to(device)};
    if (state) {
        for (int i = 0; i < 5; ++i) {
            TORCH_CHECK(optimizer->m_[i].sizes() == mm[i].sizes(), "optimizer state shape mismatch");
            optimizer->m_[i] = mm[i].to(optimizer->m_[i].device());
            optimizer->v_[i] = vv[i].to(optimizer->v_[i].device());
        }
        optimizer->step_count_ = static_cast<int>(step);
    }
    return m;
}

// ---- core/gaussian_init.cpp over csrc/knn.hip ----
namespace {
torch::Device init_device(const torch::Tensor& positions, const c10::optional<torch::Device>& device) {
    if (device.has_value()) {
        if (device->is_cuda() && !device->has_index()) return torch::Device(torch::kCUDA, c10::hip::current_device());
        return *device;
    }
    if (positions.is_cuda()) return positions.device();
    return torch::Device(torch::kCUDA, c10::hip::current_device());
}
torch::Tensor mean_distances_on(const torch::Tensor& pos, int k_neighbors, int route) {
    TORCH_CHECK(k_neighbors >= 1 && k_neighbors <= 16, "k_neighbors must be 1..16, got ", k_neighbors);
    TORCH_CHECK(route == CUGS_KNN_AUTO || route == CUGS_KNN_EXHAUSTIVE || route == CUGS_KNN_TREE, "unknown route ", route);
    const int64_t n = pos.size(0);
    auto out = torch::empty({n}, fopt(pos));
    if (n == 0) return out;
    torch::Tensor ws;
    if (route != CUGS_KNN_EXHAUSTIVE) ws = workspace(pos.device(), cugs_knn_workspace_bytes(n, k_neighbors), 7);
    check(cugs_knn_mean_distances(n, k_neighbors, ptr<float>(pos), ptr<float>(out), ws.defined() ? ws.data_ptr() : nullptr,
                                  ws.defined() ? static_cast<size_t>(ws.numel()) : 0, route, stream_of(pos)),
          "cugs_knn_mean_distances");
    return out;
}
torch::Tensor positions_on(const torch::Tensor& positions, const torch::Device& dev) {
    TORCH_CHECK(positions.dim() == 2 && positions.size(1) == 3, "positions must be [N, 3]");
    return positions.to(dev, torch::kFloat32).contiguous();
}
}  // namespace

torch::Tensor knn_mean_distances(const torch::Tensor& positions, int k_neighbors, int route,
                                 c10::optional<torch::Device> device) {
    return mean_distances_on(positions_on(positions, init_device(positions, device)), k_neighbors, route);
}

ModelTensors init_gaussians_from_sparse(const torch::Tensor& positions, const torch::Tensor& colors, int sh_degree,
                                        int k_neighbors, int route, c10::optional<torch::Device> device) {
    TORCH_CHECK(sh_degree >= 0 && sh_degree <= 3, "SH degree must be 0..", 3, ", got ", sh_degree);   // gaussian_init.cpp:77-78
    const auto dev = init_device(positions, device);
    auto pos = positions_on(positions, dev);
    const int64_t n = pos.size(0);
    TORCH_CHECK(colors.dim() == 2 && colors.size(0) == n && colors.size(1) == 3, "colors must be [N, 3]");
    TORCH_CHECK(colors.scalar_type() == torch::kUInt8, "colors must be uint8");
    auto col = colors.to(dev).contiguous();
    const int64_t C = static_cast<int64_t>(sh_degree + 1) * (sh_degree + 1);
    ModelTensors m{torch::empty({n, 3}, fopt(pos)), torch::empty({n, 3, C}, fopt(pos)), torch::empty({n, 1}, fopt(pos)),
                   torch::empty({n, 4}, fopt(pos)), torch::empty({n, 3}, fopt(pos))};
    if (n == 0) return m;                                                                            // :88-95
    auto mean = mean_distances_on(pos, k_neighbors, route);
    check(cugs_init_from_points(n, static_cast<int>(C), ptr<float>(pos), col.data_ptr<uint8_t>(), ptr<float>(mean),
                                ptr<float>(m.positions), ptr<float>(m.sh_coeffs), ptr<float>(m.opacities),
                                ptr<float>(m.rotations), ptr<float>(m.scales), stream_of(pos)),
          "cugs_init_from_points");
    return m;
}

}  // namespace cugs_hip
