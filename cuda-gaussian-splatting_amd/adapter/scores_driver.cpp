// scores_driver: contribution scores and score-based pruning through the C++ host, for
// tests/test_gpu_scores_cpp.py.
//   scores_driver.bin <dir>
// reads <dir>/{positions,sh,opacities,rotations,scales,dl_dcolor,camera0,camera1}.f32 (raw float32; a camera file holds
// the cugs_camera words: view[16] fx fy cx cy width height cam_center[3]) and writes, as raw float32,
//   a_{sum,max,count}   both views through render + accumulate_contribution_scores
//   b_{sum,max,count}   the same through contribution_scores
//   removed             the return of prune_by_scores(min_max_weight = smallest positive float) with a FusedAdam that
//                       has taken one step at learning rate 0 (moments set, parameters untouched)
//   p_{positions,sh,opacities,rotations,scales}, m_0..m_4, v_0..v_4   the pruned model and moments (group order)
#include "driver_io.hpp"

#include <limits>

static void write_scores(const std::string& dir, const char* tag, const cugs_hip::ContributionScores& s) {
    write_as_f32(dir + "/" + tag + "_sum.f32", s.weight_sum());
    write_as_f32(dir + "/" + tag + "_max.f32", s.weight_max());
    write_as_f32(dir + "/" + tag + "_count.f32", s.pixel_count());         // exact in float32 below 2^24
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const auto dev = torch::Device(torch::kCUDA, 0);
    auto load = [&](const char* name, std::vector<int64_t> shape) {
        return load_tensor(dir + "/" + name + ".f32", shape, torch::kFloat32, dev);
    };
    const std::vector<cugs_camera> cams{read_camera(dir + "/camera0.f32"), read_camera(dir + "/camera1.f32")};
    const int64_t n = static_cast<int64_t>(read_raw<float>(dir + "/opacities.f32").size());
    const int64_t c = static_cast<int64_t>(read_raw<float>(dir + "/sh.f32").size()) / (3 * n);
    const int w = cams[0].width, h = cams[0].height;
    cugs_hip::ModelTensors model{load("positions", {n, 3}), load("sh", {n, 3, c}), load("opacities", {n, 1}),
                                 load("rotations", {n, 4}), load("scales", {n, 3})};
    cugs_hip::RenderSettings settings;
    settings.active_sh_degree = 0;

    cugs_hip::ContributionScores a(n, dev);
    for (const auto& cam : cams)
        cugs_hip::accumulate_contribution_scores(a, cugs_hip::render(model, cam, settings, /*for_backward=*/false), cam);
    auto b = cugs_hip::contribution_scores(model, cams, settings);
    if (a.num_views != 2 || b.num_views != 2) { std::fprintf(stderr, "num_views is not 2\n"); return 1; }
    write_scores(dir, "a", a);
    write_scores(dir, "b", b);

    // one optimizer step at learning rate 0: the moments are those of a real step, the parameters stay as scored
    cugs_hip::FusedAdam opt({model.positions, model.sh_coeffs, model.opacities, model.scales, model.rotations},
                            {0.f, 0.f, 0.f, 0.f, 0.f});
    const auto before = model.positions.clone();
    auto out = cugs_hip::render(model, cams[0], settings);
    opt.apply_gradients(cugs_hip::render_backward(load("dl_dcolor", {h, w, 3}), out, model, cams[0], settings));
    opt.step();
    if (!torch::equal(before, model.positions)) { std::fprintf(stderr, "a step at learning rate 0 moved the model\n"); return 1; }
    const int64_t removed = cugs_hip::prune_by_scores(model, b, std::numeric_limits<float>::denorm_min(), -1.0f, &opt);
    torch::cuda::synchronize();
    if (model.positions.size(0) != n - removed || opt.exp_avg()[0].size(0) != n - removed ||
        !opt.params()[0].is_same(model.positions)) {
        std::fprintf(stderr, "the pruned model and optimizer disagree\n");
        return 1;
    }
    write_as_f32(dir + "/removed.f32", torch::full({1}, static_cast<double>(removed)));
    write_as_f32(dir + "/p_positions.f32", model.positions);
    write_as_f32(dir + "/p_sh.f32", model.sh_coeffs);
    write_as_f32(dir + "/p_opacities.f32", model.opacities);
    write_as_f32(dir + "/p_rotations.f32", model.rotations);
    write_as_f32(dir + "/p_scales.f32", model.scales);
    for (int g = 0; g < 5; ++g) {
        write_as_f32(dir + "/m_" + std::to_string(g) + ".f32", opt.exp_avg()[g]);
        write_as_f32(dir + "/v_" + std::to_string(g) + ".f32", opt.exp_avg_sq()[g]);
    }
    std::printf("scores_driver ok: n %lld, %dx%d, removed %lld\n", static_cast<long long>(n), w, h,
                static_cast<long long>(removed));
    return 0;
}
