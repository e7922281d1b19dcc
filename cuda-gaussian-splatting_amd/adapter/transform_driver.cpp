// transform_driver: a model moved by a similarity and merged through the C++ host, for
// tests/test_gpu_transform_cpp.py.
//   transform_driver.bin <dir>
// reads <dir>/{positions,sh,opacities,rotations,scales,dl_dcolor,camera0,mask}.f32 (raw float32; the camera file holds
// the cugs_camera words: view[16] fx fy cx cy width height cam_center[3]; mask is [N] with 0 / 1 as floats),
// <dir>/sim.f64 (raw float64: scale, rotation[9] row-major, translation[3]) and a second model
// <dir>/o_{positions,sh,opacities,rotations,scales}.f32, and writes, as raw float32,
//   camera_moved        view[16] of transform_camera(camera0, sim)
//   t_{positions,sh,opacities,rotations,scales}, tm_0..4, tv_0..4   model and moments (group order) after one FusedAdam
//                       step at learning rate 0 (moments set, parameters untouched) and the masked transform_gaussians
//   p_{...}, m_0..4, v_0..4                                         the same after merge_gaussians(model, other, &opt)
#include "driver_io.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const auto dev = torch::Device(torch::kCUDA, 0);
    auto load = [&](const std::string& name, std::vector<int64_t> shape) {
        return load_tensor(dir + "/" + name + ".f32", shape, torch::kFloat32, dev);
    };
    auto load_model = [&](const std::string& prefix) {
        const int64_t n = static_cast<int64_t>(read_raw<float>(dir + "/" + prefix + "opacities.f32").size());
        const int64_t c = static_cast<int64_t>(read_raw<float>(dir + "/" + prefix + "sh.f32").size()) / (3 * n);
        return cugs_hip::ModelTensors{load(prefix + "positions", {n, 3}), load(prefix + "sh", {n, 3, c}),
                                      load(prefix + "opacities", {n, 1}), load(prefix + "rotations", {n, 4}),
                                      load(prefix + "scales", {n, 3})};
    };
    const cugs_camera cam = read_camera(dir + "/camera0.f32");
    const int w = cam.width, h = cam.height;
    auto model = load_model("");
    const auto other = load_model("o_");
    const int64_t n = model.positions.size(0);
    const auto mask = load("mask", {n}).ne(0.0f);
    const auto words = read_raw<double>(dir + "/sim.f64", 13);
    cugs_hip::Similarity sim;
    sim.scale = words[0];
    for (int i = 0; i < 9; ++i) sim.rotation[i] = words[1 + i];
    for (int i = 0; i < 3; ++i) sim.translation[i] = words[10 + i];

    const cugs_camera moved = cugs_hip::transform_camera(cam, sim);
    write_as_f32(dir + "/camera_moved.f32", torch::from_blob(const_cast<float*>(moved.view), {16}, torch::kFloat32).clone());
    const auto round_trip = sim.compose(sim.inverse()).matrix();
    for (int i = 0; i < 16; ++i)
        if (std::abs(round_trip[i] - (i % 5 == 0 ? 1.0 : 0.0)) > 1e-12) { std::fprintf(stderr, "compose(inverse) is not I\n"); return 1; }

    // one optimizer step at learning rate 0: the moments are those of a real step, the parameters stay as loaded
    cugs_hip::RenderSettings settings;
    cugs_hip::FusedAdam opt({model.positions, model.sh_coeffs, model.opacities, model.scales, model.rotations},
                            {0.f, 0.f, 0.f, 0.f, 0.f});
    auto out = cugs_hip::render(model, cam, settings);
    opt.apply_gradients(cugs_hip::render_backward(load("dl_dcolor", {h, w, 3}), out, model, cam, settings));
    opt.step();

    auto dump = [&](const std::string& p, const std::string& mname, const std::string& vname) {
        write_as_f32(dir + "/" + p + "positions.f32", model.positions);
        write_as_f32(dir + "/" + p + "sh.f32", model.sh_coeffs);
        write_as_f32(dir + "/" + p + "opacities.f32", model.opacities);
        write_as_f32(dir + "/" + p + "rotations.f32", model.rotations);
        write_as_f32(dir + "/" + p + "scales.f32", model.scales);
        for (int g = 0; g < 5; ++g) {
            write_as_f32(dir + "/" + mname + std::to_string(g) + ".f32", opt.exp_avg()[g]);
            write_as_f32(dir + "/" + vname + std::to_string(g) + ".f32", opt.exp_avg_sq()[g]);
        }
    };
    const auto* before = model.positions.data_ptr<float>();
    cugs_hip::transform_gaussians(model, sim, mask, &opt);
    if (model.positions.data_ptr<float>() != before) { std::fprintf(stderr, "the transform is not in place\n"); return 1; }
    dump("t_", "tm_", "tv_");
    const int64_t total = cugs_hip::merge_gaussians(model, other, &opt);
    torch::cuda::synchronize();
    if (total != n + other.positions.size(0) || opt.exp_avg()[1].sizes() != model.sh_coeffs.sizes() ||
        !opt.params()[0].is_same(model.positions)) {
        std::fprintf(stderr, "the merged model and optimizer disagree\n");
        return 1;
    }
    dump("p_", "m_", "v_");
    // training goes on: a step on the merged model
    opt.apply_gradients(cugs_hip::render_backward(load("dl_dcolor", {h, w, 3}), cugs_hip::render(model, moved, settings),
                                                  model, moved, settings));
    opt.step();
    torch::cuda::synchronize();
    std::printf("transform_driver ok: n %lld + %lld, %dx%d\n", static_cast<long long>(n),
                static_cast<long long>(other.positions.size(0)), w, h);
    return 0;
}
