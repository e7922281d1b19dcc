// sparse_adam_driver: sparse Adam through the C++ host, for tests/test_gpu_sparse_adam_cpp.py.
//   sparse_adam_driver.bin <dir>
// reads <dir>/{positions,sh,opacities,rotations,scales,g_positions,g_sh,g_opacities,g_rotations,g_scales,dl_dcolor,
// camera}.f32 (raw float32; the camera file holds the cugs_camera words: view[16] fx fy cx cy width height
// cam_center[3]) and writes, as raw float32,
//   radii                                      render()'s radii of the view (exact in float32)
//   a_{positions,sh,opacities,rotations,scales}, a_m_0..4, a_v_0..4
//                                              two FusedAdam::step(radii) on the given gradients (group order)
//   b_{positions,sh,opacities,rotations,scales}, b_m_0..4, b_v_0..4, b_means_2d
//                                              one render_backward(..., sparse_adam = true) on a copy of the model
// and prints whether sparse_adam without the FusedAdam, and with an MCMCController, were refused.
#include "driver_io.hpp"

static void write_state(const std::string& dir, const std::string& tag, const cugs_hip::ModelTensors& m,
                        const cugs_hip::FusedAdam& opt) {
    write_as_f32(dir + "/" + tag + "_positions.f32", m.positions);
    write_as_f32(dir + "/" + tag + "_sh.f32", m.sh_coeffs);
    write_as_f32(dir + "/" + tag + "_opacities.f32", m.opacities);
    write_as_f32(dir + "/" + tag + "_rotations.f32", m.rotations);
    write_as_f32(dir + "/" + tag + "_scales.f32", m.scales);
    for (int g = 0; g < 5; ++g) {
        write_as_f32(dir + "/" + tag + "_m_" + std::to_string(g) + ".f32", opt.exp_avg()[g]);
        write_as_f32(dir + "/" + tag + "_v_" + std::to_string(g) + ".f32", opt.exp_avg_sq()[g]);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const auto dev = torch::Device(torch::kCUDA, 0);
    auto load = [&](const char* name, std::vector<int64_t> shape) {
        return load_tensor(dir + "/" + name + ".f32", shape, torch::kFloat32, dev);
    };
    try {
        const cugs_camera cam = read_camera(dir + "/camera.f32");
        const int64_t n = static_cast<int64_t>(read_raw<float>(dir + "/opacities.f32").size());
        const int64_t c = static_cast<int64_t>(read_raw<float>(dir + "/sh.f32").size()) / (3 * n);
        const int w = cam.width, h = cam.height;
        cugs_hip::ModelTensors a{load("positions", {n, 3}), load("sh", {n, 3, c}), load("opacities", {n, 1}),
                                 load("rotations", {n, 4}), load("scales", {n, 3})};
        cugs_hip::ModelTensors b{a.positions.clone(), a.sh_coeffs.clone(), a.opacities.clone(), a.rotations.clone(),
                                 a.scales.clone()};
        cugs_hip::RenderSettings settings;
        settings.active_sh_degree = 3;
        const std::array<float, 5> lrs{1.6e-4f, 2.5e-3f, 0.05f, 5e-3f, 1e-3f};

        // (a) the stand-alone masked step on given gradients: the same bytes as the Python host
        auto out = cugs_hip::render(a, cam, settings);
        write_as_f32(dir + "/radii.f32", out.radii);
        cugs_hip::FusedAdam opt({a.positions, a.sh_coeffs, a.opacities, a.scales, a.rotations}, lrs);
        cugs_hip::BackwardOutput g;
        g.dL_dpositions = load("g_positions", {n, 3}); g.dL_dsh_coeffs = load("g_sh", {n, 3, c});
        g.dL_dopacities = load("g_opacities", {n, 1}); g.dL_drotations = load("g_rotations", {n, 4});
        g.dL_dscales = load("g_scales", {n, 3});
        for (int it = 0; it < 2; ++it) {
            opt.apply_gradients(g);
            opt.step(out.radii);
        }
        torch::cuda::synchronize();
        write_state(dir, "a", a, opt);

        // (b) the fused route
        const auto dl = load("dl_dcolor", {h, w, 3});
        cugs_hip::FusedAdam opt2({b.positions, b.sh_coeffs, b.opacities, b.scales, b.rotations}, lrs);
        auto res = cugs_hip::render_backward(dl, cugs_hip::render(b, cam, settings), b, cam, settings, &opt2, nullptr, 0,
                                             {}, {}, false, false, /*sparse_adam=*/true);
        torch::cuda::synchronize();
        write_state(dir, "b", b, opt2);
        write_as_f32(dir + "/b_means_2d.f32", res.dL_dmeans_2d);

        // the refusals leave the model alone
        const auto before = b.positions.clone();
        bool needs_fused = false, no_mcmc = false;
        try {
            cugs_hip::render_backward(dl, cugs_hip::render(b, cam, settings), b, cam, settings, nullptr, nullptr, 0, {}, {},
                                      false, false, true);
        } catch (const c10::Error&) { needs_fused = true; }
        cugs_hip::MCMCController ctrl(cugs_hip::MCMCConfig{}, 5.0f);
        try {
            cugs_hip::render_backward(dl, cugs_hip::render(b, cam, settings), b, cam, settings, &opt2, &ctrl, 0, {}, {},
                                      false, false, true);
        } catch (const c10::Error&) { no_mcmc = true; }
        torch::cuda::synchronize();
        const bool untouched = torch::equal(before, b.positions);
        std::printf("sparse_adam_driver ok: n %lld, %dx%d, fused_grads_undefined=%d needs_fused=%d no_mcmc=%d untouched=%d\n",
                    static_cast<long long>(n), w, h, res.dL_dpositions.defined() ? 0 : 1, needs_fused ? 1 : 0,
                    no_mcmc ? 1 : 0, untouched ? 1 : 0);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sparse_adam_driver failed: %s\n", e.what());
        return 4;
    }
}
