// mcmc_driver.cpp — exercises N5 (MCMC densification) through the C++ host (cugs_hip_torch) on raw binary inputs
// written by tests/test_gpu_mcmc_cpp.py and writes raw outputs back, for the Python mirror to reproduce:
//   (1) regulariser -> added to the given gradients -> FusedAdam step -> position noise -> relocation (moments
//       zeroed), all deterministic: the Python host must produce the same bytes;
//   (2) render -> render_backward(..., &adam, &mcmc, step), the fused route, on a second copy of the model.
//   mcmc_driver <dir> <n> <C> <width> <height>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "driver_io.hpp"

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    if (argc < 6) return 1;
    const std::string d = argv[1];
    const int64_t n = atoll(argv[2]), C = atoll(argv[3]);
    const int w = atoi(argv[4]), h = atoi(argv[5]);
    auto load = [](const std::string& p, std::vector<int64_t> shape) { return load_tensor(p, shape, torch::kFloat32, torch::kCUDA); };
    try {
        cugs_hip::ModelTensors m{load(d + "/positions.bin", {n, 3}), load(d + "/sh_coeffs.bin", {n, 3, C}),
                                 load(d + "/opacities.bin", {n, 1}), load(d + "/rotations.bin", {n, 4}),
                                 load(d + "/scales.bin", {n, 3})};
        cugs_hip::ModelTensors m2{m.positions.clone(), m.sh_coeffs.clone(), m.opacities.clone(), m.rotations.clone(),
                                  m.scales.clone()};
        cugs_hip::MCMCConfig mc;                       // what the test's Python mirror uses
        mc.relocate_cap = 0.1f; mc.noise_lr_init = 0.5f; mc.noise_lr_final = 0.05f; mc.noise_lr_max_steps = 1;
        mc.lambda_opacity = 0.05f; mc.lambda_scale = 0.05f; mc.seed = 4242;
        cugs_hip::MCMCController ctrl(mc, 5.0f);
        const std::array<float, 5> lrs{1.6e-4f, 2.5e-3f, 0.05f, 5e-3f, 1e-3f};

        // (1) the deterministic chain of one training iteration (trainer.cpp:231-265) on given gradients
        cugs_hip::FusedAdam opt({m.positions, m.sh_coeffs, m.opacities, m.scales, m.rotations}, lrs);
        cugs_hip::BackwardOutput g;
        g.dL_dpositions = load(d + "/g_positions.bin", {n, 3});
        g.dL_dsh_coeffs = load(d + "/g_sh_coeffs.bin", {n, 3, C});
        g.dL_drotations = load(d + "/g_rotations.bin", {n, 4});
        torch::Tensor r_o, r_s;
        auto value = ctrl.compute_regularization(m, r_o, r_s);
        g.dL_dopacities = load(d + "/g_opacities.bin", {n, 1}) + r_o;
        g.dL_dscales = load(d + "/g_scales.bin", {n, 3}) + r_s;
        opt.apply_gradients(g);
        opt.step();
        ctrl.inject_noise(m, 3);
        const auto st = ctrl.relocate(m, 3, &opt);
        write_raw(d + "/out_value.bin", value.reshape({1}));
        write_raw(d + "/out_positions.bin", m.positions);
        write_raw(d + "/out_sh_coeffs.bin", m.sh_coeffs);
        write_raw(d + "/out_opacities.bin", m.opacities);
        write_raw(d + "/out_rotations.bin", m.rotations);
        write_raw(d + "/out_scales.bin", m.scales);
        printf("relocate dead=%d moved=%d total=%d should=%d,%d\n", st.num_dead, st.num_relocated, st.num_total,
               ctrl.should_relocate(500) ? 1 : 0, ctrl.should_relocate(501) ? 1 : 0);

        // (2) the fused route through render_backward
        auto camt = load_tensor(d + "/camera.bin", {26});
        const float* cf = camt.data_ptr<float>();
        cugs_camera cam{};
        for (int i = 0; i < 16; ++i) cam.view[i] = cf[i];
        cam.fx = cf[16]; cam.fy = cf[17]; cam.cx = cf[18]; cam.cy = cf[19];
        cam.width = w; cam.height = h;
        cam.cam_center[0] = cf[20]; cam.cam_center[1] = cf[21]; cam.cam_center[2] = cf[22];
        cugs_hip::RenderSettings rs;
        rs.background[0] = cf[23]; rs.background[1] = cf[24]; rs.background[2] = cf[25];
        auto dl = load(d + "/dl_dcolor.bin", {h, w, 3});
        cugs_hip::FusedAdam opt2({m2.positions, m2.sh_coeffs, m2.opacities, m2.scales, m2.rotations}, lrs);
        auto out = cugs_hip::render(m2, cam, rs);
        auto res = cugs_hip::render_backward(dl, out, m2, cam, rs, &opt2, &ctrl, 3);
        write_raw(d + "/out_fused_positions.bin", m2.positions);
        write_raw(d + "/out_fused_opacities.bin", m2.opacities);
        write_raw(d + "/out_fused_scales.bin", m2.scales);
        bool threw = false;                            // the MCMC route without the fused optimizer step is refused
        try { cugs_hip::render_backward(dl, cugs_hip::render(m2, cam, rs), m2, cam, rs, nullptr, &ctrl, 4); }
        catch (const c10::Error&) { threw = true; }
        printf("mcmc_driver ok fused_grads_undefined=%d needs_fused=%d\n", res.dL_dpositions.defined() ? 0 : 1,
               threw ? 1 : 0);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "mcmc_driver failed: %s\n", e.what());
        return 4;
    }
}
