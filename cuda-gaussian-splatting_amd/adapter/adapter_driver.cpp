// adapter_driver.cpp — exercises the C++ host path (cugs_hip_torch) on raw binary inputs written by
// tests/test_gpu_cpp_adapter.py and writes raw outputs back: render -> render_backward -> FusedAdam.step.
//   adapter_driver <dir> <n> <C> <width> <height>
#include <cstdio>
#include <algorithm>
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
        fprintf(stderr, "[driver] start\n");
        cugs_hip::ModelTensors m{load(d + "/positions.bin", {n, 3}), load(d + "/sh_coeffs.bin", {n, 3, C}),
                                 load(d + "/opacities.bin", {n, 1}), load(d + "/rotations.bin", {n, 4}),
                                 load(d + "/scales.bin", {n, 3})};
        auto camt = load_tensor(d + "/camera.bin", {26});
        const float* cf = camt.data_ptr<float>();
        cugs_camera cam{};
        for (int i = 0; i < 16; ++i) cam.view[i] = cf[i];
        cam.fx = cf[16]; cam.fy = cf[17]; cam.cx = cf[18]; cam.cy = cf[19];
        cam.width = w; cam.height = h;
        cam.cam_center[0] = cf[20]; cam.cam_center[1] = cf[21]; cam.cam_center[2] = cf[22];
        cugs_hip::RenderSettings st;
        st.background[0] = cf[23]; st.background[1] = cf[24]; st.background[2] = cf[25];
        auto g = load(d + "/dl_dcolor.bin", {h, w, 3});

        fprintf(stderr, "[driver] inputs loaded\n");
        auto out = cugs_hip::render(m, cam, st);
        fprintf(stderr, "[driver] render done\n");
        auto grads = cugs_hip::render_backward(g, out, m, cam, st);
        fprintf(stderr, "[driver] backward done\n");
        // the reference-glue path: RenderOutput as the reference's struct carries it (no packed records) -
        // render_backward rebuilds them and must give the same gradients
        {
            cugs_hip::RenderOutput stripped = out;
            stripped.packed = torch::Tensor();
            stripped.colour_gate = torch::Tensor();      // ... nor the gate bits: recomputed from the coefficients
            auto g2 = cugs_hip::render_backward(g, stripped, m, cam, st);
            const double scale = grads.dL_dsh_coeffs.abs().max().item<double>();
            const double diff = (g2.dL_dsh_coeffs - grads.dL_dsh_coeffs).abs().max().item<double>();
            const double dpos = (g2.dL_dpositions - grads.dL_dpositions).abs().max().item<double>() /
                                std::max(grads.dL_dpositions.abs().max().item<double>(), 1e-30);
            printf("glue_repack rel_dsh=%.3e rel_dpos=%.3e\n", diff / std::max(scale, 1e-30), dpos);
        }
        // a second copy of the model takes the FUSED route: backward with the optimizer step inside the projection
        // backward (cugs_project_backward_adam), on an accumulator the forward blend cleared
        cugs_hip::ModelTensors m2{m.positions.clone(), m.sh_coeffs.clone(), m.opacities.clone(), m.rotations.clone(),
                                  m.scales.clone()};
        cugs_hip::FusedAdam opt({m.positions, m.sh_coeffs, m.opacities, m.scales, m.rotations},
                                {1.6e-4f, 2.5e-3f, 0.05f, 5e-3f, 1e-3f});
        opt.apply_gradients(grads);
        opt.step();
        fprintf(stderr, "[driver] adam done\n");
        {
            cugs_hip::FusedAdam opt2({m2.positions, m2.sh_coeffs, m2.opacities, m2.scales, m2.rotations},
                                     {1.6e-4f, 2.5e-3f, 0.05f, 5e-3f, 1e-3f});
            auto out2 = cugs_hip::render(m2, cam, st);
            const bool cleared = out2.zeroed_accum.defined() && out2.zeroed_accum.abs().max().item<float>() == 0.0f;
            auto g2 = cugs_hip::render_backward(g, out2, m2, cam, st, &opt2);
            const bool consumed = !out2.zeroed_accum.defined() && !g2.dL_dpositions.defined();
            // the two routes ran separate blends (atomics order sums differently): equal up to that
            const double dpos = (m2.positions - m.positions).abs().max().item<double>();
            const double dsh = (m2.sh_coeffs - m.sh_coeffs).abs().max().item<double>();
            const double dm2d = (g2.dL_dmeans_2d - grads.dL_dmeans_2d).abs().max().item<double>() /
                                std::max(grads.dL_dmeans_2d.abs().max().item<double>(), 1e-30);
            printf("fused_adam cleared=%d consumed=%d dpos=%.3e dsh=%.3e rel_dmeans2d=%.3e\n", cleared ? 1 : 0,
                   consumed ? 1 : 0, dpos, dsh, dm2d);
        }
        // N1 through the C++ host: loss + dL/dcolor of the render against the flipped image as a target
        auto lg = cugs_hip::combined_loss_and_grad(out.color, out.color.flip(0).contiguous());
        write_raw(d + "/out_loss.bin", lg.loss.reshape({1}));
        write_raw(d + "/out_loss_grad.bin", lg.dL_dcolor);
        write_raw(d + "/out_color.bin", out.color);
        write_raw(d + "/out_n_contrib.bin", out.n_contrib);
        write_raw(d + "/out_indices.bin", out.gaussian_indices);
        write_raw(d + "/out_dpos.bin", grads.dL_dpositions);
        write_raw(d + "/out_dsh.bin", grads.dL_dsh_coeffs);
        write_raw(d + "/out_positions_after_adam.bin", m.positions);
        // N2 through the C++ host: statistics from this view, then one clone/split/prune cycle with the
        // moments carried over; the noise comes from the test so the Python host can reproduce the result
        {
            cugs_hip::DensificationConfig dc;
            dc.densify_from = 0; dc.densify_every = 5; dc.opacity_threshold = 0.05f; dc.grad_threshold = 2e-7f;
            cugs_hip::DensificationController ctrl(dc, 6.0f);
            ctrl.accumulate_gradients(grads.dL_dmeans_2d, out.radii);
            auto noise = load(d + "/split_noise.bin", {2, n, 3});
            auto stats = ctrl.densify(m, 5, noise, &opt);
            write_raw(d + "/out_densify_positions.bin", m.positions);
            write_raw(d + "/out_densify_sh.bin", m.sh_coeffs);
            write_raw(d + "/out_densify_scales.bin", m.scales);
            printf("densify before=%d cloned=%d split=%d pruned=%d after=%d\n", stats.num_before, stats.num_cloned,
                   stats.num_split, stats.num_pruned, stats.num_after);
            opt.apply_gradients(cugs_hip::render_backward(g, cugs_hip::render(m, cam, st), m, cam, st));
            opt.step();                                  // the optimizer still works on the resized model
        }
        // N4 through the C++ host: the 8-bit copy of the render, half-size float target
        {
            auto u8 = (out.color.clamp(0, 1) * 255.0f).to(torch::kUInt8).contiguous();
            write_raw(d + "/out_view_u8.bin", u8);
            write_raw(d + "/out_target_half.bin", cugs_hip::image_to_float(u8, w / 2, h / 2));
        }
        // N3 through the C++ host: checkpoint with optimizer state, read it back, compare
        {
            const std::string ply = d + "/out_model.ply";
            bool ok = cugs_hip::write_gaussian_ply(ply, m, &opt);
            cugs_hip::FusedAdam opt2({m.positions, m.sh_coeffs, m.opacities, m.scales, m.rotations},
                                     {1.6e-4f, 2.5e-3f, 0.05f, 5e-3f, 1e-3f});
            auto back = cugs_hip::read_gaussian_ply(ply, m.positions.device(), &opt2);
            ok = ok && torch::equal(back.positions, m.positions) && torch::equal(back.sh_coeffs, m.sh_coeffs) &&
                 torch::equal(back.opacities, m.opacities) && torch::equal(back.scales, m.scales) &&
                 torch::equal(back.rotations, m.rotations);
            bool threw_missing = false;
            try { cugs_hip::read_gaussian_ply(d + "/no_such.ply"); } catch (const std::runtime_error&) { threw_missing = true; }
            printf("ply roundtrip=%d missing_throws=%d\n", ok ? 1 : 0, threw_missing ? 1 : 0);
        }
        // the reference's TORCH_CHECK behaviour: a CPU tensor must be rejected with c10::Error
        bool threw = false;
        try { cugs_hip::evaluate_sh_cuda(1, torch::zeros({2, 3, 4}), torch::zeros({2, 3})); } catch (const c10::Error&) { threw = true; }
        printf("adapter_driver ok pairs=%lld torch_check=%d\n", (long long)out.gaussian_indices.numel(), threw ? 1 : 0);
        fflush(stdout);
        return threw ? 0 : 3;
    } catch (const std::exception& e) {
        fprintf(stderr, "adapter_driver failed: %s\n", e.what());
        return 4;
    }
}
