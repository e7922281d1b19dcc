// lift_driver: pixel maps lifted onto Gaussians through the C++ host, for tests/test_gpu_lift_cpp.py.
//   lift_driver.bin <dir> <num_labels> <keep_label>
// reads <dir>/{positions,sh,opacities,rotations,scales,dl_dcolor,camera0,camera1,map0,map1,err0,err1,labels}.f32 (raw
// float32; a camera file holds the cugs_camera words: view[16] fx fy cx cy width height cam_center[3]; map<i> is
// [H,W,4], err<i> [H,W], labels [H,W] with the label values as floats) and writes, as raw float32,
//   a_sums              [N,4] both views through render + lift_pixel_maps
//   b_sums              [N,4] the same through lift_maps
//   c_sums              [N,2] view 0 in labels mode, label_base 1, through render + lift_pixel_maps
//   votes, labels       vote_labels over both views ([N,num_labels], [N])
//   err_max, err_sum    error_scores over both views, by maximum and by addition
//   kept                the return of select_gaussians(labels == keep_label) with a FusedAdam that has taken one step at
//                       learning rate 0 (moments set, parameters untouched)
//   p_{positions,sh,opacities,rotations,scales}, m_0..m_4, v_0..v_4   the selected model and moments (group order)
#include "driver_io.hpp"

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s <dir> <num_labels> <keep_label>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const int num_labels = std::atoi(argv[2]), keep_label = std::atoi(argv[3]);
    const auto dev = torch::Device(torch::kCUDA, 0);
    auto load = [&](const std::string& name, std::vector<int64_t> shape) {
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
    const std::vector<torch::Tensor> maps{load("map0", {h, w, 4}), load("map1", {h, w, 4})};
    const std::vector<torch::Tensor> errs{load("err0", {h, w}), load("err1", {h, w})};
    const auto labels_2d = load("labels", {h, w}).to(torch::kInt32);

    cugs_hip::LiftedMaps a(n, dev, 4);
    for (size_t i = 0; i < cams.size(); ++i)
        cugs_hip::lift_pixel_maps(a, cugs_hip::render(model, cams[i], settings, /*for_backward=*/false), cams[i], maps[i]);
    auto b = cugs_hip::lift_maps(model, cams, maps, settings);
    if (a.num_views != 2 || b.num_views != 2 || b.channels != 4) { std::fprintf(stderr, "num_views is not 2\n"); return 1; }
    if (a.sums().data_ptr() != a.table.data_ptr()) { std::fprintf(stderr, "sums() is not a view of the table\n"); return 1; }
    write_as_f32(dir + "/a_sums.f32", a.sums());
    write_as_f32(dir + "/b_sums.f32", b.sums());
    cugs_hip::LiftedMaps cl(n, dev, 2);
    cugs_hip::lift_pixel_maps(cl, cugs_hip::render(model, cams[0], settings, /*for_backward=*/false), cams[0], {}, labels_2d, 1);
    if (cl.table.narrow(1, 2, 2).any().item<bool>()) { std::fprintf(stderr, "words 2..3 were written\n"); return 1; }
    write_as_f32(dir + "/c_sums.f32", cl.sums());

    auto voted = cugs_hip::vote_labels(model, cams, {labels_2d, labels_2d}, num_labels, settings);
    write_as_f32(dir + "/labels.out.f32", voted.first);
    write_as_f32(dir + "/votes.f32", voted.second);
    write_as_f32(dir + "/err_max.f32", cugs_hip::error_scores(model, cams, errs, settings));
    write_as_f32(dir + "/err_sum.f32", cugs_hip::error_scores(model, cams, errs, settings, /*max_over_views=*/false));

    // one optimizer step at learning rate 0: the moments are those of a real step, the parameters stay as voted on
    cugs_hip::FusedAdam opt({model.positions, model.sh_coeffs, model.opacities, model.scales, model.rotations},
                            {0.f, 0.f, 0.f, 0.f, 0.f});
    const auto before = model.positions.clone();
    auto out = cugs_hip::render(model, cams[0], settings);
    opt.apply_gradients(cugs_hip::render_backward(load("dl_dcolor", {h, w, 3}), out, model, cams[0], settings));
    opt.step();
    if (!torch::equal(before, model.positions)) { std::fprintf(stderr, "a step at learning rate 0 moved the model\n"); return 1; }
    const int64_t kept = cugs_hip::select_gaussians(model, voted.first.eq(keep_label), &opt);
    torch::cuda::synchronize();
    if (model.positions.size(0) != kept || opt.exp_avg()[0].size(0) != kept || !opt.params()[0].is_same(model.positions)) {
        std::fprintf(stderr, "the selected model and optimizer disagree\n");
        return 1;
    }
    write_as_f32(dir + "/kept.f32", torch::full({1}, static_cast<double>(kept)));
    write_as_f32(dir + "/p_positions.f32", model.positions);
    write_as_f32(dir + "/p_sh.f32", model.sh_coeffs);
    write_as_f32(dir + "/p_opacities.f32", model.opacities);
    write_as_f32(dir + "/p_rotations.f32", model.rotations);
    write_as_f32(dir + "/p_scales.f32", model.scales);
    for (int g = 0; g < 5; ++g) {
        write_as_f32(dir + "/m_" + std::to_string(g) + ".f32", opt.exp_avg()[g]);
        write_as_f32(dir + "/v_" + std::to_string(g) + ".f32", opt.exp_avg_sq()[g]);
    }
    std::printf("lift_driver ok: n %lld, %dx%d, %d labels, kept %lld\n", static_cast<long long>(n), w, h, num_labels,
                static_cast<long long>(kept));
    return 0;
}
