// depth_driver: the depth and alpha maps through the C++ host, for tests/test_gpu_depth_map_cpp.py.
//   depth_driver.bin <dir>
// reads <dir>/{positions,sh,opacities,rotations,scales,dl_dcolor,dl_ddepth,dl_dalpha,camera}.f32 (raw float32; the
// camera file holds the cugs_camera words: view[16] fx fy cx cy width height cam_center[3]), renders with
// want_depth_map = true and runs render_backward with the three map gradients, and writes
// <dir>/{depth_map,alpha,d_positions,d_rotations,d_scales,d_opacities,d_sh}.f32.
#include "driver_io.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const auto dev = torch::Device(torch::kCUDA, 0);
    auto load = [&](const char* name, std::vector<int64_t> shape) {
        return load_tensor(dir + "/" + name + ".f32", shape, torch::kFloat32, dev);
    };
    const cugs_camera cam = read_camera(dir + "/camera.f32");
    const int64_t n = static_cast<int64_t>(read_raw<float>(dir + "/opacities.f32").size());
    const int64_t c = static_cast<int64_t>(read_raw<float>(dir + "/sh.f32").size()) / (3 * n);
    const int w = cam.width, h = cam.height;
    cugs_hip::ModelTensors model{load("positions", {n, 3}), load("sh", {n, 3, c}), load("opacities", {n, 1}),
                                 load("rotations", {n, 4}), load("scales", {n, 3})};
    cugs_hip::RenderSettings settings;
    settings.active_sh_degree = 3;
    auto out = cugs_hip::render(model, cam, settings, true, /*want_depth_map=*/true);
    auto grads = cugs_hip::render_backward(load("dl_dcolor", {h, w, 3}), out, model, cam, settings, nullptr, nullptr, 0,
                                           load("dl_ddepth", {h, w}), load("dl_dalpha", {h, w}));
    torch::cuda::synchronize();
    write_as_f32(dir + "/depth_map.f32", out.depth_map);
    write_as_f32(dir + "/alpha.f32", 1.0 - out.final_T);
    write_as_f32(dir + "/d_positions.f32", grads.dL_dpositions);
    write_as_f32(dir + "/d_rotations.f32", grads.dL_drotations);
    write_as_f32(dir + "/d_scales.f32", grads.dL_dscales);
    write_as_f32(dir + "/d_opacities.f32", grads.dL_dopacities);
    write_as_f32(dir + "/d_sh.f32", grads.dL_dsh_coeffs);
    std::printf("depth_driver ok: n %lld, %dx%d\n", static_cast<long long>(n), w, h);
    return 0;
}
