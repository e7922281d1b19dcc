// envmap_driver: the environment-map composite and its backward through the C++ host, for
// tests/test_gpu_envmap_cpp.py.
//   envmap_driver.bin <dir>
// reads <dir>/manifest.txt  "<resolution> <grad_bound>", camera.f32 (the 25-word camera), orientation.f64 (9 doubles,
// row-major), env.f32 (float32 [3,R,R]), color.f32 and g.f32 (float32 [h,w,3]), final_T.f32 (float32 [h,w]).
// Writes out_image.f32, out_sample.f32 ([h,w,3]), out_dalpha.f32 ([h,w]), out_denv.f32 ([3,R,R]), out_clamped.i32 ({flag})
// from the map route, and out_bg_image.f32, out_bg_dalpha.f32, out_bg_dbg.f32 from the image route with the sample as
// the background.
#include "driver_io.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    try {
        const auto dev = torch::Device(torch::kCUDA, 0);
        std::ifstream mf(dir + "/manifest.txt");
        int res = 0;
        float grad_bound = 1.0f;
        if (!(mf >> res >> grad_bound)) { std::fprintf(stderr, "bad manifest\n"); return 2; }
        const cugs_camera cam = read_camera(dir + "/camera.f32");
        const auto orientation = read_raw<double>(dir + "/orientation.f64", 9);
        const int h = cam.height, w = cam.width;
        auto load = [&](const std::string& name, std::vector<int64_t> shape) {
            return load_tensor(dir + "/" + name, shape, torch::kFloat32, dev);
        };
        cugs_hip::EnvironmentMap env(res, dev, nullptr, orientation.data());
        env.texture().copy_(load("env.f32", {3, res, res}));
        cugs_hip::RenderOutput out;
        out.color = load("color.f32", {h, w, 3});
        out.final_T = load("final_T.f32", {h, w});
        out.depths = torch::zeros({1}, out.color.options());       // a render's per-Gaussian depths: only their presence counts here
        const auto g = load("g.f32", {h, w, 3});

        const cugs_hip::RenderSettings zero;
        const auto image = cugs_hip::composite_environment(out, cam, env, &zero);
        const auto sample = env.sample(cam);
        const auto back = cugs_hip::composite_environment_backward(g, out, cam, env, grad_bound, true, &zero);
        write_raw(dir + "/out_image.f32", image);
        write_raw(dir + "/out_sample.f32", sample);
        write_raw(dir + "/out_dalpha.f32", back.dL_dalpha);
        write_raw(dir + "/out_denv.f32", back.dL_denv);
        write_raw(dir + "/out_clamped.i32", back.clamped.reshape({1}));
        const auto bg_image = cugs_hip::composite_background(out.color, out.final_T, sample);
        const auto bg_back = cugs_hip::composite_background_backward(g, out.final_T, sample);
        write_raw(dir + "/out_bg_image.f32", bg_image);
        write_raw(dir + "/out_bg_dalpha.f32", bg_back.dL_dalpha);
        write_raw(dir + "/out_bg_dbg.f32", bg_back.dL_dbackground);

        int throws = 0;
        try { cugs_hip::EnvironmentMap bad(24, dev); } catch (const c10::Error&) { ++throws; }      // not a power of two
        cugs_hip::RenderSettings grey;
        grey.background[1] = 0.5f;
        try { cugs_hip::composite_environment(out, cam, env, &grey); } catch (const c10::Error&) { ++throws; }
        cugs_hip::RenderOutput bare = out;
        bare.depths = torch::Tensor();
        try { cugs_hip::composite_environment_backward(g, bare, cam, env); } catch (const c10::Error&) { ++throws; }
        std::printf("envmap_driver ok res=%d throws=%d\n", res, throws);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "envmap_driver failed: %s\n", e.what());
        return 4;
    }
}
