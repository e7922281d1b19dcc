// depth_loss_driver: the depth-supervision loss through the C++ host, for
// tests/test_gpu_depth_loss_cpp.py.
//   depth_loss_driver.bin <dir>
// reads <dir>/manifest.txt:
//   cases P            then P lines  "<h> <w> <inverse>"  -> case_<i>_d.f32, case_<i>_a.f32, case_<i>_t.f32 and
//                                                            case_<i>_w.f32 (float32 [h,w]: depth map, alpha, target,
//                                                            weight)
// Writes, per case, out_<i>_out.f32 ({loss, s, b, valid weight, valid count, fit_ok}), out_<i>_gd.f32, out_<i>_ga.f32
// and out_<i>_x.f32 ([h,w]: dL_ddepth_map, dL_dalpha, expected) from depth_loss with the weight and a fitted alignment.
#include "driver_io.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    try {
        const auto dev = torch::Device(torch::kCUDA, 0);
        std::ifstream mf(dir + "/manifest.txt");
        std::string word;
        int ncases = 0;
        if (!(mf >> word >> ncases) || word != "cases") { std::fprintf(stderr, "bad manifest\n"); return 2; }
        auto load = [&](const std::string& name, int h, int w) {
            return load_tensor(dir + "/" + name, {h, w}, torch::kFloat32, dev);
        };
        for (int i = 0; i < ncases; ++i) {
            int h = 0, w = 0, inverse = 0;
            if (!(mf >> h >> w >> inverse)) { std::fprintf(stderr, "bad manifest line %d\n", i); return 2; }
            const std::string stem = "case_" + std::to_string(i);
            auto d = load(stem + "_d.f32", h, w), a = load(stem + "_a.f32", h, w), t = load(stem + "_t.f32", h, w);
            auto wt = load(stem + "_w.f32", h, w);
            const auto r = cugs_hip::depth_loss(d, a, t, wt, inverse != 0, {}, true, 1e-3f, true, true);
            const std::string out = dir + "/out_" + std::to_string(i);
            write_raw(out + "_out.f32", torch::cat({r.loss.reshape({1}), r.scale_shift, r.valid_weight.reshape({1}),
                                                    r.valid_count.reshape({1}), r.fit_ok.reshape({1})}));
            write_raw(out + "_gd.f32", r.dL_ddepth_map);
            write_raw(out + "_ga.f32", r.dL_dalpha);
            write_raw(out + "_x.f32", r.expected);
        }
        bool threw = false;                                       // a fit together with a given (s, b) is a c10::Error
        if (ncases > 0) {
            auto a = torch::ones({4, 4}, torch::TensorOptions().dtype(torch::kFloat32).device(dev));
            try { cugs_hip::depth_loss(a, a, a, {}, false, torch::ones({2}, a.options()), true); } catch (const c10::Error&) { threw = true; }
        }
        std::printf("depth_loss_driver ok cases=%d bad_args_throw=%d\n", ncases, threw ? 1 : 0);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "depth_loss_driver failed: %s\n", e.what());
        return 4;
    }
}
