// normal_loss_driver: the normal-supervision loss through the C++ host, for
// tests/test_gpu_normal_loss_cpp.py.
//   normal_loss_driver.bin <dir>
// reads <dir>/manifest.txt:
//   cases P            then P lines  "<h> <w> <fx> <fy> <cx> <cy>"  -> case_<i>_d.f32, case_<i>_a.f32, case_<i>_w.f32
//                                                                      (float32 [h,w]: depth map, alpha, weight) and
//                                                                      case_<i>_t.f32 (float32 [3,h,w]: the prior)
// Writes, per case, out_<i>_out.f32 ({loss, valid weight, valid count}), out_<i>_gd.f32, out_<i>_ga.f32 ([h,w]:
// dL_ddepth_map, dL_dalpha) and out_<i>_n.f32 ([3,h,w]: the normal map) from normal_loss with the weight and
// cos_weight 0.7, l1_weight 0.3, and out_<i>_dn.f32 ([3,h,w]) from depth_to_normals.
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
        auto load = [&](const std::string& name, std::vector<int64_t> shape) {
            return load_tensor(dir + "/" + name, shape, torch::kFloat32, dev);
        };
        for (int i = 0; i < ncases; ++i) {
            int h = 0, w = 0;
            float fx = 0, fy = 0, cx = 0, cy = 0;
            if (!(mf >> h >> w >> fx >> fy >> cx >> cy)) { std::fprintf(stderr, "bad manifest line %d\n", i); return 2; }
            const std::string stem = "case_" + std::to_string(i);
            auto d = load(stem + "_d.f32", {h, w}), a = load(stem + "_a.f32", {h, w}), wt = load(stem + "_w.f32", {h, w});
            auto t = load(stem + "_t.f32", {3, h, w});
            const auto r = cugs_hip::normal_loss(d, a, fx, fy, cx, cy, t, wt, 0.7f, 0.3f, 1e-3f, true, true);
            const std::string out = dir + "/out_" + std::to_string(i);
            write_raw(out + "_out.f32", torch::cat({r.loss.reshape({1}), r.valid_weight.reshape({1}), r.valid_count.reshape({1})}));
            write_raw(out + "_gd.f32", r.dL_ddepth_map);
            write_raw(out + "_ga.f32", r.dL_dalpha);
            write_raw(out + "_n.f32", r.normals);
            write_raw(out + "_dn.f32", cugs_hip::depth_to_normals(d, a, fx, fy, cx, cy));
        }
        bool threw = false;                                       // a prior with both loss weights 0 is a c10::Error
        if (ncases > 0) {
            auto a = torch::ones({4, 4}, torch::TensorOptions().dtype(torch::kFloat32).device(dev));
            try { cugs_hip::normal_loss(a, a, 4.0f, 4.0f, 2.0f, 2.0f, torch::ones({3, 4, 4}, a.options()), {}, 0.0f, 0.0f); }
            catch (const c10::Error&) { threw = true; }
        }
        std::printf("normal_loss_driver ok cases=%d bad_args_throw=%d\n", ncases, threw ? 1 : 0);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "normal_loss_driver failed: %s\n", e.what());
        return 4;
    }
}
