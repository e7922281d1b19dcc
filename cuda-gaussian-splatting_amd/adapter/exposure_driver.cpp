// exposure_driver: the exposure-compensated, masked loss through the C++ host, for
// tests/test_gpu_exposure_cpp.py.
//   exposure_driver.bin <dir>
// reads <dir>/manifest.txt:
//   cases P            then P lines  "<h> <w> <masked> <lambda>"  -> case_<i>_c.f32, case_<i>_t.f32 (float32 [h,w,3]),
//                                                                    case_<i>_e.f32 (float32 [3,4]) and, when <masked>
//                                                                    is 1, case_<i>_m.f32 (float32 [h,w])
// Writes, per case, out_<i>_loss.f32 ({loss, L1, mean SSIM}), out_<i>_dc.f32 ([h,w,3]), out_<i>_de.f32 ([3,4]) and
// out_<i>_x.f32 ([h,w,3], the corrected image) from combined_loss_exposure.
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
            int h = 0, w = 0, masked = 0;
            float lambda = 0.2f;
            if (!(mf >> h >> w >> masked >> lambda)) { std::fprintf(stderr, "bad manifest line %d\n", i); return 2; }
            const std::string stem = "case_" + std::to_string(i);
            auto c = load(stem + "_c.f32", {h, w, 3}), t = load(stem + "_t.f32", {h, w, 3}), e = load(stem + "_e.f32", {3, 4});
            torch::Tensor m;
            if (masked) m = load(stem + "_m.f32", {h, w});
            const auto r = cugs_hip::combined_loss_exposure(c, t, lambda, e, m, true, true);
            const std::string out = dir + "/out_" + std::to_string(i);
            write_raw(out + "_loss.f32", torch::stack({r.loss, r.l1, r.ssim_mean}));
            write_raw(out + "_dc.f32", r.dL_dcolor);
            write_raw(out + "_de.f32", r.dL_dexposure);
            write_raw(out + "_x.f32", r.corrected);
        }
        bool threw = false;                                       // a [4,3] exposure is a c10::Error
        if (ncases > 0) {
            auto a = torch::zeros({4, 4, 3}, torch::TensorOptions().dtype(torch::kFloat32).device(dev));
            try { cugs_hip::combined_loss_exposure(a, a, 0.2f, torch::zeros({4, 3}, a.options())); } catch (const c10::Error&) { threw = true; }
        }
        std::printf("exposure_driver ok cases=%d bad_exposure_throws=%d\n", ncases, threw ? 1 : 0);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exposure_driver failed: %s\n", e.what());
        return 4;
    }
}
