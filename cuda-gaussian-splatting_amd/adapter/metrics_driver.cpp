// metrics_driver: the evaluation metrics through the C++ host, for tests/test_gpu_metrics_cpp.py.
//   metrics_driver.bin <dir>
// reads <dir>/manifest.txt:
//   pairs P            then P lines  "<h> <w> <u8>"      -> pair_<i>_r.bin (float32 [h,w,3]), pair_<i>_t.bin (float32, or
//                                                           uint8 when <u8> is 1)
//   views V <degree>   then V lines  "<h> <w> <name>"    -> view_<v>.u8 (uint8 [h,w,3], the cached target of camera v)
// and, when V > 0, {positions,sh,opacities,rotations,scales}.f32 and cameras.f32 (V x 25 floats: view[16] fx fy cx cy
// width height cam_center[3]).  Writes out_metrics.f32 ([P,4] from eval_metrics), out_psnr.f32 / out_ssim.f32 ([P] from
// compute_psnr / compute_ssim) and json/eval.json (evaluate(...).save_json, which creates the directory).
#include "driver_io.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    try {
        const auto dev = torch::Device(torch::kCUDA, 0);
        std::ifstream mf(dir + "/manifest.txt");
        std::string word;
        int npairs = 0, nviews = 0, degree = 0;
        if (!(mf >> word >> npairs) || word != "pairs") { std::fprintf(stderr, "bad manifest\n"); return 2; }
        auto image = [&](const std::string& name, int h, int w, bool u8) {
            return load_tensor(dir + "/" + name, {h, w, 3}, u8 ? torch::kUInt8 : torch::kFloat32, dev);
        };
        std::vector<float> metrics, psnr, ssim;
        auto table = torch::full({npairs > 0 ? npairs : 1, 4}, -7.0f, torch::TensorOptions().dtype(torch::kFloat32).device(dev));
        for (int i = 0; i < npairs; ++i) {
            int h = 0, w = 0, u8 = 0;
            mf >> h >> w >> u8;
            auto r = image("pair_" + std::to_string(i) + "_r.bin", h, w, false);
            auto t = image("pair_" + std::to_string(i) + "_t.bin", h, w, u8 != 0);
            cugs_hip::eval_metrics(r, t, table[i]);               // row i of one table, as evaluate() fills it
            psnr.push_back(cugs_hip::compute_psnr(r, t));
            ssim.push_back(cugs_hip::compute_ssim(r, t));
        }
        if (npairs > 0) {
            auto host = table.cpu();
            metrics.assign(host.data_ptr<float>(), host.data_ptr<float>() + 4 * npairs);
        }
        write_raw(dir + "/out_metrics.f32", metrics);
        write_raw(dir + "/out_psnr.f32", psnr);
        write_raw(dir + "/out_ssim.f32", ssim);

        if (!(mf >> word >> nviews >> degree) || word != "views") { std::fprintf(stderr, "bad manifest\n"); return 2; }
        std::vector<cugs_camera> cameras;
        std::vector<torch::Tensor> targets;
        std::vector<std::string> names;
        cugs_hip::ModelTensors model;
        if (nviews > 0) {
            const auto cw = read_raw<float>(dir + "/cameras.f32", static_cast<size_t>(nviews) * 25);
            for (int v = 0; v < nviews; ++v) {
                cameras.push_back(camera_from_words(cw.data() + 25 * v));
                int h = 0, w = 0;
                std::string name;
                mf >> h >> w >> name;
                targets.push_back(image("view_" + std::to_string(v) + ".u8", h, w, true));
                names.push_back(name);
            }
            auto load = [&](const char* name, std::vector<int64_t> shape) {
                return load_tensor(dir + "/" + name + ".f32", shape, torch::kFloat32, dev);
            };
            const int64_t n = static_cast<int64_t>(read_raw<float>(dir + "/opacities.f32").size());
            const int64_t c = static_cast<int64_t>(read_raw<float>(dir + "/sh.f32").size()) / (3 * n);
            model = {load("positions", {n, 3}), load("sh", {n, 3, c}), load("opacities", {n, 1}), load("rotations", {n, 4}),
                     load("scales", {n, 3})};
        }
        cugs_hip::RenderSettings settings;
        settings.active_sh_degree = degree;
        const auto res = cugs_hip::evaluate(model, cameras, targets, settings, names);
        if (!res.save_json(dir + "/json/eval.json")) { std::fprintf(stderr, "cannot write eval.json\n"); return 3; }
        bool threw = false;                                       // metrics.cpp:22-23
        if (npairs > 0) {
            auto a = torch::zeros({4, 4, 3}, torch::TensorOptions().dtype(torch::kFloat32).device(dev));
            try { cugs_hip::compute_psnr(a, a.slice(0, 0, 2)); } catch (const c10::Error&) { threw = true; }
        }
        std::printf("metrics_driver ok pairs=%d views=%zu shape_mismatch_throws=%d\n", npairs, res.per_image.size(), threw ? 1 : 0);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "metrics_driver failed: %s\n", e.what());
        return 4;
    }
}
