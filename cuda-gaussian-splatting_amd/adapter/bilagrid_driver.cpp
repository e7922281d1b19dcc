// bilagrid_driver: the bilateral-grid slice, its backward and the TV regulariser through the C++ host,
// for tests/test_gpu_bilagrid_cpp.py.
//   bilagrid_driver.bin <dir>
// reads <dir>/manifest.txt:
//   cases P            then P lines  "<h> <w> <l> <gy> <gx> <tv_weight>"  -> case_<i>_grid.f32 (float32 [12,l,gy,gx]),
//                                                                            case_<i>_c.f32 and case_<i>_g.f32 (float32 [h,w,3])
// Writes, per case, out_<i>_x.f32 ([h,w,3], corrected), out_<i>_dc.f32 ([h,w,3], dL_drendered), out_<i>_dg.f32
// ([12,l,gy,gx], dL_dgrid of the slice), out_<i>_tv.f32 ({tv}) and out_<i>_dgtv.f32 (dL_dgrid after bilagrid_tv added
// tv_weight * dtv/dgrid to a copy of it).
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
            int h = 0, w = 0, l = 0, gy = 0, gx = 0;
            float tv_weight = 1.0f;
            if (!(mf >> h >> w >> l >> gy >> gx >> tv_weight)) { std::fprintf(stderr, "bad manifest line %d\n", i); return 2; }
            const std::string stem = "case_" + std::to_string(i);
            auto grid = load(stem + "_grid.f32", {12, l, gy, gx});
            auto c = load(stem + "_c.f32", {h, w, 3}), g = load(stem + "_g.f32", {h, w, 3});
            const auto x = cugs_hip::bilagrid_slice(grid, c);
            const auto back = cugs_hip::bilagrid_slice_backward(grid, c, g);
            const auto tv = cugs_hip::bilagrid_tv(grid, tv_weight, back.dL_dgrid.clone());
            const std::string out = dir + "/out_" + std::to_string(i);
            write_raw(out + "_x.f32", x);
            write_raw(out + "_dc.f32", back.dL_drendered);
            write_raw(out + "_dg.f32", back.dL_dgrid);
            write_raw(out + "_tv.f32", tv.tv.reshape({1}));
            write_raw(out + "_dgtv.f32", tv.dL_dgrid);
        }
        bool threw = false;                                       // an [11, ...] grid is a c10::Error
        if (ncases > 0) {
            auto a = torch::zeros({4, 4, 3}, torch::TensorOptions().dtype(torch::kFloat32).device(dev));
            try { cugs_hip::bilagrid_slice(torch::zeros({11, 2, 2, 2}, a.options()), a); } catch (const c10::Error&) { threw = true; }
        }
        std::printf("bilagrid_driver ok cases=%d bad_grid_throws=%d\n", ncases, threw ? 1 : 0);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "bilagrid_driver failed: %s\n", e.what());
        return 4;
    }
}
