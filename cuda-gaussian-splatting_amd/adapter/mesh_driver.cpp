// mesh_driver: TSDF fusion and surface-net extraction through the C++ host, for
// tests/test_gpu_mesh_cpp.py.
//   mesh_driver.bin <dir>
// reads <dir>/manifest.txt:
//   volume <nx> <ny> <nz> <color 0|1> <ox> <oy> <oz> <voxel_size> <trunc> <max_weight> <min_depth>
//   views V <min_alpha> <min_weight>    then V lines  "<h> <w> <fx> <fy> <cx> <cy> <has_weight 0|1>"
//                                        -> view_<i>_m.f32 (float32 [16]: the row-major view matrix), view_<i>_d.f32,
//                                           view_<i>_a.f32 (float32 [h,w]: depth map, alpha), view_<i>_c.f32 (float32
//                                           [h,w,3], with colour), view_<i>_w.f32 (float32 [h,w], with has_weight)
// Fuses the views in one tsdf_integrate call (batches of 16 inside) and extracts.  Writes out_planes.f32 ([P,nz,ny,nx]),
// out_vertices.f32 ([V,3]), out_colors.f32 ([V,3], with colour) and out_faces.i32 ([F,3]).
#include "driver_io.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    try {
        const auto dev = torch::Device(torch::kCUDA, 0);
        std::ifstream mf(dir + "/manifest.txt");
        std::string word;
        int nx = 0, ny = 0, nz = 0, color = 0, nviews = 0;
        float origin[3] = {0, 0, 0}, vs = 0, trunc = 0, max_weight = 0, min_depth = 0, min_alpha = 0, min_weight = 0;
        if (!(mf >> word >> nx >> ny >> nz >> color >> origin[0] >> origin[1] >> origin[2] >> vs >> trunc >> max_weight >> min_depth) ||
            word != "volume") { std::fprintf(stderr, "bad manifest: volume\n"); return 2; }
        if (!(mf >> word >> nviews >> min_alpha >> min_weight) || word != "views") { std::fprintf(stderr, "bad manifest: views\n"); return 2; }
        auto load = [&](const std::string& name, std::vector<int64_t> shape) {
            return load_tensor(dir + "/" + name, shape, torch::kFloat32, dev);
        };
        auto volume = cugs_hip::make_tsdf_volume(origin, nx, ny, nz, vs, trunc, color != 0, dev, max_weight, min_depth);
        std::vector<cugs_hip::TsdfViewInput> views(static_cast<size_t>(nviews));
        for (int i = 0; i < nviews; ++i) {
            int h = 0, w = 0, has_weight = 0;
            cugs_hip::TsdfViewInput& v = views[static_cast<size_t>(i)];
            v.camera = cugs_camera{};
            if (!(mf >> h >> w >> v.camera.fx >> v.camera.fy >> v.camera.cx >> v.camera.cy >> has_weight)) {
                std::fprintf(stderr, "bad manifest line %d\n", i);
                return 2;
            }
            v.camera.width = w; v.camera.height = h;
            const std::string stem = "view_" + std::to_string(i);
            const auto m = read_raw<float>(dir + "/" + stem + "_m.f32", 16);
            for (int k = 0; k < 16; ++k) v.camera.view[k] = m[static_cast<size_t>(k)];
            v.depth_map = load(stem + "_d.f32", {h, w});
            v.alpha = load(stem + "_a.f32", {h, w});
            if (color) v.color = load(stem + "_c.f32", {h, w, 3});
            if (has_weight) v.weight = load(stem + "_w.f32", {h, w});
        }
        cugs_hip::tsdf_integrate(volume, views, min_alpha);
        const auto mesh = cugs_hip::mesh_extract(volume, min_weight);
        write_raw(dir + "/out_planes.f32", volume.planes);
        write_raw(dir + "/out_vertices.f32", mesh.vertices);
        if (color) write_raw(dir + "/out_colors.f32", mesh.colors);
        write_raw(dir + "/out_faces.i32", mesh.faces);
        bool threw = false;                                       // a volume with colour and a view without is a c10::Error
        if (color && nviews > 0) {
            auto bad = views;
            bad[0].color = torch::Tensor();
            try { cugs_hip::tsdf_integrate(volume, bad, min_alpha); }
            catch (const c10::Error&) { threw = true; }
        }
        std::printf("mesh_driver ok views=%d vertices=%lld faces=%lld bad_args_throw=%d\n", nviews,
                    static_cast<long long>(mesh.vertices.size(0)), static_cast<long long>(mesh.faces.size(0)), threw ? 1 : 0);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "mesh_driver failed: %s\n", e.what());
        return 4;
    }
}
