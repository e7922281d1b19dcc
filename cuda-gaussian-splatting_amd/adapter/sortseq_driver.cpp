// sortseq_driver: a scripted SEQUENCE of views through the C++ host's render() on one stream, for
// tests/test_gpu_sort_sequences_cpp.py - the adapter keeps its own copy of the per-stream sort state (SortState in
// cugs_hip_torch.cpp: pair-count estimate, held capacity, wide-depth counter, the keyed workspace) and every frame's
// route is chosen from what the earlier frames left behind.
//   sortseq_driver.bin <dir> <C> <scene> [<scene> ...]
// reads, per distinct scene, <dir>/<scene>.{positions,sh,opacities,rotations,scales,camera}.f32 (raw float32; a camera
// file holds the cugs_camera words: view[16] fx fy cx cy width height cam_center[3]; C coefficients per channel) and
// writes, per frame i (from 0), <dir>/frame<i>.color.f32 (the image's float32 bits), frame<i>.indices.i32 and
// frame<i>.ranges.i32 (raw int32), and prints "frame <i> <scene> pairs=<P>".
#include "driver_io.hpp"

#include <map>

struct Scene { cugs_hip::ModelTensors model; cugs_camera cam; };

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s <dir> <C> <scene> [<scene> ...]\n", argv[0]); return 2; }
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    const std::string dir = argv[1];
    const int64_t C = std::atoll(argv[2]);
    const auto dev = torch::Device(torch::kCUDA, 0);
    try {
        std::map<std::string, Scene> scenes;
        auto scene_of = [&](const std::string& name) -> Scene& {
            auto it = scenes.find(name);
            if (it != scenes.end()) return it->second;
            auto load = [&](const char* what, int64_t cols) {
                auto v = read_raw<float>(dir + "/" + name + "." + what + ".f32");
                const int64_t rows = static_cast<int64_t>(v.size()) / cols;
                return torch::from_blob(v.data(), {rows, cols}, torch::kFloat32).clone().to(dev);
            };
            Scene s;
            s.model.positions = load("positions", 3);
            s.model.sh_coeffs = load("sh", 3 * C).view({-1, 3, C});
            s.model.opacities = load("opacities", 1);
            s.model.rotations = load("rotations", 4);
            s.model.scales = load("scales", 3);
            s.cam = read_camera(dir + "/" + name + ".camera.f32");
            return scenes.emplace(name, std::move(s)).first->second;
        };
        cugs_hip::RenderSettings settings;
        settings.active_sh_degree = 3;               // render() clamps it to what the model stores
        for (int i = 3; i < argc; ++i) {
            const std::string name = argv[i];
            Scene& s = scene_of(name);
            // training frames and evaluation frames alternate, as in the Python sequences
            auto out = cugs_hip::render(s.model, s.cam, settings, /*for_backward=*/(i & 1) != 0);
            const std::string stem = dir + "/frame" + std::to_string(i - 3);
            write_raw(stem + ".color.f32", out.color);
            write_raw(stem + ".indices.i32", out.gaussian_indices);
            write_raw(stem + ".ranges.i32", out.tile_ranges);
            std::printf("frame %d %s pairs=%lld\n", i - 3, name.c_str(), static_cast<long long>(out.gaussian_indices.numel()));
        }
        std::printf("sortseq_driver ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sortseq_driver failed: %s\n", e.what());
        return 4;
    }
}
