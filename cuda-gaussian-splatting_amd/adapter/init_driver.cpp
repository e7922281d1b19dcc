// init_driver.cpp — the point-cloud initialisation through the C++ host (cugs_hip_torch) on raw binary inputs written by
// tests/test_gpu_init_cpp.py; writes the model and the mean distances back for the Python host to reproduce bit for bit.
//   init_driver <dir> <n> <sh_degree> <k_neighbors> <route>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cugs_hip_torch.hpp"

static torch::Tensor load(const std::string& p, std::vector<int64_t> shape, torch::ScalarType type) {
    auto t = torch::empty(shape, type);
    FILE* f = fopen(p.c_str(), "rb");
    const size_t bytes = static_cast<size_t>(t.numel()) * t.element_size();
    if (!f || fread(t.data_ptr(), 1, bytes, f) != bytes) { fprintf(stderr, "cannot read %s\n", p.c_str()); exit(2); }
    fclose(f);
    return t;
}
static void save(const std::string& p, const torch::Tensor& t) {
    auto c = t.to(torch::kCPU).contiguous();
    FILE* f = fopen(p.c_str(), "wb");
    fwrite(c.data_ptr(), c.element_size(), c.numel(), f);
    fclose(f);
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    if (argc < 6) return 1;
    const std::string d = argv[1];
    const int64_t n = atoll(argv[2]);
    const int degree = atoi(argv[3]), k = atoi(argv[4]), route = atoi(argv[5]);
    try {
        auto pos = load(d + "/positions.bin", {n, 3}, torch::kFloat32);          // host tensors: the layer moves them
        auto col = load(d + "/colors.bin", {n, 3}, torch::kUInt8);
        auto m = cugs_hip::init_gaussians_from_sparse(pos, col, degree, k, route);
        auto mean = cugs_hip::knn_mean_distances(pos.to(torch::kCUDA), k, route);
        save(d + "/out_mean_dist.bin", mean);
        save(d + "/out_positions.bin", m.positions);
        save(d + "/out_sh_coeffs.bin", m.sh_coeffs);
        save(d + "/out_opacities.bin", m.opacities);
        save(d + "/out_rotations.bin", m.rotations);
        save(d + "/out_scales.bin", m.scales);
        bool threw = false;                                                       // gaussian_init.cpp:77-78
        try { cugs_hip::init_gaussians_from_sparse(pos, col, 4, k, route); }
        catch (const c10::Error&) { threw = true; }
        auto empty = cugs_hip::init_gaussians_from_sparse(torch::zeros({0, 3}), torch::zeros({0, 3}, torch::kUInt8), degree, k, route);
        printf("init_driver ok n=%lld coeffs=%lld cuda=%d bad_degree_throws=%d empty=%lld\n", (long long)m.positions.size(0),
               (long long)m.sh_coeffs.size(2), m.scales.is_cuda() ? 1 : 0, threw ? 1 : 0, (long long)empty.sh_coeffs.size(0));
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "init_driver failed: %s\n", e.what());
        return 4;
    }
}
