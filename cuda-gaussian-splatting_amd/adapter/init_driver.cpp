// init_driver.cpp — the point-cloud initialisation through the C++ host (cugs_hip_torch) on raw binary inputs written by
// tests/test_gpu_init_cpp.py; writes the model and the mean distances back for the Python host to reproduce bit for bit.
//   init_driver <dir> <n> <sh_degree> <k_neighbors> <route>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "driver_io.hpp"

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    if (argc < 6) return 1;
    const std::string d = argv[1];
    const int64_t n = atoll(argv[2]);
    const int degree = atoi(argv[3]), k = atoi(argv[4]), route = atoi(argv[5]);
    try {
        auto pos = load_tensor(d + "/positions.bin", {n, 3});                      // host tensors: the layer moves them
        auto col = load_tensor(d + "/colors.bin", {n, 3}, torch::kUInt8);
        auto m = cugs_hip::init_gaussians_from_sparse(pos, col, degree, k, route);
        auto mean = cugs_hip::knn_mean_distances(pos.to(torch::kCUDA), k, route);
        write_raw(d + "/out_mean_dist.bin", mean);
        write_raw(d + "/out_positions.bin", m.positions);
        write_raw(d + "/out_sh_coeffs.bin", m.sh_coeffs);
        write_raw(d + "/out_opacities.bin", m.opacities);
        write_raw(d + "/out_rotations.bin", m.rotations);
        write_raw(d + "/out_scales.bin", m.scales);
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
