// vq_driver: k-means codebooks through the C++ host, for tests/test_gpu_vq_cpp.py.
//   vq_driver.bin <dir> <n> <d> <k> <iters>
// reads <dir>/x.f32 ([n, d] raw float32) and <dir>/weights.f32 ([n]) and writes, as raw float32 (indices and counts are
// below 2^24, so exact),
//   fit_codebook [k', d], fit_indices [n], fit_counts [k']          vq_fit(x, k, iters)
//   wfit_codebook, wfit_indices, wfit_counts                        the same with the weights
//   assign_indices [n], assign_dist [n]                             vq_assign of x against fit_codebook, with distances
#include "driver_io.hpp"

int main(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: %s <dir> <n> <d> <k> <iters>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const int64_t n = std::atoll(argv[2]), d = std::atoll(argv[3]), k = std::atoll(argv[4]);
    const int iters = std::atoi(argv[5]);
    const auto dev = torch::Device(torch::kCUDA, 0);
    const auto x = load_tensor(dir + "/x.f32", {n, d}, torch::kFloat32, dev);
    const auto weights = load_tensor(dir + "/weights.f32", {n}, torch::kFloat32, dev);

    auto dump = [&](const std::string& prefix, const cugs_hip::VqFit& fit) {
        write_as_f32(dir + "/" + prefix + "codebook.f32", fit.codebook);
        write_as_f32(dir + "/" + prefix + "indices.f32", fit.indices);
        write_as_f32(dir + "/" + prefix + "counts.f32", fit.counts);
    };
    const auto plain = cugs_hip::vq_fit(x, k, iters);
    dump("fit_", plain);
    dump("wfit_", cugs_hip::vq_fit(x, k, iters, weights));
    torch::Tensor dist;
    const auto again = cugs_hip::vq_assign(x, plain.codebook, &dist);
    write_as_f32(dir + "/assign_indices.f32", again);
    write_as_f32(dir + "/assign_dist.f32", dist);
    torch::cuda::synchronize();
    if (!again.equal(plain.indices)) { std::fprintf(stderr, "the indices of the fit are not those of its codebook\n"); return 1; }
    std::printf("vq_driver ok: n %lld d %lld k %lld iters %d\n", static_cast<long long>(n), static_cast<long long>(d),
                static_cast<long long>(plain.codebook.size(0)), iters);
    return 0;
}
