// eval_json_check.cpp — the hand-written JSON writer of eval_results.hpp on its own (no torch, no GPU): prints the
// documents tests/test_metrics_ref.py parses, and is the program to build with -fsanitize=address,undefined when the
// writer changes.
//   eval_json_check [save-path]
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "eval_results.hpp"

int main(int argc, char** argv) {
    using cugs_hip::EvalResults;
    using cugs_hip::ImageMetrics;
    EvalResults r;                                               // test_metrics.cpp:126-145
    r.mean_psnr = 25.5f; r.mean_ssim = 0.88f; r.num_gaussians = 100000; r.sh_degree = 3; r.eval_time_seconds = 12.5f;
    r.per_image.push_back(ImageMetrics{"test_001.jpg", 24.3f, 0.86f});
    r.per_image.push_back(ImageMetrics{"test_002.jpg", 26.7f, 0.90f});
    std::printf("%s\n===\n", r.to_json().c_str());
    std::printf("%s\n===\n", EvalResults{}.to_json().c_str());   // empty: the reference's early return
    EvalResults odd;                                             // escapes, control bytes, UTF-8, non-finite and extreme numbers
    odd.mean_psnr = std::numeric_limits<float>::infinity(); odd.mean_ssim = std::nanf(""); odd.eval_time_seconds = 1e-7f;
    odd.num_gaussians = -1; odd.sh_degree = 0;
    odd.per_image.push_back(ImageMetrics{std::string("a\"b\\c\n\t\x01/\xc3\xa9") + std::string(300, 'x'), 100.0f, -1.0f});
    odd.per_image.push_back(ImageMetrics{"", std::numeric_limits<float>::max(), std::numeric_limits<float>::denorm_min()});
    std::printf("%s\n", odd.to_json().c_str());
    if (argc > 1 && !r.save_json(argv[1])) return 3;
    return 0;
}
