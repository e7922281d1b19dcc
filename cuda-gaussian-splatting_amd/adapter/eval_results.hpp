// eval_results.hpp — ImageMetrics / EvalResults of training/metrics.hpp:41-62 and their JSON form (metrics.cpp:52-87),
// standard library only: the reference serialises with nlohmann::json, which this layer does not depend on, so the
// document is written by hand - the reference's keys in nlohmann's (sorted) order, 2-space indent, floats widened to
// double and printed with the shortest digits that round-trip (what dump(2) gives), non-finite numbers as null.
// Included by cugs_hip_torch.hpp; free of torch so that the writer can be built and checked on its own
// (eval_json_check.cpp).
#pragma once

#include <charconv>
#include <cmath>
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <string>
#include <vector>

namespace cugs_hip {

struct ImageMetrics {
    std::string image_name;
    float psnr = 0.0f;
    float ssim = 0.0f;
};

namespace json_detail {
inline void put_string(std::string& o, const std::string& s) {
    o += '"';
    for (const char ch : s) {
        const unsigned char c = static_cast<unsigned char>(ch);
        switch (c) {
            case '"': o += "\\\""; break;
            case '\\': o += "\\\\"; break;
            case '\b': o += "\\b"; break;
            case '\f': o += "\\f"; break;
            case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break;
            case '\t': o += "\\t"; break;
            default:
                if (c < 0x20) {
                    char buf[8];
                    std::snprintf(buf, sizeof(buf), "\\u%04x", static_cast<unsigned>(c));
                    o += buf;
                } else {
                    o += ch;                                    // UTF-8 bytes pass through
                }
        }
    }
    o += '"';
}
inline void put_number(std::string& o, float v) {
    if (!std::isfinite(v)) { o += "null"; return; }
    char buf[40];
    const auto r = std::to_chars(buf, buf + sizeof(buf), static_cast<double>(v));
    std::string s(buf, r.ptr);
    if (s.find_first_of(".e") == std::string::npos) s += ".0";  // a float stays a float: 100 -> 100.0
    o += s;
}
}  // namespace json_detail

struct EvalResults {
    float mean_psnr = 0.0f;
    float mean_ssim = 0.0f;
    std::vector<ImageMetrics> per_image;
    int num_gaussians = 0;
    int sh_degree = 0;
    float eval_time_seconds = 0.0f;

    std::string to_json() const {
        using json_detail::put_number;
        std::string o = "{\n  \"eval_time_seconds\": ";
        put_number(o, eval_time_seconds);
        o += ",\n  \"mean_psnr\": ";
        put_number(o, mean_psnr);
        o += ",\n  \"mean_ssim\": ";
        put_number(o, mean_ssim);
        o += ",\n  \"num_gaussians\": " + std::to_string(num_gaussians);
        o += ",\n  \"num_test_images\": " + std::to_string(static_cast<int>(per_image.size()));
        o += ",\n  \"per_image\": [";
        for (size_t i = 0; i < per_image.size(); ++i) {
            o += i ? ",\n    {\n      \"image_name\": " : "\n    {\n      \"image_name\": ";
            json_detail::put_string(o, per_image[i].image_name);
            o += ",\n      \"psnr\": ";
            put_number(o, per_image[i].psnr);
            o += ",\n      \"ssim\": ";
            put_number(o, per_image[i].ssim);
            o += "\n    }";
        }
        o += per_image.empty() ? "]" : "\n  ]";
        o += ",\n  \"sh_degree\": " + std::to_string(sh_degree);
        o += "\n}";
        return o;
    }

    // false if the file cannot be written (the reference logs and returns, metrics.cpp:81-84)
    bool save_json(const std::filesystem::path& path) const {
        std::error_code ec;
        if (path.has_parent_path()) std::filesystem::create_directories(path.parent_path(), ec);
        std::ofstream ofs(path);
        if (!ofs.is_open()) return false;
        ofs << to_json() << "\n";
        return static_cast<bool>(ofs);
    }
};

}  // namespace cugs_hip
