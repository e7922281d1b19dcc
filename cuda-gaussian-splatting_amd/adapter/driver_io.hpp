// driver_io.hpp — raw-file helpers shared by the test programs (*_driver.cpp, driver_io_check.cpp).  Header-only and
// for the test programs alone: the library does not include it.  The Python half is tests/cpp_driver.py; the two are
// held together by tests/test_driver_io.py.  An unreadable or short input ends the program with status 2.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "cugs_hip_torch.hpp"

// The whole file as elements of T; a non-zero expected_count must match.
template <typename T> std::vector<T> read_raw(const std::string& path, size_t expected_count = 0) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); std::exit(2); }
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    std::vector<T> v(static_cast<size_t>(bytes) / sizeof(T));
    f.read(reinterpret_cast<char*>(v.data()), bytes);
    if (expected_count && v.size() != expected_count) {
        std::fprintf(stderr, "%s: %zu elements, expected %zu\n", path.c_str(), v.size(), expected_count);
        std::exit(2);
    }
    return v;
}

// A file of exactly the shape's element count, as a tensor of that shape on `device`.
inline torch::Tensor load_tensor(const std::string& path, std::vector<int64_t> shape,
                                 torch::ScalarType dtype = torch::kFloat32, torch::Device device = torch::kCPU) {
    size_t count = 1;
    for (int64_t s : shape) count *= static_cast<size_t>(s);
    auto bytes = read_raw<uint8_t>(path);
    const size_t size = c10::elementSize(dtype);
    if (bytes.size() / size != count) {
        std::fprintf(stderr, "%s: %zu elements, expected %zu\n", path.c_str(), bytes.size() / size, count);
        std::exit(2);
    }
    return torch::from_blob(bytes.data(), shape, dtype).clone().to(device);
}

// The tensor's own dtype, detached, contiguous, from the host.
inline void write_raw(const std::string& path, const torch::Tensor& t) {
    auto c = t.detach().to(torch::kCPU).contiguous();
    std::ofstream f(path, std::ios::binary);
    f.write(static_cast<const char*>(c.data_ptr()), static_cast<std::streamsize>(c.numel() * c.element_size()));
}
inline void write_raw(const std::string& path, const std::vector<float>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(float)));
}
inline void write_as_f32(const std::string& path, const torch::Tensor& t) {     // converted on the host
    write_raw(path, t.detach().to(torch::kCPU).to(torch::kFloat32));
}

// The 25-word camera: view[16], fx fy cx cy, width height, cam_center[3], all float32 (tests/cpp_driver.py:write_camera).
inline cugs_camera camera_from_words(const float* words) {
    cugs_camera cam{};
    for (int i = 0; i < 16; ++i) cam.view[i] = words[i];
    cam.fx = words[16]; cam.fy = words[17]; cam.cx = words[18]; cam.cy = words[19];
    cam.width = static_cast<int>(words[20]); cam.height = static_cast<int>(words[21]);
    for (int i = 0; i < 3; ++i) cam.cam_center[i] = words[22 + i];
    return cam;
}
inline cugs_camera read_camera(const std::string& path) { return camera_from_words(read_raw<float>(path, 25).data()); }
