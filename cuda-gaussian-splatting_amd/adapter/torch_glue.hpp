// torch_glue.hpp — private to the library's own translation units (cugs_hip_torch.cpp, torch_*.cpp); not for users
// and not installed.  The small stateless helpers every entry point uses, and workspace(), whose pool must exist once
// per thread in the library: it is declared here and defined in cugs_hip_torch.cpp only.  render()'s sort state
// (SortState, sort_state(), kWideDepthHold, kTileOrderMinPairs) has no user outside cugs_hip_torch.cpp and stays there.
#pragma once

#include "cugs_hip_torch.hpp"

#include <c10/hip/HIPFunctions.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

namespace cugs_hip {
#pragma GCC visibility push(hidden)      // none of this is part of the library's interface

inline void check(int code, const char* what) {
    if (code != 0)
        throw std::runtime_error(std::string("HIP error in ") + what + " - " + cugs_error_string(code));
}
inline void* stream_of(const torch::Tensor& t) {
    return static_cast<void*>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}
inline torch::Tensor f32c(const torch::Tensor& t) { return t.contiguous().to(torch::kFloat32); }   // projection.cu:240-243
template <typename T> T* ptr(const torch::Tensor& t) {
    return (t.defined() && t.numel() > 0) ? t.data_ptr<T>() : nullptr;
}
inline const uint32_t* order_ptr(const torch::Tensor& tile_order) {    // [tiles, 4] int32 records, or undefined
    return tile_order.defined() ? reinterpret_cast<const uint32_t*>(tile_order.data_ptr<int32_t>()) : nullptr;
}
inline torch::TensorOptions fopt(const torch::Tensor& like) { return torch::TensorOptions().dtype(torch::kFloat32).device(like.device()); }
inline torch::TensorOptions iopt(const torch::Tensor& like) { return torch::TensorOptions().dtype(torch::kInt32).device(like.device()); }

// cugs_hip_torch.cpp: grow-only scratch per (device, current stream, kind), one pool per thread
torch::Tensor workspace(const torch::Device& dev, size_t bytes, int kind);

#pragma GCC visibility pop
}  // namespace cugs_hip
