// cugs_hip_torch.cpp — see cugs_hip_torch.hpp.  Each function: validate like the reference's
// launcher, allocate outputs with torch (the C ABI allocates nothing), pass raw pointers and
// torch's current HIP stream, turn a non-zero return into std::runtime_error.
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
namespace {

void check(int code, const char* what) {
    if (code != 0)
        throw std::runtime_error(std::string("HIP error in ") + what + " - " + cugs_error_string(code));
}
void* stream_of(const torch::Tensor& t) {
    return static_cast<void*>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}
torch::Tensor f32c(const torch::Tensor& t) { return t.contiguous().to(torch::kFloat32); }   // projection.cu:240-243
template <typename T> T* ptr(const torch::Tensor& t) {
    return (t.defined() && t.numel() > 0) ? t.data_ptr<T>() : nullptr;
}
const uint32_t* order_ptr(const torch::Tensor& tile_order) {    // [tiles, 4] int32 records, or undefined
    return tile_order.defined() ? reinterpret_cast<const uint32_t*>(tile_order.data_ptr<int32_t>()) : nullptr;
}
torch::TensorOptions fopt(const torch::Tensor& like) { return torch::TensorOptions().dtype(torch::kFloat32).device(like.device()); }
torch::TensorOptions iopt(const torch::Tensor& like) { return torch::TensorOptions().dtype(torch::kInt32).device(like.device()); }

// Returns a handle BY VALUE: a reference into the pool would dangle when a later call grows the vector.
// Scratch is per (device, CURRENT STREAM, kind): two renders queued on two streams of one device run concurrently and
// must not share a sort workspace (cugs_project_forward_keyed writes the sort keys into it).
torch::Tensor workspace(const torch::Device& dev, size_t bytes, int kind) {      // grow-only
    // intentionally leaked: device tensors must not be destroyed during static destruction, after the
    // HIP caching allocator has gone away
    static thread_local auto& pool = *new std::vector<std::tuple<torch::Device, void*, int, torch::Tensor>>();
    void* st = static_cast<void*>(c10::hip::getCurrentHIPStream(dev.index()).stream());
    // the head of a NEW buffer is cleared: the sort's control words carry over from launch to launch, and a recycled
    // block's garbage in the range flag would read as "a depth outside the fast range" (include/cugs_hip.h)
    auto make = [&] {
        auto t = torch::empty({static_cast<int64_t>(bytes + bytes / 4 + 4096)},
                              torch::TensorOptions().dtype(torch::kUInt8).device(dev));
        t.slice(0, 0, 256).zero_();
        return t;
    };
    for (auto& e : pool)
        if (std::get<0>(e) == dev && std::get<1>(e) == st && std::get<2>(e) == kind) {
            if (static_cast<size_t>(std::get<3>(e).numel()) < bytes) std::get<3>(e) = make();
            return std::get<3>(e);
        }
    pool.emplace_back(dev, st, kind, make());
    return std::get<3>(pool.back());
}

// Host-side state of render()'s predicted sort, one per (device, stream): the running pair-count estimate, the held
// capacity, the pinned word the count lands in, and how many more sorts stay on the general depth route after one
// reported a depth outside the three-pass range (-1): sticky, so that such a view does not pay a wasted sort + blend
// and a blocking re-sort on every frame; probed again after kWideDepthHold sorts.
struct SortState {
    int64_t last_pairs = -1;
    int64_t held_cap = 0;
    int wide_left = 0;
    torch::Tensor pinned;
};
constexpr int kWideDepthHold = 256;
constexpr int64_t kTileOrderMinPairs = 2000000;
SortState& sort_state(const torch::Device& dev) {
    static thread_local auto& states = *new std::map<std::pair<int, void*>, SortState>();
    return states[{dev.index(), static_cast<void*>(c10::hip::getCurrentHIPStream(dev.index()).stream())}];
}

// key_sort: cugs_project_forward_keyed - the kernel also leaves the sort's depth keys and tile rectangles in this
// device's N-level sort workspace; the caller's next sort on the stream must be cugs_sort_pairs_predicted_keyed
ProjectionOutput project_impl(const torch::Tensor& positions, const torch::Tensor& rotations,
                              const torch::Tensor& scales, const torch::Tensor& opacities,
                              const torch::Tensor& sh_coeffs, const cugs_camera& camera,
                              int active_sh_degree, float scale_modifier, bool key_sort) {
    TORCH_CHECK(positions.is_cuda(), "positions must be on CUDA");
    TORCH_CHECK(positions.dim() == 2 && positions.size(1) == 3);
    const int64_t n = positions.size(0);
    ProjectionOutput o;
    o.means_2d = torch::empty({n, 2}, fopt(positions));
    o.depths = torch::empty({n}, fopt(positions));
    o.cov_2d_inv = torch::empty({n, 3}, fopt(positions));
    o.radii = torch::empty({n}, iopt(positions));
    o.tiles_touched = torch::empty({n}, iopt(positions));
    o.opacities_act = torch::empty({n}, fopt(positions));
    o.rgb = torch::empty({n, 3}, fopt(positions));
    o.packed = torch::empty({n, CUGS_PACKED_STRIDE}, fopt(positions));
    o.colour_gate = torch::empty({n}, torch::TensorOptions().dtype(torch::kUInt8).device(positions.device()));
    if (n == 0) return o;
    auto pos = f32c(positions), rot = f32c(rotations), scl = f32c(scales), opa = f32c(opacities), sh = f32c(sh_coeffs);
    TORCH_CHECK(sh.dim() == 3 && sh.size(0) == n && sh.size(1) == 3, "sh_coeffs must be [N, 3, C]");
    if (key_sort) {
        auto ws = workspace(positions.device(), cugs_sort_workspace_bytes(n), 0);
        check(cugs_project_forward_keyed(n, static_cast<int>(sh.size(2)), active_sh_degree, ptr<float>(pos), ptr<float>(rot),
                                         ptr<float>(scl), ptr<float>(opa), ptr<float>(sh), &camera, scale_modifier,
                                         ptr<float>(o.means_2d), ptr<float>(o.depths), ptr<float>(o.cov_2d_inv),
                                         ptr<int32_t>(o.radii), ptr<int32_t>(o.tiles_touched), ptr<float>(o.opacities_act),
                                         ptr<float>(o.rgb), ptr<float>(o.packed), ptr<uint8_t>(o.colour_gate), ws.data_ptr(),
                                         ws.numel(), stream_of(positions)),
              "cugs_project_forward_keyed");
        return o;
    }
    check(cugs_project_forward(n, static_cast<int>(sh.size(2)), active_sh_degree, ptr<float>(pos), ptr<float>(rot),
                               ptr<float>(scl), ptr<float>(opa), ptr<float>(sh), &camera, scale_modifier,
                               ptr<float>(o.means_2d), ptr<float>(o.depths), ptr<float>(o.cov_2d_inv),
                               ptr<int32_t>(o.radii), ptr<int32_t>(o.tiles_touched), ptr<float>(o.opacities_act),
                               ptr<float>(o.rgb), ptr<float>(o.packed), ptr<uint8_t>(o.colour_gate), stream_of(positions)),
          "cugs_project_forward");
    return o;
}

}  // namespace

ProjectionOutput project_gaussians(const torch::Tensor& positions, const torch::Tensor& rotations,
                                   const torch::Tensor& scales, const torch::Tensor& opacities,
                                   const torch::Tensor& sh_coeffs, const cugs_camera& camera,
                                   int active_sh_degree, float scale_modifier) {
    return project_impl(positions, rotations, scales, opacities, sh_coeffs, camera, active_sh_degree, scale_modifier, false);
}

namespace {
SortingOutput sort_gaussians_impl(const torch::Tensor& means_2d, const torch::Tensor& depths, const torch::Tensor& radii,
                                  const torch::Tensor& tiles_touched, int img_w, int img_h, bool wide_depth) {
    TORCH_CHECK(means_2d.is_cuda(), "means_2d must be on CUDA");
    const int64_t n = means_2d.size(0);
    const int num_tiles = ((img_w + CUGS_TILE - 1) / CUGS_TILE) * ((img_h + CUGS_TILE - 1) / CUGS_TILE);
    SortingOutput o;
    o.tile_ranges = torch::empty({num_tiles, 2}, iopt(means_2d));
    void* st = stream_of(means_2d);
    auto tiles = tiles_touched.contiguous().to(torch::kInt32);
    auto m = means_2d.contiguous(), d = depths.contiguous(), r = radii.contiguous();
    auto ws = workspace(means_2d.device(), cugs_sort_workspace_bytes(n), 0);
    int64_t total = 0;
    if (n > 0)      // wide_depth: the general depth route at once (the caller has seen this view report -1)
        check((wide_depth ? cugs_sort_count_pairs_wide : cugs_sort_count_pairs)(
                  n, ptr<float>(m), ptr<float>(d), ptr<int32_t>(r), ptr<int32_t>(tiles), img_w, img_h, ws.data_ptr(),
                  ws.numel(), &total, st), "cugs_sort_count_pairs");
    o.total_pairs = static_cast<int>(total);
    o.gaussian_keys_sorted = torch::empty({total}, torch::TensorOptions().dtype(torch::kInt64).device(means_2d.device()));
    o.gaussian_values_sorted = torch::empty({total}, iopt(means_2d));
    if (num_tiles > 0) {
        auto wp = workspace(means_2d.device(), cugs_sort_pair_workspace_bytes(total), 1);
        check(cugs_sort_pairs(n, total, ptr<float>(m), ptr<float>(d), ptr<int32_t>(r), ptr<int32_t>(tiles), img_w, img_h,
                              ws.data_ptr(), ws.numel(), wp.data_ptr(), wp.numel(),
                              reinterpret_cast<uint64_t*>(ptr<int64_t>(o.gaussian_keys_sorted)),
                              ptr<int32_t>(o.gaussian_values_sorted), ptr<int32_t>(o.tile_ranges), st),
              "cugs_sort_pairs");
    }
    return o;
}
}  // namespace

SortingOutput sort_gaussians(const torch::Tensor& means_2d, const torch::Tensor& depths, const torch::Tensor& radii,
                             const torch::Tensor& tiles_touched, int img_w, int img_h) {
    return sort_gaussians_impl(means_2d, depths, radii, tiles_touched, img_w, img_h, false);
}

ForwardOutput rasterize_forward(const torch::Tensor& means_2d, const torch::Tensor& cov_2d_inv, const torch::Tensor& rgb,
                                const torch::Tensor& opacities, const torch::Tensor& tile_ranges,
                                const torch::Tensor& gaussian_indices, int img_w, int img_h,
                                const float background[3], const torch::Tensor& packed, const torch::Tensor& zero_buf,
                                const torch::Tensor& tile_order, const torch::Tensor& depths) {
    TORCH_CHECK(means_2d.is_cuda(), "means_2d must be on CUDA");
    ForwardOutput o;
    o.color = torch::empty({img_h, img_w, 3}, fopt(means_2d));
    o.final_T = torch::empty({img_h, img_w}, fopt(means_2d));
    o.n_contrib = torch::empty({img_h, img_w}, iopt(means_2d));
    if (depths.defined()) {
        TORCH_CHECK(depths.is_cuda() && depths.device() == means_2d.device() && depths.dim() == 1 &&
                    depths.size(0) == means_2d.size(0), "depths must be [N] on the device of means_2d");
        o.depth_map = torch::empty({img_h, img_w}, fopt(means_2d));        // every pixel is written
    }
    if (img_w == 0 || img_h == 0) {
        if (zero_buf.defined()) zero_buf.zero_();             // the promise holds without a blend launch too
        return o;
    }
    auto m = means_2d.contiguous(), c = cov_2d_inv.contiguous(), r = rgb.contiguous(), op = opacities.contiguous();
    auto tr = tile_ranges.contiguous(), gi = gaussian_indices.contiguous();
    if (zero_buf.defined())                                     // the blend also clears the backward's accumulator
        TORCH_CHECK(zero_buf.is_contiguous() && zero_buf.scalar_type() == torch::kFloat32 && zero_buf.numel() % 4 == 0,
                    "zero_buf must be a contiguous float32 tensor of a multiple of four elements");
    if (tile_order.defined())
        TORCH_CHECK(tile_order.is_contiguous() && tile_order.scalar_type() == torch::kInt32 &&
                    tile_order.numel() == 4 * tr.size(0), "tile_order must be a contiguous [tiles, 4] int32 tensor");
    const auto z = depths.defined() ? f32c(depths) : depths;    // the depth map too
    cugs_blend_forward_opts opts{};
    if (zero_buf.defined()) {                                   // the blend also clears the backward's accumulator
        opts.zero_buf = zero_buf.data_ptr();
        opts.zero_bytes = static_cast<size_t>(zero_buf.numel()) * sizeof(float);
    }
    opts.tile_order = order_ptr(tile_order);                    // workgroups handed out longest tile list first
    opts.depths = ptr<float>(z);
    opts.out_depth = ptr<float>(o.depth_map);
    check(cugs_rasterize_forward_opts(img_w, img_h, background, ptr<int32_t>(tr), ptr<int32_t>(gi), ptr<float>(m),
                                      ptr<float>(c), ptr<float>(r), ptr<float>(op), ptr<float>(packed), ptr<float>(o.color),
                                      ptr<float>(o.final_T), ptr<int32_t>(o.n_contrib), &opts, stream_of(means_2d)),
          "cugs_rasterize_forward_opts");
    return o;
}

torch::Tensor tile_order_of(const torch::Tensor& tile_ranges, int img_w, int img_h) {
    auto tr = tile_ranges.contiguous();
    auto order = torch::empty({tr.size(0), 4}, iopt(tile_ranges));     // {tile, first pair, one past the last, 0}
    if (tr.size(0) > 0)
        check(cugs_tile_order(img_w, img_h, ptr<int32_t>(tr), reinterpret_cast<uint32_t*>(order.data_ptr<int32_t>()),
                              stream_of(tile_ranges)), "cugs_tile_order");
    return order;
}

RasterizeBackwardOutput rasterize_backward(const torch::Tensor& dL_dcolor, const torch::Tensor& means_2d,
                                           const torch::Tensor& cov_2d_inv, const torch::Tensor& rgb,
                                           const torch::Tensor& opacities, const torch::Tensor& tile_ranges,
                                           const torch::Tensor& gaussian_indices, const torch::Tensor& final_T,
                                           const torch::Tensor& n_contrib, int img_w, int img_h,
                                           const float background[3], int n_gaussians, const torch::Tensor& packed,
                                           bool unpack, const torch::Tensor& zeroed_accum, const torch::Tensor& tile_order,
                                           const torch::Tensor& depths, const torch::Tensor& dL_ddepth_map,
                                           const torch::Tensor& dL_dalpha, bool want_abs_grad) {
    TORCH_CHECK(dL_dcolor.is_cuda(), "dL_dcolor must be on CUDA");
    const int64_t n = n_gaussians;
    RasterizeBackwardOutput o;
    const bool depth_route = depths.defined() || dL_ddepth_map.defined() || dL_dalpha.defined();
    if (depth_route) {
        TORCH_CHECK(depths.defined(), "the depth / alpha map gradients need the projection's depths");
        TORCH_CHECK(depths.is_cuda() && depths.device() == dL_dcolor.device() && depths.dim() == 1 && depths.size(0) == n,
                    "depths must be [N] on the device of dL_dcolor");
        for (const torch::Tensor* t : {&dL_ddepth_map, &dL_dalpha})
            if (t->defined())
                TORCH_CHECK(t->is_cuda() && t->device() == dL_dcolor.device() && t->dim() == 2 && t->size(0) == img_h &&
                            t->size(1) == img_w, "dL_ddepth_map / dL_dalpha must be [H, W] on the device of dL_dcolor");
    }
    const bool prezeroed = zeroed_accum.defined();
    if (prezeroed)
        TORCH_CHECK(zeroed_accum.is_contiguous() && zeroed_accum.dim() == 2 && zeroed_accum.size(0) == n &&
                    zeroed_accum.size(1) == CUGS_GRAD_STRIDE, "zeroed_accum must be a contiguous [N, 16] float32 tensor");
    o.grad_accum = prezeroed ? zeroed_accum : torch::empty({n, CUGS_GRAD_STRIDE}, fopt(dL_dcolor));
    if (unpack) {
        o.dL_drgb = torch::empty({n, 3}, fopt(dL_dcolor));
        o.dL_dopacity_act = torch::empty({n}, fopt(dL_dcolor));
        o.dL_dmeans_2d = torch::empty({n, 2}, fopt(dL_dcolor));
        o.dL_dcov_2d_inv = torch::empty({n, 3}, fopt(dL_dcolor));
        if (depth_route) o.dL_ddepths = torch::empty({n}, fopt(dL_dcolor));
    }
    if (want_abs_grad)
        o.dL_dmeans_2d_abs = unpack ? torch::empty({n, 2}, fopt(dL_dcolor)) : o.grad_accum.slice(1, 10, 12);
    if (n == 0) return o;
    auto g = dL_dcolor.contiguous(), m = means_2d.contiguous(), c = cov_2d_inv.contiguous(), r = rgb.contiguous();
    auto op = opacities.contiguous(), tr = tile_ranges.contiguous(), gi = gaussian_indices.contiguous();
    auto ft = final_T.contiguous(), nc = n_contrib.contiguous();
    if (tile_order.defined())
        TORCH_CHECK(tile_order.is_contiguous() && tile_order.scalar_type() == torch::kInt32 &&
                    tile_order.numel() == 4 * tr.size(0), "tile_order must be a contiguous [tiles, 4] int32 tensor");
    auto f32 = [](const torch::Tensor& t) { return t.defined() ? f32c(t) : t; };
    const auto z = f32(depths), dd = f32(dL_ddepth_map), da = f32(dL_dalpha);
    cugs_blend_backward_opts opts{};
    opts.prezeroed = prezeroed ? 1 : 0;
    opts.abs_grad = want_abs_grad ? 1 : 0;
    opts.tile_order = order_ptr(tile_order);
    opts.depths = ptr<float>(z);
    opts.dL_ddepth_map = ptr<float>(dd);
    opts.dL_dalpha = ptr<float>(da);
    opts.dL_ddepths = ptr<float>(o.dL_ddepths);
    opts.dL_dmeans_2d_abs = unpack ? ptr<float>(o.dL_dmeans_2d_abs) : nullptr;   // not unpacked: the rows' own words
    check(cugs_rasterize_backward_opts(img_w, img_h, background, ptr<int32_t>(tr), ptr<int32_t>(gi), ptr<float>(m),
                                       ptr<float>(c), ptr<float>(r), ptr<float>(op), ptr<float>(packed), ptr<float>(g),
                                       ptr<float>(ft), ptr<int32_t>(nc), n, ptr<float>(o.grad_accum),
                                       ptr<float>(o.dL_drgb), ptr<float>(o.dL_dopacity_act), ptr<float>(o.dL_dmeans_2d),
                                       ptr<float>(o.dL_dcov_2d_inv), &opts, stream_of(dL_dcolor)),
          "cugs_rasterize_backward_opts");
    return o;
}

namespace {
ProjectionBackwardOutput project_backward_impl(const torch::Tensor* accum, const torch::Tensor* colour_gate,
                                               torch::Tensor* d_means_out, const torch::Tensor& gm, const torch::Tensor& gc,
                                               const torch::Tensor& gr, const torch::Tensor& go,
                                               const torch::Tensor& positions, const torch::Tensor& rotations,
                                               const torch::Tensor& scales, const torch::Tensor& opacities,
                                               const torch::Tensor& sh_coeffs, const torch::Tensor& radii,
                                               const cugs_camera& camera, int degree, float scale_modifier,
                                               const cugs_pose_grad* pose = nullptr) {
    TORCH_CHECK(positions.is_cuda(), "positions must be on CUDA");
    const int64_t n = positions.size(0);
    ProjectionBackwardOutput o;
    o.dL_dpositions = torch::empty({n, 3}, fopt(positions));
    o.dL_drotations = torch::empty({n, 4}, fopt(positions));
    o.dL_dscales = torch::empty({n, 3}, fopt(positions));
    o.dL_dopacities = torch::empty({n, 1}, fopt(positions));
    auto sh = f32c(sh_coeffs);
    o.dL_dsh_coeffs = torch::empty_like(sh);
    if (n == 0) return o;
    auto pos = f32c(positions), rot = f32c(rotations), scl = f32c(scales), opa = f32c(opacities), rad = radii.contiguous();
    auto cm = gm.defined() ? gm.contiguous() : gm, cc = gc.defined() ? gc.contiguous() : gc;
    auto cr = gr.defined() ? gr.contiguous() : gr, co = go.defined() ? go.contiguous() : go;
    const cugs_projection_opts opts{nullptr, pose, 0};
    check(cugs_project_backward_opts(n, static_cast<int>(sh.size(2)), degree, ptr<float>(pos), ptr<float>(rot),
                                     ptr<float>(scl), ptr<float>(opa), ptr<float>(sh), ptr<int32_t>(rad),
                                     colour_gate ? ptr<uint8_t>(*colour_gate) : nullptr, &camera, scale_modifier,
                                     accum ? ptr<float>(*accum) : nullptr, ptr<float>(cm), ptr<float>(cc), ptr<float>(cr),
                                     ptr<float>(co), ptr<float>(o.dL_dpositions), ptr<float>(o.dL_drotations),
                                     ptr<float>(o.dL_dscales), ptr<float>(o.dL_dopacities), ptr<float>(o.dL_dsh_coeffs),
                                     d_means_out ? ptr<float>(*d_means_out) : nullptr, /*dL_drgb_gated_out=*/nullptr,
                                     &opts, stream_of(positions)),
          "cugs_project_backward_opts");
    return o;
}
}  // namespace

ProjectionBackwardOutput project_backward(const torch::Tensor& dL_dmeans_2d, const torch::Tensor& dL_dcov_2d_inv,
                                          const torch::Tensor& dL_drgb, const torch::Tensor& dL_dopacity_act,
                                          const torch::Tensor& positions, const torch::Tensor& rotations,
                                          const torch::Tensor& scales, const torch::Tensor& opacities,
                                          const torch::Tensor& sh_coeffs, const torch::Tensor& radii,
                                          const cugs_camera& camera, int active_sh_degree, float scale_modifier) {
    return project_backward_impl(nullptr, nullptr, nullptr, dL_dmeans_2d, dL_dcov_2d_inv, dL_drgb, dL_dopacity_act,
                                 positions, rotations, scales, opacities, sh_coeffs, radii, camera, active_sh_degree,
                                 scale_modifier);
}

torch::Tensor evaluate_sh_cuda(int degree, const torch::Tensor& sh_coeffs, const torch::Tensor& directions) {
    TORCH_CHECK(degree >= 0 && degree <= 3, "SH degree must be 0..3, got ", degree);                 // core/sh.cu:84-97
    TORCH_CHECK(sh_coeffs.is_cuda(), "sh_coeffs must be on CUDA device");
    TORCH_CHECK(directions.is_cuda(), "directions must be on CUDA device");
    TORCH_CHECK(sh_coeffs.dim() == 3 && sh_coeffs.size(1) == 3, "sh_coeffs must be [N, 3, C]");
    TORCH_CHECK(directions.dim() == 2 && directions.size(1) == 3, "directions must be [N, 3]");
    TORCH_CHECK(sh_coeffs.size(0) == directions.size(0), "Batch size mismatch");
    TORCH_CHECK(sh_coeffs.size(2) >= (degree + 1) * (degree + 1), "Need at least ", (degree + 1) * (degree + 1),
                " coefficients for degree ", degree);
    auto c = f32c(sh_coeffs), d = f32c(directions);
    auto out = torch::empty({c.size(0), 3}, fopt(c));
    if (c.size(0) == 0) return out;
    check(cugs_evaluate_sh(degree, c.size(0), static_cast<int>(c.size(2)), ptr<float>(c), ptr<float>(d), ptr<float>(out),
                           stream_of(c)), "cugs_evaluate_sh");
    return out;
}

torch::Tensor evaluate_sh_backward_cuda(int degree, const torch::Tensor& sh_coeffs, const torch::Tensor& directions,
                                        const torch::Tensor& dL_dcolor) {
    TORCH_CHECK(degree >= 0 && degree <= 3, "SH degree must be 0..3, got ", degree);                 // sh_backward.cu:120-130
    TORCH_CHECK(sh_coeffs.is_cuda() && directions.is_cuda() && dL_dcolor.is_cuda(), "inputs must be on CUDA device");
    TORCH_CHECK(sh_coeffs.dim() == 3 && sh_coeffs.size(1) == 3, "sh_coeffs must be [N, 3, C]");
    TORCH_CHECK(directions.dim() == 2 && directions.size(1) == 3, "directions must be [N, 3]");
    TORCH_CHECK(dL_dcolor.dim() == 2 && dL_dcolor.size(1) == 3, "dL_dcolor must be [N, 3]");
    auto c = f32c(sh_coeffs), d = f32c(directions), g = f32c(dL_dcolor);
    auto out = torch::empty_like(c);
    if (c.size(0) == 0) return out;
    check(cugs_evaluate_sh_backward(degree, c.size(0), static_cast<int>(c.size(2)), ptr<float>(c), ptr<float>(d),
                                    ptr<float>(g), ptr<float>(out), stream_of(c)), "cugs_evaluate_sh_backward");
    return out;
}

static int max_sh_degree(const torch::Tensor& sh) {                                                    // gaussian.hpp:47-54
    return sh.defined() ? static_cast<int>(std::sqrt(static_cast<float>(sh.size(2)))) - 1 : 0;
}

RenderOutput render(const ModelTensors& model, const cugs_camera& camera, const RenderSettings& settings,
                    bool for_backward, bool want_depth_map) {
    TORCH_CHECK(model.positions.defined() && model.positions.is_cuda(), "GaussianModel must be on CUDA device");
    const int64_t n = model.positions.size(0);
    const int w = camera.width, h = camera.height;
    RenderOutput o;
    if (n == 0) {                                                                                     // rasterizer.cpp:36-55
        o.color = torch::empty({h, w, 3}, fopt(model.positions));
        for (int ch = 0; ch < 3; ++ch) o.color.select(2, ch).fill_(settings.background[ch]);
        o.final_T = torch::ones({h, w}, fopt(model.positions));
        o.n_contrib = torch::zeros({h, w}, iopt(model.positions));
        o.means_2d = torch::empty({0, 2}, fopt(model.positions)); o.depths = torch::empty({0}, fopt(model.positions));
        o.cov_2d_inv = torch::empty({0, 3}, fopt(model.positions)); o.radii = torch::empty({0}, iopt(model.positions));
        o.rgb = torch::empty({0, 3}, fopt(model.positions)); o.opacities_act = torch::empty({0}, fopt(model.positions));
        o.gaussian_indices = torch::empty({0}, iopt(model.positions)); o.tile_ranges = torch::empty({0, 2}, iopt(model.positions));
        if (want_depth_map) o.depth_map = torch::zeros({h, w}, fopt(model.positions));
        return o;
    }
    const int degree = std::min(settings.active_sh_degree, max_sh_degree(model.sh_coeffs));
    SortState& state = sort_state(model.positions.device());
    const int num_tiles = ((w + CUGS_TILE - 1) / CUGS_TILE) * ((h + CUGS_TILE - 1) / CUGS_TILE);
    const bool predicted = state.last_pairs >= 0 && num_tiles > 0;
    const bool wide = state.wide_left > 0;       // this stream's views leave the three-pass depth range: general route
    if (wide) --state.wide_left;                 // at 0 the next sort probes the three-pass route again
    // with a prediction to sort on, the projection keys the sort's workspace in passing (one launch and 40 MB per million
    // Gaussians less; the fallbacks below, and the general depth route, rebuild the keys from the arrays)
    const bool keyed = predicted && !wide;
    auto proj = project_impl(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, camera,
                             degree, settings.scale_modifier, keyed);
    // The sort runs on the pair count predicted from this stream's previous frame (cugs_sort_pairs_predicted) and
    // the forward blend is queued behind it before the host looks at the true count: no idle device while the
    // host waits.  A prediction that was too small is detected afterwards and the exact path re-run.
    // the backward blend's accumulator, cleared in passing by the forward blend (issue-bound, HBM idle)
    torch::Tensor accum = for_backward ? torch::empty({n, CUGS_GRAD_STRIDE}, fopt(model.positions)) : torch::Tensor();
    auto blend = [&](const SortingOutput& s) {
        return rasterize_forward(proj.means_2d, proj.cov_2d_inv, proj.rgb, proj.opacities_act, s.tile_ranges,
                                 s.gaussian_values_sorted, w, h, settings.background, proj.packed, accum, s.tile_order,
                                 want_depth_map ? proj.depths : torch::Tensor());
    };
    SortingOutput srt;
    ForwardOutput fwd;
    const int64_t prev = state.last_pairs < 0 ? 0 : state.last_pairs;
    // longest-list-first order for the blend kernels' workgroups: worth making for large frames (~8 us of one workgroup
    // inside the sort's last kernel, which a small frame does not hide)
    const bool ordered = prev >= kTileOrderMinPairs;
    if (!predicted) {
        srt = sort_gaussians_impl(proj.means_2d, proj.depths, proj.radii, proj.tiles_touched, w, h, wide);
        fwd = blend(srt);
    } else {
        // capacity = estimate * 1.10 + 64 Ki, HELD while the estimate drifts below it (down to 80 %) and grown with 5 %
        // to spare: buffer sizes that follow a slowly moving pair count fragment the caching allocator
        const int64_t needed = std::min<int64_t>(prev + prev / 10 + 65536, 2147483647ll);
        int64_t cap = needed;
        if (state.held_cap > 0 && needed <= state.held_cap && state.held_cap <= needed + needed / 4) cap = state.held_cap;
        else if (state.held_cap > 0 && needed > state.held_cap) cap = std::min<int64_t>(needed + needed / 20, 2147483647ll);
        state.held_cap = cap;
        if (!state.pinned.defined()) state.pinned = torch::zeros({1}, torch::kInt64).pin_memory();
        auto total = state.pinned;
        void* st = stream_of(proj.means_2d);
        auto tiles = proj.tiles_touched.contiguous().to(torch::kInt32);
        srt.tile_ranges = torch::empty({num_tiles, 2}, iopt(proj.means_2d));
        srt.gaussian_values_sorted = torch::empty({cap}, iopt(proj.means_2d));
        auto ws = workspace(proj.means_2d.device(), cugs_sort_workspace_bytes(n), 0);
        auto wp = workspace(proj.means_2d.device(), cugs_sort_pair_workspace_bytes(cap), 1);
        if (wide) {
            check(cugs_sort_pairs_predicted_wide(
                      n, cap, ptr<float>(proj.means_2d), ptr<float>(proj.depths), ptr<int32_t>(proj.radii), ptr<int32_t>(tiles), w, h,
                      ws.data_ptr(), ws.numel(), wp.data_ptr(), wp.numel(), nullptr, ptr<int32_t>(srt.gaussian_values_sorted),
                      ptr<int32_t>(srt.tile_ranges), total.data_ptr<int64_t>(), st), "cugs_sort_pairs_predicted_wide");
            if (ordered) srt.tile_order = tile_order_of(srt.tile_ranges, w, h);
        } else if (!ordered) {
            check(cugs_sort_pairs_predicted_keyed(
                      n, cap, ptr<float>(proj.means_2d), ptr<float>(proj.depths), ptr<int32_t>(proj.radii), ptr<int32_t>(tiles), w, h,
                      ws.data_ptr(), ws.numel(), wp.data_ptr(), wp.numel(), nullptr, ptr<int32_t>(srt.gaussian_values_sorted),
                      ptr<int32_t>(srt.tile_ranges), total.data_ptr<int64_t>(), st), "cugs_sort_pairs_predicted_keyed");
        } else {
            // the sort also leaves the order the blend kernels hand their workgroups out in (longest tile list first)
            srt.tile_order = torch::empty({num_tiles, 4}, iopt(proj.means_2d));
            check(cugs_sort_pairs_predicted_keyed_ordered(
                      n, cap, ptr<float>(proj.means_2d), ptr<float>(proj.depths), ptr<int32_t>(proj.radii), ptr<int32_t>(tiles), w, h,
                      ws.data_ptr(), ws.numel(), wp.data_ptr(), wp.numel(), nullptr, ptr<int32_t>(srt.gaussian_values_sorted),
                      ptr<int32_t>(srt.tile_ranges), total.data_ptr<int64_t>(),
                      reinterpret_cast<uint32_t*>(srt.tile_order.data_ptr<int32_t>()), st), "cugs_sort_pairs_predicted_keyed_ordered");
        }
        hipEvent_t ev;
        TORCH_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess, "hipEventCreate failed");
        TORCH_CHECK(hipEventRecord(ev, static_cast<hipStream_t>(st)) == hipSuccess, "hipEventRecord failed");
        fwd = blend(srt);                                   // queued; the host has not waited yet
        const bool ok = hipEventSynchronize(ev) == hipSuccess;
        (void)hipEventDestroy(ev);
        TORCH_CHECK(ok, "hipEventSynchronize failed");
        const int64_t p = total.data_ptr<int64_t>()[0];
        TORCH_CHECK(p >= -1 && p <= 2147483647ll, "pair count exceeds the reference's int indexing");
        if (p >= 0 && p <= cap) {
            srt.total_pairs = static_cast<int>(p);
            srt.gaussian_values_sorted = srt.gaussian_values_sorted.slice(0, 0, p);
        } else {
            // prediction too small, or -1: a depth outside the three-pass sort's range - remembered for the following
            // sorts on this stream.  Exact path, blend again.
            if (p == -1) state.wide_left = kWideDepthHold;
            srt = sort_gaussians_impl(proj.means_2d, proj.depths, proj.radii, proj.tiles_touched, w, h,
                                      p == -1 || state.wide_left > 0);
            if (ordered) srt.tile_order = tile_order_of(srt.tile_ranges, w, h);
            fwd = blend(srt);
        }
    }
    // running maximum with a slow decay: views differ by tens of percent, spare capacity is cheap, a miss is not
    state.last_pairs = std::max<int64_t>(srt.total_pairs, prev - prev / 32);
    o.color = fwd.color; o.final_T = fwd.final_T; o.n_contrib = fwd.n_contrib; o.depth_map = fwd.depth_map;
    o.means_2d = proj.means_2d; o.depths = proj.depths; o.cov_2d_inv = proj.cov_2d_inv; o.radii = proj.radii;
    o.rgb = proj.rgb; o.opacities_act = proj.opacities_act;
    o.gaussian_indices = srt.gaussian_values_sorted; o.tile_ranges = srt.tile_ranges; o.packed = proj.packed;
    o.tile_order = srt.tile_order;
    o.colour_gate = proj.colour_gate;
    o.zeroed_accum = accum;
    if (accum.defined()) o.accum_used = std::make_shared<std::atomic<bool>>(false);
    return o;
}

BackwardOutput render_backward(const torch::Tensor& dL_dcolor, const RenderOutput& ro, const ModelTensors& model,
                               const cugs_camera& camera, const RenderSettings& settings, FusedAdam* fused,
                               const MCMCController* mcmc, int step, const torch::Tensor& dL_ddepth_map,
                               const torch::Tensor& dL_dalpha, bool want_camera_grad, bool want_abs_grad,
                               bool sparse_adam) {
    TORCH_CHECK(!mcmc || fused, "the fused MCMC route needs the FusedAdam (otherwise: compute_regularization, step, "
                "inject_noise)");
    TORCH_CHECK(!sparse_adam || fused, "sparse_adam needs the FusedAdam (otherwise: render_backward, apply_gradients, "
                "step(radii))");
    TORCH_CHECK(!sparse_adam || !mcmc, "sparse_adam cannot be combined with the fused MCMC route: its regulariser and "
                "noise act on every Gaussian");
    TORCH_CHECK(dL_dcolor.is_cuda(), "dL_dcolor must be on CUDA device");                             // rasterizer.cpp:122-124
    TORCH_CHECK(dL_dcolor.dim() == 3 && dL_dcolor.size(2) == 3, "dL_dcolor must be [H, W, 3]");
    TORCH_CHECK(!dL_ddepth_map.defined() || ro.depth_map.defined(),
                "dL_ddepth_map needs a render with the depth map (render(..., want_depth_map = true))");
    const bool depth_grads = dL_ddepth_map.defined() || dL_dalpha.defined();
    const int64_t n = model.positions.size(0);
    BackwardOutput o;
    if (n == 0) {                                                                                     // rasterizer.cpp:130-139
        o.dL_dpositions = torch::zeros({0, 3}, fopt(dL_dcolor)); o.dL_drotations = torch::zeros({0, 4}, fopt(dL_dcolor));
        o.dL_dscales = torch::zeros({0, 3}, fopt(dL_dcolor)); o.dL_dopacities = torch::zeros({0, 1}, fopt(dL_dcolor));
        o.dL_dsh_coeffs = torch::zeros_like(model.sh_coeffs); o.dL_dmeans_2d = torch::zeros({0, 2}, fopt(dL_dcolor));
        if (want_camera_grad) o.dL_dviewmat = torch::zeros({4, 4}, fopt(dL_dcolor));
        if (want_abs_grad) o.dL_dmeans_2d_abs = torch::zeros({0, 2}, fopt(dL_dcolor));
        return o;
    }
    const int degree = std::min(settings.active_sh_degree, max_sh_degree(model.sh_coeffs));
    // a RenderOutput that lost its packed records (e.g. it went through the reference's struct, which has no
    // field for them) gets them rebuilt - one 48 B/Gaussian launch - so the packed blend kernel runs either way
    torch::Tensor packed = ro.packed;
    if (!packed.defined() || packed.size(0) != n) {
        packed = torch::empty({n, CUGS_PACKED_STRIDE}, fopt(dL_dcolor));
        auto m = ro.means_2d.contiguous(), c = ro.cov_2d_inv.contiguous(), r = ro.rgb.contiguous(),
             op = ro.opacities_act.contiguous();
        check(cugs_pack_projected(n, ptr<float>(m), ptr<float>(c), ptr<float>(r), ptr<float>(op), ptr<float>(packed),
                                  stream_of(dL_dcolor)), "cugs_pack_projected");
    }
    // the accumulator render() had the forward blend clear is good for ONE backward
    torch::Tensor zeroed = ro.zeroed_accum;
    ro.zeroed_accum = torch::Tensor();
    if (zeroed.defined() && ro.accum_used && ro.accum_used->exchange(true)) zeroed = torch::Tensor();   // a copy used it
    if (zeroed.defined() && (zeroed.dim() != 2 || zeroed.size(0) != n)) zeroed = torch::Tensor();
    auto rb = rasterize_backward(dL_dcolor, ro.means_2d, ro.cov_2d_inv, ro.rgb, ro.opacities_act, ro.tile_ranges,
                                 ro.gaussian_indices, ro.final_T, ro.n_contrib, camera.width, camera.height,
                                 settings.background, static_cast<int>(n), packed, /*unpack=*/false, zeroed, ro.tile_order,
                                 depth_grads ? ro.depths : torch::Tensor(), dL_ddepth_map, dL_dalpha, want_abs_grad);
    o.dL_dmeans_2d_abs = rb.dL_dmeans_2d_abs;                   // a view of the rows (undefined without the flag)
    o.dL_dmeans_2d = torch::empty({n, 2}, fopt(dL_dcolor));
    // the camera gradient: its output and the reduction's workspace, both stream-ordered allocations
    cugs_pose_grad pose{};
    torch::Tensor pose_ws;
    if (want_camera_grad) {
        o.dL_dviewmat = torch::empty({4, 4}, fopt(dL_dcolor));
        const size_t bytes = cugs_pose_grad_workspace_bytes(n);
        pose_ws = torch::empty({static_cast<int64_t>(bytes)}, dL_dcolor.options().dtype(torch::kUInt8));
        pose = cugs_pose_grad{ptr<float>(o.dL_dviewmat), nullptr, pose_ws.data_ptr(), bytes};
    }
    if (fused) {                                                // a8 + a9 + a11 in one launch, parameters updated in place
        const auto& pr = fused->params();
        TORCH_CHECK(pr[0].data_ptr() == model.positions.data_ptr() && pr[1].data_ptr() == model.sh_coeffs.data_ptr(),
                    "the fused optimizer step needs the FusedAdam that was built on this model");
        TORCH_CHECK(ro.colour_gate.defined() && ro.colour_gate.size(0) == n,
                    "the fused optimizer step needs the colour_gate of cugs_hip::render");
        const cugs_adam_fused adam = fused->begin_fused_step();
        auto radii = ro.radii.contiguous(), gate = ro.colour_gate.contiguous();
        cugs_mcmc_fused mc{};
        if (mcmc) mc = mcmc->fused_args(step);
        // sparse_adam: only the Gaussians this view sees
        const cugs_projection_opts opts{mcmc ? &mc : nullptr, want_camera_grad ? &pose : nullptr, sparse_adam ? 1 : 0};
        check(cugs_project_backward_adam_opts(n, static_cast<int>(model.sh_coeffs.size(2)), degree,
                                              ptr<float>(model.positions), ptr<float>(model.rotations),
                                              ptr<float>(model.scales), ptr<float>(model.opacities),
                                              ptr<float>(model.sh_coeffs), ptr<int32_t>(radii), ptr<uint8_t>(gate), &camera,
                                              settings.scale_modifier, ptr<float>(rb.grad_accum), &adam,
                                              ptr<float>(o.dL_dmeans_2d), &opts, stream_of(dL_dcolor)),
              "cugs_project_backward_adam_opts");
        return o;
    }
    // without the gate bits (a RenderOutput that went through the reference's struct) the kernel recomputes the gate
    // from the coefficients as the reference does: the same bits, 12 C more bytes read per Gaussian
    const bool have_gate = ro.colour_gate.defined() && ro.colour_gate.dim() == 1 && ro.colour_gate.size(0) == n;
    auto pb = project_backward_impl(&rb.grad_accum, have_gate ? &ro.colour_gate : nullptr, &o.dL_dmeans_2d, {}, {}, {}, {}, model.positions,
                                    model.rotations, model.scales, model.opacities, model.sh_coeffs, ro.radii, camera, degree,
                                    settings.scale_modifier, want_camera_grad ? &pose : nullptr);
    o.dL_dpositions = pb.dL_dpositions; o.dL_drotations = pb.dL_drotations; o.dL_dscales = pb.dL_dscales;
    o.dL_dopacities = pb.dL_dopacities; o.dL_dsh_coeffs = pb.dL_dsh_coeffs;
    return o;
}

namespace {
void validate_pair(const torch::Tensor& rendered, const torch::Tensor& target) {               // loss.cpp:14-34
    for (const torch::Tensor* img : {&rendered, &target}) {
        TORCH_CHECK(img->dim() == 3, "image must be 3-dimensional [H, W, 3], got ", img->dim(), " dims");
        TORCH_CHECK(img->size(2) == 3, "image must have 3 channels, got ", img->size(2));
        TORCH_CHECK(img->dtype() == torch::kFloat32, "image must be float32, got ", img->dtype());
        TORCH_CHECK(img->is_cuda(), "image must be on a CUDA device");
    }
    TORCH_CHECK(rendered.sizes() == target.sizes(), "rendered and target must have the same shape, got ",
                rendered.sizes(), " vs ", target.sizes());
}
torch::Tensor run_loss(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_, int window_size,
                       torch::Tensor* ssim_map, torch::Tensor* grad) {
    validate_pair(rendered, target);
    TORCH_CHECK(window_size % 2 == 1, "window_size must be odd, got ", window_size);               // loss.cpp:96-97
    TORCH_CHECK(window_size >= 3, "window_size must be >= 3, got ", window_size);
    const int h = static_cast<int>(rendered.size(0)), w = static_cast<int>(rendered.size(1));
    auto r = rendered.contiguous(), t = target.contiguous();
    auto out = torch::empty({4}, fopt(rendered));
    if (ssim_map) *ssim_map = torch::empty({h, w}, fopt(rendered));
    if (grad) *grad = torch::empty({h, w, 3}, fopt(rendered));
    auto ws = workspace(rendered.device(), cugs_loss_workspace_bytes(w, h), 2);
    check(cugs_combined_loss(w, h, ptr<float>(r), ptr<float>(t), lambda_, window_size, ws.data_ptr(), ws.numel(),
                             ptr<float>(out), ssim_map ? ptr<float>(*ssim_map) : nullptr,
                             grad ? ptr<float>(*grad) : nullptr, stream_of(rendered)), "cugs_combined_loss");
    return out;
}
}  // namespace

LossAndGrad combined_loss_and_grad(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_, bool want_grad) {
    LossAndGrad o;
    auto out = run_loss(rendered, target, lambda_, 11, nullptr, want_grad ? &o.dL_dcolor : nullptr);
    o.loss = out[0]; o.l1 = out[1]; o.ssim_mean = out[2];
    return o;
}
torch::Tensor combined_loss(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_) {
    return run_loss(rendered, target, lambda_, 11, nullptr, nullptr)[0];
}
torch::Tensor ssim(const torch::Tensor& rendered, const torch::Tensor& target, int window_size) {
    torch::Tensor map;
    run_loss(rendered, target, 0.2f, window_size, &map, nullptr);
    return map;
}

ExposureLoss combined_loss_exposure(const torch::Tensor& rendered, const torch::Tensor& target, float lambda_,
                                    const torch::Tensor& exposure, const torch::Tensor& mask, bool want_grad,
                                    bool want_corrected, int window_size) {
    validate_pair(rendered, target);
    TORCH_CHECK(window_size % 2 == 1, "window_size must be odd, got ", window_size);
    TORCH_CHECK(window_size >= 3, "window_size must be >= 3, got ", window_size);
    const int h = static_cast<int>(rendered.size(0)), w = static_cast<int>(rendered.size(1));
    if (exposure.defined()) {
        TORCH_CHECK(exposure.dim() == 2 && exposure.size(0) == 3 && exposure.size(1) == 4, "exposure must be [3, 4], got ", exposure.sizes());
        TORCH_CHECK(exposure.dtype() == torch::kFloat32, "exposure must be float32, got ", exposure.dtype());
        TORCH_CHECK(exposure.is_cuda() && exposure.device() == rendered.device(), "exposure must be on the images' CUDA device");
        TORCH_CHECK(exposure.is_contiguous(), "exposure must be contiguous");
    }
    torch::Tensor m;
    if (mask.defined()) {
        TORCH_CHECK(mask.dim() == 2 && mask.size(0) == h && mask.size(1) == w, "mask must be [H, W], got ", mask.sizes());
        TORCH_CHECK(mask.dtype() == torch::kFloat32, "mask must be float32, got ", mask.dtype());
        TORCH_CHECK(mask.is_cuda() && mask.device() == rendered.device(), "mask must be on the images' CUDA device");
        m = mask.contiguous();
    }
    auto r = rendered.contiguous(), t = target.contiguous();
    auto out = torch::empty({4}, fopt(rendered));
    ExposureLoss o;
    if (want_grad) o.dL_dcolor = torch::empty({h, w, 3}, fopt(rendered));
    if (want_grad && exposure.defined()) o.dL_dexposure = torch::empty({3, 4}, fopt(rendered));
    if (want_corrected) o.corrected = torch::empty({h, w, 3}, fopt(rendered));
    cugs_loss_opts opts{};
    opts.exposure = exposure.defined() ? exposure.data_ptr<float>() : nullptr;
    opts.mask = m.defined() ? m.data_ptr<float>() : nullptr;
    opts.dL_dexposure = o.dL_dexposure.defined() ? o.dL_dexposure.data_ptr<float>() : nullptr;
    opts.corrected = o.corrected.defined() ? o.corrected.data_ptr<float>() : nullptr;
    auto ws = workspace(rendered.device(), cugs_loss_opts_workspace_bytes(w, h), 2);
    check(cugs_combined_loss_opts(w, h, ptr<float>(r), ptr<float>(t), lambda_, window_size, &opts, ws.data_ptr(), ws.numel(),
                                  ptr<float>(out), nullptr, want_grad ? o.dL_dcolor.data_ptr<float>() : nullptr,
                                  stream_of(rendered)), "cugs_combined_loss_opts");
    o.loss = out[0]; o.l1 = out[1]; o.ssim_mean = out[2];
    return o;
}

DepthLoss depth_loss(const torch::Tensor& depth_map, const torch::Tensor& alpha, const torch::Tensor& target,
                     const torch::Tensor& weight, bool inverse, const torch::Tensor& align, bool fit, float min_alpha,
                     bool want_grad, bool want_expected) {
    TORCH_CHECK(depth_map.dim() == 2, "depth_map must be 2-dimensional [H, W], got ", depth_map.dim(), " dims");
    TORCH_CHECK(depth_map.dtype() == torch::kFloat32, "depth_map must be float32, got ", depth_map.dtype());
    TORCH_CHECK(depth_map.is_cuda(), "depth_map must be on a CUDA device");
    const int h = static_cast<int>(depth_map.size(0)), w = static_cast<int>(depth_map.size(1));
    auto validate_map = [&](const torch::Tensor& t, const char* name) {
        TORCH_CHECK(t.dim() == 2 && t.size(0) == h && t.size(1) == w, name, " must be [H, W], got ", t.sizes());
        TORCH_CHECK(t.dtype() == torch::kFloat32, name, " must be float32, got ", t.dtype());
        TORCH_CHECK(t.is_cuda() && t.device() == depth_map.device(), name, " must be on the depth map's CUDA device");
    };
    validate_map(alpha, "alpha");
    validate_map(target, "target");
    torch::Tensor wt, ss;
    if (weight.defined()) { validate_map(weight, "weight"); wt = weight.contiguous(); }
    TORCH_CHECK(min_alpha > 0.0f && std::isfinite(min_alpha), "min_alpha must be positive and finite, got ", min_alpha);
    TORCH_CHECK(!(fit && align.defined()), "align must be a fit or a given (s, b), not both");
    if (align.defined()) {
        TORCH_CHECK(align.dim() == 1 && align.size(0) == 2, "align must be [2] = (s, b), got ", align.sizes());
        TORCH_CHECK(align.dtype() == torch::kFloat32, "align must be float32, got ", align.dtype());
        TORCH_CHECK(align.is_cuda() && align.device() == depth_map.device(), "align must be on the depth map's CUDA device");
        ss = align.contiguous();
    }
    auto d = depth_map.contiguous(), a = alpha.contiguous(), t = target.contiguous();
    auto out = torch::empty({8}, fopt(depth_map));
    DepthLoss o;
    if (want_grad) { o.dL_ddepth_map = torch::empty({h, w}, fopt(depth_map)); o.dL_dalpha = torch::empty({h, w}, fopt(depth_map)); }
    if (want_expected) o.expected = torch::empty({h, w}, fopt(depth_map));
    cugs_depth_loss_opts opts{};
    opts.weight = ptr<float>(wt);
    opts.scale_shift = ptr<float>(ss);
    opts.fit = fit ? 1 : 0;
    opts.inverse = inverse ? 1 : 0;
    opts.min_alpha = min_alpha;
    opts.expected = ptr<float>(o.expected);
    auto ws = workspace(depth_map.device(), cugs_depth_loss_workspace_bytes(w, h), 9);
    check(cugs_depth_loss(w, h, ptr<float>(d), ptr<float>(a), ptr<float>(t), &opts, ws.data_ptr(), ws.numel(),
                          ptr<float>(out), ptr<float>(o.dL_ddepth_map), ptr<float>(o.dL_dalpha), stream_of(depth_map)),
          "cugs_depth_loss");
    o.loss = out[0]; o.scale_shift = out.slice(0, 1, 3); o.valid_weight = out[3]; o.valid_count = out[4]; o.fit_ok = out[5];
    return o;
}

NormalLoss normal_loss(const torch::Tensor& depth_map, const torch::Tensor& alpha, float fx, float fy, float cx, float cy,
                       const torch::Tensor& target, const torch::Tensor& weight, float cos_weight, float l1_weight,
                       float min_alpha, bool want_grad, bool want_normals) {
    TORCH_CHECK(depth_map.dim() == 2, "depth_map must be 2-dimensional [H, W], got ", depth_map.dim(), " dims");
    TORCH_CHECK(depth_map.dtype() == torch::kFloat32, "depth_map must be float32, got ", depth_map.dtype());
    TORCH_CHECK(depth_map.is_cuda(), "depth_map must be on a CUDA device");
    const int h = static_cast<int>(depth_map.size(0)), w = static_cast<int>(depth_map.size(1));
    auto validate_map = [&](const torch::Tensor& t, const char* name) {
        TORCH_CHECK(t.dim() == 2 && t.size(0) == h && t.size(1) == w, name, " must be [H, W], got ", t.sizes());
        TORCH_CHECK(t.dtype() == torch::kFloat32, name, " must be float32, got ", t.dtype());
        TORCH_CHECK(t.is_cuda() && t.device() == depth_map.device(), name, " must be on the depth map's CUDA device");
    };
    validate_map(alpha, "alpha");
    TORCH_CHECK(fx > 0.0f && std::isfinite(fx) && fy > 0.0f && std::isfinite(fy), "fx, fy must be positive and finite, got ", fx, ", ", fy);
    TORCH_CHECK(std::isfinite(cx) && std::isfinite(cy), "cx, cy must be finite, got ", cx, ", ", cy);
    TORCH_CHECK(min_alpha > 0.0f && std::isfinite(min_alpha), "min_alpha must be positive and finite, got ", min_alpha);
    TORCH_CHECK(cos_weight >= 0.0f && std::isfinite(cos_weight) && l1_weight >= 0.0f && std::isfinite(l1_weight),
                "cos_weight and l1_weight must be non-negative and finite, got ", cos_weight, ", ", l1_weight);
    torch::Tensor t, wt;
    if (target.defined()) {
        TORCH_CHECK(target.dim() == 3 && target.size(0) == 3 && target.size(1) == h && target.size(2) == w,
                    "target must be [3, H, W], got ", target.sizes());
        TORCH_CHECK(target.dtype() == torch::kFloat32, "target must be float32, got ", target.dtype());
        TORCH_CHECK(target.is_cuda() && target.device() == depth_map.device(), "target must be on the depth map's CUDA device");
        TORCH_CHECK(cos_weight > 0.0f || l1_weight > 0.0f, "cos_weight and l1_weight must not both be 0");
        t = target.contiguous();
    } else {
        TORCH_CHECK(!weight.defined(), "weight needs a target");
        TORCH_CHECK(want_normals, "without a target there is only the normal map: want_normals must be set");
    }
    if (weight.defined()) { validate_map(weight, "weight"); wt = weight.contiguous(); }
    auto d = depth_map.contiguous(), a = alpha.contiguous();
    auto out = torch::empty({8}, fopt(depth_map));
    NormalLoss o;
    if (want_grad && t.defined()) { o.dL_ddepth_map = torch::empty({h, w}, fopt(depth_map)); o.dL_dalpha = torch::empty({h, w}, fopt(depth_map)); }
    if (want_normals) o.normals = torch::empty({3, h, w}, fopt(depth_map));
    cugs_normal_loss_opts opts{};
    opts.weight = ptr<float>(wt);
    opts.normals_out = ptr<float>(o.normals);
    opts.cos_weight = cos_weight;
    opts.l1_weight = l1_weight;
    opts.min_alpha = min_alpha;
    auto ws = workspace(depth_map.device(), cugs_normal_loss_workspace_bytes(w, h), 11);
    check(cugs_normal_loss(w, h, fx, fy, cx, cy, ptr<float>(d), ptr<float>(a), ptr<float>(t), &opts, ws.data_ptr(), ws.numel(),
                           ptr<float>(out), ptr<float>(o.dL_ddepth_map), ptr<float>(o.dL_dalpha), stream_of(depth_map)),
          "cugs_normal_loss");
    o.loss = out[0]; o.valid_weight = out[1]; o.valid_count = out[2];
    return o;
}

TsdfVolume make_tsdf_volume(const float origin[3], int nx, int ny, int nz, float voxel_size, float trunc, bool color,
                            const torch::Device& device, float max_weight, float min_depth) {
    TORCH_CHECK(nx > 0 && ny > 0 && nz > 0, "the voxel counts must be positive, got ", nx, ", ", ny, ", ", nz);
    TORCH_CHECK(static_cast<int64_t>(nx) * ny * nz <= 2147483647ll, "the volume does not fit 2^31 - 1 voxels");
    TORCH_CHECK(device.is_cuda(), "a TsdfVolume lives on a CUDA device");
    TsdfVolume v;
    v.planes = torch::zeros({color ? 5 : 2, nz, ny, nx}, torch::TensorOptions().dtype(torch::kFloat32).device(device));
    v.planes[0].fill_(1.0f);
    for (int k = 0; k < 3; ++k) v.origin[k] = origin[k];
    v.voxel_size = voxel_size; v.trunc = trunc; v.max_weight = max_weight; v.min_depth = min_depth;
    return v;
}

static cugs_tsdf_volume tsdf_abi(const TsdfVolume& volume) {
    const auto& p = volume.planes;
    TORCH_CHECK(p.defined() && p.dim() == 4 && (p.size(0) == 2 || p.size(0) == 5), "planes must be [2 or 5, nz, ny, nx]");
    TORCH_CHECK(p.dtype() == torch::kFloat32 && p.is_cuda() && p.is_contiguous(), "planes must be contiguous float32 on a CUDA device");
    cugs_tsdf_volume v{};
    v.planes = p.data_ptr<float>();
    v.nx = static_cast<int32_t>(p.size(3)); v.ny = static_cast<int32_t>(p.size(2)); v.nz = static_cast<int32_t>(p.size(1));
    v.color = p.size(0) == 5;
    for (int k = 0; k < 3; ++k) v.origin[k] = volume.origin[k];
    v.voxel_size = volume.voxel_size; v.trunc = volume.trunc;
    return v;
}

void tsdf_integrate(TsdfVolume& volume, const std::vector<TsdfViewInput>& views, float min_alpha) {
    const cugs_tsdf_volume vol = tsdf_abi(volume);
    TORCH_CHECK(min_alpha > 0.0f && std::isfinite(min_alpha), "min_alpha must be positive and finite, got ", min_alpha);
    cugs_tsdf_opts opts{};
    opts.min_depth = volume.min_depth; opts.min_alpha = min_alpha; opts.max_weight = volume.max_weight;
    constexpr size_t kMaxViews = 16;
    for (size_t first = 0; first < views.size(); first += kMaxViews) {
        const size_t n = std::min(kMaxViews, views.size() - first);
        std::vector<cugs_tsdf_view> table(n);
        std::vector<torch::Tensor> keep;                     // the contiguous maps, alive until the launch is queued
        for (size_t i = 0; i < n; ++i) {
            const TsdfViewInput& in = views[first + i];
            const int64_t h = in.camera.height, w = in.camera.width;
            auto map = [&](const torch::Tensor& t, const char* name, bool rgb) -> const float* {
                TORCH_CHECK(t.defined() && t.dim() == (rgb ? 3 : 2) && t.size(0) == h && t.size(1) == w && (!rgb || t.size(2) == 3),
                            name, " must be [H, W", rgb ? ", 3" : "", "] of the view's camera, got ", t.sizes());
                TORCH_CHECK(t.dtype() == torch::kFloat32, name, " must be float32, got ", t.dtype());
                TORCH_CHECK(t.is_cuda() && t.device() == volume.planes.device(), name, " must be on the volume's device");
                keep.push_back(t.contiguous());
                return keep.back().data_ptr<float>();
            };
            cugs_tsdf_view& v = table[i];
            v.camera = in.camera;
            v.depth_map = map(in.depth_map, "depth_map", false);
            v.alpha = map(in.alpha, "alpha", false);
            v.color = volume.has_color() ? map(in.color, "color", true) : nullptr;
            v.weight = in.weight.defined() ? map(in.weight, "weight", false) : nullptr;
        }
        check(cugs_tsdf_integrate(&vol, table.data(), static_cast<int>(n), &opts, stream_of(volume.planes)), "cugs_tsdf_integrate");
    }
}

Mesh mesh_extract(const TsdfVolume& volume, float min_weight) {
    const cugs_tsdf_volume vol = tsdf_abi(volume);
    TORCH_CHECK(min_weight >= 0.0f && std::isfinite(min_weight), "min_weight must be non-negative and finite, got ", min_weight);
    const auto dev = volume.planes.device();
    const size_t bytes = std::max<size_t>(cugs_mesh_workspace_bytes(vol.nx, vol.ny, vol.nz), 256);
    auto ws = torch::empty({static_cast<int64_t>(bytes)}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
    int64_t counts[2] = {0, 0};
    check(cugs_mesh_plan(&vol, min_weight, ws.data_ptr(), bytes, counts, stream_of(volume.planes)), "cugs_mesh_plan");
    Mesh m;
    m.vertices = torch::empty({counts[0], 3}, fopt(volume.planes));
    m.faces = torch::empty({counts[1], 3}, torch::TensorOptions().dtype(torch::kInt32).device(dev));
    if (volume.has_color()) m.colors = torch::empty({counts[0], 3}, fopt(volume.planes));
    check(cugs_mesh_emit(&vol, ws.data_ptr(), bytes, counts[0], counts[1], ptr<float>(m.vertices), ptr<float>(m.colors),
                         ptr<int32_t>(m.faces), stream_of(volume.planes)), "cugs_mesh_emit");
    return m;
}

torch::Tensor depth_to_normals(const torch::Tensor& depth_map, const torch::Tensor& alpha, float fx, float fy, float cx,
                               float cy, float min_alpha) {
    return normal_loss(depth_map, alpha, fx, fy, cx, cy, {}, {}, 1.0f, 0.0f, min_alpha, false, true).normals;
}

namespace {
void validate_image(const torch::Tensor& img, const char* name) {
    TORCH_CHECK(img.dim() == 3 && img.size(2) == 3, name, " must be [H, W, 3], got ", img.sizes());
    TORCH_CHECK(img.dtype() == torch::kFloat32, name, " must be float32, got ", img.dtype());
    TORCH_CHECK(img.is_cuda(), name, " must be on a CUDA device");
}
cugs_bilagrid_dims validate_grid(const torch::Tensor& grid, const torch::Device* dev) {
    TORCH_CHECK(grid.dim() == 4 && grid.size(0) == 12, "grid must be [12, L, GY, GX], got ", grid.sizes());
    for (int a = 1; a < 4; ++a)
        TORCH_CHECK(grid.size(a) >= 2 && grid.size(a) <= 64, "grid extents L, GY, GX must lie in [2, 64], got ", grid.sizes());
    TORCH_CHECK(grid.dtype() == torch::kFloat32, "grid must be float32, got ", grid.dtype());
    TORCH_CHECK(grid.is_cuda() && (!dev || grid.device() == *dev), "grid must be on the image's CUDA device");
    TORCH_CHECK(grid.is_contiguous(), "grid must be contiguous");
    cugs_bilagrid_dims d;
    d.l = static_cast<int32_t>(grid.size(1)); d.gy = static_cast<int32_t>(grid.size(2)); d.gx = static_cast<int32_t>(grid.size(3));
    return d;
}
}  // namespace

torch::Tensor bilagrid_slice(const torch::Tensor& grid, const torch::Tensor& rendered) {
    validate_image(rendered, "rendered");
    const auto dev = rendered.device();
    const auto dims = validate_grid(grid, &dev);
    auto r = rendered.contiguous();
    auto out = torch::empty_like(r);
    check(cugs_bilagrid_slice(static_cast<int>(r.size(1)), static_cast<int>(r.size(0)), &dims, ptr<float>(grid), ptr<float>(r),
                              ptr<float>(out), stream_of(r)), "cugs_bilagrid_slice");
    return out;
}

BilagridGrad bilagrid_slice_backward(const torch::Tensor& grid, const torch::Tensor& rendered,
                                     const torch::Tensor& dL_dcorrected, bool want_grid_grad, bool want_image_grad) {
    validate_image(rendered, "rendered");
    validate_image(dL_dcorrected, "dL_dcorrected");
    TORCH_CHECK(dL_dcorrected.sizes() == rendered.sizes(), "dL_dcorrected must have rendered's shape ", rendered.sizes(),
                ", got ", dL_dcorrected.sizes());
    TORCH_CHECK(dL_dcorrected.device() == rendered.device(), "dL_dcorrected must be on rendered's CUDA device");
    const auto dev = rendered.device();
    const auto dims = validate_grid(grid, &dev);
    const int h = static_cast<int>(rendered.size(0)), w = static_cast<int>(rendered.size(1));
    auto r = rendered.contiguous(), g = dL_dcorrected.contiguous();
    BilagridGrad o;
    if (want_image_grad) o.dL_drendered = torch::empty_like(r);
    if (want_grid_grad) o.dL_dgrid = torch::empty_like(grid);
    torch::Tensor ws;
    if (want_grid_grad) ws = workspace(dev, cugs_bilagrid_workspace_bytes(w, h, &dims), 10);
    check(cugs_bilagrid_slice_backward(w, h, &dims, ptr<float>(grid), ptr<float>(r), ptr<float>(g),
                                       ws.defined() ? ws.data_ptr() : nullptr, ws.defined() ? static_cast<size_t>(ws.numel()) : 0,
                                       ptr<float>(o.dL_drendered), ptr<float>(o.dL_dgrid), stream_of(r)),
          "cugs_bilagrid_slice_backward");
    return o;
}

BilagridTV bilagrid_tv(const torch::Tensor& grid, float weight, const torch::Tensor& dL_dgrid) {
    const auto dims = validate_grid(grid, nullptr);
    BilagridTV o;
    const bool accumulate = dL_dgrid.defined();
    if (accumulate) {
        TORCH_CHECK(dL_dgrid.sizes() == grid.sizes() && dL_dgrid.dtype() == torch::kFloat32 && dL_dgrid.device() == grid.device() &&
                    dL_dgrid.is_contiguous(), "dL_dgrid must be a contiguous float32 tensor of the grid's shape and device");
        o.dL_dgrid = dL_dgrid;
    } else {
        o.dL_dgrid = torch::empty_like(grid);
    }
    auto tv = torch::empty({1}, fopt(grid));
    check(cugs_bilagrid_tv(&dims, ptr<float>(grid), weight, ptr<float>(tv), ptr<float>(o.dL_dgrid), accumulate ? 1 : 0,
                           stream_of(grid)), "cugs_bilagrid_tv");
    o.tv = tv[0];
    return o;
}

FusedAdam::FusedAdam(std::array<torch::Tensor, 5> params, std::array<float, 5> lrs, AdamHyper h)
    : params_(std::move(params)), lrs_(lrs), h_(h) {
    for (int i = 0; i < 5; ++i) { m_[i] = torch::zeros_like(params_[i]); v_[i] = torch::zeros_like(params_[i]); }
}
void FusedAdam::apply_gradients(const BackwardOutput& g) {        // references, no copy (fused_adam.cu:113-120)
    grads_ = {g.dL_dpositions, g.dL_dsh_coeffs, g.dL_dopacities, g.dL_dscales, g.dL_drotations};
}
void FusedAdam::zero_grad() { for (auto& g : grads_) g = torch::Tensor(); }
cugs_adam_fused FusedAdam::begin_fused_step() {
    ++step_count_;
    cugs_adam_fused a{};
    cugs_adam_bias_correction(h_.beta1, h_.beta2, step_count_, &a.bc1, &a.bc2);
    for (int i = 0; i < 5; ++i) {
        TORCH_CHECK(params_[i].is_cuda() && params_[i].is_contiguous() && params_[i].scalar_type() == torch::kFloat32 &&
                    m_[i].is_contiguous() && v_[i].is_contiguous(),
                    "FusedAdam: the fused step needs contiguous float32 CUDA parameters and moments");
        a.m[i] = m_[i].data_ptr<float>(); a.v[i] = v_[i].data_ptr<float>(); a.lr[i] = lrs_[i];
    }
    a.beta1 = h_.beta1; a.beta2 = h_.beta2; a.eps = h_.eps;
    zero_grad();
    return a;
}
void FusedAdam::step() { step_groups(nullptr); }
void FusedAdam::step(const torch::Tensor& visible) {
    const int64_t n_rows = params_[0].size(0);
    TORCH_CHECK(visible.defined() && visible.dim() == 1 && visible.size(0) == n_rows,
                "FusedAdam: visible must be a [N] tensor with N = ", n_rows, " (RenderOutput::radii or a bool mask)");
    TORCH_CHECK(visible.is_cuda() && visible.device() == params_[0].device(),
                "FusedAdam: visible must be on the model's CUDA device");
    TORCH_CHECK(visible.scalar_type() == torch::kInt32 || visible.scalar_type() == torch::kBool,
                "FusedAdam: visible must be int32 radii or a bool mask, got ", visible.dtype());
    const torch::Tensor rows = (visible.scalar_type() == torch::kBool ? visible.to(torch::kInt32) : visible).contiguous();
    step_groups(&rows);
}
void FusedAdam::step_groups(const torch::Tensor* rows) {
    ++step_count_;
    float bc1, bc2;
    cugs_adam_bias_correction(h_.beta1, h_.beta2, step_count_, &bc1, &bc2);
    cugs_adam_group groups[5];
    std::array<torch::Tensor, 5> pc, gc, mc, vc;
    void* st = nullptr;
    for (int i = 0; i < 5; ++i) {
        groups[i] = cugs_adam_group{nullptr, nullptr, nullptr, nullptr, 0, lrs_[i], 0.f};
        if (!grads_[i].defined()) continue;                       // fused_adam.cu:156
        TORCH_CHECK(params_[i].is_cuda(), "FusedAdam: param must be on CUDA");
        TORCH_CHECK(grads_[i].is_cuda(), "FusedAdam: grad must be on CUDA");
        TORCH_CHECK(params_[i].numel() == grads_[i].numel(), "FusedAdam: param/grad size mismatch: ", params_[i].numel(),
                    " vs ", grads_[i].numel());
        pc[i] = params_[i].contiguous(); gc[i] = grads_[i].contiguous(); mc[i] = m_[i].contiguous(); vc[i] = v_[i].contiguous();
        groups[i].param = pc[i].data_ptr<float>(); groups[i].grad = gc[i].data_ptr<float>();
        groups[i].m = mc[i].data_ptr<float>(); groups[i].v = vc[i].data_ptr<float>(); groups[i].n = pc[i].numel();
        st = stream_of(params_[i]);
    }
    if (rows) {
        const int64_t n_rows = rows->size(0);
        int32_t row_elems[5];
        for (int i = 0; i < 5; ++i) {                             // floats per row: 3, 3C, 1, 3, 4
            int64_t w = 1;
            for (int64_t d = 1; d < params_[i].dim(); ++d) w *= params_[i].size(d);
            row_elems[i] = static_cast<int32_t>(w);
        }
        check(cugs_fused_adam_groups_rows(groups, 5, row_elems, rows->data_ptr<int32_t>(), n_rows, h_.beta1, h_.beta2,
                                          h_.eps, bc1, bc2, st), "cugs_fused_adam_groups_rows");
    } else {
        check(cugs_fused_adam_groups(groups, 5, h_.beta1, h_.beta2, h_.eps, bc1, bc2, st), "cugs_fused_adam_groups");
    }
    for (int i = 0; i < 5; ++i) {                                 // fused_adam.cu:216-218
        if (!grads_[i].defined()) continue;
        if (!params_[i].is_contiguous()) params_[i].copy_(pc[i]);
        if (!m_[i].is_contiguous()) m_[i].copy_(mc[i]);
        if (!v_[i].is_contiguous()) v_[i].copy_(vc[i]);
    }
}

// ---------------------------------------------------------------------------------------------
// N2: adaptive density control (optimizer/densification.cpp)
// ---------------------------------------------------------------------------------------------
bool DensificationController::should_densify(int step) const {             // densification.cpp:42-46
    return step >= config_.densify_from && step <= config_.densify_until && step % config_.densify_every == 0;
}
bool DensificationController::should_reset_opacity(int step) const {       // :48-52
    return config_.opacity_reset_every > 0 && step >= config_.densify_from && step % config_.opacity_reset_every == 0;
}
void DensificationController::reset_accumulators(int64_t n, const torch::Device& device) {   // :344-349
    auto o = torch::TensorOptions().dtype(torch::kFloat32).device(device);
    grad_accum_ = torch::zeros({n}, o); grad_count_ = torch::zeros({n}, o); max_radii_2d_ = torch::zeros({n}, o);
}
void DensificationController::accumulate_gradients(const torch::Tensor& dL_dmeans_2d, const torch::Tensor& radii) {
    TORCH_CHECK(dL_dmeans_2d.is_cuda() && radii.is_cuda(), "accumulate_gradients: tensors must be on CUDA");
    TORCH_CHECK(dL_dmeans_2d.dim() == 2 && dL_dmeans_2d.size(1) == 2, "dL_dmeans_2d must be [N, 2]");
    const int64_t n = dL_dmeans_2d.size(0);
    TORCH_CHECK(radii.numel() == n, "radii must be [N]");
    if (!grad_accum_.defined() || grad_accum_.size(0) != n) reset_accumulators(n, dL_dmeans_2d.device());
    auto r = radii.contiguous().to(torch::kInt32);
    // a strided [N,2] view (BackwardOutput::dL_dmeans_2d_abs: words 10, 11 of the accumulator rows) is read in place
    const int64_t row = n > 0 ? dL_dmeans_2d.stride(0) : 2;
    if (dL_dmeans_2d.scalar_type() == torch::kFloat32 && !dL_dmeans_2d.is_contiguous() && dL_dmeans_2d.stride(1) == 1 &&
        row >= 2 && row % 2 == 0 && reinterpret_cast<uintptr_t>(dL_dmeans_2d.data_ptr()) % 8 == 0) {
        check(cugs_densify_accumulate_strided(n, dL_dmeans_2d.data_ptr<float>(), row, ptr<int32_t>(r),
                                              ptr<float>(grad_accum_), ptr<float>(grad_count_), ptr<float>(max_radii_2d_),
                                              stream_of(dL_dmeans_2d)), "cugs_densify_accumulate_strided");
        return;
    }
    auto g = dL_dmeans_2d.contiguous().to(torch::kFloat32);
    check(cugs_densify_accumulate(n, ptr<float>(g), ptr<int32_t>(r), ptr<float>(grad_accum_), ptr<float>(grad_count_),
                                  ptr<float>(max_radii_2d_), stream_of(g)), "cugs_densify_accumulate");
}
void DensificationController::reset_opacity(ModelTensors& model) {          // :331-334
    torch::NoGradGuard no_grad;
    model.opacities.fill_(-4.59511985013459f);
}
DensificationStats DensificationController::densify(ModelTensors& model, int step, const torch::Tensor& noise_in,
                                                    FusedAdam* optimizer) {
    torch::NoGradGuard no_grad;
    DensificationStats stats;
    const int64_t n = model.positions.size(0);
    stats.num_before = stats.num_after = static_cast<int>(n);
    if (n == 0) return stats;
    TORCH_CHECK(model.positions.is_cuda(), "densify: model must be on CUDA");
    const auto dev = model.positions.device();
    if (!grad_accum_.defined() || grad_accum_.size(0) != n) reset_accumulators(n, dev);
    void* st = stream_of(model.positions);
    auto scales_c = model.scales.contiguous(), opa_c = model.opacities.contiguous();
    auto flags = torch::empty({n}, torch::TensorOptions().dtype(torch::kUInt8).device(dev));
    auto avg = torch::empty({n}, fopt(model.positions));
    const float size_thr = config_.percent_dense * scene_extent_;           // :367, :394
    const float ws_thr = 0.1f * scene_extent_;                              // :436
    const int size_pruning = config_.opacity_reset_every > 0 && step > config_.opacity_reset_every;   // :415-416
    check(cugs_densify_classify(n, ptr<float>(grad_accum_), ptr<float>(grad_count_), ptr<float>(max_radii_2d_),
                                ptr<float>(scales_c), ptr<float>(opa_c), config_.grad_threshold, size_thr,
                                config_.opacity_threshold, size_pruning, static_cast<float>(config_.max_screen_size),
                                ws_thr, flags.data_ptr<uint8_t>(), ptr<float>(avg), st), "cugs_densify_classify");
    if (config_.max_gaussians > 0) {                                        // :121-139, :184-209 (rare path: libtorch topk)
        auto clone = flags.bitwise_and(1).to(torch::kBool);
        int64_t num_clone = clone.sum().item<int64_t>();
        const int64_t budget = config_.max_gaussians - n;
        if (num_clone > budget) {
            auto keep_clone = torch::zeros_like(clone);
            if (budget > 0) keep_clone.index_fill_(0, std::get<1>(avg.masked_fill(~clone, -1.0f).topk(budget)), true);
            clone = keep_clone;
            num_clone = budget > 0 ? budget : 0;
        }
        auto split = flags.bitwise_right_shift(1).bitwise_and(1).to(torch::kBool);
        const int64_t num_split = split.sum().item<int64_t>();
        const int64_t sbudget = (config_.max_gaussians - (n + num_clone)) / 2;
        if (num_split > sbudget) {
            auto keep_split = torch::zeros_like(split);
            if (sbudget > 0) keep_split.index_fill_(0, std::get<1>(avg.masked_fill(~split, -1.0f).topk(sbudget)), true);
            split = keep_split;
        }
        flags = flags.bitwise_and(4).bitwise_or(clone.to(torch::kUInt8)).bitwise_or(split.to(torch::kUInt8).bitwise_left_shift(1)).contiguous();
    }
    auto ws = workspace(dev, cugs_densify_workspace_bytes(n), 3);
    int64_t counts[4];
    check(cugs_densify_plan(n, flags.data_ptr<uint8_t>(), ws.data_ptr(), ws.numel(), counts, st), "cugs_densify_plan");
    const int64_t n_out = counts[3];
    torch::Tensor noise = noise_in.defined() ? noise_in.contiguous().to(torch::kFloat32)
                                             : (counts[2] > 0 ? torch::randn({2, n, 3}, fopt(model.positions))
                                                              : torch::zeros({2, n, 3}, fopt(model.positions)));
    TORCH_CHECK(noise.is_cuda() && noise.dim() == 3 && noise.size(0) == 2 && noise.size(1) == n && noise.size(2) == 3,
                "noise must be [2, N, 3] on CUDA");
    std::vector<torch::Tensor> srcs, dsts;
    std::vector<cugs_densify_array> desc;
    auto add = [&](const torch::Tensor& src, int mode) {
        auto s = src.contiguous();
        auto sizes = s.sizes().vec();
        sizes[0] = n_out;
        auto d = torch::empty(sizes, fopt(model.positions));
        srcs.push_back(s); dsts.push_back(d);
        desc.push_back(cugs_densify_array{s.data_ptr<float>(), d.data_ptr<float>(), static_cast<int32_t>(s.numel() / n), mode});
        return d;
    };
    auto new_pos = add(model.positions, CUGS_DENSIFY_POSITIONS);
    auto new_sh = add(model.sh_coeffs, CUGS_DENSIFY_COPY);
    auto new_opa = add(model.opacities, CUGS_DENSIFY_COPY);
    auto new_rot = add(model.rotations, CUGS_DENSIFY_COPY);
    auto new_scl = add(model.scales, CUGS_DENSIFY_SCALES);
    std::array<torch::Tensor, 5> nm, nv;
    if (optimizer) for (int i = 0; i < 5; ++i) { nm[i] = add(optimizer->m_[i], CUGS_DENSIFY_STATE); nv[i] = add(optimizer->v_[i], CUGS_DENSIFY_STATE); }
    if (n_out > 0)
        check(cugs_densify_apply(n, n_out, ws.data_ptr(), ws.numel(), ptr<float>(noise), ptr<float>(scales_c), desc.data(),
                                 static_cast<int>(desc.size()), st), "cugs_densify_apply");
    model.positions = new_pos; model.sh_coeffs = new_sh; model.opacities = new_opa; model.rotations = new_rot; model.scales = new_scl;
    if (optimizer) {
        optimizer->params_ = {model.positions, model.sh_coeffs, model.opacities, model.scales, model.rotations};
        optimizer->m_ = nm; optimizer->v_ = nv;
        optimizer->zero_grad();
    }
    stats.num_cloned = static_cast<int>(counts[1]);
    stats.num_split = static_cast<int>(counts[2]);
    stats.num_pruned = static_cast<int>(n + counts[1] + 2 * counts[2] - n_out);   // :313-316
    stats.num_after = static_cast<int>(n_out);
    reset_accumulators(n_out, dev);                                               // :321
    return stats;
}

// N4: training target from a cached 8-bit view
torch::Tensor image_to_float(const torch::Tensor& view_u8, int width, int height) {
    TORCH_CHECK(view_u8.is_cuda() && view_u8.dtype() == torch::kUInt8 && view_u8.dim() == 3 && view_u8.size(2) == 3,
                "image must be a uint8 [H, W, 3] CUDA tensor");
    if (width <= 0 || height <= 0) throw std::runtime_error("Invalid target dimensions for resize");   // image_io.cpp:48-50
    auto src = view_u8.contiguous();
    auto dst = torch::empty({height, width, 3}, torch::TensorOptions().dtype(torch::kFloat32).device(src.device()));
    check(cugs_image_to_float(static_cast<int>(src.size(1)), static_cast<int>(src.size(0)), src.data_ptr<uint8_t>(), width,
                              height, dst.data_ptr<float>(), stream_of(src)), "cugs_image_to_float");
    return dst;
}

// ---------------------------------------------------------------------------------------------
// Evaluation metrics (training/metrics.cpp)
// ---------------------------------------------------------------------------------------------
namespace {
torch::Tensor run_eval(const torch::Tensor& rendered, const torch::Tensor& target, const torch::Tensor& out_in,
                       int window_size, const char* who) {
    TORCH_CHECK(rendered.sizes() == target.sizes(), who, ": rendered and target must have same shape");   // metrics.cpp:22-25
    TORCH_CHECK(rendered.dim() == 3 && rendered.size(2) == 3, who, ": expected [H, W, 3] tensors");
    TORCH_CHECK(rendered.dtype() == torch::kFloat32, who, ": rendered must be float32, got ", rendered.dtype());
    TORCH_CHECK(target.dtype() == torch::kFloat32 || target.dtype() == torch::kUInt8, who,
                ": target must be float32 or uint8, got ", target.dtype());
    TORCH_CHECK(rendered.is_cuda() && target.is_cuda(), who, ": rendered and target must be on a CUDA device");
    TORCH_CHECK(rendered.device() == target.device(), who, ": rendered and target must be on the same device");
    TORCH_CHECK(window_size % 2 == 1, "window_size must be odd, got ", window_size);
    TORCH_CHECK(window_size >= 3 && window_size <= 15, "window_size must be in 3..15, got ", window_size);
    torch::Tensor out = out_in;
    if (!out.defined()) {
        out = torch::empty({4}, fopt(rendered));
    } else {
        TORCH_CHECK(out.dtype() == torch::kFloat32 && out.device() == rendered.device() && out.numel() == 4 &&
                    out.is_contiguous(), who, ": out must be a contiguous float32 [4] on the images' device");
    }
    const int h = static_cast<int>(rendered.size(0)), w = static_cast<int>(rendered.size(1));
    auto r = rendered.contiguous(), t = target.contiguous();
    const bool f32 = t.dtype() == torch::kFloat32;
    auto ws = workspace(rendered.device(), cugs_eval_workspace_bytes(w, h), 8);
    check(cugs_eval_metrics(w, h, ptr<float>(r), f32 ? ptr<float>(t) : nullptr, f32 ? nullptr : ptr<uint8_t>(t),
                            window_size, ws.data_ptr(), ws.numel(), ptr<float>(out), stream_of(rendered)),
          "cugs_eval_metrics");
    return out;
}
}  // namespace

torch::Tensor eval_metrics(const torch::Tensor& rendered, const torch::Tensor& target, const torch::Tensor& out,
                           int window_size) {
    return run_eval(rendered, target, out, window_size, "eval_metrics");
}
float psnr_from_mse(float mse) {                                  // metrics.cpp:27-34
    if (mse < 1e-10f) return 100.0f;
    return 10.0f * std::log10(1.0f / mse);
}
float compute_psnr(const torch::Tensor& rendered, const torch::Tensor& target) {
    return psnr_from_mse(run_eval(rendered, target, {}, 11, "PSNR").cpu().data_ptr<float>()[0]);
}
float compute_ssim(const torch::Tensor& rendered, const torch::Tensor& target) {
    return run_eval(rendered, target, {}, 11, "SSIM").cpu().data_ptr<float>()[1];
}

EvalResults evaluate(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                     const std::vector<torch::Tensor>& targets, const RenderSettings& settings,
                     const std::vector<std::string>& names) {
    const size_t num_test = cameras.size();
    if (num_test == 0) return {};                                 // metrics.cpp:98-102
    TORCH_CHECK(targets.size() >= num_test, "evaluate: ", num_test, " cameras but ", targets.size(), " targets");
    TORCH_CHECK(names.empty() || names.size() >= num_test, "evaluate: fewer image names than cameras");
    EvalResults results;
    results.num_gaussians = static_cast<int>(model.positions.size(0));
    results.sh_degree = settings.active_sh_degree;
    const auto t_start = std::chrono::steady_clock::now();
    torch::NoGradGuard no_grad;
    auto table = torch::empty({static_cast<int64_t>(num_test), 4}, fopt(model.positions));
    for (size_t v = 0; v < num_test; ++v) {
        const cugs_camera& cam = cameras[v];
        auto color = render(model, cam, settings, /*for_backward=*/false).color;
        torch::Tensor tgt = targets[v];
        if (tgt.dtype() == torch::kUInt8 && tgt.dim() == 3 && (tgt.size(1) != cam.width || tgt.size(0) != cam.height))
            tgt = image_to_float(tgt, cam.width, cam.height);     // the reference's resize, metrics.cpp:121-128
        run_eval(color, tgt, table[static_cast<int64_t>(v)], 11, "evaluate");
    }
    const auto rows = table.cpu();                                // the one read-back
    const float* m = rows.data_ptr<float>();
    float sum_psnr = 0.0f, sum_ssim = 0.0f;
    for (size_t v = 0; v < num_test; ++v) {
        ImageMetrics im;
        if (!names.empty()) im.image_name = names[v];
        im.psnr = psnr_from_mse(m[4 * v]);
        im.ssim = m[4 * v + 1];
        results.per_image.push_back(im);
        sum_psnr += im.psnr;                                      // metrics.cpp:143-151
        sum_ssim += im.ssim;
    }
    results.mean_psnr = sum_psnr / static_cast<float>(num_test);
    results.mean_ssim = sum_ssim / static_cast<float>(num_test);
    results.eval_time_seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - t_start).count();
    return results;
}

// ---------------------------------------------------------------------------------------------
// N3: PLY checkpoints (utils/ply_io.cpp:98-196, 258-351)
// ---------------------------------------------------------------------------------------------
namespace {
std::vector<std::string> ply_model_names(int c) {                 // record order without the normals
    std::vector<std::string> n = {"x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2"};
    for (int i = 0; i < 3 * (c - 1); ++i) n.push_back("f_rest_" + std::to_string(i));
    for (const char* p : {"opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"}) n.push_back(p);
    return n;
}
}  // namespace

bool write_gaussian_ply(const std::string& path, const ModelTensors& model, const FusedAdam* optimizer) {
    const auto& p0 = model.positions;
    if (!p0.defined() || p0.dim() != 2 || p0.size(1) != 3 || !model.sh_coeffs.defined() || model.sh_coeffs.dim() != 3 ||
        model.sh_coeffs.size(0) != p0.size(0) || model.sh_coeffs.size(1) != 3 || model.opacities.numel() != p0.size(0) ||
        model.scales.numel() != 3 * p0.size(0) || model.rotations.numel() != 4 * p0.size(0))
        return false;                                             // ply_io.cpp:100-103 (is_valid)
    const auto dev = p0.is_cuda() ? p0.device() : torch::Device(torch::kCUDA, c10::hip::current_device());
    auto f32 = [&](const torch::Tensor& t) { return t.to(dev).contiguous().to(torch::kFloat32); };
    std::array<torch::Tensor, 5> pr = {f32(model.positions), f32(model.sh_coeffs), f32(model.opacities), f32(model.scales),
                                       f32(model.rotations)}, mm, vv;
    const int64_t n = pr[0].size(0);
    const int c = static_cast<int>(pr[1].size(2));
    const bool state = optimizer != nullptr;
    const float *pp[5], *pm[5], *pv[5];
    for (int i = 0; i < 5; ++i) {
        pp[i] = pr[i].data_ptr<float>();
        if (state) { mm[i] = f32(optimizer->m_[i]); vv[i] = f32(optimizer->v_[i]); pm[i] = mm[i].data_ptr<float>(); pv[i] = vv[i].data_ptr<float>(); }
    }
    const int row = cugs_ply_vertex_floats(c, state ? 1 : 0);
    auto verts = torch::empty({n, row}, fopt(pr[0]));
    check(cugs_ply_pack(n, c, pp, state ? pm : nullptr, state ? pv : nullptr, ptr<float>(verts), stream_of(pr[0])), "cugs_ply_pack");
    auto host = verts.cpu();                                      // one device-to-host copy of the finished records
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    std::string head = "ply\nformat binary_little_endian 1.0\n";
    if (state) head += "comment cugs_adam_step " + std::to_string(optimizer->step_count_) + "\n";
    head += "element vertex " + std::to_string(n) + "\n";
    auto names = ply_model_names(c);
    auto emit = [&](const std::string& prefix, bool normals) {
        for (size_t i = 0; i < names.size(); ++i) {
            head += "property float " + prefix + names[i] + "\n";
            if (normals && i == 2) head += "property float nx\nproperty float ny\nproperty float nz\n";
        }
    };
    emit("", true);
    if (state) { emit("m_", false); emit("v_", false); }
    head += "end_header\n";
    bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
    const size_t bytes = static_cast<size_t>(n) * row * sizeof(float);
    ok = ok && (bytes == 0 || fwrite(host.data_ptr<float>(), 1, bytes, f) == bytes);
    return (fclose(f) == 0) && ok;
}

ModelTensors read_gaussian_ply(const std::string& path, const torch::Device& device, FusedAdam* optimizer) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("Failed to open PLY file: " + path);
    std::string buf;
    {
        char chunk[1 << 16];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.append(chunk, got);
        fclose(f);
    }
    // parse_ply_header (ply_io.cpp:211-250)
    size_t pos = 0;
    std::vector<std::string> lines;
    while (true) {
        const size_t end = buf.find('\n', pos);
        if (end == std::string::npos) throw std::runtime_error("Not a PLY file");
        std::string line = buf.substr(pos, end - pos);
        if (!line.empty() && line.back() == '\r') line.pop_back();
        pos = end + 1;
        lines.push_back(line);
        if (line == "end_header") break;
    }
    if (lines[0].find("ply") == std::string::npos) throw std::runtime_error("Not a PLY file");
    if (lines.size() < 2 || lines[1].find("binary_little_endian") == std::string::npos)
        throw std::runtime_error("Only binary_little_endian PLY is supported");
    int64_t n = 0;
    long step = 0;
    std::vector<std::string> names;
    for (size_t i = 2; i < lines.size(); ++i) {
        char a[64] = {0}, b[64] = {0}, c3[64] = {0};
        const int got = sscanf(lines[i].c_str(), "%63s %63s %63s", a, b, c3);
        if (got >= 3 && std::string(a) == "element" && std::string(b) == "vertex") n = atoll(c3);
        else if (got >= 3 && std::string(a) == "property") names.push_back(c3);
        else if (got == 3 && std::string(a) == "comment" && std::string(b) == "cugs_adam_step") step = atol(c3);
    }
    std::map<std::string, int> index;
    for (size_t i = 0; i < names.size(); ++i) index[names[i]] = static_cast<int>(i);
    int num_rest = 0;
    while (index.count("f_rest_" + std::to_string(num_rest))) ++num_rest;
    const int c = 1 + num_rest / 3;                               // :283
    const bool state = optimizer != nullptr && index.count("m_x") && index.count("v_x");
    auto canon = ply_model_names(c);
    std::vector<int32_t> col_of;
    for (const char* prefix : {"", "m_", "v_"}) {
        if (prefix[0] && !state) break;
        for (auto& nm : canon) {
            auto it = index.find(std::string(prefix) + nm);
            if (it == index.end()) throw std::runtime_error("Missing PLY property: " + std::string(prefix) + nm);
            col_of.push_back(it->second);
        }
    }
    const int num_props = static_cast<int>(names.size());
    if (buf.size() - pos < static_cast<size_t>(n) * num_props * sizeof(float)) throw std::runtime_error("Failed to read PLY binary data");
    const auto work = device.is_cuda() ? device : torch::Device(torch::kCUDA, c10::hip::current_device());
    auto data = torch::from_blob(const_cast<char*>(buf.data() + pos), {n * num_props}, torch::kFloat32).to(work);
    auto cols = torch::from_blob(col_of.data(), {static_cast<int64_t>(col_of.size())}, torch::kInt32).to(work);
    auto o = torch::TensorOptions().dtype(torch::kFloat32).device(work);
    auto mk = [&] { return std::array<torch::Tensor, 5>{torch::empty({n, 3}, o), torch::empty({n, 3, c}, o), torch::empty({n, 1}, o),
                                                        torch::empty({n, 3}, o), torch::empty({n, 4}, o)}; };
    auto pr = mk();
    std::array<torch::Tensor, 5> mm, vv;
    float *pp[5], *pm[5], *pv[5];
    if (state) { mm = mk(); vv = mk(); }
    for (int i = 0; i < 5; ++i) { pp[i] = ptr<float>(pr[i]); if (state) { pm[i] = ptr<float>(mm[i]); pv[i] = ptr<float>(vv[i]); } }
    check(cugs_ply_unpack(n, c, num_props, ptr<float>(data), cols.data_ptr<int32_t>(), pp, state ? pm : nullptr,
                          state ? pv : nullptr, stream_of(data)), "cugs_ply_unpack");
    ModelTensors m{pr[0].to(device), pr[1].to(device), pr[2].to(device), pr[4].to(device), pr[3].to(device)};
    if (state) {
        for (int i = 0; i < 5; ++i) {
            TORCH_CHECK(optimizer->m_[i].sizes() == mm[i].sizes(), "optimizer state shape mismatch");
            optimizer->m_[i] = mm[i].to(optimizer->m_[i].device());
            optimizer->v_[i] = vv[i].to(optimizer->v_[i].device());
        }
        optimizer->step_count_ = static_cast<int>(step);
    }
    return m;
}

// ---- N5: MCMC densification (optimizer/mcmc_densification.cpp) ----
namespace {
void check_model(const ModelTensors& m, const char* what) {
    for (const torch::Tensor* t : {&m.positions, &m.sh_coeffs, &m.opacities, &m.rotations, &m.scales})
        TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->is_contiguous(), what,
                    ": the model tensors must be contiguous float32 CUDA tensors (updated in place)");
}
}  // namespace

bool MCMCController::should_relocate(int step) const {                                      // :30-34
    return step >= config_.relocate_from && step <= config_.relocate_until && step % config_.relocate_every == 0;
}

float MCMCController::noise_lr(int step) const {                                             // :40-50
    if (step >= config_.noise_lr_max_steps) return config_.noise_lr_final;
    if (step <= 0) return config_.noise_lr_init;
    const float t = static_cast<float>(step) / static_cast<float>(config_.noise_lr_max_steps);
    const float log_ratio = std::log(config_.noise_lr_final / config_.noise_lr_init);
    return config_.noise_lr_init * std::exp(t * log_ratio);
}

MCMCStats MCMCController::relocate(ModelTensors& model, int step, FusedAdam* optimizer, const torch::Tensor& sources_out) {
    MCMCStats stats;
    const int64_t n = model.positions.defined() ? model.positions.size(0) : 0;
    stats.num_total = static_cast<int>(n);
    if (n == 0) return stats;
    check_model(model, "relocate");
    const auto dev = model.positions.device();
    float* m[5];
    float* v[5];
    if (optimizer) {
        TORCH_CHECK(optimizer->params_[0].data_ptr() == model.positions.data_ptr(),
                    "relocate: the optimizer must have been built on this model");
        for (int g = 0; g < 5; ++g) {
            TORCH_CHECK(optimizer->m_[g].is_contiguous() && optimizer->v_[g].is_contiguous(),
                        "relocate: the optimizer moments must be contiguous");
            m[g] = optimizer->m_[g].data_ptr<float>();
            v[g] = optimizer->v_[g].data_ptr<float>();
        }
    }
    if (sources_out.defined())
        TORCH_CHECK(sources_out.is_cuda() && sources_out.scalar_type() == torch::kInt32 && sources_out.numel() >= n &&
                    sources_out.is_contiguous(), "sources_out must be a contiguous int32 CUDA tensor of N");
    auto ws = workspace(dev, cugs_mcmc_relocate_workspace_bytes(n), 5);
    auto out = torch::zeros({2}, iopt(model.positions));
    check(cugs_mcmc_relocate(n, static_cast<int>(model.sh_coeffs.size(2)), ptr<float>(model.positions),
                             ptr<float>(model.rotations), ptr<float>(model.scales), ptr<float>(model.opacities),
                             ptr<float>(model.sh_coeffs), config_.dead_opacity_threshold, config_.relocate_cap,
                             scene_extent_, config_.seed, static_cast<uint32_t>(step), optimizer ? m : nullptr,
                             optimizer ? v : nullptr, ws.data_ptr(), static_cast<size_t>(ws.numel()), ptr<int32_t>(out),
                             sources_out.defined() ? sources_out.data_ptr<int32_t>() : nullptr,
                             stream_of(model.positions)),
          "cugs_mcmc_relocate");
    auto host = out.to(torch::kCPU);
    stats.num_dead = host[0].item<int>();
    stats.num_relocated = host[1].item<int>();
    return stats;
}

void MCMCController::inject_noise(ModelTensors& model, int step, const torch::Tensor& noise_in) const {   // :144-161
    const int64_t n = model.positions.defined() ? model.positions.size(0) : 0;
    if (n == 0) return;
    check_model(model, "inject_noise");
    torch::Tensor noise;
    if (noise_in.defined()) {
        TORCH_CHECK(noise_in.is_cuda() && noise_in.dim() == 2 && noise_in.size(0) == n && noise_in.size(1) == 3,
                    "noise must be [N, 3] on CUDA");
        noise = f32c(noise_in);
    }
    check(cugs_mcmc_inject_noise(n, ptr<float>(model.positions), ptr<float>(model.scales), ptr<float>(model.opacities),
                                 noise_lr(step), config_.noise_gate_k, config_.noise_gate_t,
                                 noise.defined() ? ptr<float>(noise) : nullptr, config_.seed, static_cast<uint32_t>(step),
                                 stream_of(model.positions)),
          "cugs_mcmc_inject_noise");
}

torch::Tensor MCMCController::compute_regularization(const ModelTensors& model, torch::Tensor& reg_dL_dopacities,
                                                     torch::Tensor& reg_dL_dscales) const {     // :167-186
    const int64_t n = model.positions.size(0);
    auto value = torch::zeros({}, fopt(model.positions));
    reg_dL_dopacities = torch::empty({n, 1}, fopt(model.positions));
    reg_dL_dscales = torch::empty({n, 3}, fopt(model.positions));
    if (n == 0) return value;
    auto opa = f32c(model.opacities), scl = f32c(model.scales);
    auto ws = workspace(model.positions.device(), cugs_mcmc_relocate_workspace_bytes(0), 6);
    check(cugs_mcmc_regularization(n, ptr<float>(opa), ptr<float>(scl), config_.lambda_opacity, config_.lambda_scale,
                                   nullptr, nullptr, ptr<float>(reg_dL_dopacities), ptr<float>(reg_dL_dscales),
                                   ptr<float>(value), ws.data_ptr(), static_cast<size_t>(ws.numel()),
                                   stream_of(model.positions)),
          "cugs_mcmc_regularization");
    return value;
}

cugs_mcmc_fused MCMCController::fused_args(int step, const torch::Tensor& noise) const {
    cugs_mcmc_fused a{};
    a.lambda_opacity = config_.lambda_opacity; a.lambda_scale = config_.lambda_scale;
    a.noise_lr = noise_lr(step); a.gate_k = config_.noise_gate_k; a.gate_t = config_.noise_gate_t;
    a.step = static_cast<uint32_t>(step); a.seed = config_.seed;
    a.noise = noise.defined() ? noise.data_ptr<float>() : nullptr;
    return a;
}

// ---- core/gaussian_init.cpp over csrc/knn.hip ----
namespace {
torch::Device init_device(const torch::Tensor& positions, const c10::optional<torch::Device>& device) {
    if (device.has_value()) {
        if (device->is_cuda() && !device->has_index()) return torch::Device(torch::kCUDA, c10::hip::current_device());
        return *device;
    }
    if (positions.is_cuda()) return positions.device();
    return torch::Device(torch::kCUDA, c10::hip::current_device());
}
torch::Tensor mean_distances_on(const torch::Tensor& pos, int k_neighbors, int route) {
    TORCH_CHECK(k_neighbors >= 1 && k_neighbors <= 16, "k_neighbors must be 1..16, got ", k_neighbors);
    TORCH_CHECK(route == CUGS_KNN_AUTO || route == CUGS_KNN_EXHAUSTIVE || route == CUGS_KNN_TREE, "unknown route ", route);
    const int64_t n = pos.size(0);
    auto out = torch::empty({n}, fopt(pos));
    if (n == 0) return out;
    torch::Tensor ws;
    if (route != CUGS_KNN_EXHAUSTIVE) ws = workspace(pos.device(), cugs_knn_workspace_bytes(n, k_neighbors), 7);
    check(cugs_knn_mean_distances(n, k_neighbors, ptr<float>(pos), ptr<float>(out), ws.defined() ? ws.data_ptr() : nullptr,
                                  ws.defined() ? static_cast<size_t>(ws.numel()) : 0, route, stream_of(pos)),
          "cugs_knn_mean_distances");
    return out;
}
torch::Tensor positions_on(const torch::Tensor& positions, const torch::Device& dev) {
    TORCH_CHECK(positions.dim() == 2 && positions.size(1) == 3, "positions must be [N, 3]");
    return positions.to(dev, torch::kFloat32).contiguous();
}
}  // namespace

torch::Tensor knn_mean_distances(const torch::Tensor& positions, int k_neighbors, int route,
                                 c10::optional<torch::Device> device) {
    return mean_distances_on(positions_on(positions, init_device(positions, device)), k_neighbors, route);
}

ModelTensors init_gaussians_from_sparse(const torch::Tensor& positions, const torch::Tensor& colors, int sh_degree,
                                        int k_neighbors, int route, c10::optional<torch::Device> device) {
    TORCH_CHECK(sh_degree >= 0 && sh_degree <= 3, "SH degree must be 0..", 3, ", got ", sh_degree);   // gaussian_init.cpp:77-78
    const auto dev = init_device(positions, device);
    auto pos = positions_on(positions, dev);
    const int64_t n = pos.size(0);
    TORCH_CHECK(colors.dim() == 2 && colors.size(0) == n && colors.size(1) == 3, "colors must be [N, 3]");
    TORCH_CHECK(colors.scalar_type() == torch::kUInt8, "colors must be uint8");
    auto col = colors.to(dev).contiguous();
    const int64_t C = static_cast<int64_t>(sh_degree + 1) * (sh_degree + 1);
    ModelTensors m{torch::empty({n, 3}, fopt(pos)), torch::empty({n, 3, C}, fopt(pos)), torch::empty({n, 1}, fopt(pos)),
                   torch::empty({n, 4}, fopt(pos)), torch::empty({n, 3}, fopt(pos))};
    if (n == 0) return m;                                                                            // :88-95
    auto mean = mean_distances_on(pos, k_neighbors, route);
    check(cugs_init_from_points(n, static_cast<int>(C), ptr<float>(pos), col.data_ptr<uint8_t>(), ptr<float>(mean),
                                ptr<float>(m.positions), ptr<float>(m.sh_coeffs), ptr<float>(m.opacities),
                                ptr<float>(m.rotations), ptr<float>(m.scales), stream_of(pos)),
          "cugs_init_from_points");
    return m;
}

// ---- contribution scores and score-based pruning ----
ContributionScores::ContributionScores(int64_t n, const torch::Device& device)
    : table(torch::zeros({n, 4}, torch::TensorOptions().dtype(torch::kInt32).device(device))) {}
torch::Tensor ContributionScores::weight_sum() const { return table.view(torch::kFloat32).select(1, 0); }
torch::Tensor ContributionScores::weight_max() const { return table.view(torch::kFloat32).select(1, 1); }
torch::Tensor ContributionScores::pixel_count() const {
    return table.select(1, 2).to(torch::kInt64).bitwise_and(static_cast<int64_t>(0xFFFFFFFFll));
}
void ContributionScores::reset() { table.zero_(); num_views = 0; }

namespace {
void launch_scores(ContributionScores& scores, int width, int height, const torch::Tensor& tile_ranges,
                   const torch::Tensor& gaussian_indices, const torch::Tensor& means_2d, const torch::Tensor& cov_2d_inv,
                   const torch::Tensor& opacities_act, const torch::Tensor& packed, const torch::Tensor& tile_order) {
    auto tr = tile_ranges.contiguous(), gi = gaussian_indices.contiguous();
    auto m = means_2d.contiguous(), c = cov_2d_inv.contiguous(), op = opacities_act.contiguous();
    auto pk = packed.defined() ? packed.contiguous() : packed;
    if (tile_order.defined())
        TORCH_CHECK(tile_order.is_contiguous() && tile_order.scalar_type() == torch::kInt32 &&
                    tile_order.numel() == 4 * tr.size(0), "tile_order must be a contiguous [tiles, 4] int32 tensor");
    check(cugs_blend_scores(width, height, ptr<int32_t>(tr), ptr<int32_t>(gi), ptr<float>(m), ptr<float>(c), ptr<float>(op),
                            ptr<float>(pk), order_ptr(tile_order), static_cast<int>(scores.n()),
                            scores.n() > 0 ? scores.table.data_ptr() : nullptr, stream_of(scores.table)),
          "cugs_blend_scores");
    ++scores.num_views;
}
}  // namespace

void accumulate_contribution_scores(ContributionScores& scores, const RenderOutput& out, const cugs_camera& camera) {
    const int64_t n = out.means_2d.size(0);
    TORCH_CHECK(n == scores.n(), "accumulate_contribution_scores: the table holds ", scores.n(), " Gaussians, the render ", n);
    if (n == 0) { ++scores.num_views; return; }
    TORCH_CHECK(out.means_2d.device() == scores.table.device(), "accumulate_contribution_scores: the score table is on another device");
    launch_scores(scores, camera.width, camera.height, out.tile_ranges, out.gaussian_indices, out.means_2d, out.cov_2d_inv,
                  out.opacities_act, out.packed, out.tile_order);
}

ContributionScores contribution_scores(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                                       const RenderSettings& settings) {
    TORCH_CHECK(model.positions.is_cuda(), "GaussianModel must be on CUDA device");
    const int64_t n = model.positions.size(0);
    ContributionScores scores(n, model.positions.device());
    for (const auto& cam : cameras) {
        if (n == 0) { ++scores.num_views; continue; }
        auto proj = project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam,
                                      0, settings.scale_modifier);             // degree 0: the colour is not used
        auto srt = sort_gaussians(proj.means_2d, proj.depths, proj.radii, proj.tiles_touched, cam.width, cam.height);
        launch_scores(scores, cam.width, cam.height, srt.tile_ranges, srt.gaussian_values_sorted, proj.means_2d,
                      proj.cov_2d_inv, proj.opacities_act, proj.packed, {});
    }
    return scores;
}

int64_t prune_gaussians(ModelTensors& model, const torch::Tensor& prune_mask, FusedAdam* optimizer) {
    torch::NoGradGuard no_grad;
    const int64_t n = model.positions.size(0);
    TORCH_CHECK(model.positions.is_cuda(), "prune_gaussians: model must be on CUDA");
    TORCH_CHECK(prune_mask.defined() && prune_mask.scalar_type() == torch::kBool && prune_mask.dim() == 1 &&
                prune_mask.size(0) == n, "prune_gaussians: prune_mask must be a bool tensor of shape [", n, "]");
    TORCH_CHECK(prune_mask.device() == model.positions.device(), "prune_gaussians: prune_mask must be on the model's device");
    if (n == 0) return 0;
    const auto dev = model.positions.device();
    void* st = stream_of(model.positions);
    auto flags = prune_mask.logical_not().to(torch::kUInt8).bitwise_left_shift(2).contiguous();   // bit 2: keep
    auto ws = workspace(dev, cugs_densify_workspace_bytes(n), 3);
    int64_t counts[4];
    check(cugs_densify_plan(n, flags.data_ptr<uint8_t>(), ws.data_ptr(), ws.numel(), counts, st), "cugs_densify_plan");
    const int64_t n_out = counts[3];
    if (n_out == n) return 0;
    std::vector<torch::Tensor> srcs, dsts;
    std::vector<cugs_densify_array> desc;
    auto add = [&](const torch::Tensor& src, int mode) {
        auto s = src.contiguous();
        auto sizes = s.sizes().vec();
        sizes[0] = n_out;
        auto d = torch::empty(sizes, fopt(model.positions));
        srcs.push_back(s); dsts.push_back(d);
        desc.push_back(cugs_densify_array{s.data_ptr<float>(), d.data_ptr<float>(), static_cast<int32_t>(s.numel() / n), mode});
        return d;
    };
    auto new_pos = add(model.positions, CUGS_DENSIFY_COPY), new_sh = add(model.sh_coeffs, CUGS_DENSIFY_COPY);
    auto new_opa = add(model.opacities, CUGS_DENSIFY_COPY), new_rot = add(model.rotations, CUGS_DENSIFY_COPY);
    auto new_scl = add(model.scales, CUGS_DENSIFY_COPY);
    std::array<torch::Tensor, 5> nm, nv;
    if (optimizer) for (int i = 0; i < 5; ++i) { nm[i] = add(optimizer->m_[i], CUGS_DENSIFY_STATE); nv[i] = add(optimizer->v_[i], CUGS_DENSIFY_STATE); }
    if (n_out > 0)
        check(cugs_densify_apply(n, n_out, ws.data_ptr(), ws.numel(), nullptr, nullptr, desc.data(),
                                 static_cast<int>(desc.size()), st), "cugs_densify_apply");
    model.positions = new_pos; model.sh_coeffs = new_sh; model.opacities = new_opa; model.rotations = new_rot; model.scales = new_scl;
    if (optimizer) {
        optimizer->params_ = {model.positions, model.sh_coeffs, model.opacities, model.scales, model.rotations};
        optimizer->m_ = nm; optimizer->v_ = nv;
        optimizer->zero_grad();
    }
    return n - n_out;
}

int64_t prune_by_scores(ModelTensors& model, const ContributionScores& scores, float min_max_weight, float keep_fraction,
                        FusedAdam* optimizer) {
    const int64_t n = model.positions.size(0);
    TORCH_CHECK(scores.n() == n, "prune_by_scores: the table holds ", scores.n(), " Gaussians, the model ", n);
    TORCH_CHECK(min_max_weight >= 0.0f || keep_fraction >= 0.0f, "prune_by_scores: give min_max_weight, keep_fraction or both");
    if (n == 0) return 0;
    TORCH_CHECK(scores.table.device() == model.positions.device(), "prune_by_scores: the score table is on another device");
    const auto wmax = scores.weight_max();
    auto mask = wmax.eq(0.0f);
    if (min_max_weight >= 0.0f) mask = mask.logical_or(wmax.lt(min_max_weight));
    if (keep_fraction >= 0.0f) {
        TORCH_CHECK(keep_fraction <= 1.0f, "prune_by_scores: keep_fraction must lie in [0, 1]");
        const int64_t keep = std::llround(static_cast<double>(keep_fraction) * static_cast<double>(n));
        auto drop = torch::ones({n}, torch::TensorOptions().dtype(torch::kBool).device(mask.device()));
        if (keep > 0) drop.index_fill_(0, std::get<1>(scores.weight_sum().topk(keep)), false);
        mask = mask.logical_or(drop);
    }
    return prune_gaussians(model, mask, optimizer);
}

// ---- pixel maps lifted onto Gaussians ----
LiftedMaps::LiftedMaps(int64_t n, const torch::Device& device, int channels_)
    : table(torch::zeros({n, 4}, torch::TensorOptions().dtype(torch::kFloat32).device(device))), channels(channels_) {
    TORCH_CHECK(channels >= 1 && channels <= 4, "LiftedMaps: channels must be 1..4");
}
torch::Tensor LiftedMaps::sums() const { return table.narrow(1, 0, channels); }
void LiftedMaps::reset() { table.zero_(); num_views = 0; }

namespace {
// the validated, contiguous map of one launch: exactly one of the two comes back defined
std::pair<torch::Tensor, torch::Tensor> lift_map_args(const LiftedMaps& lifted, int width, int height,
                                                      const torch::Tensor& maps, const torch::Tensor& labels,
                                                      const char* what) {
    TORCH_CHECK(maps.defined() != labels.defined(), what, ": give exactly one of maps and labels");
    if (maps.defined()) {
        TORCH_CHECK(maps.device() == lifted.table.device() && maps.scalar_type() == torch::kFloat32, what,
                    ": maps must be a float32 tensor on the table's device");
        const bool ok = (maps.dim() == 3 && maps.size(0) == height && maps.size(1) == width && maps.size(2) == lifted.channels) ||
                        (lifted.channels == 1 && maps.dim() == 2 && maps.size(0) == height && maps.size(1) == width);
        TORCH_CHECK(ok, what, ": maps must be [", height, ", ", width, ", ", lifted.channels, "]");
        return {maps.contiguous(), torch::Tensor()};
    }
    TORCH_CHECK(labels.device() == lifted.table.device() && labels.scalar_type() == torch::kInt32, what,
                ": labels must be an int32 tensor on the table's device");
    TORCH_CHECK(labels.dim() == 2 && labels.size(0) == height && labels.size(1) == width, what, ": labels must be [",
                height, ", ", width, "]");
    return {torch::Tensor(), labels.contiguous()};
}

void launch_lift(LiftedMaps& lifted, int width, int height, const torch::Tensor& tile_ranges,
                 const torch::Tensor& gaussian_indices, const torch::Tensor& means_2d, const torch::Tensor& cov_2d_inv,
                 const torch::Tensor& opacities_act, const torch::Tensor& packed, const torch::Tensor& tile_order,
                 const torch::Tensor& maps, const torch::Tensor& labels, int label_base) {
    auto tr = tile_ranges.contiguous(), gi = gaussian_indices.contiguous();
    auto m = means_2d.contiguous(), c = cov_2d_inv.contiguous(), op = opacities_act.contiguous();
    auto pk = packed.defined() ? packed.contiguous() : packed;
    if (tile_order.defined())
        TORCH_CHECK(tile_order.is_contiguous() && tile_order.scalar_type() == torch::kInt32 &&
                    tile_order.numel() == 4 * tr.size(0), "tile_order must be a contiguous [tiles, 4] int32 tensor");
    check(cugs_blend_lift(width, height, ptr<int32_t>(tr), ptr<int32_t>(gi), ptr<float>(m), ptr<float>(c), ptr<float>(op),
                          ptr<float>(pk), order_ptr(tile_order), static_cast<int>(lifted.n()), ptr<float>(maps),
                          ptr<int32_t>(labels), lifted.channels, label_base,
                          lifted.n() > 0 ? lifted.table.data_ptr() : nullptr, stream_of(lifted.table)),
          "cugs_blend_lift");
    ++lifted.num_views;
}

// projection at SH degree 0 (the colour is not used), the plain sort (one host sync) and the lift launch
struct SortedView { ProjectionOutput proj; SortingOutput srt; };
SortedView sorted_view(const ModelTensors& model, const cugs_camera& cam, const RenderSettings& settings) {
    auto proj = project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam,
                                  0, settings.scale_modifier);
    auto srt = sort_gaussians(proj.means_2d, proj.depths, proj.radii, proj.tiles_touched, cam.width, cam.height);
    return {proj, srt};
}
void launch_lift_sorted(LiftedMaps& lifted, const cugs_camera& cam, const SortedView& v, const torch::Tensor& maps,
                        const torch::Tensor& labels, int label_base) {
    launch_lift(lifted, cam.width, cam.height, v.srt.tile_ranges, v.srt.gaussian_values_sorted, v.proj.means_2d,
                v.proj.cov_2d_inv, v.proj.opacities_act, v.proj.packed, {}, maps, labels, label_base);
}
}  // namespace

void lift_pixel_maps(LiftedMaps& lifted, const RenderOutput& out, const cugs_camera& camera, const torch::Tensor& maps,
                     const torch::Tensor& labels, int label_base) {
    const int64_t n = out.means_2d.size(0);
    TORCH_CHECK(n == lifted.n(), "lift_pixel_maps: the table holds ", lifted.n(), " Gaussians, the render ", n);
    auto args = lift_map_args(lifted, camera.width, camera.height, maps, labels, "lift_pixel_maps");
    if (n == 0) { ++lifted.num_views; return; }
    TORCH_CHECK(out.means_2d.device() == lifted.table.device(), "lift_pixel_maps: the table is on another device");
    launch_lift(lifted, camera.width, camera.height, out.tile_ranges, out.gaussian_indices, out.means_2d, out.cov_2d_inv,
                out.opacities_act, out.packed, out.tile_order, args.first, args.second, label_base);
}

LiftedMaps lift_maps(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                     const std::vector<torch::Tensor>& maps_per_view, const RenderSettings& settings, int channels) {
    TORCH_CHECK(model.positions.is_cuda(), "GaussianModel must be on CUDA device");
    TORCH_CHECK(maps_per_view.size() == cameras.size(), "lift_maps: one map per camera");
    if (channels <= 0)
        channels = (maps_per_view.empty() || maps_per_view[0].dim() == 2) ? 1 : static_cast<int>(maps_per_view[0].size(2));
    const int64_t n = model.positions.size(0);
    LiftedMaps lifted(n, model.positions.device(), channels);
    for (size_t i = 0; i < cameras.size(); ++i) {
        const auto& cam = cameras[i];
        auto args = lift_map_args(lifted, cam.width, cam.height, maps_per_view[i], {}, "lift_maps");
        if (n == 0) { ++lifted.num_views; continue; }
        launch_lift_sorted(lifted, cam, sorted_view(model, cam, settings), args.first, {}, 0);
    }
    return lifted;
}

std::pair<torch::Tensor, torch::Tensor> vote_labels(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                                                    const std::vector<torch::Tensor>& label_maps, int num_labels,
                                                    const RenderSettings& settings) {
    TORCH_CHECK(model.positions.is_cuda(), "GaussianModel must be on CUDA device");
    TORCH_CHECK(label_maps.size() == cameras.size(), "vote_labels: one map per camera");
    TORCH_CHECK(num_labels >= 1, "vote_labels: num_labels must be positive");
    const int64_t n = model.positions.size(0);
    std::vector<LiftedMaps> windows;
    for (int base = 0; base < num_labels; base += 4)
        windows.emplace_back(n, model.positions.device(), std::min(4, num_labels - base));
    for (size_t i = 0; i < cameras.size(); ++i) {
        const auto& cam = cameras[i];
        auto args = lift_map_args(windows[0], cam.width, cam.height, {}, label_maps[i], "vote_labels");
        if (n == 0) continue;
        const auto view = sorted_view(model, cam, settings);
        for (size_t k = 0; k < windows.size(); ++k)
            launch_lift_sorted(windows[k], cam, view, {}, args.second, static_cast<int>(4 * k));
    }
    std::vector<torch::Tensor> parts;
    for (const auto& win : windows) parts.push_back(win.sums());
    auto votes = torch::cat(parts, 1);
    auto labels = votes.argmax(1);
    auto top = votes.gather(1, labels.unsqueeze(1)).squeeze(1);
    labels = torch::where(top.gt(0.0f), labels, torch::full_like(labels, -1));
    return {labels, votes};
}

torch::Tensor error_scores(const ModelTensors& model, const std::vector<cugs_camera>& cameras,
                           const std::vector<torch::Tensor>& error_maps, const RenderSettings& settings,
                           bool max_over_views) {
    TORCH_CHECK(model.positions.is_cuda(), "GaussianModel must be on CUDA device");
    TORCH_CHECK(error_maps.size() == cameras.size(), "error_scores: one map per camera");
    const int64_t n = model.positions.size(0);
    LiftedMaps scratch(n, model.positions.device(), 1);
    auto out = torch::zeros({n}, fopt(model.positions));
    for (size_t i = 0; i < cameras.size(); ++i) {
        const auto& cam = cameras[i];
        auto args = lift_map_args(scratch, cam.width, cam.height, error_maps[i], {}, "error_scores");
        if (n == 0) continue;
        if (max_over_views) scratch.reset();
        launch_lift_sorted(scratch, cam, sorted_view(model, cam, settings), args.first, {}, 0);
        if (max_over_views) out = torch::maximum(out, scratch.sums().select(1, 0));
    }
    if (!max_over_views) out.copy_(scratch.sums().select(1, 0));
    return out;
}

int64_t select_gaussians(ModelTensors& model, const torch::Tensor& keep_mask, FusedAdam* optimizer) {
    TORCH_CHECK(keep_mask.defined() && keep_mask.scalar_type() == torch::kBool, "select_gaussians: keep_mask must be a bool tensor");
    prune_gaussians(model, keep_mask.logical_not(), optimizer);
    return model.positions.size(0);
}

// ---- a model moved by a similarity ----
Similarity Similarity::inverse() const {
    Similarity o;
    o.scale = 1.0 / scale;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o.rotation[3 * i + j] = rotation[3 * j + i];
    for (int i = 0; i < 3; ++i) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc += o.rotation[3 * i + j] * translation[j];
        o.translation[i] = -acc / scale;
    }
    return o;
}

Similarity Similarity::compose(const Similarity& other) const {
    Similarity o;
    o.scale = scale * other.scale;
    for (int i = 0; i < 3; ++i) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) {
            double r = 0.0;
            for (int k = 0; k < 3; ++k) r += rotation[3 * i + k] * other.rotation[3 * k + j];
            o.rotation[3 * i + j] = r;
            acc += rotation[3 * i + j] * other.translation[j];
        }
        o.translation[i] = scale * acc + translation[i];
    }
    return o;
}

std::array<double, 16> Similarity::matrix() const {
    std::array<double, 16> m{};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m[4 * i + j] = scale * rotation[3 * i + j];
        m[4 * i + 3] = translation[i];
    }
    m[15] = 1.0;
    return m;
}

bool Similarity::is_pure_translation() const {
    for (int i = 0; i < 9; ++i)
        if (rotation[i] != ((i % 4 == 0) ? 1.0 : 0.0)) return false;
    return scale == 1.0;
}

CugsSimilarity Similarity::to_abi() const {
    CugsSimilarity xf;
    TORCH_CHECK(cugs_similarity_init(&xf, rotation.data(), translation.data(), scale) == 0,
                "Similarity: the rotation must be a proper rotation (within 1e-4 of orthogonal, det > 0), the scale "
                "positive and every value finite");
    return xf;
}

void transform_gaussians(ModelTensors& model, const Similarity& sim, const torch::Tensor& mask, FusedAdam* optimizer) {
    const int64_t n = model.positions.size(0);
    TORCH_CHECK(model.positions.is_cuda(), "transform_gaussians: model must be on CUDA");
    const int64_t coeffs = model.sh_coeffs.size(2);
    TORCH_CHECK(coeffs == 1 || coeffs == 4 || coeffs == 9 || coeffs == 16, "transform_gaussians: sh_coeffs has ", coeffs,
                " coefficients, not 1, 4, 9 or 16");
    for (const torch::Tensor* t : {&model.positions, &model.rotations, &model.scales, &model.sh_coeffs})
        TORCH_CHECK(t->scalar_type() == torch::kFloat32 && t->is_contiguous() && t->size(0) == n,
                    "transform_gaussians: the model's tensors must be contiguous float32 [N, ...] (the update is in place)");
    torch::Tensor bytes;
    if (mask.defined()) {
        TORCH_CHECK(mask.scalar_type() == torch::kBool && mask.dim() == 1 && mask.size(0) == n,
                    "transform_gaussians: mask must be a bool tensor of shape [", n, "]");
        TORCH_CHECK(mask.device() == model.positions.device(), "transform_gaussians: mask must be on the model's device");
        bytes = mask.contiguous().view(torch::kUInt8);
    }
    const CugsSimilarity xf = sim.to_abi();
    std::vector<float*> zero;
    std::vector<int> floats;
    if (optimizer && !sim.is_pure_translation() && n > 0)
        for (int g : {0, 1, 4})                                      // positions, SH, rotations
            for (const torch::Tensor* t : {&optimizer->m_[g], &optimizer->v_[g]}) {
                TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->is_contiguous() && t->size(0) == n,
                            "transform_gaussians: the optimizer's moments must be contiguous float32 [N, ...]");
                zero.push_back(t->data_ptr<float>());
                floats.push_back(static_cast<int>(t->numel() / n));
            }
    if (n == 0) return;
    check(cugs_transform_gaussians(n, static_cast<int>(coeffs), ptr<float>(model.positions), ptr<float>(model.rotations),
                                   ptr<float>(model.scales), ptr<float>(model.sh_coeffs), ptr<uint8_t>(bytes), zero.data(),
                                   floats.data(), static_cast<int>(zero.size()), &xf, stream_of(model.positions)),
          "cugs_transform_gaussians");
}

cugs_camera transform_camera(const cugs_camera& camera, const Similarity& sim) {
    cugs_camera out = camera;
    double Rn[9], tn[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) acc += static_cast<double>(camera.view[4 * i + k]) * sim.rotation[3 * j + k];
            Rn[3 * i + j] = acc;                                     // Rc R^T
        }
    for (int i = 0; i < 3; ++i) {
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc += Rn[3 * i + j] * sim.translation[j];
        tn[i] = sim.scale * static_cast<double>(camera.view[4 * i + 3]) - acc;
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out.view[4 * i + j] = static_cast<float>(Rn[3 * i + j]);
        out.view[4 * i + 3] = static_cast<float>(tn[i]);
    }
    for (int i = 0; i < 3; ++i) {                                    // C = -R^T t of the stored float values
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) acc += static_cast<double>(out.view[4 * j + i]) * static_cast<double>(out.view[4 * j + 3]);
        out.cam_center[i] = static_cast<float>(-acc);
    }
    return out;
}

int64_t merge_gaussians(ModelTensors& model, const ModelTensors& other, FusedAdam* optimizer) {
    torch::NoGradGuard no_grad;
    TORCH_CHECK(other.positions.device() == model.positions.device(), "merge_gaussians: the models are on different devices");
    const int64_t coeffs = std::max(model.sh_coeffs.size(2), other.sh_coeffs.size(2));
    const int64_t n_new = other.positions.size(0);
    auto pad = [&](const torch::Tensor& t) {
        if (t.size(2) == coeffs) return t;
        auto out = torch::zeros({t.size(0), 3, coeffs}, t.options());
        out.slice(2, 0, t.size(2)).copy_(t);
        return out;
    };
    auto join = [](const torch::Tensor& a, const torch::Tensor& b) { return torch::cat({a, b.to(a.scalar_type())}, 0).contiguous(); };
    model.positions = join(model.positions, other.positions);
    model.sh_coeffs = join(pad(model.sh_coeffs), pad(other.sh_coeffs));
    model.opacities = join(model.opacities, other.opacities);
    model.rotations = join(model.rotations, other.rotations);
    model.scales = join(model.scales, other.scales);
    if (optimizer) {
        optimizer->params_ = {model.positions, model.sh_coeffs, model.opacities, model.scales, model.rotations};
        for (int g = 0; g < 5; ++g)
            for (auto* moments : {&optimizer->m_, &optimizer->v_}) {
                auto old = g == 1 ? pad((*moments)[g]) : (*moments)[g];
                auto sizes = old.sizes().vec();
                sizes[0] = n_new;
                (*moments)[g] = torch::cat({old, torch::zeros(sizes, old.options())}, 0).contiguous();
            }
        optimizer->zero_grad();
    }
    return model.positions.size(0);
}

}  // namespace cugs_hip
