// cugs_hip_torch.cpp — see cugs_hip_torch.hpp.  Each function: validate like the reference's
// launcher, allocate outputs with torch (the C ABI allocates nothing), pass raw pointers and
// torch's current HIP stream, turn a non-zero return into std::runtime_error.
#include "torch_glue.hpp"

namespace cugs_hip {

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

namespace {

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

}  // namespace cugs_hip
