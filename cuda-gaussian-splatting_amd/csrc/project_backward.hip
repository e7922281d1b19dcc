// project_backward.hip — per-Gaussian chain rule from 2-D gradients to (p, q, log s, logit o) fused
// with the SH colour backward (SURVEY §8 a8+a9).
//
// Replaces, in ONE launch: k_project_backward (rasterizer/projection_backward.cu:26-247), the
// recomputed view directions (projection_backward.cu:332-338), k_evaluate_sh_backward
// (core/sh_backward.cu:29-112) and five zero-fills (projection_backward.cu:275-278, sh_backward.cu:138).
// Also provides the standalone evaluate_sh_backward_cuda surface (sh_backward.cu:114-156).
//
// gfx950 mapping: one thread per Gaussian.  The [n,3,C] gradient rows (the largest write of the
// whole backward, 12C B/Gaussian) are assembled per thread in LDS (odd dword row stride) and
// leave the workgroup as contiguous 16-byte stores.  The ReLU gate (sh_backward.cu:92-100 recomputes the
// raw colour from the coefficients) comes as three bits per Gaussian from cugs_project_forward, which has the
// coefficients in LDS anyway and makes the backward's own test there (colour_gate): no re-read of the
// 12C B/Gaussian coefficients.  (The forward's clamped rgb is NOT a substitute: its rounding differs from the
// backward's recomputation, and within an ulp of zero the two disagree.)  Bound: HBM; algorithmic bytes 44+4+64(+1) read,
// 44+12C(+8) written per Gaussian.
#include "project_backward_kernels.h"

namespace {

template <int C>
int launch_shv(int64_t n, int degree, const float* pos, const float* gated, const ViewCenters& vc, float* out,
               bool aligned, hipStream_t st) {
    if (aligned)
        hipLaunchKernelGGL((k_sh_backward_views<C, true>), dim3(grid_for(n)), dim3(CUGS_BLOCK), 0, st, n, degree, pos, gated, vc, out);
    else
        hipLaunchKernelGGL((k_sh_backward_views<C, false>), dim3(grid_for(n)), dim3(CUGS_BLOCK), 0, st, n, degree, pos, gated, vc, out);
    CUGS_LAUNCH_CHECK();
    return 0;
}


template <int C>
int launch_shb(int64_t n, int degree, const float* sh, const float* dirs, const float* g, float* out,
               bool aligned, hipStream_t st) {
    if (aligned)
        hipLaunchKernelGGL((k_sh_backward<C, true>), dim3(grid_for(n)), dim3(CUGS_BLOCK), 0, st, n, degree, sh, dirs, g, out);
    else
        hipLaunchKernelGGL((k_sh_backward<C, false>), dim3(grid_for(n)), dim3(CUGS_BLOCK), 0, st, n, degree, sh, dirs, g, out);
    CUGS_LAUNCH_CHECK();
    return 0;
}

// Steps 3 to 7 of the sequence both entry points share (include/cugs_hip.h, cugs_projection_opts), behind the request's
// own check and prepare_plain / prepare_adam, whose result is `prepared`.
int finish_pb(int prepared, PBCall& c, const cugs_projection_opts& o) {
    if (prepared < 0) return prepared;
    if (o.pose) {
        const int rp = cugs_pb_check_pose(c.n, o.pose);
        if (rp != 0) return rp;
    }
    if (prepared == 1) return o.pose ? cugs_pb_pose_zeros(o.pose, c.st) : 0;
    if (o.mcmc) {
        const int rm = prepare_mcmc(c.n, o.mcmc, c.mc);
        if (rm != 0) return rm;
    }
    c.mcmc = o.mcmc != nullptr;
    c.pose_host = o.pose;
    if (o.pose) c.pose = pose_args(o.pose);
    if (o.sparse) return cugs_pb_launch_sparse(c);
    if (o.pose) return cugs_pb_launch_pose(c);
    if (o.mcmc) return cugs_pb_launch_mcmc(c);
    return c.adam ? launch_pb<true, false, false, false>(c) : launch_pb<false, false, false, false>(c);
}

}  // namespace

extern "C" int cugs_project_backward_opts(int64_t n, int num_coeffs, int active_degree, const float* positions,
                                          const float* rotations, const float* scales, const float* opacities,
                                          const float* sh_coeffs, const int32_t* radii, const uint8_t* colour_gate,
                                          const cugs_camera* camera_host, float scale_modifier,
                                          const float* grad_accum, const float* dL_dmeans_2d,
                                          const float* dL_dcov_2d_inv, const float* dL_drgb,
                                          const float* dL_dopacity_act, float* dL_dpositions, float* dL_drotations,
                                          float* dL_dscales, float* dL_dopacities, float* dL_dsh_coeffs,
                                          float* dL_dmeans_2d_out, float* dL_drgb_gated_out,
                                          const cugs_projection_opts* opts, void* stream) {
    const cugs_projection_opts o = opts ? *opts : cugs_projection_opts{};
    if (o.mcmc || o.sparse) return CUGS_EINVAL;                   // options of the fused step
    PBCall c{};
    c.n = n; c.num_coeffs = num_coeffs; c.degree = active_degree; c.st = static_cast<hipStream_t>(stream);
    const int r = prepare_plain(n, num_coeffs, active_degree, positions, rotations, scales, opacities, sh_coeffs, radii,
                                colour_gate, camera_host, scale_modifier, grad_accum, dL_dmeans_2d, dL_dcov_2d_inv, dL_drgb,
                                dL_dopacity_act, dL_dpositions, dL_drotations, dL_dscales, dL_dopacities, dL_dsh_coeffs,
                                dL_dmeans_2d_out, dL_drgb_gated_out, c.cam, c.p, c.aligned);
    return finish_pb(r, c, o);
}

extern "C" int cugs_project_backward_adam_opts(int64_t n, int num_coeffs, int active_degree, float* positions,
                                               float* rotations, float* scales, float* opacities, float* sh_coeffs,
                                               const int32_t* radii, const uint8_t* colour_gate,
                                               const cugs_camera* camera_host, float scale_modifier,
                                               const float* grad_accum, const cugs_adam_fused* adam_host,
                                               float* dL_dmeans_2d_out, const cugs_projection_opts* opts,
                                               void* stream) {
    const cugs_projection_opts o = opts ? *opts : cugs_projection_opts{};
    if (o.mcmc && o.sparse) return CUGS_EINVAL;                   // the regulariser and the noise act on every Gaussian
    PBCall c{};
    c.n = n; c.num_coeffs = num_coeffs; c.degree = active_degree; c.st = static_cast<hipStream_t>(stream);
    c.adam = true;
    const int r = prepare_adam(n, num_coeffs, active_degree, positions, rotations, scales, opacities, sh_coeffs, radii,
                               colour_gate, camera_host, scale_modifier, grad_accum, adam_host, dL_dmeans_2d_out, c.cam, c.p,
                               c.adam_args, c.aligned);
    return finish_pb(r, c, o);
}

extern "C" int cugs_project_backward(int64_t n, int num_coeffs, int active_degree, const float* positions,
                                     const float* rotations, const float* scales, const float* opacities,
                                     const float* sh_coeffs, const int32_t* radii, const uint8_t* colour_gate,
                                     const cugs_camera* camera_host, float scale_modifier,
                                     const float* grad_accum, const float* dL_dmeans_2d,
                                     const float* dL_dcov_2d_inv, const float* dL_drgb,
                                     const float* dL_dopacity_act, float* dL_dpositions, float* dL_drotations,
                                     float* dL_dscales, float* dL_dopacities, float* dL_dsh_coeffs,
                                     float* dL_dmeans_2d_out, float* dL_drgb_gated_out, void* stream) {
    return cugs_project_backward_opts(n, num_coeffs, active_degree, positions, rotations, scales, opacities, sh_coeffs, radii,
                                      colour_gate, camera_host, scale_modifier, grad_accum, dL_dmeans_2d, dL_dcov_2d_inv,
                                      dL_drgb, dL_dopacity_act, dL_dpositions, dL_drotations, dL_dscales, dL_dopacities,
                                      dL_dsh_coeffs, dL_dmeans_2d_out, dL_drgb_gated_out, nullptr, stream);
}

extern "C" int cugs_project_backward_adam(int64_t n, int num_coeffs, int active_degree, float* positions,
                                          float* rotations, float* scales, float* opacities, float* sh_coeffs,
                                          const int32_t* radii, const uint8_t* colour_gate,
                                          const cugs_camera* camera_host, float scale_modifier,
                                          const float* grad_accum, const cugs_adam_fused* adam_host,
                                          float* dL_dmeans_2d_out, void* stream) {
    return cugs_project_backward_adam_opts(n, num_coeffs, active_degree, positions, rotations, scales, opacities, sh_coeffs,
                                           radii, colour_gate, camera_host, scale_modifier, grad_accum, adam_host,
                                           dL_dmeans_2d_out, nullptr, stream);
}

extern "C" int cugs_evaluate_sh_backward(int degree, int64_t n, int num_coeffs, const float* sh_coeffs,
                                         const float* directions, const float* dL_dcolor, float* dL_dsh,
                                         void* stream) {
    if (degree < 0 || degree > 3 || n < 0) return CUGS_EINVAL;           // sh_backward.cu:120
    if ((degree + 1) * (degree + 1) > num_coeffs) return CUGS_EINVAL;
    if (n == 0) return 0;
    if (!sh_coeffs || !directions || !dL_dcolor || !dL_dsh) return CUGS_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool aligned = cugs_aligned16(sh_coeffs) && cugs_aligned16(dL_dsh);
    switch (num_coeffs) {
        case 1: return launch_shb<1>(n, degree, sh_coeffs, directions, dL_dcolor, dL_dsh, aligned, st);
        case 4: return launch_shb<4>(n, degree, sh_coeffs, directions, dL_dcolor, dL_dsh, aligned, st);
        case 9: return launch_shb<9>(n, degree, sh_coeffs, directions, dL_dcolor, dL_dsh, aligned, st);
        case 16: return launch_shb<16>(n, degree, sh_coeffs, directions, dL_dcolor, dL_dsh, aligned, st);
        default:
            hipLaunchKernelGGL(k_sh_backward_generic, dim3(grid_for(n)), dim3(CUGS_BLOCK), 0, st, n, degree,
                               num_coeffs, sh_coeffs, directions, dL_dcolor, dL_dsh);
            CUGS_LAUNCH_CHECK();
            return 0;
    }
}

extern "C" int cugs_sh_backward_views(int degree, int64_t n, int num_coeffs, const float* positions,
                                      int num_views, const float* gated_rgb_views,
                                      const float* cam_centers_host, float* dL_dsh, void* stream) {
    if (degree < 0 || degree > 3 || n < 0 || num_views < 1 || num_views > MAX_VIEWS) return CUGS_EINVAL;
    if ((degree + 1) * (degree + 1) > num_coeffs) return CUGS_EINVAL;
    if (num_coeffs != 1 && num_coeffs != 4 && num_coeffs != 9 && num_coeffs != 16) return CUGS_EINVAL;
    if (n == 0) return 0;
    if (!positions || !gated_rgb_views || !cam_centers_host || !dL_dsh) return CUGS_EINVAL;
    ViewCenters vc;
    vc.count = num_views;
    for (int v = 0; v < MAX_VIEWS; ++v)
        for (int k = 0; k < 3; ++k) vc.c[v][k] = v < num_views ? cam_centers_host[v * 3 + k] : 0.0f;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool aligned = cugs_aligned16(dL_dsh);
    switch (num_coeffs) {
        case 1: return launch_shv<1>(n, degree, positions, gated_rgb_views, vc, dL_dsh, aligned, st);
        case 4: return launch_shv<4>(n, degree, positions, gated_rgb_views, vc, dL_dsh, aligned, st);
        case 9: return launch_shv<9>(n, degree, positions, gated_rgb_views, vc, dL_dsh, aligned, st);
        default: return launch_shv<16>(n, degree, positions, gated_rgb_views, vc, dL_dsh, aligned, st);
    }
}

extern "C" int cugs_gated_colour_grad(int64_t n, const float* grad_accum, const uint8_t* colour_gate,
                                      float* dL_drgb_gated_out, void* stream) {
    if (n < 0) return CUGS_EINVAL;
    if (n == 0) return 0;
    if (!grad_accum || !colour_gate || !dL_drgb_gated_out) return CUGS_EINVAL;
    if (!cugs_aligned16(grad_accum)) return CUGS_EALIGN;
    hipLaunchKernelGGL(k_gated_colour_grad, dim3(grid_for(n)), dim3(CUGS_BLOCK), 0, static_cast<hipStream_t>(stream), n,
                       grad_accum, colour_gate, dL_drgb_gated_out);
    CUGS_LAUNCH_CHECK();
    return 0;
}
