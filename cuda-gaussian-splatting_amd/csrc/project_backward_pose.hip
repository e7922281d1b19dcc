// project_backward_pose.hip — the camera-pose gradient: cugs_project_backward_pose, _adam_pose and
// _adam_mcmc_pose.  The POSE instantiations of k_project_backward live here, in a translation unit of their own (as the
// MCMC ones do, project_backward_mcmc.hip), so that the existing instantiations keep their code.
//
// The reduction behind the launch, and the pose block's checks, are in project_backward_pose_reduce.h.
#include "project_backward_pose_reduce.h"

namespace {

template <int C, bool ADAM, bool MCMC>
int launch_pb_pose(int64_t n, int degree, const CamArgs& cam, const PBPtrs& p, bool aligned, hipStream_t st,
                   const AdamFusedArgs& adam, const McmcFusedArgs& mc, const PoseArgs& pa) {
    const dim3 grid(grid_for(n)), block(CUGS_BLOCK);
    if constexpr (C == 16) {
        if (aligned && p.colour_gate) {
            hipLaunchKernelGGL((k_project_backward<C, true, ADAM, true, MCMC, true>), grid, block, 0, st, n, degree, cam, p, adam, mc, pa);
            CUGS_LAUNCH_CHECK();
            return 0;
        }
    }
    if (aligned)
        hipLaunchKernelGGL((k_project_backward<C, true, ADAM, false, MCMC, true>), grid, block, 0, st, n, degree, cam, p, adam, mc, pa);
    else
        hipLaunchKernelGGL((k_project_backward<C, false, ADAM, false, MCMC, true>), grid, block, 0, st, n, degree, cam, p, adam, mc, pa);
    CUGS_LAUNCH_CHECK();
    return 0;
}

template <bool ADAM, bool MCMC>
int run_pose(int64_t n, int num_coeffs, int degree, const CamArgs& cam, const PBPtrs& p, bool aligned, hipStream_t st,
             const AdamFusedArgs& adam, const McmcFusedArgs& mc, const cugs_pose_grad* pose) {
    const PoseArgs pa = pose_args(pose);
    int r;
    switch (num_coeffs) {
        case 1: r = launch_pb_pose<1, ADAM, MCMC>(n, degree, cam, p, aligned, st, adam, mc, pa); break;
        case 4: r = launch_pb_pose<4, ADAM, MCMC>(n, degree, cam, p, aligned, st, adam, mc, pa); break;
        case 9: r = launch_pb_pose<9, ADAM, MCMC>(n, degree, cam, p, aligned, st, adam, mc, pa); break;
        default: r = launch_pb_pose<16, ADAM, MCMC>(n, degree, cam, p, aligned, st, adam, mc, pa); break;
    }
    if (r != 0) return r;
    return pose_reduce(n, pose, st);
}

}  // namespace

extern "C" size_t cugs_pose_grad_workspace_bytes(int64_t n) { return pose_workspace_bytes(n); }

extern "C" int cugs_project_backward_pose(int64_t n, int num_coeffs, int active_degree, const float* positions,
                                          const float* rotations, const float* scales, const float* opacities,
                                          const float* sh_coeffs, const int32_t* radii, const uint8_t* colour_gate,
                                          const cugs_camera* camera_host, float scale_modifier,
                                          const float* grad_accum, const float* dL_dmeans_2d,
                                          const float* dL_dcov_2d_inv, const float* dL_drgb,
                                          const float* dL_dopacity_act, float* dL_dpositions, float* dL_drotations,
                                          float* dL_dscales, float* dL_dopacities, float* dL_dsh_coeffs,
                                          float* dL_dmeans_2d_out, float* dL_drgb_gated_out,
                                          const cugs_pose_grad* pose_host, void* stream) {
    CamArgs cam;
    PBPtrs p;
    bool aligned;
    const int r = prepare_plain(n, num_coeffs, active_degree, positions, rotations, scales, opacities, sh_coeffs, radii,
                                colour_gate, camera_host, scale_modifier, grad_accum, dL_dmeans_2d, dL_dcov_2d_inv, dL_drgb,
                                dL_dopacity_act, dL_dpositions, dL_drotations, dL_dscales, dL_dopacities, dL_dsh_coeffs,
                                dL_dmeans_2d_out, dL_drgb_gated_out, cam, p, aligned);
    if (r < 0) return r;
    const int rp = check_pose(n, pose_host);
    if (rp != 0) return rp;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (r == 1) return pose_zeros(pose_host, st);
    return run_pose<false, false>(n, num_coeffs, active_degree, cam, p, aligned, st, AdamFusedArgs{}, McmcFusedArgs{},
                                  pose_host);
}

extern "C" int cugs_project_backward_adam_pose(int64_t n, int num_coeffs, int active_degree, float* positions,
                                               float* rotations, float* scales, float* opacities, float* sh_coeffs,
                                               const int32_t* radii, const uint8_t* colour_gate,
                                               const cugs_camera* camera_host, float scale_modifier,
                                               const float* grad_accum, const cugs_adam_fused* adam_host,
                                               float* dL_dmeans_2d_out, const cugs_pose_grad* pose_host, void* stream) {
    CamArgs cam;
    PBPtrs p;
    AdamFusedArgs a;
    bool aligned;
    const int r = prepare_adam(n, num_coeffs, active_degree, positions, rotations, scales, opacities, sh_coeffs, radii,
                               colour_gate, camera_host, scale_modifier, grad_accum, adam_host, dL_dmeans_2d_out, cam, p,
                               a, aligned);
    if (r < 0) return r;
    const int rp = check_pose(n, pose_host);
    if (rp != 0) return rp;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (r == 1) return pose_zeros(pose_host, st);
    return run_pose<true, false>(n, num_coeffs, active_degree, cam, p, aligned, st, a, McmcFusedArgs{}, pose_host);
}

extern "C" int cugs_project_backward_adam_mcmc_pose(int64_t n, int num_coeffs, int active_degree, float* positions,
                                                    float* rotations, float* scales, float* opacities,
                                                    float* sh_coeffs, const int32_t* radii, const uint8_t* colour_gate,
                                                    const cugs_camera* camera_host, float scale_modifier,
                                                    const float* grad_accum, const cugs_adam_fused* adam_host,
                                                    const cugs_mcmc_fused* mcmc_host, float* dL_dmeans_2d_out,
                                                    const cugs_pose_grad* pose_host, void* stream) {
    if (!mcmc_host) return CUGS_EINVAL;
    CamArgs cam;
    PBPtrs p;
    AdamFusedArgs a;
    bool aligned;
    const int r = prepare_adam(n, num_coeffs, active_degree, positions, rotations, scales, opacities, sh_coeffs, radii,
                               colour_gate, camera_host, scale_modifier, grad_accum, adam_host, dL_dmeans_2d_out, cam, p,
                               a, aligned);
    if (r < 0) return r;
    const int rp = check_pose(n, pose_host);
    if (rp != 0) return rp;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (r == 1) return pose_zeros(pose_host, st);
    McmcFusedArgs mc;
    const int rm = prepare_mcmc(n, mcmc_host, mc);
    if (rm != 0) return rm;
    return run_pose<true, true>(n, num_coeffs, active_degree, cam, p, aligned, st, a, mc, pose_host);
}
