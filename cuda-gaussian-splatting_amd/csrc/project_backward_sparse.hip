// project_backward_sparse.hip — the visibility-restricted fused optimizer step:
// cugs_project_backward_adam_sparse and cugs_project_backward_adam_sparse_pose.  The SPARSE instantiations of
// k_project_backward live here, in a translation unit of their own (as the MCMC and POSE ones do), so that the existing
// instantiations keep their code.  Same routes as the dense fused step: aligned or not, C = 1, 4, 9, 16, factor tile
// for aligned degree-3 storage.
#include "project_backward_pose_reduce.h"

namespace {

template <int C, bool POSE>
int launch_pb_sparse(int64_t n, int degree, const CamArgs& cam, const PBPtrs& p, bool aligned, hipStream_t st,
                     const AdamFusedArgs& adam, const PoseArgs& pa) {
    const dim3 grid(grid_for(n)), block(CUGS_BLOCK);
    if constexpr (C == 16) {
        if (aligned && p.colour_gate) {
            hipLaunchKernelGGL((k_project_backward<C, true, true, true, false, POSE, true>), grid, block, 0, st, n, degree, cam, p, adam, McmcFusedArgs{}, pa);
            CUGS_LAUNCH_CHECK();
            return 0;
        }
    }
    if (aligned)
        hipLaunchKernelGGL((k_project_backward<C, true, true, false, false, POSE, true>), grid, block, 0, st, n, degree, cam, p, adam, McmcFusedArgs{}, pa);
    else
        hipLaunchKernelGGL((k_project_backward<C, false, true, false, false, POSE, true>), grid, block, 0, st, n, degree, cam, p, adam, McmcFusedArgs{}, pa);
    CUGS_LAUNCH_CHECK();
    return 0;
}

template <bool POSE>
int run_sparse(int64_t n, int num_coeffs, int degree, const CamArgs& cam, const PBPtrs& p, bool aligned, hipStream_t st,
               const AdamFusedArgs& adam, const PoseArgs& pa) {
    switch (num_coeffs) {
        case 1: return launch_pb_sparse<1, POSE>(n, degree, cam, p, aligned, st, adam, pa);
        case 4: return launch_pb_sparse<4, POSE>(n, degree, cam, p, aligned, st, adam, pa);
        case 9: return launch_pb_sparse<9, POSE>(n, degree, cam, p, aligned, st, adam, pa);
        default: return launch_pb_sparse<16, POSE>(n, degree, cam, p, aligned, st, adam, pa);
    }
}

}  // namespace

extern "C" int cugs_project_backward_adam_sparse(int64_t n, int num_coeffs, int active_degree, float* positions,
                                                 float* rotations, float* scales, float* opacities, float* sh_coeffs,
                                                 const int32_t* radii, const uint8_t* colour_gate,
                                                 const cugs_camera* camera_host, float scale_modifier,
                                                 const float* grad_accum, const cugs_adam_fused* adam_host,
                                                 float* dL_dmeans_2d_out, void* stream) {
    CamArgs cam;
    PBPtrs p;
    AdamFusedArgs a;
    bool aligned;
    const int r = prepare_adam(n, num_coeffs, active_degree, positions, rotations, scales, opacities, sh_coeffs, radii,
                               colour_gate, camera_host, scale_modifier, grad_accum, adam_host, dL_dmeans_2d_out, cam, p,
                               a, aligned);
    if (r != 0) return r == 1 ? 0 : r;
    return run_sparse<false>(n, num_coeffs, active_degree, cam, p, aligned, static_cast<hipStream_t>(stream), a, PoseArgs{});
}

extern "C" int cugs_project_backward_adam_sparse_pose(int64_t n, int num_coeffs, int active_degree, float* positions,
                                                      float* rotations, float* scales, float* opacities,
                                                      float* sh_coeffs, const int32_t* radii, const uint8_t* colour_gate,
                                                      const cugs_camera* camera_host, float scale_modifier,
                                                      const float* grad_accum, const cugs_adam_fused* adam_host,
                                                      float* dL_dmeans_2d_out, const cugs_pose_grad* pose_host,
                                                      void* stream) {
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
    const int rl = run_sparse<true>(n, num_coeffs, active_degree, cam, p, aligned, st, a, pose_args(pose_host));
    if (rl != 0) return rl;
    return pose_reduce(n, pose_host, st);
}
