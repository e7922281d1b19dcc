// project_backward_mcmc.hip — cugs_project_backward_adam_mcmc (N5): the MCMC instantiations of k_project_backward,
// in a translation unit of their own (see project_backward_kernels.h).
#include "project_backward_kernels.h"

namespace {

template <int C>
int launch_pb_mcmc(int64_t n, int degree, const CamArgs& cam, const PBPtrs& p, bool aligned, hipStream_t st,
                   const AdamFusedArgs* adam, const McmcFusedArgs* mc) {
    if constexpr (C == 16) {
        if (aligned && p.colour_gate) {
            hipLaunchKernelGGL((k_project_backward<C, true, true, true, true>), dim3(grid_for(n)), dim3(CUGS_BLOCK), 0, st, n, degree, cam, p, *adam, *mc, PoseArgs{});
            CUGS_LAUNCH_CHECK();
            return 0;
        }
    }
    if (aligned)
        hipLaunchKernelGGL((k_project_backward<C, true, true, false, true>), dim3(grid_for(n)), dim3(CUGS_BLOCK), 0, st, n, degree, cam, p, *adam, *mc, PoseArgs{});
    else
        hipLaunchKernelGGL((k_project_backward<C, false, true, false, true>), dim3(grid_for(n)), dim3(CUGS_BLOCK), 0, st, n, degree, cam, p, *adam, *mc, PoseArgs{});
    CUGS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int cugs_project_backward_adam_mcmc(int64_t n, int num_coeffs, int active_degree, float* positions,
                                               float* rotations, float* scales, float* opacities, float* sh_coeffs,
                                               const int32_t* radii, const uint8_t* colour_gate,
                                               const cugs_camera* camera_host, float scale_modifier,
                                               const float* grad_accum, const cugs_adam_fused* adam_host,
                                               const cugs_mcmc_fused* mcmc_host, float* dL_dmeans_2d_out,
                                               void* stream) {
    if (!mcmc_host) return CUGS_EINVAL;
    CamArgs cam;
    PBPtrs p;
    AdamFusedArgs a;
    bool aligned;
    const int r = prepare_adam(n, num_coeffs, active_degree, positions, rotations, scales, opacities, sh_coeffs, radii,
                               colour_gate, camera_host, scale_modifier, grad_accum, adam_host, dL_dmeans_2d_out, cam, p,
                               a, aligned);
    if (r != 0) return r == 1 ? 0 : r;
    McmcFusedArgs mc;
    const int rm = prepare_mcmc(n, mcmc_host, mc);
    if (rm != 0) return rm;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (num_coeffs) {
        case 1: return launch_pb_mcmc<1>(n, active_degree, cam, p, aligned, st, &a, &mc);
        case 4: return launch_pb_mcmc<4>(n, active_degree, cam, p, aligned, st, &a, &mc);
        case 9: return launch_pb_mcmc<9>(n, active_degree, cam, p, aligned, st, &a, &mc);
        default: return launch_pb_mcmc<16>(n, active_degree, cam, p, aligned, st, &a, &mc);
    }
}
