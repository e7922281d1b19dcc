// project_backward_pose.hip — the camera-pose gradient: cugs_project_backward_pose, _adam_pose and
// _adam_mcmc_pose.  The POSE instantiations of k_project_backward live here, in a translation unit of their own (as the
// MCMC ones do, project_backward_mcmc.hip), so that the existing instantiations keep their code.
//
// Reduction: the projection backward leaves one fp32 partial of the twelve camera terms per workgroup
// (pose_block_partial); k_pose_slices sums at most POSE_SLICES contiguous ranges of them in fp64, k_pose_finish sums the
// slices in fp64 in slice order and rounds once to fp32.  Three launches in stream order: no float atomics, no
// cross-workgroup hand-off inside a launch, and every sum has a fixed order - the same bits from run to run.
#include "project_backward_kernels.h"

namespace {

constexpr int POSE_SLICES = 256;                            // workgroups of the first fp64 pass, at most
constexpr int POSE_GROUPS = CUGS_BLOCK / POSE_TERMS;        // 21 threads per term in a summing workgroup

inline int64_t pose_parts(int64_t n) { return (n + CUGS_BLOCK - 1) / CUGS_BLOCK; }
inline size_t pose_slice_offset(int64_t n) {
    return ((size_t)pose_parts(n) * POSE_TERMS * sizeof(float) + 255u) & ~(size_t)255u;
}

// rows [lo, hi) of a [*, 12] table summed per column in fp64: thread t adds column t % 12 of rows lo + t / 12,
// lo + t / 12 + 21, ...; the 21 sums of a column are then added in order by thread < 12, which returns the total.
template <typename T>
__device__ __forceinline__ double sum_rows12(const T* __restrict__ rows, int64_t lo, int64_t hi, double* s_sum) {
    const int t = (int)threadIdx.x, c = t % POSE_TERMS, g = t / POSE_TERMS;
    if (g < POSE_GROUPS) {
        double acc = 0.0;
        for (int64_t j = lo + g; j < hi; j += POSE_GROUPS) acc += (double)rows[j * POSE_TERMS + c];
        s_sum[g * POSE_TERMS + c] = acc;
    }
    __syncthreads();
    double tot = 0.0;
    if (t < POSE_TERMS)
        for (int k = 0; k < POSE_GROUPS; ++k) tot += s_sum[k * POSE_TERMS + t];
    return tot;
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_pose_slices(const float* __restrict__ parts, int64_t nparts, int64_t per,
                                                            double* __restrict__ slices) {
    __shared__ double s_sum[POSE_GROUPS * POSE_TERMS];
    const int64_t lo = (int64_t)blockIdx.x * per, hi = min(lo + per, nparts);
    const double tot = sum_rows12(parts, lo, hi, s_sum);
    if (threadIdx.x < POSE_TERMS) slices[(int64_t)blockIdx.x * POSE_TERMS + threadIdx.x] = tot;
}

// one workgroup: the slices' total, rounded once, in the layout of cugs_camera.view (row 3 zero)
__global__ __launch_bounds__(CUGS_BLOCK) void k_pose_finish(const double* __restrict__ slices, int nslices,
                                                            float* __restrict__ dL_dview) {
    __shared__ double s_sum[POSE_GROUPS * POSE_TERMS];
    __shared__ float s_tot[POSE_TERMS];
    const double tot = sum_rows12(slices, 0, nslices, s_sum);
    if (threadIdx.x < POSE_TERMS) s_tot[threadIdx.x] = (float)tot;
    __syncthreads();
    if (threadIdx.x < 16) {
        const int r = (int)threadIdx.x >> 2, c = (int)threadIdx.x & 3;
        dL_dview[threadIdx.x] = r == 3 ? 0.0f : c < 3 ? s_tot[r * 3 + c] : s_tot[9 + r];
    }
}

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

// the pose block's checks (before anything is queued); CUGS_E* or 0
int check_pose(int64_t n, const cugs_pose_grad* pose) {
    if (!pose || !pose->dL_dview) return CUGS_EINVAL;
    if (n <= 0) return 0;                                       // nothing but the 16 zeros is written
    if (!pose->workspace) return CUGS_EINVAL;
    if (pose->workspace_bytes < cugs_pose_grad_workspace_bytes(n)) return CUGS_EWORKSPACE;
    if (!cugs_aligned16(pose->workspace)) return CUGS_EALIGN;
    return 0;
}

template <bool ADAM, bool MCMC>
int run_pose(int64_t n, int num_coeffs, int degree, const CamArgs& cam, const PBPtrs& p, bool aligned, hipStream_t st,
             const AdamFusedArgs& adam, const McmcFusedArgs& mc, const cugs_pose_grad* pose) {
    char* ws = static_cast<char*>(pose->workspace);
    const PoseArgs pa{reinterpret_cast<float*>(ws), pose->rows};
    int r;
    switch (num_coeffs) {
        case 1: r = launch_pb_pose<1, ADAM, MCMC>(n, degree, cam, p, aligned, st, adam, mc, pa); break;
        case 4: r = launch_pb_pose<4, ADAM, MCMC>(n, degree, cam, p, aligned, st, adam, mc, pa); break;
        case 9: r = launch_pb_pose<9, ADAM, MCMC>(n, degree, cam, p, aligned, st, adam, mc, pa); break;
        default: r = launch_pb_pose<16, ADAM, MCMC>(n, degree, cam, p, aligned, st, adam, mc, pa); break;
    }
    if (r != 0) return r;
    const int64_t nparts = pose_parts(n);
    const int64_t per = (nparts + POSE_SLICES - 1) / POSE_SLICES;
    const int nslices = (int)((nparts + per - 1) / per);
    double* slices = reinterpret_cast<double*>(ws + pose_slice_offset(n));
    hipLaunchKernelGGL(k_pose_slices, dim3(nslices), dim3(CUGS_BLOCK), 0, st, pa.partial, nparts, per, slices);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pose_finish, dim3(1), dim3(CUGS_BLOCK), 0, st, slices, nslices, pose->dL_dview);
    CUGS_LAUNCH_CHECK();
    return 0;
}

int pose_zeros(const cugs_pose_grad* pose, hipStream_t st) {
    CUGS_RETURN_IF_HIP(hipMemsetAsync(pose->dL_dview, 0, 16 * sizeof(float), st));
    return 0;
}

}  // namespace

extern "C" size_t cugs_pose_grad_workspace_bytes(int64_t n) {
    if (n < 0) n = 0;
    return pose_slice_offset(n) + (size_t)POSE_SLICES * POSE_TERMS * sizeof(double);
}

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
