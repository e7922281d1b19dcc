// project_backward_pose_reduce.h — what follows a POSE instantiation of k_project_backward, shared by
// project_backward_pose.hip and project_backward_sparse.hip: the pose block's checks and the two reduction launches.
//
// Reduction: the projection backward leaves one fp32 partial of the twelve camera terms per workgroup
// (pose_block_partial); k_pose_slices sums at most POSE_SLICES contiguous ranges of them in fp64, k_pose_finish sums the
// slices in fp64 in slice order and rounds once to fp32.  Three launches in stream order: no float atomics, no
// cross-workgroup hand-off inside a launch, and every sum has a fixed order - the same bits from run to run.
#pragma once
#include "project_backward_kernels.h"

namespace {

constexpr int POSE_SLICES = 256;                            // workgroups of the first fp64 pass, at most
constexpr int POSE_GROUPS = CUGS_BLOCK / POSE_TERMS;        // 21 threads per term in a summing workgroup

inline int64_t pose_parts(int64_t n) { return (n + CUGS_BLOCK - 1) / CUGS_BLOCK; }
inline size_t pose_slice_offset(int64_t n) {
    return ((size_t)pose_parts(n) * POSE_TERMS * sizeof(float) + 255u) & ~(size_t)255u;
}
inline size_t pose_workspace_bytes(int64_t n) {
    if (n < 0) n = 0;
    return pose_slice_offset(n) + (size_t)POSE_SLICES * POSE_TERMS * sizeof(double);
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

// the pose block's checks (before anything is queued); CUGS_E* or 0
inline int check_pose(int64_t n, const cugs_pose_grad* pose) {
    if (!pose || !pose->dL_dview) return CUGS_EINVAL;
    if (n <= 0) return 0;                                       // nothing but the 16 zeros is written
    if (!pose->workspace) return CUGS_EINVAL;
    if (pose->workspace_bytes < pose_workspace_bytes(n)) return CUGS_EWORKSPACE;
    if (!cugs_aligned16(pose->workspace)) return CUGS_EALIGN;
    return 0;
}

// the two launches behind a POSE launch over n Gaussians: partials -> slices -> pose->dL_dview
inline int pose_reduce(int64_t n, const cugs_pose_grad* pose, hipStream_t st) {
    char* ws = static_cast<char*>(pose->workspace);
    const int64_t nparts = pose_parts(n);
    const int64_t per = (nparts + POSE_SLICES - 1) / POSE_SLICES;
    const int nslices = (int)((nparts + per - 1) / per);
    double* slices = reinterpret_cast<double*>(ws + pose_slice_offset(n));
    hipLaunchKernelGGL(k_pose_slices, dim3(nslices), dim3(CUGS_BLOCK), 0, st, reinterpret_cast<const float*>(ws), nparts, per,
                       slices);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pose_finish, dim3(1), dim3(CUGS_BLOCK), 0, st, slices, nslices, pose->dL_dview);
    CUGS_LAUNCH_CHECK();
    return 0;
}

inline int pose_zeros(const cugs_pose_grad* pose, hipStream_t st) {
    CUGS_RETURN_IF_HIP(hipMemsetAsync(pose->dL_dview, 0, 16 * sizeof(float), st));
    return 0;
}

}  // namespace
