// cugs_row_sums.h — the fixed-order fp64 sums of the image-space losses (depth_loss.hip, normal_loss.hip): every
// workgroup writes one row of N partials, one workgroup adds the rows.  No atomics; the order depends on the launch
// shape alone, so the sums keep their bits from run to run.
#pragma once

#include "cugs_common.h"

namespace {

// N fp64 sums of the workgroup -> row[0..N): over the wave by shuffles, then the four waves in order.
template <int N>
__device__ __forceinline__ void block_sums(double (&acc)[N], double* __restrict__ row) {
    __shared__ double s_red[N][CUGS_BLOCK / CUGS_WAVE];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k)
        for (int d = CUGS_WAVE / 2; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d);
    if ((tid & (CUGS_WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s_red[k][tid / CUGS_WAVE] = acc[k];
    }
    __syncthreads();
    if (tid < N) {
        double a = s_red[tid][0];
        for (int v = 1; v < CUGS_BLOCK / CUGS_WAVE; ++v) a += s_red[tid][v];
        row[tid] = a;
    }
}

// Rows of N fp64 partials -> s_acc[k][0], the order of loss.hip's finalize_loss: thread t takes rows t, t + 256, ...;
// then a tree.  Call with the whole workgroup.
template <int N>
__device__ __forceinline__ void reduce_rows(const double* __restrict__ partials, int nblk, double (*s_acc)[CUGS_BLOCK]) {
    double a[N];
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = 0.0;
    for (int i = threadIdx.x; i < nblk; i += CUGS_BLOCK) {
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] += partials[(size_t)N * i + k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) s_acc[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int d = CUGS_BLOCK / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) {
#pragma unroll
            for (int k = 0; k < N; ++k) s_acc[k][threadIdx.x] += s_acc[k][threadIdx.x + d];
        }
        __syncthreads();
    }
}

}  // namespace
