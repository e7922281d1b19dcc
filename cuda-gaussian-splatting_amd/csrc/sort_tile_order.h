// sort_tile_order.h — the tiles ordered by the length of their lists, for the blend kernels.
#pragma once

#include "sort_radix.h"

namespace {

// ------------------------------------------------------------------------------------
// Tile order for the blend kernels (round 3): the tiles sorted by the length of their lists, longest first - the order
// in which the blend kernels' workgroups should be handed out (they take tile_order[blockIdx.x]): a view whose splats
// cluster (every real capture) has a few hundred tiles with lists many times the mean, and in the spatial order those
// workgroups start whenever their position comes up, the last of them long after the rest of the chip has drained.
// Heaviest first, same kernels (tools/lpt_order.py, same box): 80 % of the splats on 10 % of the screen - forward blend
// 176 -> 133 us, backward 409 -> 306; 50 % on 2 % - 182 -> 150, 543 -> 400; the uniform scene unchanged (134 / 432).
// A counting sort over 513 buckets (lengths with 4 bits below the leading one, i.e. to 6 %; empty tiles last) by ONE
// workgroup; the order inside a bucket is whatever the LDS atomics make it - any permutation is a correct order.
// ------------------------------------------------------------------------------------
constexpr uint32_t ORDER_BUCKETS = 513u;          // 32 x 16 length classes + the empty tiles
constexpr uint32_t ORDER_LDS = 576u;              // dwords of LDS the procedure needs (9 buckets per lane of one wave)
__device__ __forceinline__ uint32_t order_bucket(uint32_t len) {
    if (len == 0u) return ORDER_BUCKETS - 1u;
    const uint32_t e = 31u - (uint32_t)__clz((int)len);
    const uint32_t m = e >= 4u ? (len >> (e - 4u)) & 15u : (len << (4u - e)) & 15u;
    return 511u - (e * 16u + m);
}
// By every thread of ONE workgroup (any size that is a multiple of 64).  s_hist: ORDER_LDS dwords of LDS.
// A record of the order is {tile, first pair, one past the last pair, 0}: the blend workgroup that takes it has its tile
// and its range in one 16-byte load (a bare tile id puts a second, dependent memory round trip in front of every
// workgroup: +6 % on the 100 k-Gaussian forward-only frame, whose workgroups are a few microseconds long).
template <typename LenFn, typename StartFn>
__device__ __forceinline__ void write_tile_order(uint32_t tiles, LenFn len_of, StartFn start_of, uint4* __restrict__ order,
                                                 uint32_t* s_hist) {
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    for (uint32_t b = tid; b < ORDER_LDS; b += nt) s_hist[b] = 0u;
    __syncthreads();
    for (uint32_t t = tid; t < tiles; t += nt) atomicAdd(&s_hist[order_bucket(len_of(t))], 1u);
    __syncthreads();
    if (tid < (uint32_t)CUGS_WAVE) {                                  // exclusive scan of the bucket counts by one wave
        uint32_t v[9], sum = 0u;
#pragma unroll
        for (int k = 0; k < 9; ++k) { v[k] = s_hist[tid * 9u + k]; sum += v[k]; }
        uint32_t run = wave_inclusive_scan(sum) - sum;
#pragma unroll
        for (int k = 0; k < 9; ++k) { s_hist[tid * 9u + k] = run; run += v[k]; }
    }
    __syncthreads();
    for (uint32_t t = tid; t < tiles; t += nt) {
        const uint32_t len = len_of(t), first = len ? start_of(t) : 0u;
        order[atomicAdd(&s_hist[order_bucket(len)], 1u)] = make_uint4(t, first, first + len, 0u);
    }
    __syncthreads();
}
__global__ __launch_bounds__(1024) void k_tile_order(uint32_t tiles, const int32_t* __restrict__ tile_ranges,
                                                      uint4* __restrict__ order) {
    __shared__ uint32_t s_hist[ORDER_LDS];
    write_tile_order(tiles, [&](uint32_t t) { return (uint32_t)(tile_ranges[2 * t + 1] - tile_ranges[2 * t]); },
                     [&](uint32_t t) { return (uint32_t)tile_ranges[2 * t]; }, order, s_hist);
}

}  // namespace
