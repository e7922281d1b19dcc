// cugs_score_walk.h — what the kernels that walk the forward blend's lists WITHOUT its colour share: the contribution
// scores (raster_score.hip) and the pixel-map lift (raster_lift.hip).  Both stage the
// geometry half of a record only and reduce a hit group's per-lane terms with permlane swaps.
#pragma once

#include "cugs_raster_common.h"

namespace {

// LDS record: the two geometry chunks {mx, my, a, b} {c, o, cull limit, g}.  The stride stays three float4s - an odd stride
// keeps the cull's one-record-per-lane 16-byte reads free of bank conflicts, as in the forward - the third is not used.
#define CUGS_SCORE_REC_F4 3

template <bool PACKED>
__device__ __forceinline__ void stage_geometry(const RasterSrc& s, int li, int end, float4* s_rec, float tile_cx,
                                               float tile_cy) {
    if (li >= end) return;
    const int g = s.gidx[li];
    float4 r0, r1;
    if (PACKED) {
        const float4* src = reinterpret_cast<const float4*>(s.packed + (int64_t)g * CUGS_PACKED_STRIDE);
        r0 = src[0]; r1 = src[1];
    } else {                                                       // as stage_record gathers them
        const float a = s.cov_2d_inv[g * 3 + 0], c = s.cov_2d_inv[g * 3 + 2], o = s.opa[g];
        r0 = make_float4(s.means_2d[g * 2 + 0], s.means_2d[g * 2 + 1], a, s.cov_2d_inv[g * 3 + 1]);
        r1 = make_float4(c, o, (o >= (1.0f / 255.0f)) ? logf(255.0f * o) : -1.0f, 0.0f);
    }
    r1.w = __int_as_float(g);
    cugs_stage_cull(r0, r1, tile_cx, tile_cy);                     // word 6: tau -> the cull's limit for this tile
    s_rec[threadIdx.x * CUGS_SCORE_REC_F4 + 0] = r0;
    s_rec[threadIdx.x * CUGS_SCORE_REC_F4 + 1] = r1;
}

template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }

__device__ __forceinline__ void swap_halves(float& a, float& b) {          // v_permlane32_swap: a = (a_lo, b_lo), b = (a_hi, b_hi)
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]); b = __uint_as_float(r[1]);
}
// v_permlane16_swap: odd rows of a <-> even rows of b.  Inline asm as in reduce9t: the builtin's second result comes out as
// a copy of the first with this compiler (the sum below became p + p).  The two wait states gfx950 needs between a VALU
// write and a permlane read of the same register are the s_nop in the string; the plain VALU that reads the results
// next needs none.
template <typename T>
__device__ __forceinline__ void swap_rows(T& a, T& b) {
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

}  // namespace
