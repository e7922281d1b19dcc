// cugs_raster_common.h — pieces shared by the forward and backward blend kernels.
//
// Work decomposition (gfx950): one 256-thread workgroup per 16x16 tile = 4 wave64s, each wave
// owning one 8x8 pixel QUAD of the tile (lane -> (lane&7, lane>>3)).  The tile's depth-sorted
// Gaussian list is consumed in batches of 256 records staged in LDS (one record per thread,
// three 16-byte gathers from the packed table).  Within a batch every wave first tests 64
// records at a time, one record per lane, against its own quad (`may_touch_quad`, below), turns
// the result into a 64-bit ballot mask, and then walks only the set bits: the per-pixel
// evaluation runs for the (wave, Gaussian) pairs that can matter instead of all P x 256.
//
// The cull is CONSERVATIVE and therefore invisible in the results: a record is dropped for a wave
// only when alpha < 1/255 is certain for all 64 pixel centres, with a margin that covers the
// fp32 rounding of the per-pixel power (see the derivation in cugs_blend_cull.h).  The per-pixel
// path itself (pixel_alpha) follows DESIGN.md's FMA placement contract and cugs_detmath.h, so
// every skip / clamp / termination decision equals the oracle's bit for bit.
#pragma once

#include "cugs_gaussian_math.h"
#include "cugs_blend_cull.h"      // after the HIP runtime's qualifiers are defined

#include <type_traits>

#define CUGS_REC_F4 3      // float4s per LDS record (CUGS_PACKED_STRIDE / 4)

struct RasterGeom {
    int width, height, ntx, ntiles;
    float bg0, bg1, bg2;
};

struct RasterSrc {
    const int32_t* tile_ranges;
    const int32_t* gidx;
    const float* packed;        // may be NULL -> gather from the four arrays below
    const float* means_2d;
    const float* cov_2d_inv;
    const float* rgb;
    const float* opa;
    const uint4* tile_order;    // may be NULL -> the spatial order of cugs_blend_tile; else workgroup b works on record b:
                                // {tile, first pair, one past the last pair, 0} - tile and range in ONE load (cugs_tile_order)
};

// Host side, kernel selection: f(std::true_type{}) or f(std::false_type{}) - a run-time flag becomes the template
// argument P() inside f.  Nest one call per flag.
template <typename F>
static inline void cugs_with_bool(bool flag, F&& f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

// The cull (cugs_blend_cull.h: derivation, slack, NaN behaviour) on the LDS record.  Its per-record half runs when the
// record is staged: cugs_stage_cull replaces word 6 of the geometry chunks (r0, r1) - tau = ln(255 o) in the packed
// record - by cugs_cull_limit for the tile centred at (tile_cx, tile_cy) = 16 * tile + 8; only may_touch_quad reads
// that word.  may_touch_quad, per (wave, record): can the Gaussian reach alpha >= 1/255 at ANY pixel centre of the
// rectangle of centres [qx0, qx0+wx] x [qy0, qy0+wy] (the wave's quad, or the bounding box of its pixels that are still
// active: ActiveRect below)?  `false` only when certainly not.
__device__ __forceinline__ void cugs_stage_cull(const float4& r0, float4& r1, float tile_cx, float tile_cy) {
    r1.z = cugs_cull_limit(r0.x, r0.y, r0.z, r0.w, r1.x, r1.z, tile_cx, tile_cy);
}
__device__ __forceinline__ bool may_touch_quad(float4 r0, float4 r1, float qx0, float qy0,
                                               float wx, float wy) {
    return cugs_cull_may_touch(r0.x, r0.y, r0.z, r0.w, r1.x, r1.z, qx0, qy0, wx, wy);
}

// Stage list entry `li` (if < end) into LDS slot threadIdx.x.  The LDS copy of the record carries the
// Gaussian index (as bits) in its spare word 7, so that the backward's scatter address comes
// with the same 16-byte read as the opacity.  Returns the Gaussian index (or -1).
// DEPTH (depth-map kernels): word 9 of the LDS copy - 0 in the colour chunk (r, 0, g, b) - takes
// depths[g], so that (r, z) is an aligned pair next to (g, b).  The packed HBM record is not changed.
// Word 6 of the LDS copy - tau in the packed record - takes the cull's limit for the tile centred at (tile_cx, tile_cy)
// (cugs_stage_cull): the per-record half of the cull, once per staged record instead of once per wave and test.
template <bool PACKED, bool DEPTH = false>
__device__ __forceinline__ int stage_record(const RasterSrc& s, int li, int end, float4* s_rec, float tile_cx,
                                            float tile_cy, const float* __restrict__ depths = nullptr) {
    if (li >= end) return -1;
    const int g = s.gidx[li];
    float4 r0, r1, r2;
    if (PACKED) {
        const float4* src = reinterpret_cast<const float4*>(s.packed + (int64_t)g * CUGS_PACKED_STRIDE);
        r0 = src[0]; r1 = src[1]; r2 = src[2];
    } else {
        const float a = s.cov_2d_inv[g * 3 + 0], c = s.cov_2d_inv[g * 3 + 2], o = s.opa[g];
        r0 = make_float4(s.means_2d[g * 2 + 0], s.means_2d[g * 2 + 1], a, s.cov_2d_inv[g * 3 + 1]);
        r1 = make_float4(c, o, (o >= (1.0f / 255.0f)) ? logf(255.0f * o) : -1.0f, 0.0f);
        r2 = make_float4(s.rgb[g * 3 + 0], 0.0f, s.rgb[g * 3 + 1], s.rgb[g * 3 + 2]);
    }
    r1.w = __int_as_float(g);
    cugs_stage_cull(r0, r1, tile_cx, tile_cy);
    if (DEPTH) r2.y = depths[g];
    s_rec[threadIdx.x * CUGS_REC_F4 + 0] = r0;
    s_rec[threadIdx.x * CUGS_REC_F4 + 1] = r1;
    s_rec[threadIdx.x * CUGS_REC_F4 + 2] = r2;
    return g;
}

// Bounding box, in quad coordinates 0..7, of the lanes set in `active` (lane = y*8 + x; active != 0).
// Pure scalar bit arithmetic on the wave-uniform ballot.  Pixels that are finished (or outside the
// image) can no longer be affected by any Gaussian, so culling against the box of the remaining
// ones stays conservative and prunes the tail where only a few pixels of a quad are still open.
struct ActiveRect { float x0, y0, wx, wy; };
__device__ __forceinline__ ActiveRect active_rect(unsigned long long active, float quad_cx, float quad_cy) {
    unsigned cols = (unsigned)active | (unsigned)(active >> 32);
    cols |= cols >> 16;
    cols |= cols >> 8;
    cols &= 0xFFu;
    const int x0 = __builtin_ctz(cols), x1 = 31 - __builtin_clz(cols);
    const int y0 = __builtin_ctzll(active) >> 3, y1 = (63 - __builtin_clzll(active)) >> 3;
    return ActiveRect{quad_cx + (float)x0, quad_cy + (float)y0, (float)(x1 - x0), (float)(y1 - y0)};
}

// ---------------------------------------------------------------------------------------
// Hit groups.  Both blend kernels take the set bits of a sub-batch's hit mask FOUR at a time: the bits are popped first -
// scalar work on the wave-uniform ballot - and the four per-pixel steps that follow are straight-line code with ONE
// "is any pixel of mine still open" vote behind them instead of one per step.  A step taken after the last pixel closed
// changes nothing.  Forward: `open == 0` is folded into alpha, so the step's alpha and weight are exactly 0.  Backward:
// a closed pixel has rem < 0, so k = sat(passf * rem) == 0 and with it al, weight and the gates are exactly 0; only
// rem itself moves, further below zero.
// The backward keeps the four LDS record indices (float4 units, < 768) in the 16-bit fields of one 64-bit scalar.
// ---------------------------------------------------------------------------------------
#define CUGS_HIT_GROUP 4
__device__ __forceinline__ unsigned cugs_pop_hit_desc(unsigned long long& mask) {       // highest set bit; mask != 0
    const unsigned bit = 63u - (unsigned)__builtin_clzll(mask);
    mask &= ~(1ull << bit);
    return bit;
}
__device__ __forceinline__ unsigned cugs_pop_hit_asc(unsigned long long& mask) {        // lowest set bit; mask != 0
    const unsigned bit = (unsigned)__builtin_ctzll(mask);
    mask &= mask - 1ull;
    return bit;
}
// the four highest bits of `mask` (at least four are set) as record indices rec_base + bit * CUGS_REC_F4, first popped
// in field 0
__device__ __forceinline__ unsigned long long cugs_pop_hits4_desc(unsigned long long& mask, unsigned rec_base) {
    const unsigned r0 = rec_base + cugs_pop_hit_desc(mask) * CUGS_REC_F4;
    const unsigned r1 = rec_base + cugs_pop_hit_desc(mask) * CUGS_REC_F4;
    const unsigned r2 = rec_base + cugs_pop_hit_desc(mask) * CUGS_REC_F4;
    const unsigned r3 = rec_base + cugs_pop_hit_desc(mask) * CUGS_REC_F4;
    return (unsigned long long)(r0 | (r1 << 16)) | ((unsigned long long)(r2 | (r3 << 16)) << 32);
}
__device__ __forceinline__ int cugs_hit(unsigned long long hitrecs, int field) {
    return (int)((hitrecs >> (16 * field)) & 0xFFFFull);
}
__device__ __forceinline__ unsigned long long cugs_set_hit(unsigned long long hitrecs, int field, unsigned rec) {
    return (hitrecs & ~(0xFFFFull << (16 * field))) | ((unsigned long long)rec << (16 * field));
}

// forward.cu:124-141 / backward.cu:123-137 for one pixel, written so that every per-lane decision
// stays in VECTOR registers.  (hipcc keeps a C++ `bool` that differs per lane as a 64-bit lane mask in
// scalar registers and turns `a && b`, `done |= x` into s_and/s_or_b64; a CU has ONE scalar unit for its
// four SIMDs, and the ~45 scalar instructions per step this produced cost more issue time than the
// ~110 vector ones.)  The pixel's "still open" state is a float flag (1 or 0) multiplied into the
// opacity, and skips become alpha = 0, which makes every later product exactly zero.
// The two blends keep that state differently:
//   * forward (and the score kernel): open = [T >= 1/255], recomputed from T in one instruction per step.  T never
//     increases and a closed pixel has alpha = 0, so its T - and the flag - no longer change; a pixel outside the
//     image starts with T = 0.  `open` IS folded into the opacity there: count, T and C must freeze.
//   * backward: the counter rem = n_contrib - passers so far (an integer-valued float; closed <=> rem < 0) is the
//     whole state.  It passes open = 1.0f here: a closed pixel that still sees a passer only takes rem further below
//     zero (lists are far shorter than 2^24, so this stays exact) and the step's k = sat(passf * rem_before) is 0.
//
// Decisions are the oracle's, bit for bit.  FMA placement contract:
//   u = fma(a,dx,b*dy); v = fma(b,dx,c*dy); q = fma(dx,u,dy*v); power = -0.5f*q (never formed here);
//   e = cugs_blend_exp_q(q) = exp(-q/2) clamped below at exp(-6) (cugs_detmath.h: the oracle calls the same
//   function, so e has the same bits there);
//   * power > 0 <=> q < 0 -> skipped: q * 2^127 + 1 (<= -1 for every normal negative q, >= 1 for q >= 0) joins
//     the minimum with 0.99, so alpha comes out negative and fails the 1/255 test;
//   * power < -6: e = exp(-6)(1 + 1e-6) = 0.00248 and opacity <= 1, so alpha < 1/255 = 0.00392 is certain - the
//     oracle reaches the same skip through its alpha test;
//   * open == 0 (forward, score kernel) -> alpha = 0 < 1/255 -> skipped.
// Returns alpha if the Gaussian passes at this pixel, else exactly 0.
struct PixelEval { float dx, dy, gx, gy, e; };
// min(0.99, o e^power) with the power > 0 skip and the open flag folded in, BEFORE the alpha >= 1/255 test.
__device__ __forceinline__ float pixel_alpha_raw(float pxf, float pyf, float mx, float my, float a, float b,
                                                 float c, float o, float open, PixelEval& r) {
    r.dx = pxf - mx;
    r.dy = pyf - my;
    r.gx = fmaf(a, r.dx, b * r.dy);
    r.gy = fmaf(b, r.dx, c * r.dy);
    const float q = fmaf(r.dx, r.gx, r.dy * r.gy);
    r.e = cugs_blend_exp_q(q);
    // q * 2^127 + 1 is >= 1 for q >= 0 and <= -1 for every normal q < 0: as third operand of the minimum it leaves
    // min(alpha, 0.99) alone or turns it negative - below 1/255, skipped (one v_fma + one v_min3)
    const float gate = fmaf(q, 0x1p127f, 1.0f);
    return __builtin_fminf(__builtin_fminf((o * open) * r.e, 0.99f), gate);   // o * 1.0f is exact
}
__device__ __forceinline__ float pixel_alpha(float pxf, float pyf, float mx, float my, float a, float b,
                                             float c, float o, float open, PixelEval& r) {
    const float alpha = pixel_alpha_raw(pxf, pyf, mx, my, a, b, c, o, open, r);
    return (alpha < (1.0f / 255.0f)) ? 0.0f : alpha;
}

// ---------------------------------------------------------------------------------------
// Cost model behind the choices below (tools/microbench/valu_rate.hip on MI355X, 8 waves per SIMD,
// chip-wide wave-instructions per second, plain fma/mul/add = 1 unit):
//   v_fma/v_mul/v_add/v_mov (also with `clamp`)  950 G/s   1.0      v_max/v_min/v_med3            585 G/s  1.6
//   DPP add (any control, any bank mask)       560-590     1.6-1.7  v_cmp (vcc or sgpr pair)      560     1.7
//   v_cndmask (sgpr mask)                        518       1.85     v_rcp/v_exp, v_permlane*_swap 300     3.2
// The blend kernels are bound by this issue rate, so per-lane decisions are kept as 0/1 FLOATS produced by
// `v_fma ... clamp` and multiplied in (1 unit each) instead of v_cmp + v_cndmask (3.55 units a pair), and the
// wave reduction avoids v_cndmask altogether.
// ---------------------------------------------------------------------------------------

// saturate(a*b + c) in one instruction (v_fma_f32 ... clamp).
__device__ __forceinline__ float sat_fma(float a, float b, float c) {
    return __builtin_amdgcn_fmed3f(fmaf(a, b, c), 0.0f, 1.0f);
}
__device__ __forceinline__ float sat_add(float a, float b) { return __builtin_amdgcn_fmed3f(a + b, 0.0f, 1.0f); }
// saturate(a*b) in one instruction (v_mul_f32 ... clamp).  NaN -> 0 (dx10 clamp).
__device__ __forceinline__ float sat_mul(float a, float b) { return __builtin_amdgcn_fmed3f(a * b, 0.0f, 1.0f); }

// 1.0f if x >= 1/255 (the reference's `alpha < 1/255 -> skip`, forward.cu:141 / backward.cu:137) else 0.0f, exactly,
// for every non-NaN x <= 2^31: with p = the float just below 1/255, x >= 1/255 <=> x > p <=> x - p >= ulp = 2^-31.
// The fma rounds (x - p) * 2^32 once: >= 2 when x passes, <= 0 when it does not.  NaN -> 0 (dx10 clamp).
#define CUGS_ALPHA_MIN_PRED 0x1.01010p-8f      /* 0x3B808080: pred(1.0f/255.0f), 1/255 = 0x3B808081 */
__device__ __forceinline__ float passes_alpha_min(float x) {
    return sat_fma(x, 0x1p32f, -CUGS_ALPHA_MIN_PRED * 0x1p32f);
}
// 1.0f if x < 0.99f else 0.0f (x <= 0.99f always here): 0.99f - x >= ulp(0.5..1) = 2^-24.
__device__ __forceinline__ float below_alpha_cap(float x) { return sat_fma(x, -0x1p32f, 0.99f * 0x1p32f); }

// ---------------------------------------------------------------------------------------
// reduce9t: sums NINE per-lane values across the 64 lanes of a wave and leaves each total in a different
// lane ("transpose-reduce": at every halving step two partner lanes exchange the half of the values they
// will not keep, so the number of live values halves as the number of lanes sharing a sum doubles),
// without a single v_cndmask:
//   stage 1  row_mirror (i <-> 15-i, side = lane bit 3 = banks {0,1} | {2,3}):  9 -> 5 values.
//            The "keep mine / give the other" selection is the DPP BANK MASK: `x + dpp(x)` written to banks
//            0,1 from one register and to banks 2,3 from the other (two DPP adds per pair, 3.4 units instead of
//            two selects + one DPP add, 5.3).  The first pair needs no selection at all: the caller hands it
//            over already swizzled (cA holds value 0 in side-0 lanes and value 1 in side-1 lanes, cB the
//            opposite - for the blend backward these are dL/dcolour products whose per-lane factor is
//            swizzled once per kernel), so it is ONE DPP add.
//   stage 2  row_half_mirror (i <-> i^7, side = lane bit 2 = banks {0,2} | {1,3}):  5 -> 3, same trick.
//   stage 3  v_permlane16_swap (rows 0<->1, 2<->3): swaps odd rows of x with even rows of y, so x + y is the
//            transposed pair sum with no selection: 3 -> 2 (the odd value is summed with a copy of itself).
//   stage 4  v_permlane32_swap (halves): 2 -> 1.
//   stages 5, 6  the four lanes of each bank still hold partial sums of the same value: two quad_perm adds.
// 13 DPP adds + 3 swaps + 5 plain = ~37 units (the select-based version: 57).  All 64 lanes must be active.
//
// Result: lane L returns the WAVE total of slot reduce9t_slot(L); within rows 0..2 every lane of a bank holds
// the same total, the first lane of each bank is designated to deliver:
//   row 0: banks 0..3 -> slots 0, 2, 1, 3;  row 1: banks 0..3 -> slots 4, 6, 5, 8;  row 2: slot 7.
// Slot k is the k-th value in the argument order (v0 v1 | v2 v3 | v4 v5 | v6 v8 | v7), where the caller passes
// v0/v1 swizzled as described.
//
// Hand-scheduled inline asm: hipcc pads nothing inside an asm statement, so the wait states gfx950 needs
// between a VALU write and a DPP / permlane read of the same register (2) are s_nops in the string; the
// instruction order keeps producers and DPP consumers at least two instructions apart elsewhere.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ int reduce9t_slot(int lane) {
    if (lane & 3) return -1;
    const int bank = (lane >> 2) & 3, row = lane >> 4;
    const int perm[4] = {0, 2, 1, 3};
    if (row == 0) return perm[bank];
    if (row == 1) return bank == 3 ? 8 : 4 + perm[bank];
    if (row == 2 && bank == 0) return 7;
    return -1;
}

__device__ __forceinline__ float reduce9t(float cA, float cB, float v2, float v3, float v4, float v5, float v6,
                                          float v8, float v7) {
    float a0, a1, a2, a3, a4, b0, b1, b2, d;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %10, %9 row_mirror row_mask:0xf bank_mask:0xf\n\t"       // a0 = cA + mirror(cB)
        "v_add_f32_dpp %1, %11, %11 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a1 = v2 + mirror(v2) | v3 + mirror(v3)
        "v_add_f32_dpp %1, %12, %12 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %2, %13, %13 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a2 = v4 | v5
        "v_add_f32_dpp %2, %14, %14 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %3, %15, %15 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a3 = v6 | v8
        "v_add_f32_dpp %3, %16, %16 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %4, %17, %17 row_mirror row_mask:0xf bank_mask:0xf\n\t"      // a4 = v7
        "v_add_f32_dpp %5, %0, %0 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"   // b0 = a0 | a1
        "v_add_f32_dpp %5, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %7, %4, %4 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"   // b2 = a4
        "v_add_f32_dpp %6, %2, %2 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"   // b1 = a2 | a3
        "v_add_f32_dpp %6, %3, %3 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "v_mov_b32 %8, %7\n\t"                                                      // d = copy of b2
        "s_nop 1\n\t"
        "v_permlane16_swap_b32 %5, %6\n\t"                                          // rows: (b0,b1) transposed
        "v_permlane16_swap_b32 %7, %8\n\t"
        "v_add_f32 %5, %5, %6\n\t"                                                  // c0
        "v_add_f32 %7, %7, %8\n\t"                                                  // c1
        "s_nop 1\n\t"
        "v_permlane32_swap_b32 %5, %7\n\t"                                          // halves: (c0,c1) transposed
        "v_add_f32 %8, %5, %7\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %8, %8, %8 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %8, %8, %8 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3), "=&v"(a4), "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(d)
        : "v"(cA), "v"(cB), "v"(v2), "v"(v3), "v"(v4), "v"(v5), "v"(v6), "v"(v8), "v"(v7));
    return d;
}

// ---------------------------------------------------------------------------------------
// reduce9r16: the same transpose-reduce inside each 16-lane DPP ROW independently (four rows = four different
// Gaussians in the blend backward's second phase).  Stages 1 and 2 as in reduce9t (bank-masked DPP, first pair
// swizzled by lane bit 3); the two in-bank stages use selects (side = lane bit 1, then bit 0): there is no mask
// finer than a bank.  9 -> 5 -> 3 -> 2 -> 1 values; ~36 units per call = 9 per row.
// Result, per row: lane r (0..15) returns the ROW total of slot reduce9r16_slot(r):
//   r = 4*bank + 0 -> slots 0, 2, 1, 3 (bank 0..3);  r = 4*bank + 2 -> slots 4, 6, 5, 8;  r = 1 -> slot 7.
// ---------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ float xchg_add(bool side, float a, float b) {
    return (side ? b : a) + dpp_mov<CTRL>(side ? a : b);
}

__device__ __forceinline__ int reduce9r16_slot(int lane) {
    const int r = lane & 15, bank = r >> 2;
    const int perm[4] = {0, 2, 1, 3};
    if ((r & 3) == 0) return perm[bank];
    if ((r & 3) == 2) return bank == 3 ? 8 : 4 + perm[bank];
    if (r == 1) return 7;
    return -1;
}

// the two in-bank stages (selects on lane bits 1, 0) shared by reduce9r16 and reduce10r16
__device__ __forceinline__ float reduce_r16_tail(float b0, float b1, float b2, int lane) {
    const bool s1 = (lane & 2) != 0, s0 = (lane & 1) != 0;
    const float c0 = xchg_add<0x4E>(s1, b0, b1);                   // quad_perm [2,3,0,1]
    const float c1 = b2 + dpp_mov<0x4E>(b2);
    return xchg_add<0xB1>(s0, c0, c1);                             // quad_perm [1,0,3,2]
}

__device__ __forceinline__ float reduce9r16(float cA, float cB, float v2, float v3, float v4, float v5, float v6,
                                            float v8, float v7, int lane) {
    float a0, a1, a2, a3, a4, b0, b1, b2;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %9, %8 row_mirror row_mask:0xf bank_mask:0xf\n\t"        // a0 = cA + mirror(cB)
        "v_add_f32_dpp %1, %10, %10 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a1 = v2 | v3
        "v_add_f32_dpp %1, %11, %11 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %2, %12, %12 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a2 = v4 | v5
        "v_add_f32_dpp %2, %13, %13 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %3, %14, %14 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a3 = v6 | v8
        "v_add_f32_dpp %3, %15, %15 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %4, %16, %16 row_mirror row_mask:0xf bank_mask:0xf\n\t"      // a4 = v7
        "v_add_f32_dpp %5, %0, %0 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"   // b0 = a0 | a1
        "v_add_f32_dpp %5, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %7, %4, %4 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"   // b2 = a4
        "v_add_f32_dpp %6, %2, %2 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"   // b1 = a2 | a3
        "v_add_f32_dpp %6, %3, %3 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "s_nop 1\n\t"                                                               // the compiler's DPP reads b1 next
        : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3), "=&v"(a4), "=&v"(b0), "=&v"(b1), "=&v"(b2)
        : "v"(cA), "v"(cB), "v"(v2), "v"(v3), "v"(v4), "v"(v5), "v"(v6), "v"(v8), "v"(v7));
    return reduce_r16_tail(b0, b1, b2, lane);
}

// reduce10r16: reduce9r16 with a TENTH value v9 (the depth-map backward's sum of weight * dL/dD).  Stage 1's a4 = v7
// uses no bank selection in reduce9r16 - both halves of a row carry v7 - so it takes v7 | v9 with bank masks 0x3 / 0xc
// (one more DPP add) and everything after it is unchanged: the v7 total lands in lanes r = 1 and 5 of the row as
// before, the v9 total in lanes r = 9 and 13.
// Result, per row: as reduce9r16 plus r = 9 -> slot 9 (reduce10r16_slot).
__device__ __forceinline__ int reduce10r16_slot(int lane) {
    return ((lane & 15) == 9) ? 9 : reduce9r16_slot(lane);
}

__device__ __forceinline__ float reduce10r16(float cA, float cB, float v2, float v3, float v4, float v5, float v6,
                                             float v8, float v7, float v9, int lane) {
    float a0, a1, a2, a3, a4, b0, b1, b2;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %9, %8 row_mirror row_mask:0xf bank_mask:0xf\n\t"        // a0 = cA + mirror(cB)
        "v_add_f32_dpp %1, %10, %10 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a1 = v2 | v3
        "v_add_f32_dpp %1, %11, %11 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %2, %12, %12 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a2 = v4 | v5
        "v_add_f32_dpp %2, %13, %13 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %3, %14, %14 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a3 = v6 | v8
        "v_add_f32_dpp %3, %15, %15 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %4, %16, %16 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a4 = v7 | v9
        "v_add_f32_dpp %4, %17, %17 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %5, %0, %0 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"   // b0 = a0 | a1
        "v_add_f32_dpp %5, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %7, %4, %4 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"   // b2 = a4 (v7 | v9 per half)
        "v_add_f32_dpp %6, %2, %2 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"   // b1 = a2 | a3
        "v_add_f32_dpp %6, %3, %3 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "s_nop 1\n\t"                                                               // the compiler's DPP reads b1 next
        : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3), "=&v"(a4), "=&v"(b0), "=&v"(b1), "=&v"(b2)
        : "v"(cA), "v"(cB), "v"(v2), "v"(v3), "v"(v4), "v"(v5), "v"(v6), "v"(v8), "v"(v7), "v"(v9));
    return reduce_r16_tail(b0, b1, b2, lane);
}

// reduce12ar16: reduce10r16 with an ELEVENTH and TWELFTH value v10, v11 (the AbsGrad backward's two sums of absolute
// per-pixel mean gradients).  Stage 1 gains a sixth pair a5 = v10 | v11 (two DPP adds); stage 2's
// b2 = a4, which uses no bank selection in reduce10r16 - banks 0 and 1 both carry v7, banks 2 and 3 both v9 - takes
// a4 | a5 with bank masks 0x5 / 0xa (one more DPP add).  Everything after it is unchanged: the v7 total lands in lanes
// r = 1 and 3 of the row, v10 in r = 5 and 7, v9 in r = 9 and 11, v11 in r = 13 and 15.  17 DPP adds in stages 1 and 2.
// Result, per row: as reduce10r16 plus r = 5 -> slot 10, r = 13 -> slot 11.  `with9` false (no depth route: the
// caller passes v9 = 0): lane r = 9 is not designated either.
__device__ __forceinline__ int reduce12ar16_slot(int lane, bool with9) {
    const int r = lane & 15;
    if (r == 5) return 10;
    if (r == 13) return 11;
    if (r == 9) return with9 ? 9 : -1;
    return reduce9r16_slot(lane);
}

__device__ __forceinline__ float reduce12ar16(float cA, float cB, float v2, float v3, float v4, float v5, float v6,
                                              float v8, float v7, float v9, float v10, float v11, int lane) {
    float a0, a1, a2, a3, a4, a5, b0, b1, b2;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %10, %9 row_mirror row_mask:0xf bank_mask:0xf\n\t"       // a0 = cA + mirror(cB)
        "v_add_f32_dpp %1, %11, %11 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a1 = v2 | v3
        "v_add_f32_dpp %1, %12, %12 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %2, %13, %13 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a2 = v4 | v5
        "v_add_f32_dpp %2, %14, %14 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %3, %15, %15 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a3 = v6 | v8
        "v_add_f32_dpp %3, %16, %16 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %4, %17, %17 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a4 = v7 | v9
        "v_add_f32_dpp %4, %18, %18 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %5, %19, %19 row_mirror row_mask:0xf bank_mask:0x3\n\t"      // a5 = v10 | v11
        "v_add_f32_dpp %5, %20, %20 row_mirror row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %6, %0, %0 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"   // b0 = a0 | a1
        "v_add_f32_dpp %6, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %8, %4, %4 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"   // b2 = a4 | a5 (v7, v10, v9, v11 per bank)
        "v_add_f32_dpp %8, %5, %5 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %7, %2, %2 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"   // b1 = a2 | a3
        "v_add_f32_dpp %7, %3, %3 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
        "s_nop 1\n\t"                                                               // the compiler's DPP reads b1 next
        : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3), "=&v"(a4), "=&v"(a5), "=&v"(b0), "=&v"(b1), "=&v"(b2)
        : "v"(cA), "v"(cB), "v"(v2), "v"(v3), "v"(v4), "v"(v5), "v"(v6), "v"(v8), "v"(v7), "v"(v9), "v"(v10), "v"(v11));
    return reduce_r16_tail(b0, b1, b2, lane);
}

// reduce12r16: the transpose-reduce of TWELVE per-lane values inside each 16-lane DPP row (the camera-pose backward's
// per-Gaussian rows, project_backward_kernels.h), in plain builtins - it runs once per workgroup, not per blend step, so
// the selects cost nothing that matters.  Stage 1 row_mirror (side = lane bit 3): 12 -> 6; stage 2 row_half_mirror
// (bit 2): 6 -> 3; stage 3 quad_perm [2,3,0,1] (bit 1): 3 -> 2 (values 0 | 1 exchanged, value 2 summed by both);
// stage 4 quad_perm [1,0,3,2] (bit 0): 2 -> 1.  The partners of the four stages are lane ^ 15, ^ 7, ^ 2, ^ 1, which
// together reach all sixteen lanes of the row.  All 64 lanes must be active.
// Result, per row: lane r returns the ROW total of slot reduce12r16_slot(r) = (r&1 ? 2 : (r>>1)&1) + 3*((r>>2)&1) +
// 6*((r>>3)&1); lanes with r&3 == 3 hold a second copy of a slot (-1: not designated).
__device__ __forceinline__ int reduce12r16_slot(int lane) {
    const int r = lane & 15;
    if ((r & 3) == 3) return -1;
    return ((r & 1) ? 2 : ((r >> 1) & 1)) + 3 * ((r >> 2) & 1) + 6 * ((r >> 3) & 1);
}

__device__ __forceinline__ float reduce12r16(const float (&v)[12], int lane) {
    const bool s3 = (lane & 8) != 0, s2 = (lane & 4) != 0;
    float u[6], w[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) u[k] = xchg_add<0x140>(s3, v[k], v[k + 6]);       // row_mirror
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = xchg_add<0x141>(s2, u[k], u[k + 3]);       // row_half_mirror
    return reduce_r16_tail(w[0], w[1], w[2], lane);                                // quad_perm stages
}
