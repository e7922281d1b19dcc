// raster_backward.hip — back-to-front replay of the blend and the 2-D gradient scatter.
//
// Replaces rasterize_backward / k_rasterize_backward (rasterizer/backward.cu:239-306, :31-233) and
// its four zero-fills (backward.cu:259-262).  Reference quirks kept:
//   Q1 contributors are COUNTED from the end of the tile list; the walk stops once the count
//      exceeds the forward's n_contrib (backward.cu:140-145);
//   Q2 T /= max(1-alpha, 1e-5) (:150-151; alpha <= 0.99 makes the max a no-op); a clamped alpha
//      (o e^power >= 0.99) zeroes dL/do and dL/dpower but dL/drgb still flows (:181-191);
//   Q3 dL/db is the combined off-diagonal derivative -dx dy (:211).
//
// What is different from the reference is the scatter.  The reference issues nine float atomics
// per (pixel, Gaussian) contribution (backward.cu:217-228).  Here all 64 pixels of a wave look at
// the same Gaussian in the same step, so the partials are summed across the wave first (through LDS and a
// 16-lane DPP reduction, see the kernel's comment) and leave it as ONE atomic wave-instruction per four
// Gaussians, nine active lanes per Gaussian hitting nine consecutive floats of its 64-byte-aligned
// accumulator row - a single memory-side request each (MI355X_MICROARCH.md, Global float atomics).
//
// The kernel is bound by VALU issue (profiles/README.md), so the step is written for instruction
// count, priced with the measured costs in cugs_raster_common.h:
//   * every per-lane decision is a 0/1 float made by `v_fma ... clamp` and multiplied in: no v_cmp /
//     v_cndmask pairs.  The Q1 counter `rem` = n_contrib - passers so far is the pixel's whole state: it is open
//     while rem >= 0, and a step contributes where k = sat(passf * rem_before) - ONE v_mul ... clamp.  The open flag
//     is not folded into the opacity here (the forward needs that, to freeze count, T and C): a closed pixel that
//     still sees a passer only takes rem further below zero, k stays 0, and with k == 0 the step's al, weight and
//     gates are exactly 0 and rcp(1) = 1 - T and D keep their bits;
//   * the colour accumulators S_c (backward.cu:83-87, 196-198) only ever enter as sum_c dL/dC_c S_c:
//     that ONE dot product D is carried instead (D += weight * G, G = sum_c dL/dC_c c_c);
//   * the five geometric gradients are accumulated as the MOMENTS of dL/dpower over the pixel offsets,
//     M1 = sum dpw (dx, dy), M2 = sum dpw (dx^2, dx dy, dy^2) - two products fewer per step than
//     dpw * (a dx + b dy) etc.; the per-Gaussian linear map to dL/dmean2d = Sigma'^-1 M1 and
//     dL/dSigma'^-1 = (-M2xx/2, -M2xy, -M2yy/2) is applied once per Gaussian by the consumer
//     (k_project_backward / k_unpack_grads).  Accumulator row: {drgb[3], dopa, M1x, M1y, M2xx, M2xy, M2yy};
//   * T *= rcp(1 - al) needs no "did it contribute" select: v_rcp_f32(1.0f) is exactly 1.0f
//     (tests/test_gpu_reduce9.py checks it on the device).
// DEPTH (the depth route of cugs_blend_backward_opts): the depth map is a colour channel with c = z (record word 9)
// and background 0, the alpha map 1 - final_T one with c = 1 and background 0.  dL/dD joins the per-step dot product
// (G += dL/dD z: one FMA) and phase 2 forms a TENTH sum, sum weight * dL/dD = dL/dz, delivered to word 9 of the row by
// reduce10r16.  dL/dA needs no per-step work: sum_i alpha_i T_i + final_T = 1, so the channel (c = 1, bg = 0) has the
// gradient of (c = 0, bg = -1), which only enters D's starting value (D -= final_T dL/dA).
// ABS (cugs_blend_backward_opts::abs_grad): the AbsGrad densification signal.  Phase 2 also forms, per
// Gaussian, sum |dL/dpower (a dx + b dy)| and sum |dL/dpower (b dx + c dy)| over the pixels - the per-pixel summands of
// dL/dmean2d with fabs around each - and reduce12ar16 delivers them to words 10 and 11 of the row.  Phase 1 is unchanged.
// The summation order differs from any sequential order; the oracle accumulates in fp64.
// Per-contribution VALUES (not decisions) use v_rcp_f32 and fused multiply-adds: 1 ulp-level
// differences from the oracle's divisions, far inside the 1e-4 bar.
#include "cugs_raster_common.h"

#include <cstdlib>

#ifdef CUGS_DEV
bool cugs_dev_backward_stats();
#endif

namespace {

// Two phases per wave:
//   phase 1, once per (wave, Gaussian) step, lane = pixel of the wave's 8x8 quad: the decisions, the T and D
//     recurrences and the two per-pixel scalars every gradient of this contribution is made of -
//     weight = alpha T (for dL/dcolour) and v3 = gated dL/dalpha * e (dL/dopacity; dL/dpower = v3 * opacity) -
//     written to LDS as one 8-byte store per lane;
//   phase 2, once per CUGS_BWD_HITS steps, lane = (Gaussian h = lane / 16, pixel group g = lane % 16 of four
//     horizontally adjacent pixels): reads its Gaussian's contributions back, forms the nine sums over its four
//     pixels (the per-lane constants are the pixels' dL/dcolour and coordinates; dy is common to the four, so
//     sum dpw dy, dx dy, dy^2 follow from the others), reduces them across the 16 lanes of its DPP row
//     (reduce9r16) and issues one atomic instruction: nine lanes per Gaussian, one 64-byte request each.
// Against reducing nine values over 64 lanes in every step (38 units) this costs ~19 units per step; the pending
// Gaussians are flushed before the record batch they point into is re-staged.
#define CUGS_BWD_HITS 4
static_assert(CUGS_BWD_HITS == CUGS_HIT_GROUP, "a hit group is one flush");
#ifndef CUGS_BWD_ABS_WAVES
#define CUGS_BWD_ABS_WAVES 7         /* the ABS variants' occupancy target */
#endif
#ifndef CUGS_BWD_HSTRIDE
#define CUGS_BWD_HSTRIDE 64        /* float2 per Gaussian block: the 64 pixels, no padding - see the LDS budget below */
#endif

// WIDE: accumulator larger than 4 GiB (n > 2^26 rows): 64-bit scatter addresses.
// STATS (dev builds only): step counters written to accumulator row `stats_row` (tools/ablate_backward.py).
// DEPTH: the depth / alpha maps' gradients too (dL_ddepth_map, dL_dalpha: [H,W], either may be NULL = zero).
// ABS: the absolute 2-D mean gradients too (words 10, 11 of the row); with or without DEPTH.
template <bool PACKED, bool WIDE, bool STATS, bool DEPTH = false, bool ABS = false>
__global__ __launch_bounds__(CUGS_BLOCK) __attribute__((amdgpu_waves_per_eu(ABS ? CUGS_BWD_ABS_WAVES : (DEPTH ? 7 : 8))))
void k_raster_backward(RasterGeom geo, RasterSrc src,
                                                                const float* __restrict__ dL_dcolor,
                                                                const float* __restrict__ final_T,
                                                                const int32_t* __restrict__ n_contrib,
                                                                float* __restrict__ grad_accum, int64_t stats_row,
                                                                const float* __restrict__ depths,
                                                                const float* __restrict__ dL_ddepth_map,
                                                                const float* __restrict__ dL_dalpha) {
    // LDS budget: 12288 B of records + 8192 B of contributions = 20480 B = 1/8 of a CU's 160 KB, so EIGHT workgroups
    // (32 waves, the CU's limit) are resident instead of the seven that 20.8 KB allowed (round 2: 16 bytes of padding
    // per contribution block, 64 + 16 bytes of hit-record and vote words).  The record index of each pending Gaussian
    // travels in a wave-uniform 64-bit scalar (16 bits each), and a wave's "all my pixels are done" vote sits in the
    // first word of its own - at that point idle - contribution block (see the loop head).
    __shared__ float4 s_rec[CUGS_BLOCK * CUGS_REC_F4];
    __shared__ float2 s_contrib[4][CUGS_BWD_HITS][CUGS_BWD_HSTRIDE];

#ifdef CUGS_DEV
    const bool no_atomics = stats_row == -2;       // development build: the kernel without its scatter (timing only; tools/ablate_backward.py)
#else
    constexpr bool no_atomics = false;
#endif
    // heaviest tile first when the caller brings an order (cugs_tile_order: kernel-uniform), else the spatial order
    unsigned tile;
    int range_start, range_end;
    if (src.tile_order) {
        const uint4 rec = src.tile_order[blockIdx.x];
        tile = rec.x; range_start = (int)rec.y; range_end = (int)rec.z;
    } else {
        tile = cugs_blend_tile(blockIdx.x, (unsigned)geo.ntx, (unsigned)(geo.ntiles / geo.ntx));
        range_start = src.tile_ranges[tile * 2 + 0];
        range_end = src.tile_ranges[tile * 2 + 1];
    }
    const int tile_x = (int)(tile % (unsigned)geo.ntx), tile_y = (int)(tile / (unsigned)geo.ntx);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int quad_x = tile_x * CUGS_TILE + (wave & 1) * 8, quad_y = tile_y * CUGS_TILE + (wave >> 1) * 8;
    const int px = quad_x + (lane & 7), py = quad_y + (lane >> 3);
    const bool inside = (px < geo.width) && (py < geo.height);
    const float pxf = (float)px + 0.5f, pyf = (float)py + 0.5f;
    const float qx0 = (float)quad_x + 0.5f, qy0 = (float)quad_y + 0.5f;
    const float tile_cx = (float)(tile_x * CUGS_TILE + CUGS_TILE / 2), tile_cy = (float)(tile_y * CUGS_TILE + CUGS_TILE / 2);

    const int num_in_range = range_end - range_start;
    const int num_batches = (num_in_range + CUGS_BLOCK - 1) / CUGS_BLOCK;

    const int pix = py * geo.width + px;
    float T = inside ? final_T[pix] : 0.0f;
    const int max_contrib = inside ? n_contrib[pix] : 0;
    float dC0 = 0.0f, dC1 = 0.0f, dC2 = 0.0f;
    if (inside) {
        dC0 = dL_dcolor[pix * 3 + 0];
        dC1 = dL_dcolor[pix * 3 + 1];
        dC2 = dL_dcolor[pix * 3 + 2];
    }
    float dDp = 0.0f;                                            // DEPTH: this pixel's dL/dD
    if (DEPTH && inside && dL_ddepth_map) dDp = dL_ddepth_map[pix];
    // ---- phase-2 constants: this lane's Gaussian slot h and its four pixels (row gy, columns gx0 .. gx0+3)
    const int h2 = lane >> 4, g2i = lane & 15;
    const int gx0 = quad_x + (g2i & 1) * 4, gy = quad_y + (g2i >> 1);
    const float px2 = (float)gx0 + 0.5f, py2 = (float)gy + 0.5f;
    // reduce9r16 takes its first pair swizzled: red in lanes with bit 3 clear, green in the others
    const bool side = (lane & 8) != 0;
    float eA[4], eB[4], e2[4], eZ[4];                        // eZ: DEPTH only, the four pixels' dL/dD
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float r = 0.0f, gg = 0.0f, bb = 0.0f, zz = 0.0f;
        if (gx0 + i < geo.width && gy < geo.height) {
            const int pq = gy * geo.width + gx0 + i, q = pq * 3;
            r = dL_dcolor[q + 0]; gg = dL_dcolor[q + 1]; bb = dL_dcolor[q + 2];
            if (DEPTH && dL_ddepth_map) zz = dL_ddepth_map[pq];
        }
        eA[i] = side ? gg : r; eB[i] = side ? r : gg; e2[i] = bb; eZ[i] = zz;
    }
    const int slot2 = ABS ? reduce12ar16_slot(lane, DEPTH) : DEPTH ? reduce10r16_slot(lane) : reduce9r16_slot(lane);
    const unsigned slot_off = (unsigned)(slot2 < 0 ? 0 : slot2) * 4u;
    unsigned long long hitrecs = 0ull;                       // record (float4) index of pending Gaussian h in bits [16h, 16h+16);
                                                             // stale slots of a partial flush stay valid indices

    // D = sum_c dL/dC_c * (colour accumulated behind the current Gaussian), starting from the background
    float D = fmaf(dC2, T * geo.bg2, fmaf(dC1, T * geo.bg1, dC0 * (T * geo.bg0)));      // backward.cu:83-87
    if (DEPTH && inside && dL_dalpha) D = fmaf(-T, dL_dalpha[pix], D);    // the alpha map: channel (c = 0, bg = -1)
    // rem = n_contrib - (passing Gaussians seen so far, counted from the END: Q1).  A pixel stops - without
    // contributing - at the passer that takes rem below zero (backward.cu:141-145); a pixel with
    // n_contrib == 0, or outside the image, starts out finished.  A pixel is open <=> rem >= 0; rem is an
    // integer-valued float, and a finished pixel that sees further passers only takes it further below zero (exact: a
    // tile list is far shorter than 2^24).
    float rem = (inside && max_contrib > 0) ? (float)max_contrib : -1.0f;
    bool wave_done = (__ballot(rem >= 0.0f) == 0ull);
    // The hit loop works in GROUPS of CUGS_BWD_HITS hits: the record indices are popped from the sub-batch's hit mask
    // first (scalar work, constant shifts), then the four phase-1 steps run as straight-line code with constant
    // contribution slots, ONE "all my pixels are closed" vote follows, then phase 2.  `pending` counts the hits of an
    // unfinished group: popped into hitrecs[0 .. pending) at the end of a sub-batch, NOT yet evaluated; the next
    // sub-batch of the same 256-record batch tops the group up (its cull then sees open pixels up to three steps
    // old - a larger rectangle, so still conservative), the end of the batch runs what is left one step at a time.
    int pending = 0;                                            // wave-uniform, 0 .. CUGS_BWD_HITS - 1 between groups
    unsigned st_steps = 0, st_contrib = 0, st_lanes = 0, st_batches = 0, st_tested = 0, st_open = 0;   // STATS only

    // phase 2 for the `cnt` pending Gaussians of this wave
    auto flush = [&](int cnt) {
        const int rec = (int)((hitrecs >> (16 * h2)) & 0xFFFFull);                     // float4 index of the record
        const float4* c4 = reinterpret_cast<const float4*>(&s_contrib[wave][h2][g2i * 4]);
        const float4 p01 = c4[0], p23 = c4[1];                                         // (weight, v3) x 4 pixels
        float4 head;                                                                   // mean x, y (ABS: and a, b)
        if (ABS) {
            head = s_rec[rec];
        } else {
            const float2 m = *reinterpret_cast<const float2*>(&s_rec[rec]);
            head = make_float4(m.x, m.y, 0.0f, 0.0f);
        }
        const float2 mean = make_float2(head.x, head.y);
        const float4 tail = s_rec[rec + 1];                                            // c, opacity, cull limit, index
        const float dy = py2 - mean.y;
        const float dx0 = px2 - mean.x, dx1 = dx0 + 1.0f, dx2 = dx0 + 2.0f, dx3 = dx0 + 3.0f;
        float t = p01.y * dx0;
        float A = p01.y, M1 = t, Mxx = t * dx0;
        float RA = p01.x * eA[0], RB = p01.x * eB[0], R2 = p01.x * e2[0];
        t = p01.w * dx1; A += p01.w; M1 += t; Mxx = fmaf(t, dx1, Mxx);
        RA = fmaf(p01.z, eA[1], RA); RB = fmaf(p01.z, eB[1], RB); R2 = fmaf(p01.z, e2[1], R2);
        t = p23.y * dx2; A += p23.y; M1 += t; Mxx = fmaf(t, dx2, Mxx);
        RA = fmaf(p23.x, eA[2], RA); RB = fmaf(p23.x, eB[2], RB); R2 = fmaf(p23.x, e2[2], R2);
        t = p23.w * dx3; A += p23.w; M1 += t; Mxx = fmaf(t, dx3, Mxx);
        RA = fmaf(p23.z, eA[3], RA); RB = fmaf(p23.z, eB[3], RB); R2 = fmaf(p23.z, e2[3], R2);
        // dL/dpower = v3 * opacity (alpha = opacity * e where the gate is open); dy is common to the four pixels
        const float oA = tail.y * A;
        M1 *= tail.y; Mxx *= tail.y;
        const float M1y = dy * oA, Myy = dy * M1y, Mxy = dy * M1;
        float total;
        if (ABS) {
            // |dL/dpower (a dx_k + b dy)| = |v3_k| |opacity| |a dx_k + b dy|, the same with (b, c): one FMA for the
            // linear form, one multiply-add with both factors' sign bits cleared (source modifiers) per pixel and sum
            const float bdy = head.w * dy, cdy = tail.x * dy;
            float SX = fabsf(p01.y) * fabsf(fmaf(head.z, dx0, bdy));
            float SY = fabsf(p01.y) * fabsf(fmaf(head.w, dx0, cdy));
            SX = fmaf(fabsf(p01.w), fabsf(fmaf(head.z, dx1, bdy)), SX);
            SY = fmaf(fabsf(p01.w), fabsf(fmaf(head.w, dx1, cdy)), SY);
            SX = fmaf(fabsf(p23.y), fabsf(fmaf(head.z, dx2, bdy)), SX);
            SY = fmaf(fabsf(p23.y), fabsf(fmaf(head.w, dx2, cdy)), SY);
            SX = fmaf(fabsf(p23.w), fabsf(fmaf(head.z, dx3, bdy)), SX);
            SY = fmaf(fabsf(p23.w), fabsf(fmaf(head.w, dx3, cdy)), SY);
            const float ao = fabsf(tail.y);
            SX *= ao; SY *= ao;
            float RZ = 0.0f;
            if (DEPTH) {
                RZ = p01.x * eZ[0];
                RZ = fmaf(p01.z, eZ[1], RZ); RZ = fmaf(p23.x, eZ[2], RZ); RZ = fmaf(p23.z, eZ[3], RZ);
            }
            total = reduce12ar16(RA, RB, R2, A, M1, M1y, Mxx, Myy, Mxy, RZ, SX, SY, lane);
        } else if (DEPTH) {
            float RZ = p01.x * eZ[0];
            RZ = fmaf(p01.z, eZ[1], RZ); RZ = fmaf(p23.x, eZ[2], RZ); RZ = fmaf(p23.z, eZ[3], RZ);
            total = reduce10r16(RA, RB, R2, A, M1, M1y, Mxx, Myy, Mxy, RZ, lane);
        } else {
            total = reduce9r16(RA, RB, R2, A, M1, M1y, Mxx, Myy, Mxy, lane);
        }
        if (slot2 >= 0 && h2 < cnt && !no_atomics) {
            const int g = __float_as_int(tail.w);
            if (WIDE) {
                atomicAdd(grad_accum + (int64_t)g * CUGS_GRAD_STRIDE + slot2, total);
            } else {
                const unsigned off = ((unsigned)g << 6) + slot_off;               // row bytes = 4 * CUGS_GRAD_STRIDE = 64
                atomicAdd(reinterpret_cast<float*>(reinterpret_cast<char*>(grad_accum) + off), total);
            }
        }
    };

    // phase 1 for the record at float4 index `rec` (wave-uniform); its contribution goes to slot `slot` of the wave's
    // block.  Inlined at each call: in the group loop `slot` is a constant and the store takes an immediate offset.
    auto step = [&](const int rec, const int slot) __attribute__((always_inline)) {
        if (STATS) ++st_steps;
        const float4 g0 = s_rec[rec], g1 = s_rec[rec + 1], col = s_rec[rec + 2];
        const float o = g1.y;

        // ---- decisions (backward.cu:123-145) as 0/1 floats
        PixelEval e;
        // open = 1.0f: the counter alone closes a pixel (see the header comment); o * 1.0f folds away
        const float alpha = pixel_alpha_raw(pxf, pyf, g0.x, g0.y, g0.z, g0.w, g1.x, o, 1.0f, e);
        const float passf = passes_alpha_min(alpha);           // alpha >= 1/255: exactly 0 or 1
        // 1: this Gaussian contributes here - it passes and rem >= 1 BEFORE it is counted (the passer that takes rem
        // below zero stops the pixel without contributing, Q1); rem <= 0, a finished pixel included, clamps to 0
        const float k = sat_mul(passf, rem);
        rem -= passf;                                          // contributors counted from the END (Q1)
        const float al = alpha * k;
        // clamp gate (backward.cu:181-191): o e >= 0.99 <=> alpha == 0.99f zeroes dL/do and dL/dpower,
        // dL/drgb still flows
        const float gk = k * below_alpha_cap(alpha);

        // ---- values (v_rcp_f32 + FMAs); k == 0 makes both outputs exactly zero
        const float rcp = __builtin_amdgcn_rcpf(1.0f - al);    // al <= 0.99; rcp(1) == 1 exactly
        T *= rcp;                                              // T_before = T_after / (1 - alpha)
        const float weight = al * T;
        float G = fmaf(dC2, col.w, fmaf(dC1, col.z, dC0 * col.x));
        if (DEPTH) G = fmaf(dDp, col.y, G);                    // + dL/dD z (record word 9)
        const float gate = fmaf(T, G, -(rcp * D)) * gk;        // dL/dalpha, gated
        D = fmaf(weight, G, D);
        if (STATS) {
            const unsigned long long lm = __ballot(k != 0.0f);
            if (lm) { ++st_contrib; st_lanes += __popcll(lm); st_open += __popcll(__ballot(rem >= 0.0f)); }
        }
        s_contrib[wave][slot][lane] = make_float2(weight, gate * e.e);
    };

    for (int batch = num_batches - 1; batch >= 0; --batch) {
        // The vote word is the first word of the wave's own contribution block: every pending Gaussian has been flushed
        // when a wave arrives here, nobody else touches the block, all four waves read the words between this barrier
        // and the next, and the block is written again (phase 1) only after that next barrier.
        if (lane == 0) s_contrib[wave][0][0].x = wave_done ? 1.0f : 0.0f;
        __syncthreads();
        if (s_contrib[0][0][0].x * s_contrib[1][0][0].x * s_contrib[2][0][0].x * s_contrib[3][0][0].x != 0.0f) break;

        stage_record<PACKED, DEPTH>(src, range_start + batch * CUGS_BLOCK + tid, range_end, s_rec, tile_cx, tile_cy, depths);
        __syncthreads();

        if (STATS && !wave_done) ++st_batches;
        if (!wave_done) {
            const int batch_count = min(CUGS_BLOCK, num_in_range - batch * CUGS_BLOCK);
            const int nsub = (batch_count + CUGS_WAVE - 1) / CUGS_WAVE;
            for (int sub = nsub - 1; sub >= 0 && !wave_done; --sub) {
                const int j = sub * CUGS_WAVE + lane;
                const ActiveRect ar = active_rect(__ballot(rem >= 0.0f), qx0, qy0);   // !wave_done => non-empty
                bool hit = false;
                if (j < batch_count)
                    hit = may_touch_quad(s_rec[j * CUGS_REC_F4 + 0], s_rec[j * CUGS_REC_F4 + 1], ar.x0, ar.y0, ar.wx,
                                         ar.wy);
                unsigned long long mask = __ballot(hit);
                if (STATS) st_tested += min(CUGS_WAVE, batch_count - sub * CUGS_WAVE);
                const unsigned rec_sub = (unsigned)(sub * CUGS_WAVE * CUGS_REC_F4);
                // ---- whole groups: four hits (back to front: highest bit first), straight-line
                while (pending + __popcll(mask) >= CUGS_BWD_HITS) {
                    if (pending == 0) {
                        hitrecs = cugs_pop_hits4_desc(mask, rec_sub);       // constant shifts
                    } else {                                               // top up the group a sub-batch left behind
                        do hitrecs = cugs_set_hit(hitrecs, pending, rec_sub + cugs_pop_hit_desc(mask) * CUGS_REC_F4);
                        while (++pending < CUGS_BWD_HITS);
                        pending = 0;
                    }
                    step(cugs_hit(hitrecs, 0), 0);
                    step(cugs_hit(hitrecs, 1), 1);
                    step(cugs_hit(hitrecs, 2), 2);
                    step(cugs_hit(hitrecs, 3), 3);
                    // ONE vote per group.  A step taken after the last pixel closed has rem < 0, so k == 0, in every
                    // lane: al = 0, rcp(1) = 1, weight = gate = 0 - T and D stay, rem only sinks further, the sums gain
                    // a zero.
                    const bool closed = (__ballot(rem >= 0.0f) == 0ull);
                    flush(CUGS_BWD_HITS);
                    if (closed) { wave_done = true; mask = 0ull; break; }
                }
                // ---- fewer than four left: they wait, as record indices, for the next sub-batch of this batch
                while (mask != 0ull) {
                    hitrecs = cugs_set_hit(hitrecs, pending, rec_sub + cugs_pop_hit_desc(mask) * CUGS_REC_F4);
                    ++pending;
                }
            }
            if (pending) {                 // the partial group: before s_rec is re-staged (and at the end of the wave's walk)
                for (int p = 0; p < pending; ++p) step(cugs_hit(hitrecs, p), p);
                if (__ballot(rem >= 0.0f) == 0ull) wave_done = true;
                flush(pending);
                pending = 0;
            }
        }
        // the next iteration's first barrier orders this batch's LDS reads before the re-staging
    }
    if (STATS && lane == 0) {
        float* st = grad_accum + (int64_t)stats_row * CUGS_GRAD_STRIDE;
        atomicAdd(&st[0], (float)st_steps); atomicAdd(&st[1], (float)st_contrib); atomicAdd(&st[2], (float)st_lanes);
        atomicAdd(&st[3], (float)st_batches); atomicAdd(&st[4], (float)st_tested); atomicAdd(&st[5], (float)num_batches);
        atomicAdd(&st[7], (float)st_open);
    }
}

// grad_accum rows -> the four reference-layout tensors of RasterizeBackwardOutput (backward.hpp); applies the
// per-Gaussian map from the accumulated moments (see the header comment) with Sigma'^-1 = (a, b, c).
// DEPTH: also dL_ddepths [n] from word 9.  ABS: also dL_dmeans_abs [n,2] from words 10 and 11.
template <bool PACKED, bool DEPTH = false, bool ABS = false>
__global__ __launch_bounds__(CUGS_BLOCK) void k_unpack_grads(int64_t n, const float* __restrict__ acc,
                                                             const float* __restrict__ packed,
                                                             const float* __restrict__ cov_2d_inv,
                                                             float* __restrict__ dL_drgb,
                                                             float* __restrict__ dL_dopa,
                                                             float* __restrict__ dL_dmeans,
                                                             float* __restrict__ dL_dcov,
                                                             float* __restrict__ dL_ddepths,
                                                             float* __restrict__ dL_dmeans_abs) {
    const int64_t i = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4* row = reinterpret_cast<const float4*>(acc + i * CUGS_GRAD_STRIDE);
    const float4 r0 = row[0], r1 = row[1];
    float r2;
    if (ABS) {
        const float4 w = row[2];                                                    // M2yy, dL_dz, abs x, abs y
        r2 = w.x;
        if (DEPTH) dL_ddepths[i] = w.y;
        *reinterpret_cast<float2*>(dL_dmeans_abs + i * 2) = make_float2(w.z, w.w);
    } else if (DEPTH) {
        const float2 w89 = *reinterpret_cast<const float2*>(acc + i * CUGS_GRAD_STRIDE + 8);
        r2 = w89.x;
        dL_ddepths[i] = w89.y;
    } else {
        r2 = acc[i * CUGS_GRAD_STRIDE + 8];
    }
    float a, b, c;
    if (PACKED) {
        const float4* rec = reinterpret_cast<const float4*>(packed + i * CUGS_PACKED_STRIDE);
        const float4 p0 = rec[0];
        a = p0.z; b = p0.w; c = rec[1].x;
    } else {
        a = cov_2d_inv[i * 3 + 0]; b = cov_2d_inv[i * 3 + 1]; c = cov_2d_inv[i * 3 + 2];
    }
    dL_drgb[i * 3 + 0] = r0.x; dL_drgb[i * 3 + 1] = r0.y; dL_drgb[i * 3 + 2] = r0.z;
    dL_dopa[i] = r0.w;
    const GradMoments m{r1.x, r1.y, r1.z, r1.w, r2};
    const Grad2D g = grads_from_moments(m, a, b, c);
    dL_dmeans[i * 2 + 0] = g.mx; dL_dmeans[i * 2 + 1] = g.my;
    dL_dcov[i * 3 + 0] = g.a; dL_dcov[i * 3 + 1] = g.b; dL_dcov[i * 3 + 2] = g.c;
}

}  // namespace

extern "C" int cugs_rasterize_backward_opts(int width, int height, const float background_host[3],
                                            const int32_t* tile_ranges, const int32_t* gaussian_indices,
                                            const float* means_2d, const float* cov_2d_inv, const float* rgb,
                                            const float* opacities_act, const float* packed,
                                            const float* dL_dcolor, const float* final_T,
                                            const int32_t* n_contrib, int64_t n, float* grad_accum,
                                            float* dL_drgb, float* dL_dopacity_act, float* dL_dmeans_2d,
                                            float* dL_dcov_2d_inv, const cugs_blend_backward_opts* opts, void* stream) {
    const cugs_blend_backward_opts o = opts ? *opts : cugs_blend_backward_opts{};
    const bool depth_map = o.depths || o.dL_ddepth_map || o.dL_dalpha;    // all NULL: the colour-only kernels
    const bool abs_grad = o.abs_grad != 0;
    if (width < 0 || height < 0 || n < 0 || !background_host) return CUGS_EINVAL;
    if (n == 0) return 0;
    if (!grad_accum) return CUGS_EINVAL;
    if ((reinterpret_cast<uintptr_t>(grad_accum) & 63u) != 0) return CUGS_EALIGN;
    const int n_soa = (dL_drgb != nullptr) + (dL_dopacity_act != nullptr) + (dL_dmeans_2d != nullptr) +
                      (dL_dcov_2d_inv != nullptr);
    if (n_soa != 0 && n_soa != 4) return CUGS_EINVAL;
    if (depth_map && (n_soa == 4) != (o.dL_ddepths != nullptr)) return CUGS_EINVAL;   // dL_ddepths with the four, not alone
    if (!depth_map && o.dL_ddepths) return CUGS_EINVAL;                               // ... and on the depth route only
    if (abs_grad && (n_soa == 4) != (o.dL_dmeans_2d_abs != nullptr)) return CUGS_EINVAL;   // the same for the absolute tensor
    if (n_soa == 4 && !packed && !cov_2d_inv) return CUGS_EINVAL;
    if (packed && !cugs_aligned16(packed)) return CUGS_EALIGN;
    if (o.tile_order && !cugs_aligned16(o.tile_order)) return CUGS_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t rows = n;
#ifdef CUGS_DEV
    const bool stats = cugs_dev_backward_stats();          // the caller allocated n + 1 rows (tools/ablate_backward.py)
    if (stats) rows = n + 1;
#endif
    if (!o.prezeroed || rows != n)
        CUGS_RETURN_IF_HIP(hipMemsetAsync(grad_accum, 0, sizeof(float) * CUGS_GRAD_STRIDE * (size_t)rows, st));

    const int ntx = (width + CUGS_TILE - 1) / CUGS_TILE, nty = (height + CUGS_TILE - 1) / CUGS_TILE;
    if (ntx > 0 && nty > 0 && gaussian_indices) {               // backward.cu:267-269; NULL indices = no pairs
        if (!tile_ranges || !dL_dcolor || !final_T || !n_contrib) return CUGS_EINVAL;
        if (!packed && (!means_2d || !cov_2d_inv || !rgb || !opacities_act)) return CUGS_EINVAL;
        if (depth_map && !o.depths) return CUGS_EINVAL;
        if ((int64_t)width * height > 2147483647ll / 3) return CUGS_EOVERFLOW;
        RasterGeom geo{width, height, ntx, ntx * nty, background_host[0], background_host[1], background_host[2]};
        RasterSrc src{tile_ranges, gaussian_indices, packed, means_2d, cov_2d_inv, rgb, opacities_act, reinterpret_cast<const uint4*>(o.tile_order)};
        const bool wide = rows > (int64_t(1) << 26);            // 64-byte rows beyond a 32-bit byte offset
        int64_t stats_arg = n;                                  // STATS builds: the row that takes the counters
#ifdef CUGS_DEV
        if (const char* e = std::getenv("CUGS_BWD_NO_ATOMICS")) if (e[0] == '1') stats_arg = -2;
#endif
        const auto launch = [&](auto* kernel) {
            hipLaunchKernelGGL(kernel, dim3(geo.ntiles), dim3(CUGS_BLOCK), 0, st, geo, src, dL_dcolor, final_T, n_contrib,
                               grad_accum, stats_arg, o.depths, o.dL_ddepth_map, o.dL_dalpha);
        };
#ifdef CUGS_DEV
        if (stats && !depth_map && !abs_grad)                   // no step counters on the DEPTH and ABS routes
            cugs_with_bool(packed != nullptr, [&](auto P) { launch(k_raster_backward<P(), true, true>); });
        else
#endif
        cugs_with_bool(packed != nullptr, [&](auto P) { cugs_with_bool(wide, [&](auto W) {
            cugs_with_bool(depth_map, [&](auto D) { cugs_with_bool(abs_grad, [&](auto A) {
                launch(k_raster_backward<P(), W(), false, D(), A()>);
            }); });
        }); });
        CUGS_LAUNCH_CHECK();
    }
    if (n_soa == 4) {
        const dim3 grid((unsigned)((n + CUGS_BLOCK - 1) / CUGS_BLOCK));
        cugs_with_bool(packed != nullptr, [&](auto P) { cugs_with_bool(depth_map, [&](auto D) {
            cugs_with_bool(abs_grad, [&](auto A) {
                hipLaunchKernelGGL((k_unpack_grads<P(), D(), A()>), grid, dim3(CUGS_BLOCK), 0, st, n, grad_accum, packed,
                                   cov_2d_inv, dL_drgb, dL_dopacity_act, dL_dmeans_2d, dL_dcov_2d_inv, o.dL_ddepths,
                                   o.dL_dmeans_2d_abs);
            });
        }); });
        CUGS_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int cugs_rasterize_backward(int width, int height, const float background_host[3],
                                       const int32_t* tile_ranges, const int32_t* gaussian_indices,
                                       const float* means_2d, const float* cov_2d_inv, const float* rgb,
                                       const float* opacities_act, const float* packed,
                                       const float* dL_dcolor, const float* final_T,
                                       const int32_t* n_contrib, int64_t n, float* grad_accum,
                                       float* dL_drgb, float* dL_dopacity_act, float* dL_dmeans_2d,
                                       float* dL_dcov_2d_inv, void* stream) {
    return cugs_rasterize_backward_opts(width, height, background_host, tile_ranges, gaussian_indices, means_2d, cov_2d_inv,
                                        rgb, opacities_act, packed, dL_dcolor, final_T, n_contrib, n, grad_accum, dL_drgb,
                                        dL_dopacity_act, dL_dmeans_2d, dL_dcov_2d_inv, nullptr, stream);
}

#ifdef CUGS_DEV
// ---- development hooks (libcugs_hip_dev.so only; not part of include/cugs_hip.h) ------------------
// cugsdbg_reduce9: one wave runs reduce9t on caller data.  in: [9][64] floats (value k of lane l at k*64+l,
// k = slot); out: [64] floats (each lane's result), slots: [64] ints.
// cugsdbg_rcp: out[i] = v_rcp_f32(in[i]).
// cugsdbg_may_touch_quad: see k_dbg_may_touch_quad.
namespace {
__global__ void k_dbg_reduce9(const float* __restrict__ in, float* __restrict__ out, int* __restrict__ slots) {
    const int l = threadIdx.x;
    const bool side = (l & 8) != 0;
    const float v0 = in[0 * 64 + l], v1 = in[1 * 64 + l];
    out[l] = reduce9t(side ? v1 : v0, side ? v0 : v1, in[2 * 64 + l], in[3 * 64 + l], in[4 * 64 + l], in[5 * 64 + l],
                      in[6 * 64 + l], in[8 * 64 + l], in[7 * 64 + l]);
    slots[l] = reduce9t_slot(l);
}
// four independent rows: in [9][64], out [64] (each lane's row total), slots [64]
__global__ void k_dbg_reduce9r16(const float* __restrict__ in, float* __restrict__ out, int* __restrict__ slots) {
    const int l = threadIdx.x;
    const bool side = (l & 8) != 0;
    const float v0 = in[0 * 64 + l], v1 = in[1 * 64 + l];
    out[l] = reduce9r16(side ? v1 : v0, side ? v0 : v1, in[2 * 64 + l], in[3 * 64 + l], in[4 * 64 + l], in[5 * 64 + l],
                        in[6 * 64 + l], in[8 * 64 + l], in[7 * 64 + l], l);
    slots[l] = reduce9r16_slot(l);
}
// reduce10r16: in [10][64] (value k of lane l at k*64+l), out [64], slots [64]
__global__ void k_dbg_reduce10r16(const float* __restrict__ in, float* __restrict__ out, int* __restrict__ slots) {
    const int l = threadIdx.x;
    const bool side = (l & 8) != 0;
    const float v0 = in[0 * 64 + l], v1 = in[1 * 64 + l];
    out[l] = reduce10r16(side ? v1 : v0, side ? v0 : v1, in[2 * 64 + l], in[3 * 64 + l], in[4 * 64 + l], in[5 * 64 + l],
                         in[6 * 64 + l], in[8 * 64 + l], in[7 * 64 + l], in[9 * 64 + l], l);
    slots[l] = reduce10r16_slot(l);
}
// reduce12ar16: in [12][64] (value k of lane l at k*64+l), out [64], slots [64] (with the depth slot 9), slots_nodepth [64]
__global__ void k_dbg_reduce12ar16(const float* __restrict__ in, float* __restrict__ out, int* __restrict__ slots,
                                   int* __restrict__ slots_nodepth) {
    const int l = threadIdx.x;
    const bool side = (l & 8) != 0;
    const float v0 = in[0 * 64 + l], v1 = in[1 * 64 + l];
    out[l] = reduce12ar16(side ? v1 : v0, side ? v0 : v1, in[2 * 64 + l], in[3 * 64 + l], in[4 * 64 + l], in[5 * 64 + l],
                          in[6 * 64 + l], in[8 * 64 + l], in[7 * 64 + l], in[9 * 64 + l], in[10 * 64 + l], in[11 * 64 + l],
                          l);
    slots[l] = reduce12ar16_slot(l, true);
    slots_nodepth[l] = reduce12ar16_slot(l, false);
}
__global__ void k_dbg_rcp(const float* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __builtin_amdgcn_rcpf(in[i]);
}
__global__ void k_dbg_blend_exp(const float* __restrict__ q, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = cugs_blend_exp_q(q[i]);
}
// cugsdbg_may_touch_quad: the blends' cull against their own per-pixel decisions, one case per thread.
// in: [n][8] floats {mean x, mean y, a, b, c, opacity, quad x, quad y} (quad x, y: the quad's integer pixel origin),
// masks [n] (the open pixels, lane = y*8 + x; non-zero).  The record is made by write_packed (tau = ln(255 o) included),
// staged by cugs_stage_cull for the 16-aligned tile that holds the quad's origin, and read back as the blends read it
// (an origin that is no multiple of 8 lets the quad reach up to 4 px past that tile: the limit's B is then that much
// short, against a slack 16 times what the roundings need).
// out: hit [n] (may_touch_quad against active_rect(mask)), pass [n] (bit l: lane l
// is open and pixel_alpha_raw + passes_alpha_min lets the Gaussian through there), rect [n][4] (active_rect, relative
// to the quad's first pixel centre).
__global__ void k_dbg_may_touch_quad(int n, const float* __restrict__ in, const unsigned long long* __restrict__ masks,
                                     int* __restrict__ hit, unsigned long long* __restrict__ pass,
                                     float* __restrict__ rect) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* c = in + (int64_t)i * 8;
    alignas(16) float rec[CUGS_PACKED_STRIDE];
    write_packed(rec, 0, c[0], c[1], Sym2{c[2], c[3], c[4]}, 0.0f, 0.0f, 0.0f, c[5]);
    const float4 r0 = reinterpret_cast<const float4*>(rec)[0];
    float4 r1 = reinterpret_cast<const float4*>(rec)[1];
    const int quad_x = (int)c[6], quad_y = (int)c[7];
    // staged as the blends stage it, for the 16-aligned tile of the quad's origin
    cugs_stage_cull(r0, r1, (float)((quad_x & ~(CUGS_TILE - 1)) + CUGS_TILE / 2), (float)((quad_y & ~(CUGS_TILE - 1)) + CUGS_TILE / 2));
    const float qx0 = (float)quad_x + 0.5f, qy0 = (float)quad_y + 0.5f;
    const unsigned long long active = masks[i];
    const ActiveRect ar = active_rect(active, qx0, qy0);
    hit[i] = may_touch_quad(r0, r1, ar.x0, ar.y0, ar.wx, ar.wy) ? 1 : 0;
    unsigned long long p = 0ull;
    for (int l = 0; l < 64; ++l) {
        const float pxf = (float)(quad_x + (l & 7)) + 0.5f, pyf = (float)(quad_y + (l >> 3)) + 0.5f;
        const float open = ((active >> l) & 1ull) ? 1.0f : 0.0f;
        PixelEval e;
        const float alpha = pixel_alpha_raw(pxf, pyf, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, open, e);
        if (passes_alpha_min(alpha) != 0.0f) p |= 1ull << l;
    }
    pass[i] = p;
    rect[(int64_t)i * 4 + 0] = ar.x0 - qx0; rect[(int64_t)i * 4 + 1] = ar.y0 - qy0;
    rect[(int64_t)i * 4 + 2] = ar.wx; rect[(int64_t)i * 4 + 3] = ar.wy;
}
bool g_dev_backward_stats = false;
}  // namespace
bool cugs_dev_backward_stats() { return g_dev_backward_stats; }
extern "C" int cugsdbg_backward_stats(int on) { g_dev_backward_stats = (on != 0); return 0; }
extern "C" int cugsdbg_reduce9(const float* in, float* out, int* slots, void* stream) {
    hipLaunchKernelGGL(k_dbg_reduce9, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), in, out, slots);
    CUGS_LAUNCH_CHECK();
    return 0;
}
extern "C" int cugsdbg_reduce9r16(const float* in, float* out, int* slots, void* stream) {
    hipLaunchKernelGGL(k_dbg_reduce9r16, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), in, out, slots);
    CUGS_LAUNCH_CHECK();
    return 0;
}
extern "C" int cugsdbg_reduce10r16(const float* in, float* out, int* slots, void* stream) {
    hipLaunchKernelGGL(k_dbg_reduce10r16, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), in, out, slots);
    CUGS_LAUNCH_CHECK();
    return 0;
}
extern "C" int cugsdbg_reduce12ar16(const float* in, float* out, int* slots, int* slots_nodepth, void* stream) {
    hipLaunchKernelGGL(k_dbg_reduce12ar16, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), in, out, slots,
                       slots_nodepth);
    CUGS_LAUNCH_CHECK();
    return 0;
}
extern "C" int cugsdbg_blend_exp_q(const float* q, float* out, int n, void* stream) {
    hipLaunchKernelGGL(k_dbg_blend_exp, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), q, out, n);
    CUGS_LAUNCH_CHECK();
    return 0;
}
extern "C" int cugsdbg_rcp(const float* in, float* out, int n, void* stream) {
    hipLaunchKernelGGL(k_dbg_rcp, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), in, out, n);
    CUGS_LAUNCH_CHECK();
    return 0;
}
extern "C" int cugsdbg_may_touch_quad(int n, const float* in, const unsigned long long* masks, int* hit,
                                      unsigned long long* pass, float* rect, void* stream) {
    if (n <= 0) return n == 0 ? 0 : CUGS_EINVAL;
    hipLaunchKernelGGL(k_dbg_may_touch_quad, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), n, in,
                       masks, hit, pass, rect);
    CUGS_LAUNCH_CHECK();
    return 0;
}
#endif
