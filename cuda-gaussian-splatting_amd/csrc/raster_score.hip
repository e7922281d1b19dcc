// raster_score.hip — per-Gaussian contribution scores from the forward blend's walk.
//
// For every Gaussian, three statistics of its blend weight w = alpha * T over the pixels of one view: the SUM of w
// (Mini-Splatting's importance), the MAXIMUM of w (RadSplat's pruning rule) and the NUMBER of pixels it contributes to
// (LightGaussian's hit count).  The kernel is the forward blend without its colour: the same geometry
// (cugs_raster_common.h: one workgroup per tile, four waves on 8x8 quads, 256-record LDS batches, may_touch_quad against
// the active rectangle, hit groups of CUGS_HIT_GROUP, optional tile order, per-wave and whole-tile early exit) and the
// same per-pixel decisions through pixel_alpha_raw / passes_alpha_min: power > 0 skipped, alpha = min(0.99, o e^power)
// skipped below 1/255, T *= 1 - alpha, the pixel closes at T < 1/255.  w = al * T is the forward's product, bit for bit.
// It reads the geometry half of a record only (32 B of the 48) and writes no image.
//
// Scatter: a hit group's four steps are reduced together (reduce4_sum_max: four sums and four maxima in 18 cross-lane
// instructions), then one lane per step adds {sum, max, count} to row g of the score table [n,4] of 32-bit words:
//   word 0  sum of w, float        atomicAdd (float), as raster_backward.hip does for its rows
//   word 1  max of w, float bits   atomicMax on the word as unsigned: w >= 0, so the bit order is the value order and a
//                                  zeroed table is the identity
//   word 2  pixel count, uint32    atomicAdd (unsigned); wraps at 2^32
//   word 3  padding, never written: a row is one 16-byte piece of one cache line
// Steps in which no lane passes (a wave-uniform test on the ballot) send nothing.  The table is accumulated into, never
// cleared here: V views are V launches into one table.  Maximum and count do not depend on the order of the atomics;
// the sum does, in its last bits (each wave's partial sum is a fixed tree and so the same from run to run).
#include "cugs_score_walk.h"     // stage_geometry, swap_halves, swap_rows, dpp_mov_i: shared with raster_lift.hip

namespace {

// Wave totals of FOUR per-lane weights at once: their sums and their maxima.  A transpose-reduce as reduce9t's
// (cugs_raster_common.h), with the two row stages FIRST: while there are still partner values to trade, a permlane swap
// needs no selection - swap_halves(w0, w1) leaves w0's two halves side by side in one register and w1's in the other, so
// ONE add (and ONE max of the same swapped registers) folds two values into a register whose lower half belongs to w0
// and whose upper half to w1; swap_rows does the same between the pairs.  After the two stages one register holds, per
// 16-lane row, partial sums of one value - rows 0..3: w0, w2, w1, w3 - and four plain DPP steps finish each row.
// 4 swaps + 6 + 8 = 18 instructions for eight reductions (eight butterflies: 48; folding inside the rows with bank
// masks first leaves the row stages without a partner and costs a copy per swap: 28).
// Every lane of row r returns the totals of weight {0, 2, 1, 3}[r].  The maxima are taken on the bit patterns as SIGNED
// integers: for w >= +0 that is the float order, and a -0.0 (a skipped lane's al = alpha * 0 with the negative alpha of
// the power > 0 gate) is INT_MIN and never wins against a lane that passed.  All 64 lanes must be active.
__device__ __forceinline__ void reduce4_sum_max(float w0, float w1, float w2, float w3, float& sum, int& mx) {
    swap_halves(w0, w1);
    swap_halves(w2, w3);
    float p = w0 + w1, q = w2 + w3;
    int mp = max(__float_as_int(w0), __float_as_int(w1)), mq = max(__float_as_int(w2), __float_as_int(w3));
    swap_rows(p, q);
    swap_rows(mp, mq);
    float s = p + q;
    int m = max(mp, mq);
    s += dpp_mov<0x140>(s); m = max(m, dpp_mov_i<0x140>(m));               // row_mirror
    s += dpp_mov<0x141>(s); m = max(m, dpp_mov_i<0x141>(m));               // row_half_mirror
    s += dpp_mov<0xB1>(s);  m = max(m, dpp_mov_i<0xB1>(m));                // quad_perm [1,0,3,2]
    s += dpp_mov<0x4E>(s);  m = max(m, dpp_mov_i<0x4E>(m));                // quad_perm [2,3,0,1]
    sum = s; mx = m;
}

template <bool PACKED>
__global__ __launch_bounds__(CUGS_BLOCK) void k_blend_scores(RasterGeom geo, RasterSrc src, unsigned* __restrict__ scores) {
    __shared__ float4 s_rec[CUGS_BLOCK * CUGS_SCORE_REC_F4];
    __shared__ int s_wave_done[4];

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

    float T = inside ? 1.0f : 0.0f;                     // outside the image: closed from the start, as in the forward
    float open = inside ? 1.0f : 0.0f;                  // 1 while the pixel still blends, 0 once T < 1/255
    bool wave_done = (__ballot(open != 0.0f) == 0ull);
    const int row = lane >> 4;                          // reduce4_sum_max: row r delivers step {0, 2, 1, 3}[r]
    const bool deliver = (lane & 15) == 0;

    // one (wave, Gaussian) step of the forward blend without its colour: this lane's weight, the number of lanes that
    // passed (wave-uniform) and the Gaussian's index (word 7 of the LDS record: wave-uniform)
    auto step = [&](const float4* rp, float& weight, unsigned& passed, int& g) __attribute__((always_inline)) {
        const float4 g0 = rp[0], g1 = rp[1];
        PixelEval e;
        const float alpha = pixel_alpha_raw(pxf, pyf, g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, open, e);
        const float passf = passes_alpha_min(alpha);           // alpha >= 1/255
        const float al = alpha * passf;
        weight = al * T;                                        // the forward's product: exactly 0 where skipped or closed
        T *= (1.0f - al);
        open = passes_alpha_min(T);                             // the forward's flag chain: T never increases
        passed = (unsigned)__popcll(__ballot(passf != 0.0f));
        g = __float_as_int(g1.w);
    };
    // the scatter of up to four steps (a missing step: weight 0, passed 0)
    auto scatter = [&](float w0, float w1, float w2, float w3, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                       int g0, int g1, int g2, int g3) __attribute__((always_inline)) {
        if ((c0 | c1 | c2 | c3) == 0u) return;                  // wave-uniform: no lane passed in any of them
        float sum;
        int mx;
        reduce4_sum_max(w0, w1, w2, w3, sum, mx);
        const unsigned c = row == 0 ? c0 : row == 1 ? c2 : row == 2 ? c1 : c3;
        const int g = row == 0 ? g0 : row == 1 ? g2 : row == 2 ? g1 : g3;
        if (deliver && c != 0u) {                               // c != 0: a lane passed, so sum > 0 and mx is its bits
            unsigned* r = scores + (int64_t)g * 4;
            atomicAdd(reinterpret_cast<float*>(r), sum);
            atomicMax(r + 1, (unsigned)mx);
            atomicAdd(r + 2, c);
        }
    };

    for (int batch = 0; batch < num_batches; ++batch) {
        if (lane == 0) s_wave_done[wave] = wave_done ? 1 : 0;
        __syncthreads();
        if (s_wave_done[0] & s_wave_done[1] & s_wave_done[2] & s_wave_done[3]) break;

        stage_geometry<PACKED>(src, range_start + batch * CUGS_BLOCK + tid, range_end, s_rec, tile_cx, tile_cy);
        __syncthreads();

        if (!wave_done) {
            const int batch_count = min(CUGS_BLOCK, num_in_range - batch * CUGS_BLOCK);
            for (int sub = 0; sub * CUGS_WAVE < batch_count && !wave_done; ++sub) {
                const int j = sub * CUGS_WAVE + lane;
                const ActiveRect ar = active_rect(__ballot(open != 0.0f), qx0, qy0);   // !wave_done => non-empty
                bool hit = false;
                if (j < batch_count)
                    hit = may_touch_quad(s_rec[j * CUGS_SCORE_REC_F4 + 0], s_rec[j * CUGS_SCORE_REC_F4 + 1], ar.x0, ar.y0,
                                         ar.wx, ar.wy);
                unsigned long long mask = __ballot(hit);
                const float4* sub_rec = s_rec + sub * CUGS_WAVE * CUGS_SCORE_REC_F4;
                float w0, w1, w2, w3;
                unsigned c0, c1, c2, c3;
                int g0, g1, g2, g3;
                // whole groups, front to back, as the forward takes them: four steps, one scatter, one vote
                while (__popcll(mask) >= CUGS_HIT_GROUP) {
                    const float4* r0 = sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4;
                    const float4* r1 = sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4;
                    const float4* r2 = sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4;
                    const float4* r3 = sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4;
                    step(r0, w0, c0, g0); step(r1, w1, c1, g1); step(r2, w2, c2, g2); step(r3, w3, c3, g3);
                    scatter(w0, w1, w2, w3, c0, c1, c2, c3, g0, g1, g2, g3);
                    if (__ballot(open != 0.0f) == 0ull) { wave_done = true; mask = 0ull; break; }
                }
                if (mask != 0ull) {                                         // the sub-batch's last one to three hits
                    w1 = w2 = 0.0f; c1 = c2 = 0u; g1 = g2 = 0;
                    step(sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4, w0, c0, g0);
                    if (mask != 0ull) step(sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4, w1, c1, g1);
                    if (mask != 0ull) step(sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4, w2, c2, g2);
                    scatter(w0, w1, w2, 0.0f, c0, c1, c2, 0u, g0, g1, g2, 0);
                    if (__ballot(open != 0.0f) == 0ull) wave_done = true;
                }
            }
        }
    }
}

}  // namespace

extern "C" int cugs_blend_scores(int width, int height, const int32_t* tile_ranges, const int32_t* gaussian_indices,
                                 const float* means_2d, const float* cov_2d_inv, const float* opacities_act,
                                 const float* packed, const void* tile_order, int n, void* scores, void* stream) {
    if (width < 0 || height < 0 || n < 0) return CUGS_EINVAL;
    if (n > 0 && !scores) return CUGS_EINVAL;
    // gaussian_indices and the per-Gaussian sources may be NULL for an empty pair list (every tile range is {0,0} and
    // nothing is dereferenced).  With indices present a source is required.
    if (gaussian_indices && !packed && (!means_2d || !cov_2d_inv || !opacities_act)) return CUGS_EINVAL;
    if (packed && !cugs_aligned16(packed)) return CUGS_EALIGN;
    if (tile_order && !cugs_aligned16(tile_order)) return CUGS_EALIGN;
    if (scores && !cugs_aligned16(scores)) return CUGS_EALIGN;
    const int ntx = (width + CUGS_TILE - 1) / CUGS_TILE, nty = (height + CUGS_TILE - 1) / CUGS_TILE;
    if (n == 0 || ntx == 0 || nty == 0) return 0;                // nothing can contribute: the table stays as it is
    if (!tile_ranges) return CUGS_EINVAL;
    if ((int64_t)ntx * nty > 2147483647ll) return CUGS_EOVERFLOW;
    RasterGeom geo{width, height, ntx, ntx * nty, 0.0f, 0.0f, 0.0f};
    RasterSrc src{tile_ranges, gaussian_indices, packed, means_2d, cov_2d_inv, nullptr, opacities_act,
                  reinterpret_cast<const uint4*>(tile_order)};
    cugs_with_bool(packed != nullptr, [&](auto P) {
        hipLaunchKernelGGL((k_blend_scores<P()>), dim3(geo.ntiles), dim3(CUGS_BLOCK), 0, static_cast<hipStream_t>(stream),
                           geo, src, static_cast<unsigned*>(scores));
    });
    CUGS_LAUNCH_CHECK();
    return 0;
}
