// raster_lift.hip — pixel maps lifted onto Gaussians by the forward blend's walk.
//
// For every Gaussian g and channel c, S[g,c] = sum over the pixels p of w_g(p) * M_c(p), where w = alpha * T is the
// forward's blend weight and M a per-pixel map with C = 1..4 channels: a float map [H,W,C] (an error image, a residual,
// a mask), or, in LABELS mode, the C indicator maps [label(p) == label_base + c] of an int32 label image [H,W].
// The kernel is k_blend_scores (raster_score.hip) with a weighted scatter: the same geometry (one workgroup per tile,
// four waves on 8x8 quads, 256-record LDS batches of the two geometry chunks, cugs_stage_cull / may_touch_quad against
// the active rectangle, hit groups of CUGS_HIT_GROUP, optional tile order, per-wave and whole-tile early exit) and the
// same per-pixel decisions through pixel_alpha_raw / passes_alpha_min, so w = al * T is the forward's product, bit for
// bit.  The forward and backward blend kernels are not involved.
//
// Map read: before the walk every lane reads its pixel's C values once, with plain dword loads (no alignment of the map
// is required); a lane outside the image loads nothing and holds zeros.
// Term: t_c = (w > 0) ? w * m_c : 0 - one fp32 multiply behind a select.  The select makes a skipped or closed lane
// contribute exactly 0 whatever its map value: a NaN or Inf at a pixel reaches only the Gaussians that blend onto it.
// Reduction: the 4 C terms of a hit group are summed across the wave by a fixed tree (reduce_lift below), so a wave's
// partial sums are the same from run to run; a ragged last group pads with zero terms.
// Delivery: lanes 0..C-1 of 16-lane row r hold the C channel sums of step {0, 2, 1, 3}[r], and ONE float atomicAdd
// instruction per hit group adds them to words 0..C-1 of row g of the table [n,4], for each step in which a lane
// passed (4 C active lanes at most; the C words of a row are one request of adjacent lanes, the backward blend's row
// shape).  Groups in which no lane passed send nothing (a wave-uniform test).  Words C..3 of a row are never written.
// The table is accumulated into and never cleared here; the last bits of a sum depend on the order of the atomics.
#include "cugs_score_walk.h"

namespace {

// Wave totals of the 4 C terms t[step][channel] of a hit group.  Per channel, the two row stages of reduce4_sum_max
// (raster_score.hip) come first - swap_halves, add, swap_rows, add: no selection while there are partner values to
// trade - and leave one register whose 16-lane rows 0..3 hold partial sums of steps 0, 2, 1, 3; row_mirror and
// row_half_mirror fold lanes 8 and 4 apart.  The two quad stages then transpose the C channel registers over lane bits
// 1 and 0 (xchg_add: the side keeps one register and receives the partner's copy of it), so that lane l of every quad
// ends with channel l:
//   C = 4   bit 1: (ch0 | ch2), (ch1 | ch3)    bit 0: (those two)     lanes 0..3 = ch 0, 1, 2, 3
//   C = 3   bit 1: (ch0 | ch2), ch1 plain      bit 0: (those two)     lanes 0..3 = ch 0, 1, 2, 1
//   C = 2   bit 1: both plain                  bit 0: (ch0 | ch1)     lanes 0..3 = ch 0, 1, 0, 1
//   C = 1   both plain                                                 every lane = ch 0
// Swaps: 3 C; adds: 3 C plain + 2 C DPP + the quad stages.  t[s][c] of different (s, c) never meet in an addition.
// All 64 lanes must be active.
template <int C>
__device__ __forceinline__ float reduce_lift(float (&t)[4][C], int lane) {
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        swap_halves(t[0][c], t[1][c]);
        swap_halves(t[2][c], t[3][c]);
        float p = t[0][c] + t[1][c], q = t[2][c] + t[3][c];
        swap_rows(p, q);
        float s = p + q;
        s += dpp_mov<0x140>(s);                                     // row_mirror
        s += dpp_mov<0x141>(s);                                     // row_half_mirror
        v[c] = s;
    }
    const bool s1 = (lane & 2) != 0, s0 = (lane & 1) != 0;
    if constexpr (C == 1) {
        float s = v[0];
        s += dpp_mov<0x4E>(s);                                      // quad_perm [2,3,0,1]
        s += dpp_mov<0xB1>(s);                                      // quad_perm [1,0,3,2]
        return s;
    } else if constexpr (C == 2) {
        const float a = v[0] + dpp_mov<0x4E>(v[0]), b = v[1] + dpp_mov<0x4E>(v[1]);
        return xchg_add<0xB1>(s0, a, b);
    } else if constexpr (C == 3) {
        const float a = xchg_add<0x4E>(s1, v[0], v[2]);
        const float b = v[1] + dpp_mov<0x4E>(v[1]);
        return xchg_add<0xB1>(s0, a, b);
    } else {
        const float a = xchg_add<0x4E>(s1, v[0], v[2]);
        const float b = xchg_add<0x4E>(s1, v[1], v[3]);
        return xchg_add<0xB1>(s0, a, b);
    }
}

template <bool PACKED, int C, bool LABELS>
__global__ __launch_bounds__(CUGS_BLOCK) void k_blend_lift(RasterGeom geo, RasterSrc src, const float* __restrict__ maps,
                                                           const int32_t* __restrict__ labels, int label_base,
                                                           float* __restrict__ table) {
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

    // this pixel's map values, read once; outside the image nothing is loaded
    float m[C];
#pragma unroll
    for (int c = 0; c < C; ++c) m[c] = 0.0f;
    if (inside) {
        const int64_t pix = (int64_t)py * geo.width + px;
        if (LABELS) {
            // a label outside the window, negatives included, matches no channel (unsigned: the difference cannot overflow)
            const unsigned rel = (unsigned)labels[pix] - (unsigned)label_base;
#pragma unroll
            for (int c = 0; c < C; ++c) m[c] = (rel == (unsigned)c) ? 1.0f : 0.0f;
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) m[c] = maps[pix * C + c];
        }
    }

    float T = inside ? 1.0f : 0.0f;                     // outside the image: closed from the start, as in the forward
    float open = inside ? 1.0f : 0.0f;                  // 1 while the pixel still blends, 0 once T < 1/255
    bool wave_done = (__ballot(open != 0.0f) == 0ull);
    const int row = lane >> 4;                          // reduce_lift: row r delivers step {0, 2, 1, 3}[r]
    const int word = lane & 15;                         // and its lane `word` < C the sum of channel `word`
    const bool deliver = word < C;

    // one (wave, Gaussian) step of the forward blend without its colour: this lane's C terms, the number of lanes that
    // passed (wave-uniform) and the Gaussian's index (word 7 of the LDS record: wave-uniform)
    auto step = [&](const float4* rp, float (&t)[C], unsigned& passed, int& g) __attribute__((always_inline)) {
        const float4 g0 = rp[0], g1 = rp[1];
        PixelEval e;
        const float alpha = pixel_alpha_raw(pxf, pyf, g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, open, e);
        const float passf = passes_alpha_min(alpha);           // alpha >= 1/255
        const float al = alpha * passf;
        const float weight = al * T;                            // the forward's product: exactly 0 where skipped or closed
        T *= (1.0f - al);
        open = passes_alpha_min(T);                             // the forward's flag chain: T never increases
        passed = (unsigned)__popcll(__ballot(passf != 0.0f));
        g = __float_as_int(g1.w);
        const bool on = weight > 0.0f;                          // false for +0, -0 and NaN
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] = on ? weight * m[c] : 0.0f;
    };
    // the scatter of up to four steps (a missing step: terms 0, passed 0)
    auto scatter = [&](float (&t)[4][C], unsigned c0, unsigned c1, unsigned c2, unsigned c3, int g0, int g1, int g2,
                       int g3) __attribute__((always_inline)) {
        if ((c0 | c1 | c2 | c3) == 0u) return;                  // wave-uniform: no lane passed in any of them
        const float sum = reduce_lift<C>(t, lane);
        const unsigned c = row == 0 ? c0 : row == 1 ? c2 : row == 2 ? c1 : c3;
        const int g = row == 0 ? g0 : row == 1 ? g2 : row == 2 ? g1 : g3;
        if (deliver && c != 0u) atomicAdd(table + (int64_t)g * 4 + word, sum);     // the group's one atomic
    };
    auto clear = [&](float (&t)[C]) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] = 0.0f;
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
                float t[4][C];
                unsigned c0, c1, c2, c3;
                int g0, g1, g2, g3;
                // whole groups, front to back, as the forward takes them: four steps, one scatter, one vote
                while (__popcll(mask) >= CUGS_HIT_GROUP) {
                    const float4* r0 = sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4;
                    const float4* r1 = sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4;
                    const float4* r2 = sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4;
                    const float4* r3 = sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4;
                    step(r0, t[0], c0, g0); step(r1, t[1], c1, g1); step(r2, t[2], c2, g2); step(r3, t[3], c3, g3);
                    scatter(t, c0, c1, c2, c3, g0, g1, g2, g3);
                    if (__ballot(open != 0.0f) == 0ull) { wave_done = true; mask = 0ull; break; }
                }
                if (mask != 0ull) {                                         // the sub-batch's last one to three hits
                    clear(t[1]); clear(t[2]); clear(t[3]);
                    c1 = c2 = 0u; g1 = g2 = 0;
                    step(sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4, t[0], c0, g0);
                    if (mask != 0ull) step(sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4, t[1], c1, g1);
                    if (mask != 0ull) step(sub_rec + cugs_pop_hit_asc(mask) * CUGS_SCORE_REC_F4, t[2], c2, g2);
                    scatter(t, c0, c1, c2, 0u, g0, g1, g2, 0);
                    if (__ballot(open != 0.0f) == 0ull) wave_done = true;
                }
            }
        }
    }
}

template <bool PACKED, bool LABELS>
void launch_lift(int channels, const RasterGeom& geo, const RasterSrc& src, const float* maps, const int32_t* labels,
                 int label_base, float* table, hipStream_t stream) {
    const dim3 grid(geo.ntiles), block(CUGS_BLOCK);
    switch (channels) {
    case 1: hipLaunchKernelGGL((k_blend_lift<PACKED, 1, LABELS>), grid, block, 0, stream, geo, src, maps, labels, label_base, table); break;
    case 2: hipLaunchKernelGGL((k_blend_lift<PACKED, 2, LABELS>), grid, block, 0, stream, geo, src, maps, labels, label_base, table); break;
    case 3: hipLaunchKernelGGL((k_blend_lift<PACKED, 3, LABELS>), grid, block, 0, stream, geo, src, maps, labels, label_base, table); break;
    default: hipLaunchKernelGGL((k_blend_lift<PACKED, 4, LABELS>), grid, block, 0, stream, geo, src, maps, labels, label_base, table); break;
    }
}

}  // namespace

extern "C" int cugs_blend_lift(int width, int height, const int32_t* tile_ranges, const int32_t* gaussian_indices,
                               const float* means_2d, const float* cov_2d_inv, const float* opacities_act,
                               const float* packed, const void* tile_order, int n, const float* maps,
                               const int32_t* labels, int channels, int label_base, void* table, void* stream) {
    if (width < 0 || height < 0 || n < 0) return CUGS_EINVAL;
    if (channels < 1 || channels > 4) return CUGS_EINVAL;
    const int ntx = (width + CUGS_TILE - 1) / CUGS_TILE, nty = (height + CUGS_TILE - 1) / CUGS_TILE;
    const bool launches = n > 0 && ntx > 0 && nty > 0;
    if (launches && ((maps != nullptr) == (labels != nullptr))) return CUGS_EINVAL;   // exactly one of the two
    if (n > 0 && !table) return CUGS_EINVAL;
    // gaussian_indices and the per-Gaussian sources may be NULL for an empty pair list (every tile range is {0,0} and
    // nothing is dereferenced).  With indices present a source is required.
    if (gaussian_indices && !packed && (!means_2d || !cov_2d_inv || !opacities_act)) return CUGS_EINVAL;
    if (launches && !tile_ranges) return CUGS_EINVAL;
    if (packed && !cugs_aligned16(packed)) return CUGS_EALIGN;
    if (tile_order && !cugs_aligned16(tile_order)) return CUGS_EALIGN;
    if (table && !cugs_aligned16(table)) return CUGS_EALIGN;
    if (!launches) return 0;                                     // nothing can contribute: the table stays as it is
    if ((int64_t)ntx * nty > 2147483647ll) return CUGS_EOVERFLOW;
    RasterGeom geo{width, height, ntx, ntx * nty, 0.0f, 0.0f, 0.0f};
    RasterSrc src{tile_ranges, gaussian_indices, packed, means_2d, cov_2d_inv, nullptr, opacities_act,
                  reinterpret_cast<const uint4*>(tile_order)};
    const hipStream_t st = static_cast<hipStream_t>(stream);
    float* tab = static_cast<float*>(table);
    cugs_with_bool(packed != nullptr, [&](auto P) {
        cugs_with_bool(labels != nullptr, [&](auto L) {
            launch_lift<P(), L()>(channels, geo, src, maps, labels, label_base, tab, st);
        });
    });
    CUGS_LAUNCH_CHECK();
    return 0;
}
