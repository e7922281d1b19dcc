// normal_loss.hip — normal supervision from the rendered depth (not in the reference): the surface
// normal of the expected depth d = D / A of render()'s depth and alpha maps (back-projected through a pinhole camera,
// central differences, n = Py x Px: the 2DGS depth_to_normal, pointing at the camera), its cosine and/or L1 distance
// to a normal prior, and the analytic dL/dD and dL/dA for render_backward.
//
// Replaces, per iteration: where / div / the back-projection / four slices / cross / norm / where / div / the two
// distances and the autograd pass back through all of them in libtorch (a few dozen element-wise launches).
//
//   k_normal_loss      forward and backward in one launch.  A workgroup owns a TW x TH = 64 x 16 tile of pixels:
//                        1. d (and "depth-valid") for the tile and a halo of 2 -> LDS, one division per pixel;
//                        2. for the tile and a halo of 1: the normal, the loss term and dl/dPx, dl/dPy -> LDS (the
//                           normal map and the fp64 sums from the tile's own pixels only);
//                        3. each tile pixel GATHERS  gP = ((gPx(u-1,v) - gPx(u+1,v)) + gPy(u,v-1)) - gPy(u,v+1)  and
//                           writes dL/dD, dL/dA.
//                      A halo pixel is recomputed with the operations of its owner in the same order, so a pixel's
//                      result does not depend on where the tile edges fall.  One row {sum w l, sum of valid w, valid
//                      count} of fp64 partials per workgroup.
//   k_normal_finalize  one workgroup: the rows in the fixed order of depth_loss.hip -> loss_out[8].
// No atomics, no per-pixel scratch in global memory, no host sync, no allocation: the same bits from run to run.
//
// Every float step below is one correctly rounded operation (-ffp-contract=off, IEEE division and square root);
// tests/normal_loss_ref.py is its numpy mirror, op for op.  Traffic: 8 B read per pixel (+12 B prior, +4 B weight), 8 B
// written (+12 B normal map); the halo's reads hit the L2.
#include "cugs_common.h"
#include "cugs_row_sums.h"   // block_sums, reduce_rows

#include <math.h>

namespace {

// The tile: four pixels per thread, a row of 64 = two 128-byte lines.  What a tile costs beyond its own pixels is its
// halo: 68 x 20 / 1024 = 1.33 divisions for d and 66 x 18 / 1024 = 1.16 stencils per pixel, in five passes of the
// workgroup with 93 % of their lanes busy.  Measured against 32 x 8 (1.69 and 1.33; four times the rows of partials):
// 37.1 against 40.7 us at 1080p, the finalize kernel 4.6 against 8.9 us.
constexpr int TW = 64, TH = 16;
static_assert((TW * TH) % CUGS_BLOCK == 0, "whole passes of the workgroup over the tile");
constexpr int DW = TW + 4, DH = TH + 4;         // d with a halo of 2
constexpr int GW = TW + 2, GH = TH + 2;         // the stencil gradients with a halo of 1
constexpr int NSUM = 3;                         // sum w l, sum of valid w, count

struct NormalArgs {
    int width, height;
    float fx, fy, cx, cy, cos_weight, l1_weight, min_alpha, inv_n;
};

__device__ __forceinline__ float sign_of(float x) { return (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : 0.0f); }

template <bool HAS_W, bool HAS_T, bool WANT_N>
__global__ __launch_bounds__(CUGS_BLOCK) void k_normal_loss(NormalArgs g, int ntx, const float* __restrict__ D,
                                                            const float* __restrict__ A, const float* __restrict__ t,
                                                            const float* __restrict__ w, float* __restrict__ normals,
                                                            float* __restrict__ gD, float* __restrict__ gA,
                                                            double* __restrict__ partials) {
    __shared__ float s_d[DH][DW];               // expected depth, 0 where not depth-valid
    __shared__ unsigned char s_ok[DH][DW];      // depth-valid
    __shared__ float s_ax[DW], s_ay[DH];        // ((u + 0.5) - cx) / fx, ((v + 0.5) - cy) / fy
    __shared__ float s_g[6][GH][GW];            // dl/dPx (0..2), dl/dPy (3..5); 0 where not loss-valid
    __shared__ unsigned char s_lv[GH][GW];      // loss-valid
    const int tid = threadIdx.x;
    const int tile_y = (int)(blockIdx.x / (unsigned)ntx), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)ntx);
    const int u0 = tile_x * TW, v0 = tile_y * TH;
    const int W = g.width, H = g.height;
    const size_t plane = (size_t)W * (size_t)H;

    // 1. expected depth with a halo of 2; a pixel outside the image is not depth-valid
    for (int i = tid; i < DH * DW; i += CUGS_BLOCK) {
        const int ly = i / DW, lx = i - ly * DW;
        const int u = u0 - 2 + lx, v = v0 - 2 + ly;
        const bool in = u >= 0 && u < W && v >= 0 && v < H;
        const size_t p = in ? (size_t)v * W + u : 0;
        const float a = in ? A[p] : 0.0f, dd = in ? D[p] : 0.0f;
        const bool ok = a > g.min_alpha;
        s_d[ly][lx] = ok ? dd / (ok ? a : 1.0f) : 0.0f;
        s_ok[ly][lx] = ok;
    }
    static_assert(DW <= CUGS_BLOCK / 2 && DH <= CUGS_BLOCK / 2, "the columns in the first half of the workgroup, the rows in the second");
    if (tid < DW) s_ax[tid] = (((float)(u0 - 2 + tid) + 0.5f) - g.cx) / g.fx;
    else if (tid >= CUGS_BLOCK / 2 && tid < CUGS_BLOCK / 2 + DH)
        s_ay[tid - CUGS_BLOCK / 2] = (((float)(v0 - 2 + tid - CUGS_BLOCK / 2) + 0.5f) - g.cy) / g.fy;
    __syncthreads();

    // 2. normal, loss term and the gradients to the two differences, for the tile and a halo of 1
    double acc[NSUM] = {0.0, 0.0, 0.0};
    for (int i = tid; i < GH * GW; i += CUGS_BLOCK) {
        const int gy = i / GW, gx = i - gy * GW;
        const int u = u0 - 1 + gx, v = v0 - 1 + gy;
        const int lx = gx + 1, ly = gy + 1;
        const bool interior = u >= 1 && u <= W - 2 && v >= 1 && v <= H - 2;
        const bool ok5 = interior && s_ok[ly][lx] && s_ok[ly][lx - 1] && s_ok[ly][lx + 1] && s_ok[ly - 1][lx] && s_ok[ly + 1][lx];
        const float dl = s_d[ly][lx - 1], dr = s_d[ly][lx + 1], du = s_d[ly - 1][lx], dn = s_d[ly + 1][lx];
        const float axc = s_ax[lx], ayc = s_ay[ly];
        // P = (ax d, ay d, d);  Px = P(u+1, v) - P(u-1, v),  Py = P(u, v+1) - P(u, v-1)
        const float Px0 = s_ax[lx + 1] * dr - s_ax[lx - 1] * dl, Px1 = ayc * dr - ayc * dl, Px2 = dr - dl;
        const float Py0 = axc * dn - axc * du, Py1 = s_ay[ly + 1] * dn - s_ay[ly - 1] * du, Py2 = dn - du;
        // n = Py x Px
        const float n0 = Py1 * Px2 - Py2 * Px1, n1 = Py2 * Px0 - Py0 * Px2, n2 = Py0 * Px1 - Py1 * Px0;
        const float nn = (n0 * n0 + n1 * n1) + n2 * n2;
        const bool nvalid = ok5 && nn > 0.0f && nn < INFINITY;
        const float rl = 1.0f / sqrtf(nvalid ? nn : 1.0f);
        const float h0 = nvalid ? n0 * rl : 0.0f, h1 = nvalid ? n1 * rl : 0.0f, h2 = nvalid ? n2 * rl : 0.0f;
        const bool in_tile = gx >= 1 && gx <= TW && gy >= 1 && gy <= TH && u < W && v < H;
        const size_t p = (size_t)(in_tile || interior ? v : 0) * W + (in_tile || interior ? u : 0);
        if constexpr (WANT_N) {
            if (in_tile) { normals[p] = h0; normals[plane + p] = h1; normals[2 * plane + p] = h2; }
        }
        if constexpr (HAS_T) {
            const float t0 = interior ? t[p] : 0.0f, t1 = interior ? t[plane + p] : 0.0f, t2 = interior ? t[2 * plane + p] : 0.0f;
            float wv = 1.0f;
            if constexpr (HAS_W) wv = interior ? w[p] : 0.0f;
            const float tt = (t0 * t0 + t1 * t1) + t2 * t2;
            const bool lvalid = nvalid && wv > 0.0f && tt > 0.0f && tt < INFINITY;
            const float rt = 1.0f / sqrtf(lvalid ? tt : 1.0f);
            const float q0 = t0 * rt, q1 = t1 * rt, q2 = t2 * rt;                 // the unit prior
            const float dot = (h0 * q0 + h1 * q1) + h2 * q2;
            const float e0 = h0 - q0, e1 = h1 - q1, e2 = h2 - q2;
            const float l1 = (fabsf(e0) + fabsf(e1)) + fabsf(e2);
            const float term = wv * (g.cos_weight * (1.0f - dot) + g.l1_weight * l1);
            if (in_tile && lvalid) { acc[0] += (double)term; acc[1] += (double)wv; acc[2] += 1.0; }
            // dl/dn^ = (w / (H W)) (l1_weight sgn(n^ - t^) - cos_weight t^)
            const float wn = wv * g.inv_n;
            const float b0 = wn * (g.l1_weight * sign_of(e0) - g.cos_weight * q0);
            const float b1 = wn * (g.l1_weight * sign_of(e1) - g.cos_weight * q1);
            const float b2 = wn * (g.l1_weight * sign_of(e2) - g.cos_weight * q2);
            // dl/dn = (dl/dn^ - n^ (n^ . dl/dn^)) / |n|
            const float s = (h0 * b0 + h1 * b1) + h2 * b2;
            const float c0 = (b0 - h0 * s) * rl, c1 = (b1 - h1 * s) * rl, c2 = (b2 - h2 * s) * rl;
            // n = Py x Px:  dl/dPx = dl/dn x Py,  dl/dPy = Px x dl/dn
            s_g[0][gy][gx] = lvalid ? c1 * Py2 - c2 * Py1 : 0.0f;
            s_g[1][gy][gx] = lvalid ? c2 * Py0 - c0 * Py2 : 0.0f;
            s_g[2][gy][gx] = lvalid ? c0 * Py1 - c1 * Py0 : 0.0f;
            s_g[3][gy][gx] = lvalid ? Px1 * c2 - Px2 * c1 : 0.0f;
            s_g[4][gy][gx] = lvalid ? Px2 * c0 - Px0 * c2 : 0.0f;
            s_g[5][gy][gx] = lvalid ? Px0 * c1 - Px1 * c0 : 0.0f;
            s_lv[gy][gx] = lvalid;
        }
    }
    if constexpr (HAS_T) {
        __syncthreads();

        // 3. gather: P(u, v) is the +1 end of Px(u-1, v) and Py(u, v-1), the -1 end of Px(u+1, v) and Py(u, v+1)
        if (gD || gA) {
            for (int i = tid; i < TW * TH; i += CUGS_BLOCK) {
                const int ty = i / TW, tx = i - ty * TW;
                const int u = u0 + tx, v = v0 + ty;
                if (u >= W || v >= H) continue;
                const int gx = tx + 1, gy = ty + 1;
                const bool any = s_lv[gy][gx - 1] || s_lv[gy][gx + 1] || s_lv[gy - 1][gx] || s_lv[gy + 1][gx];
                float gP[3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    gP[k] = ((s_g[k][gy][gx - 1] - s_g[k][gy][gx + 1]) + s_g[3 + k][gy - 1][gx]) - s_g[3 + k][gy + 1][gx];
                const float gd = (gP[0] * s_ax[tx + 2] + gP[1] * s_ay[ty + 2]) + gP[2];      // dP/dd = (ax, ay, 1)
                const size_t p = (size_t)v * W + u;
                const float a = any ? A[p] : 1.0f;          // any: the pixel is depth-valid, A > min_alpha > 0
                const float d = s_d[ty + 2][tx + 2];
                if (gD) gD[p] = any ? gd / a : 0.0f;
                if (gA) gA[p] = any ? -((gd * d) / a) : 0.0f;
            }
        }
        block_sums<NSUM>(acc, partials + (size_t)NSUM * blockIdx.x);
    }
}

// out = {loss, sum of valid w, valid count, 0, 0, 0, 0, 0}; the mean is over all H W pixels whatever the mask.
__global__ __launch_bounds__(CUGS_BLOCK) void k_normal_finalize(const double* __restrict__ partials, int nblk, double count,
                                                                 float* __restrict__ out) {
    __shared__ double s_acc[NSUM][CUGS_BLOCK];
    reduce_rows<NSUM>(partials, nblk, s_acc);
    if (threadIdx.x == 0) {
        out[0] = (float)(s_acc[0][0] / count);
        out[1] = (float)s_acc[1][0];
        out[2] = (float)s_acc[2][0];
#pragma unroll
        for (int k = 3; k < 8; ++k) out[k] = 0.0f;
    }
}

size_t round256(size_t b) { return (b + 255) / 256 * 256; }
size_t tiles_x(int width) { return ((size_t)width + TW - 1) / TW; }
size_t tiles_y(int height) { return ((size_t)height + TH - 1) / TH; }

bool finite_nonneg(float x) { return x >= 0.0f && x < INFINITY; }
bool finite(float x) { return x > -INFINITY && x < INFINITY; }

}  // namespace

// One row of three fp64 partials per tile.
extern "C" size_t cugs_normal_loss_workspace_bytes(int width, int height) {
    if (width < 0 || height < 0) return 0;
    return round256(sizeof(double) * NSUM * tiles_x(width) * tiles_y(height));
}

extern "C" int cugs_normal_loss(int width, int height, float fx, float fy, float cx, float cy, const float* depth_map,
                                const float* alpha, const float* target, const cugs_normal_loss_opts* opts, void* workspace,
                                size_t workspace_bytes, float* loss_out, float* dL_ddepth_map, float* dL_dalpha, void* stream) {
    if (width <= 0 || height <= 0 || !depth_map || !alpha || !opts || !workspace || !loss_out) return CUGS_EINVAL;
    if (!(opts->min_alpha > 0.0f && opts->min_alpha < INFINITY)) return CUGS_EINVAL;
    if (!(fx > 0.0f && fx < INFINITY && fy > 0.0f && fy < INFINITY && finite(cx) && finite(cy))) return CUGS_EINVAL;
    if (!finite_nonneg(opts->cos_weight) || !finite_nonneg(opts->l1_weight)) return CUGS_EINVAL;
    if (target && !(opts->cos_weight > 0.0f || opts->l1_weight > 0.0f)) return CUGS_EINVAL;
    // without a prior there is only the normal map to write
    if (!target && (!opts->normals_out || opts->weight || dL_ddepth_map || dL_dalpha)) return CUGS_EINVAL;
    if (workspace_bytes < cugs_normal_loss_workspace_bytes(width, height)) return CUGS_EWORKSPACE;
    const int64_t n = (int64_t)width * height;
    if (n > 2147483647ll) return CUGS_EOVERFLOW;
    const size_t ntx = tiles_x(width), ntiles = ntx * tiles_y(height);          // <= 2^31 - 1 too
    NormalArgs g;
    g.width = width; g.height = height;
    g.fx = fx; g.fy = fy; g.cx = cx; g.cy = cy;
    g.cos_weight = opts->cos_weight; g.l1_weight = opts->l1_weight; g.min_alpha = opts->min_alpha;
    g.inv_n = 1.0f / (float)n;
    double* const rows = static_cast<double*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)ntiles), block(CUGS_BLOCK);
#define CUGS_NORMAL_LOSS(HW, HT, WN) \
    hipLaunchKernelGGL((k_normal_loss<HW, HT, WN>), grid, block, 0, st, g, (int)ntx, depth_map, alpha, target, opts->weight, \
                       opts->normals_out, dL_ddepth_map, dL_dalpha, rows)
    const bool has_w = opts->weight != nullptr, want_n = opts->normals_out != nullptr;
    if (!target) CUGS_NORMAL_LOSS(false, false, true);
    else if (has_w) { if (want_n) CUGS_NORMAL_LOSS(true, true, true); else CUGS_NORMAL_LOSS(true, true, false); }
    else { if (want_n) CUGS_NORMAL_LOSS(false, true, true); else CUGS_NORMAL_LOSS(false, true, false); }
#undef CUGS_NORMAL_LOSS
    CUGS_LAUNCH_CHECK();
    // no prior: no rows were written, the three sums are 0
    hipLaunchKernelGGL(k_normal_finalize, dim3(1), block, 0, st, rows, target ? (int)ntiles : 0, (double)n, loss_out);
    CUGS_LAUNCH_CHECK();
    return 0;
}
