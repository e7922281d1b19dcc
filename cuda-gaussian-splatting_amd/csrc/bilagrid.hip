// bilagrid.hip — per-view bilateral-grid colour correction (not in the reference): a 3-D lattice
// G [12, L, GY, GX] of 3x4 affine colour transforms [A | b] (coefficient k = 4 i + j), indexed by pixel position and
// luminance, sliced per pixel with trilinear weights; its backward (image gradient WITH the term through the luminance
// guidance, and the grid gradient); and the total-variation regulariser of the grid with its analytic gradient.
//
// Replaces, per iteration: grid_sample on a 5-D tensor + einsum forward, and their autograd backward (which scatters
// the grid gradient with float atomics) in libtorch.
//
// The fp32 operation order (normative; tests/bilagrid_ref.py is its numpy mirror, op for op; every step below is one
// correctly rounded operation: -ffp-contract=off).  sx = (float)(GX-1) / (float)(W-1) (0 when W = 1), sy likewise, both
// formed once on the host.  For pixel (x, y) with colour c = (r, g, b):
//   fx = (float)x * sx;   x0 = min((int)fx, GX-2);   tx = fx - (float)x0          (y likewise)
//   luma = (0.299f r + 0.587f g) + 0.114f b;   zs = luma * (float)(L-1);   fz = min(max(zs, 0), (float)(L-1))
//   z0 = min((int)fz, L-2);   tz = fz - (float)z0;   inside = 0 <= zs <= L-1
//   lerp(a, b, t) = a + t * (b - a)
//   per coefficient k, with a.. the four values of G[k] at level z0 and b.. those at z0+1 (rows y0, y0+1; columns x0, x0+1):
//     p0 = lerp(lerp(a00, a01, tx), lerp(a10, a11, tx), ty);   p1 likewise from b..;   D_k = p1 - p0;   E_k = p0 + tz * D_k
//   corrected_i = ((E[4i] r + E[4i+1] g) + E[4i+2] b) + E[4i+3]
// Backward, with g = dL/dcorrected:
//   q_i = ((D[4i] r + D[4i+1] g) + D[4i+2] b) + D[4i+3]                 (d corrected_i / d fz)
//   s = inside ? ((g_0 q_0 + g_1 q_1) + g_2 q_2) * (float)(L-1) : 0
//   dL_drendered_j = ((E[j] g_0 + E[4+j] g_1) + E[8+j] g_2) + s * lw_j,   lw = (0.299f, 0.587f, 0.114f)
// The lerp form (rather than eight weight products) makes a lattice that is constant over a pixel's eight corners come
// out exactly: b - a = 0, so E_k is that constant and D_k = 0.  Hence the IDENTITY grid returns `rendered` and
// dL_drendered = g bit for bit (1 c + 0 = c; the one exception is a -0.0 input, which comes back as +0.0).
// tx (ty) may exceed 1 by an ulp in the last column (row), where (float)(W-1) * sx rounds above GX-1: the same formula
// then extrapolates by that ulp.
//
// Grid gradient: dL_dG[k, z, y, x] = sum_p w(p; z, y, x) g_i(p) [c(p), 1]_j with the product weights
// wxy = {(1-ty)(1-tx), (1-ty) tx, ty (1-tx), ty tx} and wz = 1-tz at z0, tz at z0+1 - no float atomics, no host sync, no
// allocation, fixed orders: the same bits from run to run.  (float)x * sx is monotone in x, so the image splits exactly
// into the (GX-1)(GY-1) xy-cells of the lattice, each a rectangle whose bounds host and device find with the same
// cell_of() by bisection.
//   k_bilagrid_cells    one workgroup per CHUNK = 1024 pixels of a cell (row-major inside the cell; a thread keeps its
//                       four pixels' twelve products g_i [c, 1]_j in registers), Q = ceil(largest cell / CHUNK) chunks
//                       for every cell.  It loops over the L levels: each lane adds (wxy wz) * products into 4 x 12
//                       register sums (fmaf), a folding butterfly sums them over the wave (51 shuffles for the 48 sums),
//                       the four waves are added in order, and [cell][chunk][z][corner][12] goes to the workspace.
//   k_bilagrid_combine  one thread per grid element: its up to 4 cells x Q partials in a fixed order in fp64 -> float.
//   k_bilagrid_pixels   the slice (and, as <true>, the image gradient) on the same decomposition: the workgroup
//                       copies its cell's four vertex columns (48 L floats, at most 12 KiB) to LDS as
//                       [z][corner][12] and every pixel samples them with 24 16-byte LDS reads.  12 B read and 12 B
//                       written per pixel (24 B and 12 B backward); consecutive lanes take consecutive pixels of a
//                       row of the cell.
// Where the grid lives: at (16,16,8) its 96 KiB would fit LDS whole, but the interface admits 64^3 vertices (12 MiB),
// which do not; read straight from global memory (it stays in L2) the slice issues 96 scattered 4-byte loads per pixel,
// whose lanes differ in z and so in cache line, and is bound by the vector L1's address rate - measured 0.139 ms per
// 1080p image, 360 GB/s of image traffic.  A cell's four columns are all a pixel needs, they fit LDS for every
// admissible L, and the partition into cells is the one the grid gradient needs anyway: one route for every grid size.
//
// k_bilagrid_tv: one workgroup of 1024 threads (the grid is tiny); tv = sum over the axes z, y, x of the mean squared
// forward difference, differences and sums in fp64 (thread t takes elements t, t + 1024, ...; then a tree), and the
// analytic gradient weight * sum_axis (2 / N_axis) ((G_i - G_i-1) - (G_i+1 - G_i)), formed in fp64, written or added to
// dL_dgrid.
#include "cugs_common.h"

#include <math.h>

namespace {

constexpr int PPT = 4;                      // pixels per thread
constexpr int CHUNK = CUGS_BLOCK * PPT;     // pixels of a cell per workgroup
constexpr int NSUM = 48;                    // 4 xy-corners x 12 coefficients
constexpr int NWAVE = CUGS_BLOCK / CUGS_WAVE;
constexpr int GRID_MIN = 2, GRID_MAX = 64;

struct Dims { int L, GY, GX; };

// Lattice cell of pixel coordinate v along an axis with `ncell` cells (scale s = (n_vertices - 1) / (extent - 1)).
__host__ __device__ inline int cell_of(int v, float s, int ncell) {
    const int c = (int)((float)v * s);
    return c < ncell - 1 ? c : ncell - 1;
}
// Smallest v in [0, extent] with cell_of(v) >= c (extent if none): cell c covers [cell_begin(c), cell_begin(c + 1)).
__host__ __device__ inline int cell_begin(int c, float s, int ncell, int extent) {
    if (c >= ncell) return extent;
    int lo = 0, hi = extent;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cell_of(mid, s, ncell) >= c) hi = mid; else lo = mid + 1;
    }
    return lo;
}

struct Coord { int x0, y0, z0; float tx, ty, tz; bool inside; };

__device__ __forceinline__ Coord coord_of(int x, int y, float r, float g, float b, float sx, float sy, Dims d) {
    Coord c;
    const float fx = (float)x * sx, fy = (float)y * sy;
    c.x0 = min((int)fx, d.GX - 2);
    c.y0 = min((int)fy, d.GY - 2);
    c.tx = fx - (float)c.x0;
    c.ty = fy - (float)c.y0;
    const float luma = (0.299f * r + 0.587f * g) + 0.114f * b;
    const float top = (float)(d.L - 1);
    const float zs = luma * top;
    const float fz = fminf(fmaxf(zs, 0.0f), top);              // a NaN luma reads as 0
    c.inside = zs >= 0.0f && zs <= top;
    c.z0 = min((int)fz, d.L - 2);
    c.tz = fz - (float)c.z0;
    return c;
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

constexpr int ZSTRIDE = 52;                 // floats per level of the LDS tile: 4 corners x 12, padded (see load_tile)

// The geometry of a workgroup's chunk: its xy-cell's rectangle of the image.
struct CellRect { int cx, cy, xb, yb, wc; int64_t count; };

__device__ __forceinline__ CellRect cell_rect(int cell, int width, int height, Dims d, float sx, float sy) {
    const int ncx = d.GX - 1, ncy = d.GY - 1;
    CellRect r;
    r.cy = cell / ncx;
    r.cx = cell - r.cy * ncx;
    r.xb = cell_begin(r.cx, sx, ncx, width);
    r.yb = cell_begin(r.cy, sy, ncy, height);
    r.wc = cell_begin(r.cx + 1, sx, ncx, width) - r.xb;
    r.count = (int64_t)r.wc * (cell_begin(r.cy + 1, sy, ncy, height) - r.yb);
    return r;
}

// The four vertex columns of cell (cx, cy) -> LDS as [z][corner 2 dy + dx][12 coefficients]: what every pixel of the
// cell samples.  52 floats per level keep the rows 16-byte aligned and put the levels z = 0..7 on disjoint banks for
// the 16-byte reads (52 z mod 64 = 0, 52, 40, 28, 16, 4, 56, 44, four banks each): lanes differ only in z.
__device__ __forceinline__ void load_tile(const float* __restrict__ grid, Dims d, int cx, int cy, float* __restrict__ s_g) {
    for (int i = threadIdx.x; i < d.L * NSUM; i += CUGS_BLOCK) {
        const int z = i / NSUM, rem = i - z * NSUM, corner = rem / 12, k = rem - corner * 12;
        s_g[z * ZSTRIDE + rem] = grid[(((size_t)k * d.L + z) * d.GY + cy + (corner >> 1)) * d.GX + cx + (corner & 1)];
    }
}

// E = the sliced 3x4 transform, D = its derivative along fz, from the cell's tile: four coefficients (one 16-byte read
// per corner and level) at a time.
__device__ __forceinline__ void sample(const float* __restrict__ s_g, const Coord& c, float (&E)[12], float (&D)[12]) {
    const float4* lo = reinterpret_cast<const float4*>(s_g + c.z0 * ZSTRIDE);
    const float4* hi = reinterpret_cast<const float4*>(s_g + (c.z0 + 1) * ZSTRIDE);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float4 a4[4] = {lo[q], lo[3 + q], lo[6 + q], lo[9 + q]}, b4[4] = {hi[q], hi[3 + q], hi[6 + q], hi[9 + q]};
        const float a[4][4] = {{a4[0].x, a4[0].y, a4[0].z, a4[0].w}, {a4[1].x, a4[1].y, a4[1].z, a4[1].w},
                               {a4[2].x, a4[2].y, a4[2].z, a4[2].w}, {a4[3].x, a4[3].y, a4[3].z, a4[3].w}};
        const float b[4][4] = {{b4[0].x, b4[0].y, b4[0].z, b4[0].w}, {b4[1].x, b4[1].y, b4[1].z, b4[1].w},
                               {b4[2].x, b4[2].y, b4[2].z, b4[2].w}, {b4[3].x, b4[3].y, b4[3].z, b4[3].w}};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float p0 = lerp(lerp(a[0][e], a[1][e], c.tx), lerp(a[2][e], a[3][e], c.tx), c.ty);
            const float p1 = lerp(lerp(b[0][e], b[1][e], c.tx), lerp(b[2][e], b[3][e], c.tx), c.ty);
            D[4 * q + e] = p1 - p0;
            E[4 * q + e] = p0 + c.tz * D[4 * q + e];
        }
    }
}

// The slice and, as <true>, the image gradient: one workgroup per chunk of an xy-cell, as k_bilagrid_cells.
template <bool BWD>
__global__ __launch_bounds__(CUGS_BLOCK) void k_bilagrid_pixels(int width, int height, Dims d, float sx, float sy, int nchunk,
                                                                const float* __restrict__ grid,
                                                                const float* __restrict__ rendered,
                                                                const float* __restrict__ dL_dcorrected,
                                                                float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_g[GRID_MAX * ZSTRIDE];
    const int cell = blockIdx.x / nchunk, chunk = blockIdx.x - cell * nchunk;
    const CellRect rc = cell_rect(cell, width, height, d, sx, sy);
    if ((int64_t)chunk * CHUNK >= rc.count) return;                     // the whole workgroup: no barrier is skipped
    load_tile(grid, d, rc.cx, rc.cy, s_g);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int64_t i = (int64_t)chunk * CHUNK + j * CUGS_BLOCK + threadIdx.x;
        if (i >= rc.count) break;
        const int row = (int)(i / rc.wc), col = (int)(i - (int64_t)row * rc.wc);
        const int x = rc.xb + col, y = rc.yb + row;
        const int64_t p = 3 * ((int64_t)y * width + x);
        const float r = rendered[p], g = rendered[p + 1], b = rendered[p + 2];
        const Coord c = coord_of(x, y, r, g, b, sx, sy, d);
        float E[12], D[12], o[3];
        sample(s_g, c, E, D);
        if constexpr (BWD) {
            const float g0 = dL_dcorrected[p], g1 = dL_dcorrected[p + 1], g2 = dL_dcorrected[p + 2];
            float q[3];
#pragma unroll
            for (int n = 0; n < 3; ++n) q[n] = ((D[4 * n] * r + D[4 * n + 1] * g) + D[4 * n + 2] * b) + D[4 * n + 3];
            const float s = c.inside ? ((g0 * q[0] + g1 * q[1]) + g2 * q[2]) * (float)(d.L - 1) : 0.0f;
            const float lw[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
            for (int n = 0; n < 3; ++n) o[n] = ((E[n] * g0 + E[4 + n] * g1) + E[8 + n] * g2) + s * lw[n];
        } else {
#pragma unroll
            for (int n = 0; n < 3; ++n) o[n] = ((E[4 * n] * r + E[4 * n + 1] * g) + E[4 * n + 2] * b) + E[4 * n + 3];
        }
        out[p] = o[0]; out[p + 1] = o[1]; out[p + 2] = o[2];
    }
}

// One step of the folding butterfly: the lane pairs at distance DIST split the 2 H live sums between them - the lower
// lane keeps sums [0, H) and hands over [H, 2 H), the upper one the reverse - and each adds what it receives.
template <int H, int DIST>
__device__ __forceinline__ void fold(float (&v)[NSUM], int lane) {
    const bool hi = (lane & DIST) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const float keep = hi ? v[i + H] : v[i], send = hi ? v[i] : v[i + H];
        v[i] = keep + __shfl_xor(send, DIST);
    }
}

// The wave's 48 sums: after four folds a lane holds three, (24 b5 + 12 b4 + 6 b3 + 3 b2) + {0, 1, 2} by its lane bits;
// two plain butterfly steps finish them.  A fixed tree: the same bits whatever the run.  Returns the first index.
__device__ __forceinline__ int wave_sums(float (&v)[NSUM], int lane) {
    fold<24, 32>(v, lane);
    fold<12, 16>(v, lane);
    fold<6, 8>(v, lane);
    fold<3, 4>(v, lane);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[i] += __shfl_xor(v[i], 2);
        v[i] += __shfl_xor(v[i], 1);
    }
    return 24 * ((lane >> 5) & 1) + 12 * ((lane >> 4) & 1) + 6 * ((lane >> 3) & 1) + 3 * ((lane >> 2) & 1);
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_bilagrid_cells(int width, int height, Dims d, float sx, float sy, int nchunk,
                                                               const float* __restrict__ rendered,
                                                               const float* __restrict__ dL_dcorrected,
                                                               float* __restrict__ partials) {
    __shared__ float s_part[NWAVE][NSUM];
    const int cell = blockIdx.x / nchunk, chunk = blockIdx.x - cell * nchunk;
    const CellRect rc = cell_rect(cell, width, height, d, sx, sy);
    const int xb = rc.xb, yb = rc.yb, wc = rc.wc;
    const int64_t count = rc.count;
    const int tid = threadIdx.x, lane = tid & (CUGS_WAVE - 1), wave = tid / CUGS_WAVE;

    // the thread's pixels: linear indices chunk * CHUNK + j * CUGS_BLOCK + tid of the cell, row-major
    float prod[PPT][12], wxy[PPT][4], tz[PPT];
    int z0[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int64_t i = (int64_t)chunk * CHUNK + j * CUGS_BLOCK + tid;
        const bool in = i < count;
        const int row = in ? (int)(i / wc) : 0, col = in ? (int)(i - (int64_t)row * wc) : 0;
        const int x = in ? xb + col : 0, y = in ? yb + row : 0;
        const int64_t p = (int64_t)y * width + x;
        const float r = in ? rendered[3 * p] : 0.0f, g = in ? rendered[3 * p + 1] : 0.0f, b = in ? rendered[3 * p + 2] : 0.0f;
        const float g0 = in ? dL_dcorrected[3 * p] : 0.0f, g1 = in ? dL_dcorrected[3 * p + 1] : 0.0f;
        const float g2 = in ? dL_dcorrected[3 * p + 2] : 0.0f;
        const Coord c = coord_of(x, y, r, g, b, sx, sy, d);
        const float ux = 1.0f - c.tx, uy = 1.0f - c.ty, live = in ? 1.0f : 0.0f;    // a slot past the cell adds +0.0
        wxy[j][0] = live * (uy * ux); wxy[j][1] = live * (uy * c.tx);
        wxy[j][2] = live * (c.ty * ux); wxy[j][3] = live * (c.ty * c.tx);
        z0[j] = c.z0;
        tz[j] = c.tz;
        const float gi[3] = {g0, g1, g2};
#pragma unroll
        for (int i3 = 0; i3 < 3; ++i3) {
            prod[j][4 * i3] = gi[i3] * r; prod[j][4 * i3 + 1] = gi[i3] * g;
            prod[j][4 * i3 + 2] = gi[i3] * b; prod[j][4 * i3 + 3] = gi[i3];
        }
    }

    float* const dst = partials + (size_t)blockIdx.x * d.L * NSUM;
    for (int z = 0; z < d.L; ++z) {
        float acc[NSUM];
#pragma unroll
        for (int k = 0; k < NSUM; ++k) acc[k] = 0.0f;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const float wz = (z == z0[j]) ? 1.0f - tz[j] : ((z == z0[j] + 1) ? tz[j] : 0.0f);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float w = wxy[j][c] * wz;
#pragma unroll
                for (int k = 0; k < 12; ++k) acc[12 * c + k] = fmaf(w, prod[j][k], acc[12 * c + k]);
            }
        }
        const int first = wave_sums(acc, lane);
        if ((lane & 3) == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) s_part[wave][first + i] = acc[i];
        }
        __syncthreads();
        if (tid < NSUM) {
            float a = s_part[0][tid];
#pragma unroll
            for (int v = 1; v < NWAVE; ++v) a += s_part[v][tid];
            dst[(size_t)z * NSUM + tid] = a;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_bilagrid_combine(Dims d, int nchunk, const float* __restrict__ partials,
                                                                 float* __restrict__ dL_dgrid) {
    const int total = 12 * d.L * d.GY * d.GX;
    const int e = blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (e >= total) return;
    const int x = e % d.GX, y = (e / d.GX) % d.GY, z = (e / (d.GX * d.GY)) % d.L, k = e / (d.GX * d.GY * d.L);
    const int ncx = d.GX - 1, ncy = d.GY - 1;
    double a = 0.0;
    for (int dy = 0; dy < 2; ++dy) {
        const int cy = y - dy;
        if (cy < 0 || cy >= ncy) continue;
        for (int dx = 0; dx < 2; ++dx) {
            const int cx = x - dx;
            if (cx < 0 || cx >= ncx) continue;
            const float* src = partials + (((size_t)(cy * ncx + cx) * nchunk) * d.L + z) * NSUM + 12 * (2 * dy + dx) + k;
            for (int q = 0; q < nchunk; ++q) a += (double)src[(size_t)q * d.L * NSUM];
        }
    }
    dL_dgrid[e] = (float)a;
}

constexpr int TV_BLOCK = 1024;               // the one workgroup of k_bilagrid_tv

__global__ __launch_bounds__(TV_BLOCK) void k_bilagrid_tv(Dims d, const float* __restrict__ grid, float weight,
                                                            float* __restrict__ tv_out, float* __restrict__ dL_dgrid,
                                                            int accumulate) {
    __shared__ double s_acc[3][TV_BLOCK];
    const int total = 12 * d.L * d.GY * d.GX;
    const int stride[3] = {d.GY * d.GX, d.GX, 1};                      // z, y, x
    const int extent[3] = {d.L, d.GY, d.GX};
    double inv[3], sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 3; ++a) inv[a] = 1.0 / ((double)(total / extent[a]) * (extent[a] - 1));
    for (int e = threadIdx.x; e < total; e += TV_BLOCK) {
        const int at[3] = {(e / stride[0]) % d.L, (e / d.GX) % d.GY, e % d.GX};
        const double v = (double)grid[e];
        double g = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (at[a] + 1 < extent[a]) {
                const double f = (double)grid[e + stride[a]] - v;
                sum[a] += f * f;
                g -= 2.0 * inv[a] * f;
            }
            if (at[a] > 0) g += 2.0 * inv[a] * (v - (double)grid[e - stride[a]]);
        }
        if (dL_dgrid) {
            const float t = (float)((double)weight * g);
            dL_dgrid[e] = accumulate ? dL_dgrid[e] + t : t;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) s_acc[a][threadIdx.x] = sum[a];
    __syncthreads();
    for (int s = TV_BLOCK / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int a = 0; a < 3; ++a) s_acc[a][threadIdx.x] += s_acc[a][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && tv_out) tv_out[0] = (float)((s_acc[0][0] * inv[0] + s_acc[1][0] * inv[1]) + s_acc[2][0] * inv[2]);
}

size_t round256(size_t b) { return (b + 255) / 256 * 256; }

bool dims_ok(const cugs_bilagrid_dims* g) {
    return g && g->l >= GRID_MIN && g->l <= GRID_MAX && g->gy >= GRID_MIN && g->gy <= GRID_MAX && g->gx >= GRID_MIN &&
           g->gx <= GRID_MAX;
}
float axis_scale(int nvert, int extent) { return extent > 1 ? (float)(nvert - 1) / (float)(extent - 1) : 0.0f; }
int widest_cell(int nvert, int extent) {
    const float s = axis_scale(nvert, extent);
    int best = 0, b = 0;
    for (int c = 0; c < nvert - 1; ++c) {
        const int e = cell_begin(c + 1, s, nvert - 1, extent);
        if (e - b > best) best = e - b;
        b = e;
    }
    return best;
}
// Q: chunks per cell, from the largest cell of this image and lattice
size_t chunks_per_cell(int width, int height, const cugs_bilagrid_dims* g) {
    const size_t cellmax = (size_t)widest_cell(g->gx, width) * (size_t)widest_cell(g->gy, height);
    return cellmax ? (cellmax + CHUNK - 1) / CHUNK : 1;
}

}  // namespace

// [cell][chunk][z][corner][12] floats
extern "C" size_t cugs_bilagrid_workspace_bytes(int width, int height, const cugs_bilagrid_dims* dims) {
    if (width <= 0 || height <= 0 || !dims_ok(dims)) return 0;
    const size_t cells = (size_t)(dims->gx - 1) * (dims->gy - 1);
    return round256(sizeof(float) * NSUM * dims->l * cells * chunks_per_cell(width, height, dims));
}

extern "C" int cugs_bilagrid_slice(int width, int height, const cugs_bilagrid_dims* dims, const float* grid,
                                   const float* rendered, float* corrected, void* stream) {
    if (width <= 0 || height <= 0 || !dims_ok(dims) || !grid || !rendered || !corrected) return CUGS_EINVAL;
    if ((int64_t)width * height > 2147483647ll) return CUGS_EOVERFLOW;
    const Dims d{dims->l, dims->gy, dims->gx};
    const size_t nchunk = chunks_per_cell(width, height, dims);         // x cells: below 2^22 + 63^2 workgroups
    const unsigned nblk = (unsigned)((size_t)(d.GX - 1) * (d.GY - 1) * nchunk);
    hipLaunchKernelGGL(k_bilagrid_pixels<false>, dim3(nblk), dim3(CUGS_BLOCK), 0, static_cast<hipStream_t>(stream), width, height,
                       d, axis_scale(d.GX, width), axis_scale(d.GY, height), (int)nchunk, grid, rendered,
                       static_cast<const float*>(nullptr), corrected);
    CUGS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cugs_bilagrid_slice_backward(int width, int height, const cugs_bilagrid_dims* dims, const float* grid,
                                            const float* rendered, const float* dL_dcorrected, void* workspace,
                                            size_t workspace_bytes, float* dL_drendered, float* dL_dgrid, void* stream) {
    if (width <= 0 || height <= 0 || !dims_ok(dims) || !grid || !rendered || !dL_dcorrected) return CUGS_EINVAL;
    if (dL_dgrid && !workspace) return CUGS_EINVAL;
    if (dL_dgrid && workspace_bytes < cugs_bilagrid_workspace_bytes(width, height, dims)) return CUGS_EWORKSPACE;
    if ((int64_t)width * height > 2147483647ll) return CUGS_EOVERFLOW;
    const Dims d{dims->l, dims->gy, dims->gx};
    const float sx = axis_scale(d.GX, width), sy = axis_scale(d.GY, height);
    const size_t nchunk = chunks_per_cell(width, height, dims);
    const dim3 blocks((unsigned)((size_t)(d.GX - 1) * (d.GY - 1) * nchunk)), threads(CUGS_BLOCK);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dL_drendered) {
        hipLaunchKernelGGL(k_bilagrid_pixels<true>, blocks, threads, 0, st, width, height, d, sx, sy, (int)nchunk, grid, rendered,
                           dL_dcorrected, dL_drendered);
        CUGS_LAUNCH_CHECK();
    }
    if (dL_dgrid) {
        float* const partials = static_cast<float*>(workspace);
        hipLaunchKernelGGL(k_bilagrid_cells, blocks, threads, 0, st, width, height, d, sx, sy, (int)nchunk, rendered,
                           dL_dcorrected, partials);
        CUGS_LAUNCH_CHECK();
        const int total = 12 * d.L * d.GY * d.GX;
        hipLaunchKernelGGL(k_bilagrid_combine, dim3((total + CUGS_BLOCK - 1) / CUGS_BLOCK), threads, 0, st, d, (int)nchunk,
                           partials, dL_dgrid);
        CUGS_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int cugs_bilagrid_tv(const cugs_bilagrid_dims* dims, const float* grid, float weight, float* tv_out,
                                float* dL_dgrid, int accumulate, void* stream) {
    if (!dims_ok(dims) || !grid || (!tv_out && !dL_dgrid)) return CUGS_EINVAL;
    const Dims d{dims->l, dims->gy, dims->gx};
    hipLaunchKernelGGL(k_bilagrid_tv, dim3(1), dim3(TV_BLOCK), 0, static_cast<hipStream_t>(stream), d, grid, weight, tv_out,
                       dL_dgrid, accumulate);
    CUGS_LAUNCH_CHECK();
    return 0;
}
