// metrics.hip — evaluation metrics of one rendered view against its target (training/metrics.cpp:21-46): MSE (for
// PSNR), mean SSIM, mean |x - y| and max |x - y| as four device floats, no host sync.
//
// Replaces, per view: (rendered - target).pow(2).mean().item() and ssim(rendered, target).mean().item() (five grouped
// 11x11 conv2d's, ~20 elementwise kernels, two blocking read-backs) and, with an 8-bit target, the x 1/255 expansion
// to float that precedes them (data/image_io.cpp:35-39).
//
// One pass over 16x16 pixel tiles, the tile edge, halo (window/2 in LDS) and zero padding of loss.hip's k_ssim_stats, and
// the same per-pixel SSIM arithmetic, operation for operation: -ffp-contract=off leaves only the explicit fmaf's fused,
// so the per-pixel values, the per-tile fp64 partials and - with the reduction order of finalize_loss (thread t takes
// tiles t, t + 256, ...; then a tree) - the means are the bits cugs_combined_loss puts into loss_out[2] and [1].
// What evaluation does not need is gone: the three derivative maps (36 B/pixel written) and the SSIM map.  Reads 24
// B/pixel with a float target, 15 B/pixel with an 8-bit one (converted in registers: (float)b * (1.0f / 255.0f), the
// expression of views.hip's texel()); writes 32 B per tile.  A second one-workgroup launch reduces the partials.
// NaN in an input reaches every sum that pixel takes part in (the reference's behaviour); the maximum, which fmaxf
// alone would keep clean, is set to NaN when the L1 sum is.
#include "cugs_common.h"

namespace {

constexpr int LT = 16;            // tile edge
constexpr int MAX_R = 7;          // window sizes 3..15
constexpr int MAX_E = LT + 2 * MAX_R;
constexpr int NSUM = 4;           // per-tile partials: sum |d|, sum SSIM, sum d^2 (fp64), max |d|

struct Window { float w[2 * MAX_R + 1]; int r; };

__device__ __forceinline__ float to_float(float v) { return v; }
__device__ __forceinline__ float to_float(uint8_t b) { return (float)b * (1.0f / 255.0f); }       // image_io.cpp:35-39

// The input tiles in LDS, interleaved [.,.,3] layout as in loss.hip: a tile row of E pixels is E*3 consecutive elements,
// the horizontal pass sees 48 output "columns" with a tap stride of 3.  With a compile-time radius every thread issues
// all its loads first and the pair (x, y) of element e goes to s_x[2e], s_x[2e+1] (one ds_read_b64 feeds a packed FMA).
template <int RT, typename TY>
__device__ __forceinline__ void load_pair(const float* __restrict__ xr, const TY* __restrict__ yt, float* s_x, float* s_y,
                                          int tx0, int ty0, int R, int E, int w, int h) {
    const int row_f = E * 3, total = E * row_f, w3 = w * 3;
    if constexpr (RT > 0) {
        constexpr int ET = LT + 2 * RT, PER = (ET * ET * 3 + CUGS_BLOCK - 1) / CUGS_BLOCK;
        float vx[PER];
        TY vy[PER];
        bool okv[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = (int)threadIdx.x + i * CUGS_BLOCK;
            const int ey = e / row_f, ef = e - ey * row_f;
            const int gy = ty0 + ey - R, gxf = (tx0 - R) * 3 + ef;      // element index within the image row
            const bool ok = e < total && gy >= 0 && gy < h && gxf >= 0 && gxf < w3;
            const int64_t off = ok ? (int64_t)gy * w3 + gxf : 0;
            vx[i] = xr[off]; vy[i] = yt[off]; okv[i] = ok;
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = (int)threadIdx.x + i * CUGS_BLOCK;
            if (e < total)                                              // zero padding
                reinterpret_cast<float2*>(s_x)[e] = okv[i] ? make_float2(vx[i], to_float(vy[i])) : make_float2(0.0f, 0.0f);
        }
    } else {
        for (int e = threadIdx.x; e < total; e += CUGS_BLOCK) {
            const int ey = e / row_f, ef = e - ey * row_f;
            const int gy = ty0 + ey - R, gxf = (tx0 - R) * 3 + ef;
            const bool ok = gy >= 0 && gy < h && gxf >= 0 && gxf < w3;
            const int64_t off = (int64_t)gy * w3 + gxf;
            s_x[e] = ok ? xr[off] : 0.0f;
            s_y[e] = ok ? to_float(yt[off]) : 0.0f;
        }
    }
}

template <int RT, typename TY>
__global__ __launch_bounds__(CUGS_BLOCK) void k_eval_stats(int w, int h, Window win, const float* __restrict__ xr,
                                                           const TY* __restrict__ yt, double* __restrict__ sums) {
    constexpr int CW = LT * 3;                                           // 48 float columns per tile row
    // As in k_ssim_stats: with a compile-time radius the horizontal sums pass through registers and overwrite the
    // input tiles (25 KB for the 11-tap window: 6 blocks per CU); the cross-wave reduction at the end borrows the
    // pool too, so the block holds no LDS beyond it.
    constexpr bool ALIAS = RT > 0;
    constexpr int ET = ALIAS ? LT + 2 * RT : MAX_E;
    constexpr int IN_F = ET * ET * 3, H_F = ET * CW;
    constexpr int POOL = ALIAS ? (2 * IN_F > 5 * H_F ? 2 * IN_F : 5 * H_F) : 2 * IN_F + 5 * H_F;
    __shared__ __attribute__((aligned(16))) float s_pool[POOL];
    static_assert(sizeof(s_pool) >= NSUM * 4 * sizeof(double), "the block reduction borrows the tile pool");
    float* const s_x = s_pool;
    float* const s_y = s_pool + IN_F;
    float* const s_hp = ALIAS ? s_pool : s_pool + 2 * IN_F;             // plane k at s_hp + k * H_F
    const int R = RT > 0 ? RT : win.r, E = LT + 2 * R;
    const int tx0 = blockIdx.x * LT, ty0 = blockIdx.y * LT;
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int px = tx0 + lx, py = ty0 + ly;
    const bool inside = px < w && py < h;
    typedef float v2f __attribute__((ext_vector_type(2)));
    load_pair<RT, TY>(xr, yt, s_x, s_y, tx0, ty0, R, E, w, h);
    __syncthreads();
    // x - y at this thread's pixel, read before the tiles can be overwritten
    float dc[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int c = ((ly + R) * E + lx + R) * 3 + ch;
        if constexpr (ALIAS) {
            const float2 xy = reinterpret_cast<const float2*>(s_pool)[c];
            dc[ch] = xy.x - xy.y;
        } else {
            dc[ch] = s_x[c] - s_y[c];
        }
    }
    // horizontal pass: E rows x 48 float columns (16 pixels x 3 channels), tap stride 3
    if constexpr (ALIAS) {
        constexpr int PER_H = (H_F + CUGS_BLOCK - 1) / CUGS_BLOCK;
        const v2f* s_xy = reinterpret_cast<const v2f*>(s_pool);
        v2f acc_ab[PER_H], acc_sq[PER_H];
        float acc_xy[PER_H];
#pragma unroll
        for (int i = 0; i < PER_H; ++i) {
            const int e = tid + i * CUGS_BLOCK;
            acc_ab[i] = (v2f){0.0f, 0.0f}; acc_sq[i] = (v2f){0.0f, 0.0f}; acc_xy[i] = 0.0f;
            if (e < H_F) {
                const int ey = e / CW, cf = e - ey * CW;
                const v2f* row = s_xy + ey * E * 3 + cf;
#pragma unroll
                for (int k = 0; k <= 2 * R; ++k) {
                    const float wk = win.w[k];
                    const v2f xy = row[3 * k], wk2 = {wk, wk};
                    acc_ab[i] = __builtin_elementwise_fma(wk2, xy, acc_ab[i]);
                    acc_sq[i] = __builtin_elementwise_fma(wk2, xy * xy, acc_sq[i]);
                    acc_xy[i] = fmaf(wk, xy.x * xy.y, acc_xy[i]);
                }
            }
        }
        __syncthreads();                                                 // every read of the input tiles is done
        v2f* h_ab = reinterpret_cast<v2f*>(s_pool);
        v2f* h_sq = reinterpret_cast<v2f*>(s_pool + 2 * H_F);
        float* h_xy = s_pool + 4 * H_F;
#pragma unroll
        for (int i = 0; i < PER_H; ++i) {
            const int e = tid + i * CUGS_BLOCK;
            if (e < H_F) { h_ab[e] = acc_ab[i]; h_sq[e] = acc_sq[i]; h_xy[e] = acc_xy[i]; }
        }
    } else {
        for (int e = tid; e < E * CW; e += CUGS_BLOCK) {
            const int ey = e / CW, cf = e - ey * CW;
            const float* rx = s_x + ey * E * 3 + cf;
            const float* ry = s_y + ey * E * 3 + cf;
            float a = 0.0f, b = 0.0f, aa = 0.0f, bb = 0.0f, ab = 0.0f;
            for (int k = 0; k <= 2 * R; ++k) {
                const float wk = win.w[k], xv = rx[3 * k], yv = ry[3 * k];
                a = fmaf(wk, xv, a); b = fmaf(wk, yv, b);
                aa = fmaf(wk, xv * xv, aa); bb = fmaf(wk, yv * yv, bb); ab = fmaf(wk, xv * yv, ab);
            }
            s_hp[e] = a; s_hp[H_F + e] = b; s_hp[2 * H_F + e] = aa; s_hp[3 * H_F + e] = bb; s_hp[4 * H_F + e] = ab;
        }
    }
    __syncthreads();
    double l1_acc = 0.0, ss_acc = 0.0, sq_acc = 0.0;
    float mx = 0.0f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float m = 0.0f, n = 0.0f, p = 0.0f, q = 0.0f, r = 0.0f;
        if constexpr (ALIAS) {
            const v2f* h_ab = reinterpret_cast<const v2f*>(s_pool);
            const v2f* h_sq = reinterpret_cast<const v2f*>(s_pool + 2 * H_F);
            const float* h_xy = s_pool + 4 * H_F;
            v2f mn = {0.0f, 0.0f}, pq = {0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k <= 2 * R; ++k) {
                const float wk = win.w[k];
                const v2f wk2 = {wk, wk};
                const int e = (ly + k) * CW + lx * 3 + ch;
                mn = __builtin_elementwise_fma(wk2, h_ab[e], mn);
                pq = __builtin_elementwise_fma(wk2, h_sq[e], pq);
                r = fmaf(wk, h_xy[e], r);
            }
            m = mn.x; n = mn.y; p = pq.x; q = pq.y;
        } else {
            for (int k = 0; k <= 2 * R; ++k) {
                const float wk = win.w[k];
                const int e = (ly + k) * CW + lx * 3 + ch;
                m = fmaf(wk, s_hp[e], m); n = fmaf(wk, s_hp[H_F + e], n); p = fmaf(wk, s_hp[2 * H_F + e], p);
                q = fmaf(wk, s_hp[3 * H_F + e], q); r = fmaf(wk, s_hp[4 * H_F + e], r);
            }
        }
        if (inside) {
            const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
            const float mn = m * n, mm = m * m, nn = n * n;
            const float A1 = 2.0f * mn + C1, A2 = 2.0f * (r - mn) + C2;
            const float B1 = mm + nn + C1, B2 = (p - mm) + (q - nn) + C2;
            const float inv = 1.0f / (B1 * B2);
            const float S = A1 * A2 * inv;
            const float d = dc[ch], ad = fabsf(d);
            ss_acc += (double)S;
            l1_acc += (double)ad;
            sq_acc += (double)d * (double)d;
            mx = fmaxf(mx, ad);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        l1_acc += __shfl_xor(l1_acc, d); ss_acc += __shfl_xor(ss_acc, d); sq_acc += __shfl_xor(sq_acc, d);
        mx = fmaxf(mx, __shfl_xor(mx, d));
    }
    __syncthreads();                                                     // every read of the horizontal sums is done
    double (*s_red)[4] = reinterpret_cast<double (*)[4]>(s_pool);
    if ((tid & 63) == 0) {
        s_red[0][tid >> 6] = l1_acc; s_red[1][tid >> 6] = ss_acc; s_red[2][tid >> 6] = sq_acc; s_red[3][tid >> 6] = (double)mx;
    }
    __syncthreads();
    if (tid == 0) {
        // one row of partials per tile, summed in fp64 in tile order by k_eval_finalize: deterministic
        double* row = sums + NSUM * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        row[0] = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
        row[1] = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
        row[2] = s_red[2][0] + s_red[2][1] + s_red[2][2] + s_red[2][3];
        row[3] = fmax(fmax(s_red[3][0], s_red[3][1]), fmax(s_red[3][2], s_red[3][3]));
    }
}

// The per-tile partials -> out[0] = MSE, [1] = mean SSIM, [2] = L1 mean, [3] = max |x - y|; one workgroup, fp64, the
// order of loss.hip's finalize_loss (thread t takes tiles t, t + 256, ...; then a tree).
__global__ __launch_bounds__(CUGS_BLOCK) void k_eval_finalize(const double* __restrict__ partials, int nblk, double count,
                                                               float* __restrict__ out) {
    __shared__ double s_acc[NSUM][CUGS_BLOCK];
    double a = 0.0, b = 0.0, c = 0.0, m = 0.0;
    for (int i = threadIdx.x; i < nblk; i += CUGS_BLOCK) {
        a += partials[NSUM * i]; b += partials[NSUM * i + 1]; c += partials[NSUM * i + 2];
        m = fmax(m, partials[NSUM * i + 3]);
    }
    s_acc[0][threadIdx.x] = a; s_acc[1][threadIdx.x] = b; s_acc[2][threadIdx.x] = c; s_acc[3][threadIdx.x] = m;
    __syncthreads();
    for (int d = CUGS_BLOCK / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) {
            s_acc[0][threadIdx.x] += s_acc[0][threadIdx.x + d];
            s_acc[1][threadIdx.x] += s_acc[1][threadIdx.x + d];
            s_acc[2][threadIdx.x] += s_acc[2][threadIdx.x + d];
            s_acc[3][threadIdx.x] = fmax(s_acc[3][threadIdx.x], s_acc[3][threadIdx.x + d]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double l1 = s_acc[0][0] / count, ss = s_acc[1][0] / count, mse = s_acc[2][0] / count;
        out[0] = (float)mse;
        out[1] = (float)ss;
        out[2] = (float)l1;
        out[3] = (l1 != l1) ? (float)l1 : (float)s_acc[3][0];            // fmax drops a NaN, the sum keeps it
    }
}

template <typename TY>
int launch_eval(int width, int height, const Window& win, const float* rendered, const TY* target, double* sums,
                hipStream_t st) {
    dim3 grid((width + LT - 1) / LT, (height + LT - 1) / LT), block(CUGS_BLOCK);
    if (win.r == 5)      // the reference's default window (11): compile-time radius
        hipLaunchKernelGGL((k_eval_stats<5, TY>), grid, block, 0, st, width, height, win, rendered, target, sums);
    else
        hipLaunchKernelGGL((k_eval_stats<0, TY>), grid, block, 0, st, width, height, win, rendered, target, sums);
    CUGS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" size_t cugs_eval_workspace_bytes(int width, int height) {
    if (width < 0 || height < 0) return 0;
    const size_t tiles = (size_t)((width + LT - 1) / LT) * (size_t)((height + LT - 1) / LT);
    return 256 + (sizeof(double) * NSUM * tiles + 255) / 256 * 256;
}

extern "C" int cugs_eval_metrics(int width, int height, const float* rendered, const float* target_f32,
                                 const uint8_t* target_u8, int window_size, void* workspace, size_t workspace_bytes,
                                 float* metrics_out, void* stream) {
    if (width < 0 || height < 0) return CUGS_EINVAL;
    if (window_size % 2 != 1 || window_size < 3 || window_size > 2 * MAX_R + 1) return CUGS_EINVAL;   // loss.cpp:96-97
    if (width == 0 || height == 0) return 0;
    if ((target_f32 != nullptr) == (target_u8 != nullptr)) return CUGS_EINVAL;            // exactly one target
    if (!rendered || !metrics_out || !workspace) return CUGS_EINVAL;
    if (workspace_bytes < cugs_eval_workspace_bytes(width, height)) return CUGS_EINVAL;
    if ((int64_t)width * height > 2147483647ll / 3) return CUGS_EOVERFLOW;
    hipStream_t st = static_cast<hipStream_t>(stream);

    // get_gaussian_kernel (loss.cpp:47-83), as cugs_combined_loss forms it: the separable factor of the rank-one
    // window, u = k1 / sqrt(sum(k1 (x) k1)).
    Window win;
    win.r = window_size / 2;
    float k1[2 * MAX_R + 1];
    float s1 = 0.0f;
    for (int i = 0; i < window_size; ++i) {
        const float x = (float)(i - win.r);
        k1[i] = expf(-x * x / (2.0f * 1.5f * 1.5f));
        s1 += k1[i];
    }
    double s2 = 0.0;
    for (int i = 0; i < window_size; ++i) k1[i] /= s1;
    for (int i = 0; i < window_size; ++i)
        for (int j = 0; j < window_size; ++j) s2 += (double)(k1[i] * k1[j]);
    for (int i = 0; i < 2 * MAX_R + 1; ++i) win.w[i] = i < window_size ? (float)((double)k1[i] / sqrt(s2)) : 0.0f;

    const size_t tiles = (size_t)((width + LT - 1) / LT) * (size_t)((height + LT - 1) / LT);
    double* sums = reinterpret_cast<double*>(static_cast<char*>(workspace) + 256);        // [tiles][NSUM] partials
    const int rc = target_f32 ? launch_eval(width, height, win, rendered, target_f32, sums, st)
                              : launch_eval(width, height, win, rendered, target_u8, sums, st);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(k_eval_finalize, dim3(1), dim3(CUGS_BLOCK), 0, st, sums, (int)tiles, (double)width * height * 3.0,
                       metrics_out);
    CUGS_LAUNCH_CHECK();
    return 0;
}
