// depth_loss.hip — depth supervision (not in the reference): the masked, optionally weighted L1 loss of
// the expected depth x = D / A (or, in inverse space, x = A / D) of render()'s depth and alpha maps against a depth
// prior t' = s t + b, and its analytic dL/dD and dL/dA for render_backward; (s, b) is (1, 0), given by the caller, or
// the weighted least-squares fit of t to x over the valid pixels, solved on the device.
//
// Replaces, per iteration: where / div / the masked five sums and the 2x2 solve / abs / sign / both gradients in
// libtorch (a dozen element-wise launches over the image and usually a read-back for the solve).
//
//   k_depth_stats     (fit only) the sums w, w t, w x, w t^2, w t x and the count over the valid pixels, one row of fp64
//                     partials per workgroup;
//   k_depth_fit       (fit only) one workgroup: the rows in a fixed order (thread t takes rows t, t + 256, ...; then a
//                     tree, as k_eval_finalize), the 2x2 solve in fp64 -> s, b, fit_ok as floats in the workspace head;
//   k_depth_loss      one pass over the image: reads (s, b) from device memory, writes dL/dD, dL/dA, optionally x, and
//                     one row {sum w |r|, sum of valid w, valid count} of fp64 partials per workgroup;
//   k_depth_finalize  one workgroup: the rows in the same fixed order -> loss_out[8].
// No float atomics, no host sync, no allocation, fixed reduction orders: the same bits from run to run.
//
// (s, b) is a CONSTANT in the gradient: a fit enters dL/dD and dL/dA only through t', never through ds/dx or db/dx,
// as in every trainer that fits the alignment under no_grad.
//
// The image is a flat run of H W pixels (no window, no tiles): a thread owns four consecutive pixels - one 16-byte
// access per map where every base is 16-byte aligned and the four lie inside the image, scalar accesses otherwise (the
// tail, unaligned views) - and a workgroup 1024.  The pixel-to-thread map does not depend on the access width, so
// neither do the sums.  HBM-bound: 12-16 B read and 8-12 B written per pixel; the fit pass reads 12-16 B more.
// Every float step below is one correctly rounded operation (-ffp-contract=off, IEEE division); tests/depth_loss_ref.py
// is its numpy mirror, op for op.
#include "cugs_common.h"
#include "cugs_row_sums.h"   // block_sums, reduce_rows

#include <math.h>

namespace {

constexpr int PPT = 4;                          // pixels per thread
constexpr int CHUNK = CUGS_BLOCK * PPT;         // pixels per workgroup = per row of partials
constexpr int NFIT = 6;                         // sum w, w t, w x, w t^2, w t x, count
constexpr int NLOSS = 3;                        // sum w |r|, sum of valid w, count
constexpr int HEAD = 256;                       // workspace head: float {s, b, fit_ok} of the fit

struct Pixels { float D[PPT], A[PPT], t[PPT], w[PPT]; };      // w: only with a weight map (else 1, see weight_of)

// The thread's four pixels.  One outside the image reads as A = 0: invalid, adds +0.0 to every sum, stores nothing.
template <bool HAS_W>
__device__ __forceinline__ void load_pixels(const float* __restrict__ D, const float* __restrict__ A,
                                            const float* __restrict__ t, const float* __restrict__ w, int64_t p0,
                                            int64_t n, bool vec, Pixels& px) {
    if (vec && p0 + PPT <= n) {
        const float4 d4 = *reinterpret_cast<const float4*>(D + p0), a4 = *reinterpret_cast<const float4*>(A + p0);
        const float4 t4 = *reinterpret_cast<const float4*>(t + p0);
        px.D[0] = d4.x; px.D[1] = d4.y; px.D[2] = d4.z; px.D[3] = d4.w;
        px.A[0] = a4.x; px.A[1] = a4.y; px.A[2] = a4.z; px.A[3] = a4.w;
        px.t[0] = t4.x; px.t[1] = t4.y; px.t[2] = t4.z; px.t[3] = t4.w;
        if constexpr (HAS_W) {
            const float4 w4 = *reinterpret_cast<const float4*>(w + p0);
            px.w[0] = w4.x; px.w[1] = w4.y; px.w[2] = w4.z; px.w[3] = w4.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const bool in = p0 + k < n;
            const int64_t p = in ? p0 + k : 0;
            px.D[k] = in ? D[p] : 0.0f;
            px.A[k] = in ? A[p] : 0.0f;
            px.t[k] = in ? t[p] : 0.0f;
            if constexpr (HAS_W) px.w[k] = in ? w[p] : 0.0f;
        }
    }
}

template <bool HAS_W>
__device__ __forceinline__ float weight_of(const Pixels& px, int k) { if constexpr (HAS_W) return px.w[k]; else return 1.0f; }

// valid: A > min_alpha, w > 0, 0 < t < +inf (a NaN fails every comparison) and, in inverse space, D > 0.
// x = D / A (INV: A / D) at a valid pixel, 0 elsewhere - the divisor of a valid pixel is positive.
template <bool INV>
__device__ __forceinline__ bool expected_depth(float D, float A, float t, float w, float min_alpha, float& x) {
    bool valid = A > min_alpha && w > 0.0f && t > 0.0f && t < INFINITY;
    if constexpr (INV) valid = valid && D > 0.0f;
    const float num = INV ? A : D, den = INV ? D : A;
    x = valid ? num / (valid ? den : 1.0f) : 0.0f;
    return valid;
}

template <bool INV, bool HAS_W>
__global__ __launch_bounds__(CUGS_BLOCK) void k_depth_stats(int64_t n, const float* __restrict__ D,
                                                            const float* __restrict__ A, const float* __restrict__ t,
                                                            const float* __restrict__ w, float min_alpha, int vec,
                                                            double* __restrict__ partials) {
    const int64_t p0 = ((int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x) * PPT;
    Pixels px;
    load_pixels<HAS_W>(D, A, t, w, p0, n, vec != 0, px);
    double acc[NFIT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        float x;
        const float wk = weight_of<HAS_W>(px, k);
        if (expected_depth<INV>(px.D[k], px.A[k], px.t[k], wk, min_alpha, x)) {
            const double wd = (double)wk, td = (double)px.t[k], xd = (double)x, wt = wd * td;
            acc[0] += wd; acc[1] += wt; acc[2] += wd * xd; acc[3] += wt * td; acc[4] += wt * xd; acc[5] += 1.0;
        }
    }
    block_sums<NFIT>(acc, partials + (size_t)NFIT * blockIdx.x);
}

// min sum w (s t + b - x)^2: the normal equations by Cramer's rule in fp64.  Accepted with two or more valid pixels
// and a determinant above 1e-12 of its leading product (a constant target has none); otherwise (1, 0), fit_ok = 0.
__global__ __launch_bounds__(CUGS_BLOCK) void k_depth_fit(const double* __restrict__ partials, int nblk,
                                                           float* __restrict__ fit) {
    __shared__ double s_acc[NFIT][CUGS_BLOCK];
    reduce_rows<NFIT>(partials, nblk, s_acc);
    if (threadIdx.x == 0) {
        const double Sw = s_acc[0][0], St = s_acc[1][0], Sx = s_acc[2][0], Stt = s_acc[3][0], Stx = s_acc[4][0];
        const double det = Sw * Stt - St * St;
        const bool ok = s_acc[5][0] >= 2.0 && det > 1e-12 * Sw * Stt;
        const double s = ok ? (Sw * Stx - St * Sx) / det : 1.0, b = ok ? (Stt * Sx - St * Stx) / det : 0.0;
        fit[0] = (float)s;
        fit[1] = (float)b;
        fit[2] = ok ? 1.0f : 0.0f;
    }
}

template <bool INV, bool HAS_W>
__global__ __launch_bounds__(CUGS_BLOCK) void k_depth_loss(int64_t n, const float* __restrict__ D,
                                                           const float* __restrict__ A, const float* __restrict__ t,
                                                           const float* __restrict__ w, const float* __restrict__ ss,
                                                           float min_alpha, float inv_n, int vec, float* __restrict__ gD,
                                                           float* __restrict__ gA, float* __restrict__ expected,
                                                           double* __restrict__ partials) {
    const int64_t p0 = ((int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x) * PPT;
    const float s = ss ? ss[0] : 1.0f, b = ss ? ss[1] : 0.0f;
    Pixels px;
    load_pixels<HAS_W>(D, A, t, w, p0, n, vec != 0, px);
    double acc[NLOSS] = {0.0, 0.0, 0.0};
    float oD[PPT], oA[PPT], oX[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        float x;
        const float wk = weight_of<HAS_W>(px, k);
        const bool valid = expected_depth<INV>(px.D[k], px.A[k], px.t[k], wk, min_alpha, x);
        const float tp = s * px.t[k] + b;                                   // two roundings
        const float r = x - tp;
        const float sgn = (r > 0.0f) ? 1.0f : ((r < 0.0f) ? -1.0f : 0.0f);
        const float gx = (wk * sgn) * inv_n;
        const float den = valid ? (INV ? px.D[k] : px.A[k]) : 1.0f;
        const float direct = gx / den, through = -((gx * x) / den);        // d/d numerator, d/d denominator
        oD[k] = valid ? (INV ? through : direct) : 0.0f;
        oA[k] = valid ? (INV ? direct : through) : 0.0f;
        oX[k] = x;
        if (valid) { acc[0] += (double)(wk * fabsf(r)); acc[1] += (double)wk; acc[2] += 1.0; }
    }
    if (vec && p0 + PPT <= n) {
        if (gD) *reinterpret_cast<float4*>(gD + p0) = make_float4(oD[0], oD[1], oD[2], oD[3]);
        if (gA) *reinterpret_cast<float4*>(gA + p0) = make_float4(oA[0], oA[1], oA[2], oA[3]);
        if (expected) *reinterpret_cast<float4*>(expected + p0) = make_float4(oX[0], oX[1], oX[2], oX[3]);
    } else {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            if (p0 + k < n) {
                if (gD) gD[p0 + k] = oD[k];
                if (gA) gA[p0 + k] = oA[k];
                if (expected) expected[p0 + k] = oX[k];
            }
        }
    }
    block_sums<NLOSS>(acc, partials + (size_t)NLOSS * blockIdx.x);
}

// out = {loss, s, b, sum of valid w, valid count, fit_ok, 0, 0}; the mean is over all H W pixels whatever the mask.
__global__ __launch_bounds__(CUGS_BLOCK) void k_depth_finalize(const double* __restrict__ partials, int nblk, double count,
                                                                const float* __restrict__ ss, const float* __restrict__ fit,
                                                                float* __restrict__ out) {
    __shared__ double s_acc[NLOSS][CUGS_BLOCK];
    reduce_rows<NLOSS>(partials, nblk, s_acc);
    if (threadIdx.x == 0) {
        out[0] = (float)(s_acc[0][0] / count);
        out[1] = ss ? ss[0] : 1.0f;
        out[2] = ss ? ss[1] : 0.0f;
        out[3] = (float)s_acc[1][0];
        out[4] = (float)s_acc[2][0];
        out[5] = fit ? fit[2] : 1.0f;
        out[6] = 0.0f;
        out[7] = 0.0f;
    }
}

size_t round256(size_t b) { return (b + 255) / 256 * 256; }
size_t row_count(int width, int height) { return ((size_t)width * (size_t)height + CHUNK - 1) / CHUNK; }

template <bool INV, bool HAS_W>
int run_depth_loss(int64_t n, int nblk, const float* D, const float* A, const float* t, const cugs_depth_loss_opts& o,
                   int vec, float* fit, double* fit_rows, double* loss_rows, float* loss_out, float* gD, float* gA,
                   hipStream_t st) {
    const dim3 grid(nblk), block(CUGS_BLOCK);
    const float* ss = o.scale_shift;
    if (o.fit) {
        hipLaunchKernelGGL((k_depth_stats<INV, HAS_W>), grid, block, 0, st, n, D, A, t, o.weight, o.min_alpha, vec, fit_rows);
        CUGS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_depth_fit, dim3(1), block, 0, st, fit_rows, nblk, fit);
        CUGS_LAUNCH_CHECK();
        ss = fit;
    }
    const float inv_n = 1.0f / (float)n;
    hipLaunchKernelGGL((k_depth_loss<INV, HAS_W>), grid, block, 0, st, n, D, A, t, o.weight, ss, o.min_alpha, inv_n, vec, gD,
                       gA, o.expected, loss_rows);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_depth_finalize, dim3(1), block, 0, st, loss_rows, nblk, (double)n, ss,
                       o.fit ? fit : static_cast<const float*>(nullptr), loss_out);
    CUGS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// The head (s, b, fit_ok of a fit), then the [rows][6] fp64 partials of the fit and the [rows][3] of the loss.
extern "C" size_t cugs_depth_loss_workspace_bytes(int width, int height) {
    if (width < 0 || height < 0) return 0;
    const size_t rows = row_count(width, height);
    return HEAD + round256(sizeof(double) * NFIT * rows) + round256(sizeof(double) * NLOSS * rows);
}

extern "C" int cugs_depth_loss(int width, int height, const float* depth_map, const float* alpha, const float* target,
                               const cugs_depth_loss_opts* opts, void* workspace, size_t workspace_bytes, float* loss_out,
                               float* dL_ddepth_map, float* dL_dalpha, void* stream) {
    if (width <= 0 || height <= 0 || !depth_map || !alpha || !target || !opts || !workspace || !loss_out) return CUGS_EINVAL;
    if (!(opts->min_alpha > 0.0f && opts->min_alpha < INFINITY)) return CUGS_EINVAL;
    if (opts->fit && opts->scale_shift) return CUGS_EINVAL;
    if (workspace_bytes < cugs_depth_loss_workspace_bytes(width, height)) return CUGS_EWORKSPACE;
    const int64_t n = (int64_t)width * height;
    if (n > 2147483647ll) return CUGS_EOVERFLOW;
    const size_t rows = row_count(width, height);
    char* const base = static_cast<char*>(workspace);
    float* const fit = reinterpret_cast<float*>(base);
    double* const fit_rows = reinterpret_cast<double*>(base + HEAD);
    double* const loss_rows = reinterpret_cast<double*>(base + HEAD + round256(sizeof(double) * NFIT * rows));
    // 16-byte accesses only where every map that is touched allows them
    const int vec = cugs_aligned16(depth_map) && cugs_aligned16(alpha) && cugs_aligned16(target) &&
                    cugs_aligned16(opts->weight) && cugs_aligned16(opts->expected) && cugs_aligned16(dL_ddepth_map) &&
                    cugs_aligned16(dL_dalpha);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool inv = opts->inverse != 0, has_w = opts->weight != nullptr;
#define CUGS_DEPTH_LOSS(I, W) \
    run_depth_loss<I, W>(n, (int)rows, depth_map, alpha, target, *opts, vec, fit, fit_rows, loss_rows, loss_out, \
                         dL_ddepth_map, dL_dalpha, st)
    if (inv) return has_w ? CUGS_DEPTH_LOSS(true, true) : CUGS_DEPTH_LOSS(true, false);
    return has_w ? CUGS_DEPTH_LOSS(false, true) : CUGS_DEPTH_LOSS(false, false);
#undef CUGS_DEPTH_LOSS
}
