// envmap.hip — environment-map background (not in the reference): the pixels the Gaussians leave open
// show a learnable octahedral sky map E [3, R, R], sampled bilinearly in the direction of the pixel's ray and blended
// in behind the render as I = C + T B, with the gradients to the map and - through dL/dalpha - to the Gaussians.
//
// Replaces, per view: per-pixel directions / a normalisation / the map coordinates / grid_sample / a multiply-add and
// the autograd pass back through all of them in libtorch.
//
//   k_env_composite           one thread per pixel: ray -> octahedral coordinates -> four folded taps -> lerp ->
//                             fmaf(T, B, C).  ENV = false takes B from a caller's background image instead.
//   k_env_composite_backward  one thread per pixel: recomputes the taps; dL/dalpha = -sum_c g_c B_c; each tap's share
//                             w_k T g_c goes to an int64 table as rint(share * 2^F) through 64-bit integer atomics (a
//                             share of exactly 0 - every covered pixel, T = 0 - is not sent).
//   k_env_clear / k_env_finish  clear the table and the flag word / table -> fp32 [3, R, R].
// The arithmetic is fixed step by step in include/cugs_hip.h (one correctly rounded fp32 operation per step, fmaf only
// where written; -ffp-contract=off) and mirrored by tests/envmap_ref.py.  No float atomics, no host sync, no allocation:
// the same bytes from run to run.
//
// Memory: a wave reads or writes 64 consecutive pixels = 768 contiguous bytes of an [H, W, 3] image in three dword
// accesses of stride 12 B; every fetched line is used whole, so the 3-float stride costs instructions, not traffic.
// Forward 28 B per pixel (12 + 4 read, 12 written); the map's taps hit the L2 (R = 1024: 12 MB).
#include "cugs_common.h"

#include <math.h>

namespace {

constexpr int ENV_R_MIN = 4, ENV_R_MAX = 2048;
constexpr int ENV_E_MIN = -60, ENV_E_MAX = 24;      // grad_bound rounded up to 2^e

struct EnvArgs {
    float m[9];
    float fx, fy, cx, cy;
    int width, height, res;
};

struct EnvTaps {
    int idx[4];          // E00, E01, E10, E11: j * R + i of the folded tap
    float a, b;
};

// step 5: fold a tap outside [0, R) back by the octahedral rule; i, j in [-1, R] come out in [0, R)
__device__ __forceinline__ int env_fold(int i, int j, int R) {
    if (i < 0) { i = -1 - i; j = R - 1 - j; }
    else if (i >= R) { i = 2 * R - 1 - i; j = R - 1 - j; }
    if (j < 0) { j = -1 - j; i = R - 1 - i; }
    else if (j >= R) { j = 2 * R - 1 - j; i = R - 1 - i; }
    return j * R + i;
}

__device__ __forceinline__ float env_sgn(float t) { return t >= 0.0f ? 1.0f : -1.0f; }

// steps 1-5 for pixel (u, v)
__device__ __forceinline__ EnvTaps env_taps(const EnvArgs& g, int u, int v) {
    const float ax = (((float)u + 0.5f) - g.cx) / g.fx;
    const float ay = (((float)v + 0.5f) - g.cy) / g.fy;
    const float d0 = fmaf(g.m[0], ax, fmaf(g.m[1], ay, g.m[2]));
    const float d1 = fmaf(g.m[3], ax, fmaf(g.m[4], ay, g.m[5]));
    const float d2 = fmaf(g.m[6], ax, fmaf(g.m[7], ay, g.m[8]));
    const float s = (fabsf(d0) + fabsf(d1)) + fabsf(d2);
    const bool ok = s > 0.0f && s < INFINITY;
    const float sd = ok ? s : 1.0f;
    const float n0 = d0 / sd, n1 = d1 / sd, n2 = d2 / sd;
    float x = n0, y = n1;
    if (n2 < 0.0f) {
        x = (1.0f - fabsf(n1)) * env_sgn(n0);
        y = (1.0f - fabsf(n0)) * env_sgn(n1);
    }
    if (!ok) { x = 0.0f; y = 0.0f; }
    const int R = g.res;
    const float h = 0.5f * (float)R, h1 = h - 0.5f;
    const float sx = fmaf(x, h, h1), sy = fmaf(y, h, h1);
    const float fx0 = fminf(fmaxf(floorf(sx), -1.0f), (float)(R - 1));      // NaN -> -1
    const float fy0 = fminf(fmaxf(floorf(sy), -1.0f), (float)(R - 1));
    const int i0 = (int)fx0, j0 = (int)fy0;
    EnvTaps t;
    t.a = sx - fx0;
    t.b = sy - fy0;
    t.idx[0] = env_fold(i0, j0, R);
    t.idx[1] = env_fold(i0 + 1, j0, R);
    t.idx[2] = env_fold(i0, j0 + 1, R);
    t.idx[3] = env_fold(i0 + 1, j0 + 1, R);
    return t;
}

// step 6 for one channel plane
__device__ __forceinline__ float env_lerp(const float* __restrict__ E, const EnvTaps& t) {
    const float e00 = E[t.idx[0]], e01 = E[t.idx[1]], e10 = E[t.idx[2]], e11 = E[t.idx[3]];
    const float top = fmaf(t.a, e01 - e00, e00);
    const float bot = fmaf(t.a, e11 - e10, e10);
    return fmaf(t.b, bot - top, top);
}

template <bool ENV>
__global__ __launch_bounds__(CUGS_BLOCK) void k_env_composite(EnvArgs g, const float* __restrict__ env,
                                                              const float* __restrict__ background,
                                                              const float* __restrict__ color,
                                                              const float* __restrict__ final_T,
                                                              float* __restrict__ image, float* __restrict__ sample) {
    const int64_t p64 = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (p64 >= (int64_t)g.width * g.height) return;
    const int p = (int)p64;
    float B[3];
    if constexpr (ENV) {
        const int v = p / g.width, u = p - v * g.width;
        const EnvTaps t = env_taps(g, u, v);
        const size_t plane = (size_t)g.res * g.res;
#pragma unroll
        for (int c = 0; c < 3; ++c) B[c] = env_lerp(env + c * plane, t);
        if (sample) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sample[3 * (size_t)p + c] = B[c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) B[c] = background[3 * (size_t)p + c];
    }
    if (image) {
        const float T = final_T[p];
#pragma unroll
        for (int c = 0; c < 3; ++c) image[3 * (size_t)p + c] = fmaf(T, B[c], color[3 * (size_t)p + c]);
    }
}

template <bool ENV>
__global__ __launch_bounds__(CUGS_BLOCK) void k_env_composite_backward(EnvArgs g, const float* __restrict__ env,
                                                                       const float* __restrict__ background,
                                                                       const float* __restrict__ grad,
                                                                       const float* __restrict__ final_T, float bound,
                                                                       double scale, float* __restrict__ dL_dalpha,
                                                                       unsigned long long* __restrict__ table,
                                                                       float* __restrict__ dL_dbackground,
                                                                       int32_t* __restrict__ clamped) {
    const int64_t p64 = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (p64 >= (int64_t)g.width * g.height) return;
    const int p = (int)p64;
    float gc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) gc[c] = grad[3 * (size_t)p + c];
    float B[3];
    EnvTaps t;
    if constexpr (ENV) {
        const int v = p / g.width, u = p - v * g.width;
        t = env_taps(g, u, v);
        const size_t plane = (size_t)g.res * g.res;
        if (dL_dalpha) {
#pragma unroll
            for (int c = 0; c < 3; ++c) B[c] = env_lerp(env + c * plane, t);
        }
    } else {
        if (dL_dalpha) {
#pragma unroll
            for (int c = 0; c < 3; ++c) B[c] = background[3 * (size_t)p + c];
        }
    }
    if (dL_dalpha) dL_dalpha[p] = -fmaf(gc[2], B[2], fmaf(gc[1], B[1], gc[0] * B[0]));
    if constexpr (ENV) {
        if (!table) return;
    } else {
        if (!dL_dbackground) return;
    }
    const float T = final_T[p];
    if constexpr (!ENV) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dL_dbackground[3 * (size_t)p + c] = T * gc[c];
    } else {
        const float oma = 1.0f - t.a, omb = 1.0f - t.b;
        const float w[4] = {oma * omb, t.a * omb, oma * t.b, t.a * t.b};
        const size_t plane = (size_t)g.res * g.res;
        bool over = false;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float tg = T * gc[c];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float sh = w[k] * tg;
                if (!(fabsf(sh) <= bound)) {
                    over = true;
                    sh = (sh != sh) ? 0.0f : copysignf(bound, sh);
                }
                const long long q = __double2ll_rn((double)sh * scale);
                if (q != 0) atomicAdd(table + c * plane + t.idx[k], (unsigned long long)q);
            }
        }
        if (over) *clamped = 1;          // every writer stores the same word
    }
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_env_clear(int64_t words, unsigned long long* __restrict__ table,
                                                          int32_t* __restrict__ clamped) {
    const int64_t e = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (e < words) table[e] = 0ull;
    if (e == 0) *clamped = 0;
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_env_finish(int64_t words, const long long* __restrict__ table,
                                                           double inv_scale, float* __restrict__ dL_denv) {
    const int64_t e = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (e < words) dL_denv[e] = (float)((double)table[e] * inv_scale);
}

bool env_finite(float x) { return x > -INFINITY && x < INFINITY; }
bool env_aligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }
bool env_res_ok(int r) { return r >= ENV_R_MIN && r <= ENV_R_MAX && (r & (r - 1)) == 0; }

bool env_view_ok(const cugs_envmap_view* v, bool env) {
    if (!v || v->width <= 0 || v->height <= 0) return false;
    if (!env) return true;
    if (!env_res_ok(v->resolution)) return false;
    if (!(v->fx > 0.0f && v->fx < INFINITY && v->fy > 0.0f && v->fy < INFINITY)) return false;
    if (!env_finite(v->cx) || !env_finite(v->cy)) return false;
    for (int i = 0; i < 9; ++i)
        if (!env_finite(v->m[i])) return false;
    return true;
}

EnvArgs env_args(const cugs_envmap_view* v) {
    EnvArgs g;
    for (int i = 0; i < 9; ++i) g.m[i] = v->m[i];
    g.fx = v->fx; g.fy = v->fy; g.cx = v->cx; g.cy = v->cy;
    g.width = v->width; g.height = v->height; g.res = v->resolution;
    return g;
}

// the e of the smallest 2^e >= bound, or INT_MIN for a bound outside [2^ENV_E_MIN, 2^ENV_E_MAX]
int env_bound_exp(float bound) {
    if (!(bound > 0.0f && bound < INFINITY)) return INT32_MIN;
    int e;
    const float f = frexpf(bound, &e);          // bound = f 2^e, f in [0.5, 1)
    if (f == 0.5f) --e;                         // a power of two already
    return (e < ENV_E_MIN || e > ENV_E_MAX) ? INT32_MIN : e;
}

}  // namespace

extern "C" int cugs_envmap_view_init(cugs_envmap_view* out, const cugs_camera* camera, const double* orientation,
                                     int resolution) {
    if (!out || !camera || !env_res_ok(resolution)) return CUGS_EINVAL;
    static const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double* O = orientation ? orientation : eye;
    for (int i = 0; i < 9; ++i)
        if (!(O[i] > -INFINITY && O[i] < INFINITY)) return CUGS_EINVAL;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            // (O R^T)[i][j] = sum_k O[i][k] R[j][k]; view is row-major, R[j][k] = view[4j + k]
            const double r0 = (double)camera->view[4 * j], r1 = (double)camera->view[4 * j + 1], r2 = (double)camera->view[4 * j + 2];
            out->m[3 * i + j] = (float)((O[3 * i] * r0 + O[3 * i + 1] * r1) + O[3 * i + 2] * r2);
        }
    out->fx = camera->fx; out->fy = camera->fy; out->cx = camera->cx; out->cy = camera->cy;
    out->width = camera->width; out->height = camera->height; out->resolution = resolution;
    return env_view_ok(out, true) ? 0 : CUGS_EINVAL;
}

extern "C" size_t cugs_envmap_workspace_bytes(int resolution) {
    if (!env_res_ok(resolution)) return 0;
    return sizeof(long long) * 3 * (size_t)resolution * (size_t)resolution;
}

extern "C" int cugs_envmap_frac_bits(int width, int height, float grad_bound) {
    if (width <= 0 || height <= 0) return CUGS_EINVAL;
    const int e = env_bound_exp(grad_bound);
    if (e == INT32_MIN) return CUGS_EINVAL;
    const int64_t n = (int64_t)width * height;
    if (n > 2147483647ll) return CUGS_EOVERFLOW;
    int q = 0;
    while ((4 * n) >> q) ++q;                   // 4 H W < 2^q
    return 61 - q - e;
}

extern "C" int cugs_envmap_composite(const cugs_envmap_view* view, const float* env, const float* background,
                                     const float* color, const float* final_T, float* image, float* sample, void* stream) {
    if ((env != nullptr) == (background != nullptr)) return CUGS_EINVAL;
    if (!env_view_ok(view, env != nullptr)) return CUGS_EINVAL;
    if (!image && !sample) return CUGS_EINVAL;
    if (image && (!color || !final_T)) return CUGS_EINVAL;
    if (sample && !env) return CUGS_EINVAL;
    const int64_t n = (int64_t)view->width * view->height;
    if (n > 2147483647ll) return CUGS_EOVERFLOW;
    if (!env_aligned(env, 3) || !env_aligned(background, 3) || !env_aligned(color, 3) || !env_aligned(final_T, 3) ||
        !env_aligned(image, 3) || !env_aligned(sample, 3))
        return CUGS_EALIGN;
    const EnvArgs g = env_args(view);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + CUGS_BLOCK - 1) / CUGS_BLOCK)), block(CUGS_BLOCK);
    if (env) hipLaunchKernelGGL(k_env_composite<true>, grid, block, 0, st, g, env, background, color, final_T, image, sample);
    else hipLaunchKernelGGL(k_env_composite<false>, grid, block, 0, st, g, env, background, color, final_T, image, sample);
    CUGS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cugs_envmap_composite_backward(const cugs_envmap_view* view, const float* env, const float* background,
                                              const float* dL_dimage, const float* final_T, float grad_bound,
                                              void* workspace, size_t workspace_bytes, float* dL_dalpha, float* dL_denv,
                                              float* dL_dbackground, int32_t* clamped, void* stream) {
    if ((env != nullptr) == (background != nullptr)) return CUGS_EINVAL;
    if (!env_view_ok(view, env != nullptr)) return CUGS_EINVAL;
    if (!dL_dimage) return CUGS_EINVAL;
    if (env ? dL_dbackground != nullptr : dL_denv != nullptr) return CUGS_EINVAL;
    if ((dL_denv || dL_dbackground) && !final_T) return CUGS_EINVAL;
    if (dL_denv && (!workspace || !clamped)) return CUGS_EINVAL;
    int frac = 0, e = 0;
    if (dL_denv) {
        e = env_bound_exp(grad_bound);
        if (e == INT32_MIN) return CUGS_EINVAL;
    }
    const int64_t n = (int64_t)view->width * view->height;
    if (n > 2147483647ll) return CUGS_EOVERFLOW;
    if (dL_denv && workspace_bytes < cugs_envmap_workspace_bytes(view->resolution)) return CUGS_EWORKSPACE;
    if (!env_aligned(env, 3) || !env_aligned(background, 3) || !env_aligned(dL_dimage, 3) || !env_aligned(final_T, 3) ||
        !env_aligned(dL_dalpha, 3) || !env_aligned(dL_denv, 3) || !env_aligned(dL_dbackground, 3) ||
        !env_aligned(clamped, 3) || (dL_denv && !env_aligned(workspace, 7)))
        return CUGS_EALIGN;
    if (!dL_dalpha && !dL_denv && !dL_dbackground) return 0;

    const EnvArgs g = env_args(view);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + CUGS_BLOCK - 1) / CUGS_BLOCK)), block(CUGS_BLOCK);
    unsigned long long* table = dL_denv ? static_cast<unsigned long long*>(workspace) : nullptr;
    const int64_t words = dL_denv ? 3 * (int64_t)view->resolution * view->resolution : 0;
    const dim3 tgrid((unsigned)((words + CUGS_BLOCK - 1) / CUGS_BLOCK));
    if (dL_denv) {
        frac = cugs_envmap_frac_bits(view->width, view->height, grad_bound);
        hipLaunchKernelGGL(k_env_clear, tgrid, block, 0, st, words, table, clamped);
        CUGS_LAUNCH_CHECK();
    }
    const float bound = ldexpf(1.0f, e);
    if (env) hipLaunchKernelGGL(k_env_composite_backward<true>, grid, block, 0, st, g, env, background, dL_dimage, final_T,
                                bound, ldexp(1.0, frac), dL_dalpha, table, dL_dbackground, clamped);
    else hipLaunchKernelGGL(k_env_composite_backward<false>, grid, block, 0, st, g, env, background, dL_dimage, final_T,
                            bound, ldexp(1.0, frac), dL_dalpha, table, dL_dbackground, clamped);
    CUGS_LAUNCH_CHECK();
    if (dL_denv) {
        hipLaunchKernelGGL(k_env_finish, tgrid, block, 0, st, words, reinterpret_cast<const long long*>(table),
                           ldexp(1.0, -frac), dL_denv);
        CUGS_LAUNCH_CHECK();
    }
    return 0;
}
