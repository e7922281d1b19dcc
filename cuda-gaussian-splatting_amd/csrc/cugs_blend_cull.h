// cugs_blend_cull.h — the blend kernels' conservative cull: can a Gaussian reach alpha >= 1/255 at ANY pixel centre of a
// rectangle of centres inside one 16x16 tile?  Two pieces: cugs_cull_limit, once per staged record (stage_record and the
// score kernel's staging put its result into word 6 of the LDS record, where the packed record carries tau), and
// cugs_cull_may_touch, once per (wave, record) against the wave's live active rectangle.
// Plain float C++ with no other header of the project behind it: the blends call it on the device, and
// tests/test_cull_host.py compiles it for the host against brute force in double precision and the previous formula.
//
// alpha = min(0.99, o * exp(power)) >= 1/255 needs -power <= tau := ln(255 o)  (tau < 0: never; the record stores
// tau = -1 for o < 1/255, where o * exp(power <= 0) <= o < 1/255 exactly).  -power = q/2 with
// q(d) = a dx^2 + 2 b dx dy + c dy^2, d = centre - mean.  So the record is dropped when  q_min > 2 (tau + slack),
// q_min the minimum of q over the rectangle.
//
// Rounding: the oracle's fp32 power differs from the exact one by at most ~4 ulp of B = |a| X^2 + 2 |b| X Y + |c| Y^2
// (X, Y the largest |offset|); q_min here carries a similar error; ocml logf ~2 ulp; cugs_blend_exp_q <= 1e-6 relative.
// The slack 0.01 tau + 0.05 + 4e-6 B dominates all of it by orders of magnitude.
#pragma once

#if defined(__HIPCC__)
#define CUGS_CULL_HD __host__ __device__ __forceinline__
#else
#define CUGS_CULL_HD static inline
#endif

// clamp v into [lo, hi] (lo <= hi): one v_med3_f32 on the device.  A NaN v gives lo on both sides.
CUGS_CULL_HD float cugs_cull_clamp(float v, float lo, float hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(v, lo, hi);
#else
    return __builtin_fminf(__builtin_fmaxf(v, lo), hi);
#endif
}
CUGS_CULL_HD float cugs_cull_rcp(float x) {            // cull only: 1 ulp is irrelevant
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}

// Everything of the test that belongs to the record and its tile, computed ONCE when the record is staged: the largest
// q_min that still may touch, 2 (1.01 tau + 0.05 + 4e-6 Bt), with the guards folded into its value:
//   -1           if !(tau >= 0) (a NaN tau included): culled by every wave;
//   +inf or NaN  if !(a > 0 && c > 0), NaN if the mean or b is: never culled (the test's comparisons are false);
// (tcx, tcy): the centre of the 16x16 tile, i.e. 16 * tile + 8: every pixel centre of the tile lies within 7.5 of it.
// Bt = a Xt^2 + 2 |b| Xt Yt + c Yt^2 with Xt = |mx - tcx| + 7.5 >= |centre x - mx| (Yt likewise) bounds B for EVERY
// rectangle of centres inside the tile, so against a B taken from the rectangle itself the slack only grows.  Xt is
// rounded twice and can come out an ulp or two below a rectangle's own fp32 X; the factor on Bt is therefore
// 4.00001e-6 instead of 4e-6 (2.5e-6 relative, against < 1.5e-6 for the roundings of Xt, Yt and of the products), so
// that the limit is never below the one made from the rectangle, in fp32 as well.
CUGS_CULL_HD float cugs_cull_limit(float mx, float my, float a, float b, float c, float tau, float tcx, float tcy) {
    const float Xt = __builtin_fabsf(mx - tcx) + 7.5f, Yt = __builtin_fabsf(my - tcy) + 7.5f;
    const float Bt = a * Xt * Xt + 2.0f * __builtin_fabsf(b) * Xt * Yt + c * Yt * Yt;
    const float thr = tau * 1.01f + 0.05f + 4.00001e-6f * Bt;
    // never culled = +inf or NaN, made without a literal: rcp(1) = 1 exactly, rcp(0) = +inf, and |lim| is lim itself for
    // a, c > 0 and tau >= 0 (then thr >= 0.05); a literal +inf would sit in a vector register for the whole kernel, and
    // the backward blend has none to spare
    const float lim = __builtin_fabsf(thr + thr) * cugs_cull_rcp((a > 0.0f && c > 0.0f) ? 1.0f : 0.0f);
    return (tau >= 0.0f) ? lim : -1.0f;
}

// The test: may the Gaussian (mean, conic a b c, `lim` from cugs_cull_limit) touch the rectangle of pixel centres
// [qx0, qx0 + wx] x [qy0, qy0 + wy] (wx, wy >= 0; inside the tile lim was made for)?  `false` only when certainly not.
//
// q is convex with its minimum, 0, at the mean.  Over a rectangle that does not contain the mean the minimum lies on an
// edge FACING the mean (a point of a far edge is reached from the mean through a near edge, where q is smaller), and
// along an edge q is a 1-D convex parabola (a, c > 0), minimised at the clamped vertex.  With the near-edge coordinate
// taken as the clamp of 0 - xe = clamp(0, lx, hx): 0 when the mean is inside the x-range, else the nearer end - the two
// candidates
//     qx = min over y of q(xe, y),   qy = min over x of q(x, ye)
// need no case distinction, q_min = min(qx, qy):
//   * mean inside both ranges: xe = ye = 0, the vertices clamp to 0, qx = qy = 0;
//   * mean inside the x-range only: xe = 0, the vertex -b xe / c is 0, so qx = q(0, clamp(0, ly, hy)) = q(0, ye) is
//     the value of q at ONE point of the edge y = ye that qy is minimised over: qx >= qy, and qy is the true minimum
//     (in fp32 the two may swap by an ulp: the smaller one is taken, the conservative side); symmetrically in y;
//   * mean outside both: the two near edges, as before.
// No compare and no select; a NaN q_min makes the comparison false -> not culled.
CUGS_CULL_HD bool cugs_cull_may_touch(float mx, float my, float a, float b, float c, float lim, float qx0, float qy0,
                                      float wx, float wy) {
    const float ia = cugs_cull_rcp(a), ic = cugs_cull_rcp(c);
    const float lx = qx0 - mx, hx = lx + wx, ly = qy0 - my, hy = ly + wy;
    const float xe = cugs_cull_clamp(0.0f, lx, hx), ye = cugs_cull_clamp(0.0f, ly, hy);
    const float yv = cugs_cull_clamp(-b * xe * ic, ly, hy);
    const float xv = cugs_cull_clamp(-b * ye * ia, lx, hx);
    const float b2 = b + b;
    const float qx = a * xe * xe + b2 * xe * yv + c * yv * yv;
    const float qy = a * xv * xv + b2 * xv * ye + c * ye * ye;
    const float qmin = __builtin_fminf(qx, qy);
    return !(lim < 0.0f) && !(qmin > lim);          // a NaN lim or q_min: not culled
}
