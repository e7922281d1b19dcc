"""The blends' cull (csrc/cugs_blend_cull.h: cugs_cull_limit once per staged record, cugs_cull_may_touch once per wave and
record) compiled for the host and checked, on more than a million cases, against brute force in double precision and
against the formula it replaces (copied into the driver as prev_may_touch: compares and selects around the minimum, the
threshold rebuilt from the rectangle's own B at every test).

Families, as tests/test_gpu_cull.py's: opacities at and a few ulp above 1/255, means on the alpha = 1/255 contour of a pixel
of the rectangle and a few ulp off the rectangle's edges, condition numbers up to 1e6 with |b| close to sqrt(ac), tiny and
huge splats, every rectangle size 1..8 x 1..8 at every place of a quad, tiles with origin 0, 1904 and 4000 in either
axis.  And a scene-like family: depth 2..10, log-scales -4.6 +- 0.5 through a 1497.6 px focal length plus the 0.3 px^2
low-pass, sigmoid(N(0,1)) opacities, means wherever the 3-sigma box meets the tile.

Asserted:
 (a) never culled when a pixel centre of the rectangle has q/2 <= tau in double precision;
 (b) every record the previous formula keeps is kept;
 (c) scene-like family: the records kept that the previous formula rejects (the slack now bounds B over the whole tile)
     are at most 1e-3 of those it keeps;
 (d) a <= 0, c <= 0 or a NaN mean: never culled; tau < 0: always culled."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-gaussian-splatting_amd", "csrc")

ADVERSARIAL = 1 << 20
SCENE = 1 << 19
GUARDS = 1 << 16

DRIVER = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include "cugs_blend_cull.h"

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t next64() {                                   // splitmix64
    uint64_t z = (g_s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }          // [0, 1)
static double uni(double lo, double hi) { return lo + (hi - lo) * uni(); }
static int below(int n) { return (int)(next64() % (uint64_t)n); }
static double gauss() { return std::sqrt(-2.0 * std::log(1.0 - uni())) * std::cos(6.283185307179586 * uni()); }
static float ulps(float x, int k) {
    for (; k > 0; --k) x = std::nextafterf(x, INFINITY);
    for (; k < 0; ++k) x = std::nextafterf(x, -INFINITY);
    return x;
}

static float clamp3(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
// the formula cugs_blend_cull.h replaces, with plain stand-ins for v_rcp_f32, v_med3_f32 and v_max_f32
static bool prev_may_touch(float mx, float my, float a, float b, float c, float tau, float qx0, float qy0, float wx,
                           float wy) {
    if (!(tau >= 0.0f)) return false;
    if (!(a > 0.0f && c > 0.0f)) return true;
    const float ia = 1.0f / a, ic = 1.0f / c;
    const float lx = qx0 - mx, hx = lx + wx, ly = qy0 - my, hy = ly + wy;
    const bool inside = (lx <= 0.0f) && (hx >= 0.0f) && (ly <= 0.0f) && (hy >= 0.0f);
    const float X = fmaxf(-lx, hx), Y = fmaxf(-ly, hy);
    const float B = a * X * X + 2.0f * fabsf(b) * X * Y + c * Y * Y;
    const float b2 = b + b;
    const float xe = (lx > 0.0f) ? lx : hx, ye = (ly > 0.0f) ? ly : hy;
    const float yv = clamp3(-b * xe * ic, ly, hy);
    const float xv = clamp3(-b * ye * ia, lx, hx);
    const float qx = a * xe * xe + b2 * xe * yv + c * yv * yv;
    const float qy = a * xv * xv + b2 * xv * ye + c * ye * ye;
    const bool out_x = !((lx <= 0.0f) && (hx >= 0.0f)), out_y = !((ly <= 0.0f) && (hy >= 0.0f));
    const float qmin = inside ? 0.0f : fminf(out_x ? qx : 3.0e38f, out_y ? qy : 3.0e38f);
    return !(0.5f * qmin > tau * 1.01f + 0.05f + 4e-6f * B);
}

struct Case { float mx, my, a, b, c, tau; int tile_x, tile_y, x0, y0, wx, wy; };    // x0, y0: first pixel of the rectangle

static float tau_of(float o) { return (o >= (1.0f / 255.0f)) ? logf(255.0f * o) : -1.0f; }     // as write_packed
static bool staged_may_touch(const Case& k) {
    const float lim = cugs_cull_limit(k.mx, k.my, k.a, k.b, k.c, k.tau, (float)(k.tile_x + 8), (float)(k.tile_y + 8));
    return cugs_cull_may_touch(k.mx, k.my, k.a, k.b, k.c, lim, (float)k.x0 + 0.5f, (float)k.y0 + 0.5f, (float)k.wx,
                               (float)k.wy);
}
static bool prev_of(const Case& k) {
    return prev_may_touch(k.mx, k.my, k.a, k.b, k.c, k.tau, (float)k.x0 + 0.5f, (float)k.y0 + 0.5f, (float)k.wx,
                          (float)k.wy);
}
// brute force: does any pixel centre of the rectangle have q/2 <= tau, in double
static bool truth(const Case& k) {
    if (!(k.tau >= 0.0f)) return false;
    for (int y = k.y0; y <= k.y0 + k.wy; ++y)
        for (int x = k.x0; x <= k.x0 + k.wx; ++x) {
            const double dx = (double)x + 0.5 - (double)k.mx, dy = (double)y + 0.5 - (double)k.my;
            const double q = (double)k.a * dx * dx + 2.0 * (double)k.b * dx * dy + (double)k.c * dy * dy;
            if (0.5 * q <= (double)k.tau) return true;
        }
    return false;
}

// tile (origin 0, 1904 or 4000 per axis), quad of the tile, rectangle of size (i % 8 + 1) x (i / 8 % 8 + 1) inside the quad
static void place(Case& k, long i) {
    static const int org[3] = {0, 1904, 4000};
    k.tile_x = org[below(3)]; k.tile_y = org[below(3)];
    k.wx = (int)(i % 8); k.wy = (int)((i / 8) % 8);
    k.x0 = k.tile_x + 8 * below(2) + below(8 - k.wx);
    k.y0 = k.tile_y + 8 * below(2) + below(8 - k.wy);
}

static void adversarial(Case& k, long i) {
    place(k, i);
    const double l1 = std::pow(10.0, uni(-5.0, std::log10(3.3)));
    double kappa = std::pow(10.0, uni(0.0, 6.0));
    if (uni() < 0.3) kappa = std::pow(10.0, uni(4.0, 6.0));
    const double l2 = std::fmax(l1 / kappa, 1e-7);
    const double th = uni(0.0, 3.141592653589793), cs = std::cos(th), sn = std::sin(th);
    k.a = (float)(l1 * cs * cs + l2 * sn * sn);
    k.b = (float)((l1 - l2) * sn * cs);
    k.c = (float)(l1 * sn * sn + l2 * cs * cs);
    const float lo = 1.0f / 255.0f;
    float o;
    switch (below(6)) {
        case 0: o = lo; break;
        case 1: o = ulps(lo, 1 + below(15)); break;
        case 2: o = (float)((double)lo * (1.0 + std::pow(10.0, uni(-6.0, -1.0)))); break;
        case 3: o = (float)uni((double)lo, 0.99); break;
        case 4: o = (float)uni(0.98, 1.0); break;
        default: o = (below(2) ? ulps(lo, -1 - below(15)) : (float)uni(0.0, (double)lo)); break;     // below 1/255: tau = -1
    }
    k.tau = tau_of(o);
    const int fam = below(5);
    if (fam <= 2) {                                           // on the alpha = 1/255 contour of a pixel of the rectangle
        const double pcx = k.x0 + below(k.wx + 1) + 0.5, pcy = k.y0 + below(k.wy + 1) + 0.5;
        const double u = uni(0.0, 6.283185307179586), ux = std::cos(u), uy = std::sin(u);
        const double qf = (double)k.a * ux * ux + 2.0 * (double)k.b * ux * uy + (double)k.c * uy * uy;
        const double delta = uni() < 0.2 ? 0.0 : uni(-1e-3, 1e-3);
        const double t = std::sqrt(std::fmax(2.0 * std::fmax((double)k.tau, 0.0) * (1.0 + delta), 0.0) / std::fmax(qf, 1e-30));
        k.mx = (float)(pcx - t * ux); k.my = (float)(pcy - t * uy);
    } else if (fam == 3) {                                    // a few ulp off an edge of the rectangle
        const float ex = (float)(below(2) ? k.x0 : k.x0 + k.wx) + 0.5f, ey = (float)(below(2) ? k.y0 : k.y0 + k.wy) + 0.5f;
        k.mx = ulps(ex, below(9) - 4);
        k.my = below(2) ? ulps(ey, below(9) - 4) : (float)(k.y0 + uni(-20.0, 28.0));
    } else {                                                  // anywhere around the quad
        const double sig = std::fmin(1.0 / std::sqrt(std::fmin(l2, 3.3)), 4000.0);
        k.mx = (float)(k.x0 + 4.0 + gauss() * sig); k.my = (float)(k.y0 + 4.0 + gauss() * sig);
    }
}

static void scene_like(Case& k, long i) {
    place(k, i);
    const double z = uni(2.0, 10.0), f = 1497.6;
    const double s1 = f * std::exp(-4.6 + 0.5 * gauss()) / z, s2 = f * std::exp(-4.6 + 0.5 * gauss()) / z;
    const double th = uni(0.0, 3.141592653589793), cs = std::cos(th), sn = std::sin(th);
    const double cxx = s1 * s1 * cs * cs + s2 * s2 * sn * sn + 0.3, cyy = s1 * s1 * sn * sn + s2 * s2 * cs * cs + 0.3;
    const double cxy = (s1 * s1 - s2 * s2) * sn * cs, det = cxx * cyy - cxy * cxy;
    k.a = (float)(cyy / det); k.b = (float)(-cxy / det); k.c = (float)(cxx / det);
    k.tau = tau_of((float)(1.0 / (1.0 + std::exp(-gauss()))));
    const double rx = std::ceil(3.0 * std::sqrt(cxx)), ry = std::ceil(3.0 * std::sqrt(cyy));      // the binning's box
    k.mx = (float)uni(k.tile_x - rx, k.tile_x + 16.0 + rx);
    k.my = (float)uni(k.tile_y - ry, k.tile_y + 16.0 + ry);
}

int main(int argc, char** argv) {
    const long n_adv = atol(argv[1]), n_scene = atol(argv[2]), n_guard = atol(argv[3]);
    long cases = 0, real = 0, touched = 0, kept = 0, lost = 0, prev_kept = 0, prev_lost_now = 0;
    long scene_prev_kept = 0, scene_extra = 0, scene_kept = 0;
    long guard_culled = 0, guard_neg_kept = 0, guards = 0;
    for (int fam = 0; fam < 2; ++fam) {
        const long n = fam ? n_scene : n_adv;
        for (long i = 0; i < n; ++i) {
            Case k;
            if (fam) scene_like(k, i); else adversarial(k, i);
            ++cases;
            const bool conic = (double)k.a * (double)k.c - (double)k.b * (double)k.b > 0.0 && k.a > 0.0f && k.c > 0.0f;
            const bool now = staged_may_touch(k), prev = prev_of(k);
            if (conic) {                                                        // (a)
                ++real;
                const bool t = truth(k);
                touched += t; kept += now;
                if (t && !now) {
                    if (++lost <= 5) fprintf(stderr, "lost: %a %a %a %a %a tau %a rect %d %d %d %d tile %d %d\n", k.mx, k.my, k.a, k.b, k.c, k.tau, k.x0, k.y0, k.wx, k.wy, k.tile_x, k.tile_y);
                }
            }
            prev_kept += prev;                                                  // (b)
            if (prev && !now) {
                if (++prev_lost_now <= 5) fprintf(stderr, "kept before: %a %a %a %a %a tau %a rect %d %d %d %d tile %d %d\n", k.mx, k.my, k.a, k.b, k.c, k.tau, k.x0, k.y0, k.wx, k.wy, k.tile_x, k.tile_y);
            }
            if (fam) { scene_prev_kept += prev; scene_kept += now; scene_extra += (now && !prev); }      // (c)
        }
    }
    for (long i = 0; i < n_guard; ++i) {                                        // (d)
        Case k;
        if (i & 1) scene_like(k, i); else adversarial(k, i);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        Case g = k;
        if (!(g.tau >= 0.0f)) g.tau = (float)uni(0.0, 5.5);
        switch (i % 6) {
            case 0: g.a = 0.0f; break;
            case 1: g.a = -g.a; break;
            case 2: g.c = 0.0f; break;
            case 3: g.c = -g.c; break;
            case 4: g.mx = nan; break;
            default: g.my = nan; if (i % 12 == 5) g.mx = nan; break;
        }
        ++guards;
        guard_culled += !staged_may_touch(g);
        Case m = k;                                                             // tau < 0 (and a NaN tau): always culled
        m.tau = (i % 5 == 0) ? nan : (i % 5 == 1) ? -1.0f : (float)-uni(1e-30, 10.0);
        if (i % 7 == 0) m.mx = nan;
        if (i % 11 == 0) m.a = -m.a;
        guard_neg_kept += staged_may_touch(m);
    }
    printf("{\"cases\": %ld, \"real\": %ld, \"touched\": %ld, \"kept\": %ld, \"lost\": %ld, \"prev_kept\": %ld, "
           "\"prev_lost_now\": %ld, \"scene_prev_kept\": %ld, \"scene_kept\": %ld, \"scene_extra\": %ld, \"guards\": %ld, "
           "\"guard_culled\": %ld, \"guard_neg_kept\": %ld}\n",
           cases, real, touched, kept, lost, prev_kept, prev_lost_now, scene_prev_kept, scene_kept, scene_extra, guards,
           guard_culled, guard_neg_kept);
    return 0;
}
"""


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    tmp = tmp_path_factory.mktemp("cull_host")
    src, exe = tmp / "cull.cpp", tmp / "cull"
    src.write_text(DRIVER)
    # -ffp-contract=off: the products and sums round one by one, as the device build's do
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe),
                    str(src)], check=True)
    res = subprocess.run([str(exe), str(ADVERSARIAL), str(SCENE), str(GUARDS)], check=True, timeout=120,
                         capture_output=True, text=True)
    print(res.stderr, res.stdout)
    return json.loads(res.stdout)


def test_enough_cases_and_both_outcomes(counts):
    c = counts
    assert c["cases"] >= 1_000_000 and c["real"] > 0.95 * c["cases"]
    # not vacuous: many records touch, many are culled, and the margin is met from both sides
    assert c["touched"] > 0.2 * c["real"]
    assert c["real"] - c["kept"] > 0.1 * c["real"]
    assert c["kept"] > c["touched"]


def test_never_culled_when_a_pixel_centre_passes_in_double(counts):
    assert counts["lost"] == 0


def test_every_record_the_previous_formula_keeps_is_kept(counts):
    assert counts["prev_kept"] > 0.2 * counts["cases"]
    assert counts["prev_lost_now"] == 0


def test_tile_wide_slack_adds_at_most_a_thousandth_on_scene_like_records(counts):
    c = counts
    assert c["scene_prev_kept"] > 10_000 and c["scene_kept"] < 0.9 * SCENE
    print(f"scene-like: {c['scene_extra']} kept beyond the previous formula's {c['scene_prev_kept']} "
          f"({c['scene_extra'] / c['scene_prev_kept']:.2e})")
    assert c["scene_extra"] <= 1e-3 * c["scene_prev_kept"]


def test_guards(counts):
    assert counts["guards"] == GUARDS
    assert counts["guard_culled"] == 0          # a <= 0, c <= 0, NaN mean: never culled
    assert counts["guard_neg_kept"] == 0        # tau < 0 or NaN: always culled
