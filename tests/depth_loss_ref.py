"""CPU reference for the depth-supervision loss (csrc/depth_loss.hip, cugs_amd.depth_loss): a numpy
float32 mirror of the definition in include/cugs_hip.h, op for op - every float step one correctly rounded numpy
operation, the sums in float64.

  make_case(h, w, inverse)   D, A, t, w (float32 [h,w]) with hand-placed pixels for every clause of "valid"
  fit(...)                   the five fp64 sums over the valid pixels and the 2x2 solve -> (s, b, fit_ok), unrounded
  reference(...)             dL/dD, dL/dA, expected (float32, the bytes the kernel must give) and the fp64 sums of the
                             loss at a given float32 (s, b)

The kernel's fp64 sums take another order than numpy's; both are within ~2^-53 n relative of the exact sum, far below
half a float32 ulp, so after the final rounding to float32 the loss, the weight sum and (with the conditioning asserted
in make_case) the fitted s, b differ by at most one ulp - the argument of metrics_ref.exact.

Shared by tests/test_depth_loss_ref.py (CPU) and the GPU tests; callers must not modify a case's arrays."""
import numpy as np

F = np.float32
MIN_ALPHA = 1e-3

# (h, w): 35 pixels, a scalar tail of 3 | one full workgroup's quarter | 1961 pixels: two workgroups, tail of 1 |
# four full workgroups | 264 workgroups: more rows of partials than the finalize kernels have threads (256), so the
# strided sum and the tree both run
SHAPES = [(7, 5), (16, 16), (37, 53), (64, 64), (540, 500)]
CHUNK = 1024                         # pixels per workgroup = per row of partials (depth_loss.hip)

# flat indices of the hand-placed pixels (all other quantities of such a pixel are valid ones)
P_BELOW, P_EQUAL, P_ABOVE, P_NAN, P_INF, P_NEG, P_D0 = 0, 1, 2, 5, 9, 13, 17
# P_EXACT = h*w - 1: x == t exactly (sgn = 0 without alignment), inside the scalar tail where there is one


def expected_depth(D, A, t, w, inverse, min_alpha=MIN_ALPHA):
    """(valid, x, divisor with 1 where invalid)."""
    valid = (A > F(min_alpha)) & (w > 0) & (t > 0) & (t < np.inf)
    if inverse:
        valid &= D > 0
    num, den = (A, D) if inverse else (D, A)
    den = np.where(valid, den, F(1.0)).astype(F)
    x = np.where(valid, (num / den).astype(F), F(0.0)).astype(F)
    return valid, x, den


def make_case(h, w, inverse):
    """dict(D, A, t, w: float32 [h,w]; inverse; h, width; exact: the flat index of the x == t pixel).  A uniform with
    ~10 % exact zeros, D = A z with z in [2, 8], t an affine distortion of z plus noise (inverse: its reciprocal) with
    ~10 % zeros, w uniform with ~15 % zeros, and the hand-placed pixels above."""
    rng = np.random.default_rng(h * 100003 + w * 17 + int(inverse))
    n = h * w
    z = rng.uniform(2.0, 8.0, n).astype(F)
    A = rng.uniform(0.05, 1.0, n).astype(F)
    A[rng.random(n) < 0.10] = 0.0
    t = (F(0.7) * z + F(0.5) + rng.normal(0.0, 0.1, n).astype(F)).astype(F)      # affine distortion of z plus noise
    if inverse:
        t = (F(1.0) / t).astype(F)
    t[rng.random(n) < 0.10] = 0.0
    wt = rng.uniform(0.1, 1.0, n).astype(F)
    wt[rng.random(n) < 0.15] = 0.0
    hand = [P_BELOW, P_EQUAL, P_ABOVE, P_NAN, P_INF, P_NEG, P_D0, n - 1]
    for p in hand:                                                              # valid in every respect ...
        A[p], wt[p], t[p] = F(0.5), F(0.75), (F(1.0) / F(4.0) if inverse else F(4.0))
    A[P_BELOW] = np.nextafter(F(MIN_ALPHA), F(0.0))                             # ... but the one under test
    A[P_EQUAL] = F(MIN_ALPHA)
    A[P_ABOVE] = np.nextafter(F(MIN_ALPHA), F(1.0))
    D = (A * z).astype(F)
    t[P_NAN], t[P_INF], t[P_NEG] = np.nan, np.inf, F(-1.0)
    D[P_D0] = 0.0                                                               # depth space: x = 0; inverse: invalid
    with np.errstate(all="ignore"):
        t[n - 1] = (A[n - 1] / D[n - 1]) if inverse else (D[n - 1] / A[n - 1])  # x == t: sgn = 0, still counted
        valid, x, _ = expected_depth(D, A, t, wt, inverse)
    case = dict(D=D.reshape(h, w), A=A.reshape(h, w), t=t.reshape(h, w), w=wt.reshape(h, w), inverse=bool(inverse),
                h=h, width=w, exact=n - 1)
    # the conditions every case must meet (a prototype of this recipe gave 0.64-0.74 and 0.05-0.08)
    for weighted in (False, True):
        f = fit(case, weighted)
        assert f["valid_fraction"] >= 0.5, (h, w, inverse, f["valid_fraction"])
        assert f["fit_ok"] and f["relvar"] >= 0.02, (h, w, inverse, f["relvar"])
    assert valid[n - 1] and not valid[P_BELOW] and not valid[P_EQUAL] and valid[P_ABOVE]
    assert not (valid[P_NAN] or valid[P_INF] or valid[P_NEG]) and valid[P_D0] == (not inverse)
    return case


def _weight(case, weighted):
    return case["w"] if weighted else np.ones_like(case["A"])


def fit(case, weighted, target=None, min_alpha=MIN_ALPHA):
    """min sum_valid w (s t + b - x)^2 from the five fp64 sums (terms formed in double from the float values), by
    Cramer's rule as k_depth_fit: dict(s, b as float64, fit_ok, relvar = det / (Sw Stt), n_valid, valid_fraction)."""
    t = case["t"] if target is None else target
    wt = _weight(case, weighted)
    with np.errstate(all="ignore"):
        valid, x, _ = expected_depth(case["D"], case["A"], t, wt, case["inverse"], min_alpha)
    wd, td, xd = (a[valid].astype(np.float64) for a in (wt, t, x))
    wtd = wd * td
    Sw, St, Sx, Stt, Stx = wd.sum(), wtd.sum(), (wd * xd).sum(), (wtd * td).sum(), (wtd * xd).sum()
    det = Sw * Stt - St * St
    n_valid = int(valid.sum())
    ok = n_valid >= 2 and det > 1e-12 * Sw * Stt
    s, b = ((Sw * Stx - St * Sx) / det, (Stt * Sx - St * Stx) / det) if ok else (1.0, 0.0)
    return dict(s=float(s), b=float(b), fit_ok=bool(ok), relvar=float(det / (Sw * Stt)) if Sw * Stt > 0 else 0.0,
                n_valid=n_valid, valid_fraction=n_valid / valid.size)


def reference(case, weighted, s=1.0, b=0.0, target=None, min_alpha=MIN_ALPHA):
    """The definition at the float32 (s, b): dict(gD, gA, expected: float32 [h,w]; valid; n_valid; loss64 and sw64 the
    unrounded float64 results, loss and sw their float32 roundings)."""
    D, A = case["D"], case["A"]
    t = case["t"] if target is None else target
    wt = _weight(case, weighted)
    n = D.size
    with np.errstate(all="ignore"):
        valid, x, den = expected_depth(D, A, t, wt, case["inverse"], min_alpha)
        tp = ((F(s) * t).astype(F) + F(b)).astype(F)                            # two roundings
        r = (x - tp).astype(F)
        sgn = np.where(r > 0, F(1.0), np.where(r < 0, F(-1.0), F(0.0))).astype(F)
        inv_n = F(1.0) / F(n)
        gx = ((wt * sgn).astype(F) * inv_n).astype(F)
        direct = (gx / den).astype(F)
        through = (-(((gx * x).astype(F) / den).astype(F))).astype(F)
        g_num, g_den = np.where(valid, direct, F(0.0)).astype(F), np.where(valid, through, F(0.0)).astype(F)
        term = (wt * np.abs(r)).astype(F)
    gD, gA = (g_den, g_num) if case["inverse"] else (g_num, g_den)
    loss64 = float(term[valid].astype(np.float64).sum() / float(n))
    sw64 = float(wt[valid].astype(np.float64).sum())
    return dict(gD=gD, gA=gA, expected=x, valid=valid, n_valid=int(valid.sum()), loss64=loss64, loss=F(loss64),
                sw64=sw64, sw=F(sw64), r=r)


_cases = {}


def case(h, w, inverse):
    """make_case, built once per (shape, space) and shared."""
    key = (h, w, bool(inverse))
    if key not in _cases:
        _cases[key] = make_case(h, w, inverse)
    return _cases[key]


def ulp_distance(a, b):
    """Steps between two finite float32 values (through zero too)."""
    def key(v):
        i = int(np.float32(v).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))
