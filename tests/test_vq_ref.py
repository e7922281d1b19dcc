"""tests/vq_ref.py, the numpy mirror of the vector-quantisation kernels, checked on its own (no GPU): its float32 fmaf
against libm's bit for bit, its assignment against an fp64 brute force within the error bound of an fp32 chain, and the
monotone distortion of its Lloyd iterations."""
import ctypes as C
import ctypes.util

import numpy as np

import vq_ref as vr

F32, F64 = np.float32, np.float64


def _libm_fmaf():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
    return libm.fmaf


def _same_bits(a, b, c):
    fmaf = _libm_fmaf()
    a, b, c = (np.ascontiguousarray(v, F32) for v in (a, b, c))
    want = np.array([fmaf(float(p), float(q), float(r)) for p, q, r in zip(a, b, c)], F32)
    got = vr.fma32(a, b, c)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad[:5], a[bad[:5]], b[bad[:5]], c[bad[:5]], got[bad[:5]], want[bad[:5]])


def _rng(key):
    return np.random.Generator(np.random.Philox(key=key))


def test_fma32_equals_libm_on_random_triples():
    rng = _rng(2701)
    n = 20000
    spread = lambda: (rng.standard_normal(n) * np.exp2(rng.integers(-20, 21, n))).astype(F32)
    _same_bits(spread(), spread(), spread())
    _same_bits(rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n))
    tiny = lambda: (rng.standard_normal(n) * np.exp2(rng.integers(-75, -55, n))).astype(F32)    # subnormal results
    _same_bits(tiny(), tiny(), tiny() * F32(2.0 ** -60))


def test_fma32_equals_libm_where_the_sum_cancels():
    rng = _rng(2702)
    n = 20000
    a, b = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    c = -(a.astype(F64) * b.astype(F64)).astype(F32)              # c = -fl(a b): the sum is the product's rounding error
    _same_bits(a, b, c)
    ulps = rng.integers(-3, 4, n)
    _same_bits(a, b, (c.view(np.int32) + ulps.astype(np.int32)).view(F32))


def test_fma32_equals_libm_on_half_ulp_cases():
    """a = 1 + i 2^-12, b = 1 + j 2^-12 with odd i, j: a b = 1 + (i + j) 2^-12 + i j 2^-24 ends in the 2^-24 bit, exactly
    half an ulp of [1, 2); c of any size below breaks the tie, and a float64 sum loses a c below 2^-53."""
    rng = _rng(2703)
    n = 20000
    i, j = 2 * rng.integers(0, 1024, n) + 1, 2 * rng.integers(0, 1024, n) + 1
    a, b = (1.0 + i * 2.0 ** -12).astype(F32), (1.0 + j * 2.0 ** -12).astype(F32)
    assert np.all(a.astype(F64) * b.astype(F64) != (a.astype(F64) * b.astype(F64)).astype(F32))   # inexact in fp32
    sign = np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
    for e in (-30, -52, -53, -54, -60, -100, -140):
        _same_bits(a, b, (sign * 2.0 ** e).astype(F32))
    _same_bits(a, b, np.zeros(n, F32))                            # the tie itself: to even
    scale = np.exp2(rng.integers(-40, 41, n)).astype(F32)         # the same in other binades
    _same_bits(a * scale, b, (sign * 2.0 ** -70).astype(F32) * scale)
    _same_bits(-a, b, (sign * 2.0 ** -60).astype(F32))


def test_mirror_assign_is_within_the_chain_bound_of_an_fp64_search():
    """The chosen code's fp64 score exceeds the fp64 minimum by at most the error bounds of the two fp32 scores
    compared: (d + 3) 2^-24 (h_j + sum_t |x_t c_jt|) each, the bound of a length-d fmaf chain, the product by 0.5 and
    the subtraction."""
    for key, (n, k, d) in enumerate([(200, 37, 45), (64, 50, 9), (150, 300, 24), (40, 7, 1)]):
        rng = _rng(2710 + key)
        x = rng.standard_normal((n, d)).astype(F32)
        cb = (x[rng.integers(0, n, k)] + 0.05 * rng.standard_normal((k, d))).astype(F32)   # near codes: close calls
        got, dist = vr.mirror_assign(x, cb, return_dist=True)
        x64, c64 = x.astype(F64), cb.astype(F64)
        h = 0.5 * np.sum(c64 * c64, axis=1)
        score = h[None, :] - x64 @ c64.T
        bound = (d + 3) * 2.0 ** -24 * (h[None, :] + np.abs(x64) @ np.abs(c64).T)
        best = np.argmin(score, axis=1)
        rows = np.arange(n)
        assert np.all(score[rows, got] - score[rows, best] <= bound[rows, got] + bound[rows, best])
        exact = np.sum((x64 - c64[got]) ** 2, axis=1)
        assert np.all(np.abs(dist.astype(F64) - exact) <= (d + 3) * 2.0 ** -24 * exact + 1e-40)


def test_mirror_assign_ties_and_nan():
    rng = _rng(2720)
    x = rng.standard_normal((30, 9)).astype(F32)
    cb = rng.standard_normal((12, 9)).astype(F32)
    cb[2] = cb[7] = cb[11] = x[4]
    x[9] = x[4]
    x[5, 3] = np.nan
    got = vr.mirror_assign(x, cb)
    assert got[4] == 2 and got[9] == 2 and got[5] == 0
    clean = x.copy()
    clean[5] = 0.0
    assert np.array_equal(np.delete(got, 5), np.delete(vr.mirror_assign(clean, cb), 5))
    assert vr.mirror_assign(np.full((2, 3), np.nan, F32), cb[:, :3]).tolist() == [0, 0]


def test_mirror_update_rules():
    rng = _rng(2730)
    x = rng.standard_normal((50, 6)).astype(F32)
    cb = rng.standard_normal((5, 6)).astype(F32)
    assign = rng.integers(0, 4, 50).astype(np.int32)              # code 4 stays empty
    assign[:3] = -1
    assign[3] = 5                                                 # outside [0, k): skipped as well
    w = rng.uniform(0.0, 2.0, 50).astype(F32)
    w[assign == 3] = 0.0                                          # members without weight: the code keeps its bits
    new, counts = vr.mirror_update(x, assign, cb, 40, w)
    assert np.array_equal(new[4].view(np.uint32), cb[4].view(np.uint32))
    assert np.array_equal(new[3].view(np.uint32), cb[3].view(np.uint32))
    assert counts.tolist() == [int(np.sum(assign == j)) for j in range(5)] and counts[4] == 0
    for j in range(3):
        m = assign == j
        mean = (w[m, None].astype(F64) * x[m]).sum(0) / w[m].astype(F64).sum()
        assert np.max(np.abs(new[j] - mean)) <= 1e-6 * (1.0 + np.max(np.abs(mean)))
    plain, _ = vr.mirror_update(x, assign, cb, 40)
    assert np.max(np.abs(plain[0] - x[assign == 0].astype(F64).mean(0))) <= 1e-6


def test_mirror_fit_never_raises_the_distortion():
    """Neither step of a Lloyd iteration can raise sum w |x - c_a|^2; the margin of 1e-5 sum w |x|^2 covers the fp32
    rounding of the centroids and of the scores."""
    for key, weighted in ((2740, False), (2741, True)):
        rng = _rng(key)
        n, k, d = 600, 40, 24
        centres = rng.standard_normal((12, d))
        x = (centres[rng.integers(0, 12, n)] + 0.3 * rng.standard_normal((n, d))).astype(F32)
        w = rng.uniform(0.0, 3.0, n).astype(F32) if weighted else None
        w64 = np.ones(n) if w is None else w.astype(F64)
        margin = 1e-5 * float(np.sum(w64 * np.sum(x.astype(F64) ** 2, axis=1)))
        distortion = lambda cb, a: float(np.sum(w64 * np.sum((x.astype(F64) - cb.astype(F64)[a]) ** 2, axis=1)))
        bits = vr.frac_bits_for(n, float(np.max(np.abs(x))), 1.0 if w is None else float(w.max()))
        cb = x[(np.arange(k) * n) // k].copy()
        last = np.inf
        for _ in range(6):
            a = vr.mirror_assign(x, cb)
            now = distortion(cb, a)
            assert now <= last + margin
            cb, _ = vr.mirror_update(x, a, cb, bits, w)
            after = distortion(cb, a)
            assert after <= now + margin
            last = after
        got_cb, got_a, got_counts = vr.mirror_fit(x, k, iters=6, weights=w)
        assert np.array_equal(got_cb.view(np.uint32), cb.view(np.uint32))
        assert np.array_equal(got_a, vr.mirror_assign(x, cb)) and got_counts.sum() == n


def test_mirror_fit_takes_at_most_n_codes_and_an_init():
    rng = _rng(2750)
    x = rng.standard_normal((5, 3)).astype(F32)
    cb, a, counts = vr.mirror_fit(x, 9, iters=2)
    assert cb.shape == (5, 3) and np.array_equal(cb, x) and a.tolist() == [0, 1, 2, 3, 4] and counts.tolist() == [1] * 5
    init = x[[3, 1]].copy()
    cb, a, _ = vr.mirror_fit(x, 2, iters=0, init=init)
    assert np.array_equal(cb, init) and a[3] == 0 and a[1] == 1
