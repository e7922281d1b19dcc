"""The numpy mirror of csrc/vq.hip (arithmetic: include/cugs_hip.h): an exact float32 fmaf, the assignment with its
lowest-index and NaN rules, the int64 fixed-point update, and the fit loop of compress.vq_fit."""
import math

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, bit for bit.  The product of two float32 is exact in float64; the sum with c is
    taken with TwoSum, and where it is inexact the float64 sum is replaced by the neighbour - on the side of the error -
    whose last bit is odd (round to odd), so that the final rounding to float32 sees on which side of a float32
    half-way point the exact value lies.  A plain float64 evaluation rounds twice and gets those cases wrong.
    Only a sum that sits exactly on such a half-way point (or below the normal float32 range, where the half-way points
    are coarser) can be changed by this, so only those elements take the slow path."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        p = a.astype(F64) * b.astype(F64)
        s = np.atleast_1d(p + c.astype(F64))
        r = s.astype(F32)
        low = s.view(I64) & I64(0x1FFFFFFF)
        sus = ((low == I64(0x10000000)) | (np.abs(s) < 2.0 ** -126)) & np.isfinite(s)
        if sus.any():
            ps, cs, ss = np.atleast_1d(p)[sus], np.atleast_1d(c.astype(F64))[sus], s[sus]
            bb = ss - ps
            err = (ps - (ss - bb)) + (cs - bb)                    # TwoSum: ps + cs = ss + err exactly
            bits = ss.view(I64).copy()
            fix = (err != 0.0) & ((bits & 1) == 0)
            away = (err > 0.0) == (ss > 0.0)                      # the exact value is larger in magnitude than ss
            bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
            r[sus] = bits.view(F64).astype(F32)
    return r.reshape(np.shape(p))


def mirror_half_norms(codebook):
    """h[j] = 0.5f * the ascending fmaf chain of c[j,t]^2."""
    cb = np.asarray(codebook, F32)
    acc = np.zeros(cb.shape[0], F32)
    for t in range(cb.shape[1]):
        acc = fma32(cb[:, t], cb[:, t], acc)
    return F32(0.5) * acc


def mirror_scores(x, codebook, block=256):
    """score[i,j] = h[j] - dot(i,j), dot the ascending fmaf chain from 0."""
    x, cb = np.asarray(x, F32), np.asarray(codebook, F32)
    h = mirror_half_norms(cb)
    out = np.empty((x.shape[0], cb.shape[0]), F32)
    with np.errstate(all="ignore"):
        for r0 in range(0, x.shape[0], block):
            xb = x[r0:r0 + block]
            acc = np.zeros((xb.shape[0], cb.shape[0]), F32)
            for t in range(x.shape[1]):
                acc = fma32(xb[:, t, None], cb[None, :, t], acc)
            out[r0:r0 + block] = h[None, :] - acc
    return out


def mirror_assign(x, codebook, return_dist=False):
    """The strict-< running best from (+inf, 0): the first index of the smallest non-NaN score, 0 where there is none.
    dist: acc = acc + (x - c)^2 ascending, every operation in float32."""
    x, cb = np.asarray(x, F32), np.asarray(codebook, F32)
    sc = mirror_scores(x, cb)
    sc = np.where(np.isnan(sc), F32(np.inf), sc)
    assign = np.argmin(sc, axis=1).astype(np.int32)               # the first minimum; all +inf gives 0
    if not return_dist:
        return assign
    acc = np.zeros(x.shape[0], F32)
    with np.errstate(all="ignore"):
        for t in range(x.shape[1]):
            df = x[:, t] - cb[assign, t]
            acc = acc + df * df
    return assign, acc


def mirror_update(x, assign, codebook, frac_bits, weights=None):
    """(new codebook, counts): int64 sums of rint(w x 2^F) and rint(w 2^F), one float64 division per element where the
    denominator is positive; rows with assign outside [0, k) are left out."""
    x, cb = np.asarray(x, F32), np.asarray(codebook, F32)
    k = cb.shape[0]
    assign = np.asarray(assign)
    valid = (assign >= 0) & (assign < k)
    w = np.ones(x.shape[0], F64) if weights is None else np.asarray(weights, F32).astype(F64)
    scale = 2.0 ** int(frac_bits)
    vx = np.rint(w[:, None] * x.astype(F64) * scale).astype(I64)
    vw = np.rint(w * scale).astype(I64)
    num, den = np.zeros(cb.shape, I64), np.zeros(k, I64)
    np.add.at(num, assign[valid], vx[valid])
    np.add.at(den, assign[valid], vw[valid])
    counts = np.bincount(assign[valid], minlength=k).astype(np.int32)
    new = cb.copy()
    m = den > 0
    new[m] = (num[m].astype(F64) / den[m, None].astype(F64)).astype(F32)
    return new, counts


def frac_bits_for(n, x_max, w_max=1.0):
    """61 minus the binary exponents of n and of max(w_max x_max, w_max), at most 62 (the rule of compress.vq_frac_bits,
    restated)."""
    big = max(float(w_max) * float(x_max), float(w_max))
    if big <= 0.0:
        return 62
    return min(61 - math.frexp(float(max(n, 1)))[1] - math.frexp(big)[1], 62)


def mirror_fit(x, k, iters=10, weights=None, init=None):
    """(codebook [k', d], indices [n], counts [k']) as compress.vq_fit: first codebook init or the rows (j n) // k'."""
    x = np.asarray(x, F32)
    n = x.shape[0]
    kk = min(int(k), n)
    cb = np.asarray(init, F32).copy() if init is not None else x[(np.arange(kk, dtype=I64) * n) // kk].copy()
    w_max = 1.0 if weights is None else float(np.max(np.asarray(weights, F32)))
    bits = frac_bits_for(n, float(np.max(np.abs(x))), w_max)
    for _ in range(int(iters)):
        cb, _ = mirror_update(x, mirror_assign(x, cb), cb, bits, weights)
    assign = mirror_assign(x, cb)
    return cb, assign, np.bincount(assign, minlength=kk).astype(np.int32)
