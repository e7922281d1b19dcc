"""numpy restatement of the reference's MCMC densification (optimizer/mcmc_densification.cpp) with the boundary
differences of DESIGN §4.12: the counter-based Philox4x32-10 + Box-Muller draws instead of torch's generator, and
sampling weights quantised to 2^-24.  Sigmoid and exp come from the oracle's cugs_expf (orc.expf), so dead
classification, weights and gates match the device exactly.  Test infrastructure (not collected by pytest)."""
from __future__ import annotations

import numpy as np

f32 = np.float32
STREAM_NOISE, STREAM_JITTER, STREAM_SAMPLE = 0, 1, 2
LOG_TEN = f32(np.log(f32(10.0)))                       # std::log(10.0f)
LOW_OPACITY = f32(np.log(f32(0.01) / f32(0.99)))       # std::log(0.01f / 0.99f)
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 (Random123 constants); arguments are uint32 scalars or arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & _M32, (p0 >> s32) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return np.stack([x.astype(np.uint32) for x in c], axis=-1)


def bits(seed: int, stream_id: int, step: int, index) -> np.ndarray:
    """[..., 4] uint32: the words of the draw at counter (index_lo, index_hi, stream_id, step), key seed."""
    idx = np.asarray(index, dtype=np.uint64)
    return philox4x32_10(idx & _M32, idx >> np.uint64(32), np.uint32(stream_id & 0xFFFFFFFF),
                         np.uint32(step & 0xFFFFFFFF), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def uniform(x) -> np.ndarray:
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24


def normals_from_words(w: np.ndarray) -> np.ndarray:
    """Box-Muller on (w0, w1) and (w2, w3), the first three normals (float64, rounded once to float32)."""
    u0, u1, u2, u3 = (uniform(w[..., k]) for k in range(4))
    r0, r1 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    out = np.stack([r0 * np.cos(2 * np.pi * u1), r0 * np.sin(2 * np.pi * u1), r1 * np.cos(2 * np.pi * u3)], -1)
    return out.astype(f32)


def normals(seed: int, stream_id: int, step: int, index) -> np.ndarray:
    return normals_from_words(bits(seed, stream_id, step, index))


def mulhi64(a, b):
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    s32 = np.uint64(32)
    al, ah, bl, bh = a & _M32, a >> s32, b & _M32, b >> s32
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> s32) + (lh & _M32) + (hl & _M32)
    return hh + (lh >> s32) + (hl >> s32) + (mid >> s32)


class MCMCRef:
    """MCMCController (mcmc_densification.cpp) on float32 numpy arrays; `orc` is the oracle module."""

    def __init__(self, orc, scene_extent: float, dead_opacity_threshold=0.005, relocate_cap=0.05,
                 noise_gate_k=100.0, noise_gate_t=0.995, lambda_opacity=0.01, lambda_scale=0.01, seed=0):
        self.orc, self.extent = orc, f32(scene_extent)
        self.thr, self.cap = f32(dead_opacity_threshold), f32(relocate_cap)
        self.k, self.t = f32(noise_gate_k), f32(noise_gate_t)
        self.lo, self.ls, self.seed = f32(lambda_opacity), f32(lambda_scale), int(seed)

    def sigmoid(self, x):
        x = np.asarray(x, f32)
        return (f32(1.0) / (f32(1.0) + self.orc.expf(-x))).astype(f32)

    # :167-186 (torch's order: mean's 1/numel, then sigmoid_backward / exp_backward)
    def regularization(self, opa, scl):
        n = opa.shape[0]
        y = self.sigmoid(opa)
        e = self.orc.expf(scl)
        co, cs = f32(self.lo / f32(n)), f32(self.ls / f32(3 * n))
        g_o = ((co * (f32(1.0) - y)).astype(f32) * y).astype(f32)
        g_s = (cs * e).astype(f32)
        value = float(self.lo) * float(np.mean(y.astype(np.float64))) + \
            float(self.ls) * float(np.mean(e.astype(np.float64)))
        return value, g_o, g_s

    # :144-161
    def inject_noise(self, pos, scl, opa, lr, noise):
        gate = self.sigmoid((-self.k * (self.sigmoid(opa) - self.t)).astype(f32))       # [N, 1]
        d = ((f32(lr) * self.orc.expf(scl)).astype(f32) * gate).astype(f32)
        return (pos + (d * noise).astype(f32)).astype(f32)

    # :56-138 with the counter-based draw; returns the new arrays and (num_dead, num_relocated, dead rows, sources)
    def relocate(self, m: dict, step: int):
        m = {k: np.array(v, f32, copy=True) for k, v in m.items()}
        n = m["positions"].shape[0]
        y = self.sigmoid(m["opacities"][:, 0])
        dead = y < self.thr
        nd = int(dead.sum())
        na = n - nd
        empty = np.zeros(0, np.int64)
        if nd == 0 or na == 0:
            return m, (nd, 0, empty, empty)
        capf = f32(self.cap * f32(n))
        cap_rows = 0 if not capf > 0 else (n if capf >= f32(n) else int(capf))
        w = np.where(dead, 0, np.rint(y * f32(16777216.0))).astype(np.uint64)
        cdf = np.cumsum(w, dtype=np.uint64)
        total = cdf[-1]
        M = 0 if total == 0 else min(nd, cap_rows)
        dst = np.nonzero(dead)[0][:M]
        if M == 0:
            return m, (nd, 0, empty, empty)
        r = bits(self.seed, STREAM_SAMPLE, step, np.arange(M, dtype=np.uint64))
        r64 = (r[:, 1].astype(np.uint64) << np.uint64(32)) | r[:, 0].astype(np.uint64)
        x = mulhi64(r64, total)
        src = np.searchsorted(cdf, x, side="right")             # the first i with cdf[i] > x
        z = normals(self.seed, STREAM_JITTER, step, dst.astype(np.uint64))
        m["sh_coeffs"][dst] = m["sh_coeffs"][src]
        m["rotations"][dst] = m["rotations"][src]
        m["positions"][dst] = (m["positions"][src] + ((z * self.extent).astype(f32) * f32(0.01)).astype(f32)).astype(f32)
        m["scales"][dst] = (m["scales"][src] - LOG_TEN).astype(f32)
        m["opacities"][dst] = LOW_OPACITY
        return m, (nd, M, dst, src)


def should_relocate(step, relocate_from=500, relocate_until=15000, relocate_every=100):
    return step >= relocate_from and step <= relocate_until and step % relocate_every == 0
