"""The numpy mirrors of csrc/envmap.hip (arithmetic: include/cugs_hip.h): a float32 one that follows the
kernels operation for operation (fma32 is an exact fmaf), an fp64 one of the same mathematics, a CLAMP variant of the tap
addressing (what the octahedral fold is there to avoid), the fixed-point sum of the map gradient, and the cameras and
shapes the tests share."""
import math

import numpy as np

from vq_ref import fma32

F32, F64, I64 = np.float32, np.float64, np.int64

SHAPES = ((17, 33), (48, 64))                 # (H, W): neither a multiple of 16, more than one workgroup
RESOLUTIONS = (4, 16)                         # R = 4: nearly every sample folds
UP_MINUS_Y = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], F64)      # world -y is the map's +z (zenith at the centre)


def _rot(axis, angle):
    c, s = math.cos(angle), math.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(3)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def orientation_tilted():
    """A non-identity orientation with entries that are not floats: -y up, then 0.3 rad about the map's x."""
    return np.ascontiguousarray(_rot(0, 0.3) @ UP_MINUS_Y, dtype=F64)


def cameras(h, w):
    """name -> dict(R [3,3] f32 world-to-camera, fx, fy, cx, cy, width, height).  The centred ones put the principal
    point on a pixel centre, so that pixel's ray is the camera axis exactly: +z and -z are the two poles of the map (the
    -z one an octahedron vertex folded to a corner, through sgn(0)); -y is a vertex on the z = 0 diamond."""
    ccx, ccy = float(w // 2) + 0.5, float(h // 2) + 0.5
    f = 0.6 * w                                                        # a wide view: every camera crosses fold lines
    base = dict(fx=f, fy=0.9 * f, cx=ccx, cy=ccy, width=w, height=h)
    look_pz = np.eye(3)
    look_mz = np.diag([-1.0, 1.0, -1.0])
    look_px = np.array([[0, 0, -1.0], [0, 1, 0], [1, 0, 0]])           # camera z = world +x
    look_my = np.array([[1, 0, 0.0], [0, 0, 1], [0, -1, 0]])           # camera z = world -y
    oblique = _rot(1, 2.1) @ _rot(0, -0.7) @ _rot(2, 0.4)
    out = {}
    for name, rot in (("+z", look_pz), ("-z", look_mz), ("+x", look_px), ("axis-y", look_my)):
        out[name] = dict(base, R=np.ascontiguousarray(rot, dtype=F32))
    out["oblique"] = dict(base, R=np.ascontiguousarray(oblique, dtype=F32), fx=0.45 * w, fy=0.5 * w,
                          cx=0.37 * w, cy=0.71 * h)
    return out


def cases():
    """(label, h, w, res, camera, orientation or None): every shape x resolution x camera, and one tilted orientation."""
    out = []
    for h, w in SHAPES:
        for res in RESOLUTIONS:
            for name, cam in cameras(h, w).items():
                out.append((f"{h}x{w}-R{res}-{name}", h, w, res, cam, None))
    h, w = SHAPES[0]
    out.append((f"{h}x{w}-R16-oblique-tilted", h, w, 16, cameras(h, w)["oblique"], orientation_tilted()))
    out.append((f"{h}x{w}-R4-+x-up-y", h, w, 4, cameras(h, w)["+x"], UP_MINUS_Y.copy()))
    return out


def case_data(h, w, res, seed=0):
    """(E [3,R,R], C [H,W,3], T [H,W], g [H,W,3]) float32: T has exact zeros (covered), exact ones (open) and values
    between; |g| < 1."""
    rng = np.random.default_rng(1000 * h + 10 * res + seed)
    E = rng.random((3, res, res), dtype=F32)
    C = rng.random((h, w, 3), dtype=F32)
    T = rng.random((h, w), dtype=F32)
    T[rng.random((h, w)) < 0.25] = 0.0
    T[rng.random((h, w)) < 0.25] = 1.0
    g = (rng.random((h, w, 3), dtype=F32) - F32(0.5)) * F32(1.9)
    return E, C, T, g


def view_matrix(rot, orientation=None):
    """m [9] float32 = O R^T, each entry (O[i][0] R[j][0] + O[i][1] R[j][1]) + O[i][2] R[j][2] in fp64, rounded once."""
    rot = np.asarray(rot, F32)
    o = np.eye(3) if orientation is None else np.asarray(orientation, F64)
    m = np.empty(9, F32)
    for i in range(3):
        for j in range(3):
            r0, r1, r2 = (float(rot[j, k]) for k in range(3))
            m[3 * i + j] = F32((float(o[i, 0]) * r0 + float(o[i, 1]) * r1) + float(o[i, 2]) * r2)
    return m


def fold(i, j, res, wrap="fold"):
    """Step 5 on integer arrays: (i, j) in [-1, R] -> the flat index j R + i of the folded (or clamped) tap."""
    i, j = i.copy(), j.copy()
    if wrap == "clamp":
        return np.clip(j, 0, res - 1) * res + np.clip(i, 0, res - 1)
    lo, hi = i < 0, i >= res
    i = np.where(lo, -1 - i, np.where(hi, 2 * res - 1 - i, i))
    j = np.where(lo | hi, res - 1 - j, j)
    lo, hi = j < 0, j >= res
    j = np.where(lo, -1 - j, np.where(hi, 2 * res - 1 - j, j))
    i = np.where(lo | hi, res - 1 - i, i)
    return j * res + i


def _octa(n0, n1, n2, one):
    sg = lambda t: np.where(t >= 0, one, -one)
    low = n2 < 0
    x = np.where(low, (one - np.abs(n1)) * sg(n0), n0)
    y = np.where(low, (one - np.abs(n0)) * sg(n1), n1)
    return x, y


def taps32(cam, res, orientation=None, wrap="fold"):
    """Steps 1-5 for every pixel, float32 op for op: (idx [H W, 4] of E00 E01 E10 E11, a [H W], b [H W])."""
    m = view_matrix(cam["R"], orientation)
    h, w = cam["height"], cam["width"]
    u = np.tile(np.arange(w, dtype=F32), h)
    v = np.repeat(np.arange(h, dtype=F32), w)
    with np.errstate(all="ignore"):
        ax = ((u + F32(0.5)) - F32(cam["cx"])) / F32(cam["fx"])
        ay = ((v + F32(0.5)) - F32(cam["cy"])) / F32(cam["fy"])
        d = [fma32(m[3 * k], ax, fma32(m[3 * k + 1], ay, np.full_like(ax, m[3 * k + 2]))) for k in range(3)]
        s = (np.abs(d[0]) + np.abs(d[1])) + np.abs(d[2])
        ok = (s > 0) & (s < np.inf)
        sd = np.where(ok, s, F32(1))
        n0, n1, n2 = d[0] / sd, d[1] / sd, d[2] / sd
        x, y = _octa(n0, n1, n2, F32(1))
        x, y = np.where(ok, x, F32(0)), np.where(ok, y, F32(0))
        hh = F32(0.5) * F32(res)
        h1 = hh - F32(0.5)
        sx, sy = fma32(x, hh, np.full_like(x, h1)), fma32(y, hh, np.full_like(y, h1))
        fx0 = np.minimum(np.maximum(np.floor(sx), F32(-1)), F32(res - 1))
        fy0 = np.minimum(np.maximum(np.floor(sy), F32(-1)), F32(res - 1))
        a, b = sx - fx0, sy - fy0
    assert a.dtype == F32 and b.dtype == F32
    i0, j0 = fx0.astype(I64), fy0.astype(I64)
    idx = np.stack([fold(i0, j0, res, wrap), fold(i0 + 1, j0, res, wrap), fold(i0, j0 + 1, res, wrap),
                    fold(i0 + 1, j0 + 1, res, wrap)], axis=1)
    return idx, a, b


def sample32(E, taps, h, w):
    """Step 6: B [H,W,3] float32."""
    idx, a, b = taps
    E = np.asarray(E, F32)
    res = E.shape[1]
    out = np.empty((h * w, 3), F32)
    for c in range(3):
        e = E[c].reshape(res * res)[idx]                               # [H W, 4]
        top = fma32(a, e[:, 1] - e[:, 0], e[:, 0])
        bot = fma32(a, e[:, 3] - e[:, 2], e[:, 2])
        out[:, c] = fma32(b, bot - top, top)
    return out.reshape(h, w, 3)


def composite32(C, T, B):
    """Step 7: fmaf(T, B, C)."""
    return fma32(np.asarray(T, F32)[..., None], B, C)


def dalpha32(g, B):
    """-fmaf(g2, B2, fmaf(g1, B1, g0 * B0))."""
    g, B = np.asarray(g, F32), np.asarray(B, F32)
    return -fma32(g[..., 2], B[..., 2], fma32(g[..., 1], B[..., 1], g[..., 0] * B[..., 0]))


def frac_bits(h, w, grad_bound=1.0):
    """F = 61 - q - e: 2^e the smallest power of two >= grad_bound, 4 H W < 2^q."""
    mant, e = math.frexp(float(F32(grad_bound)))
    if mant == 0.5:
        e -= 1
    return 61 - (4 * h * w).bit_length() - e, e


def denv32(taps, g, T, res, grad_bound=1.0, order=None):
    """The fixed-point map gradient: (dL_denv [3,R,R] float32, table [3,R R] int64, clamped 0/1).  `order`: a
    permutation of the pixels, the order their shares are added in (the result must not depend on it)."""
    idx, a, b = taps
    g, T = np.asarray(g, F32), np.asarray(T, F32)
    h, w = T.shape
    fb, e = frac_bits(h, w, grad_bound)
    bound = F32(2.0 ** e)
    oma, omb = F32(1) - a, F32(1) - b
    wk = [oma * omb, a * omb, oma * b, a * b]
    table = np.zeros((3, res * res), I64)
    clamped = 0
    order = np.arange(h * w) if order is None else np.asarray(order)
    with np.errstate(all="ignore"):
        for c in range(3):
            tg = T.reshape(-1) * g.reshape(-1, 3)[:, c]
            for k in range(4):
                sh = wk[k] * tg
                assert sh.dtype == F32
                over = ~(np.abs(sh) <= bound)
                if over.any():
                    clamped = 1
                    sh = np.where(over, np.where(np.isnan(sh), F32(0), np.copysign(bound, sh)), sh)
                q = np.rint(sh.astype(F64) * 2.0 ** fb).astype(I64)
                np.add.at(table[c], idx[order, k], q[order])
    grad = (table.astype(F64) * 2.0 ** -fb).astype(F32).reshape(3, res, res)
    return grad, table, clamped


# ---- fp64: the same mathematics without the float32 roundings -------------------------------------------------------

def dir_to_xy64(d):
    """Octahedral coordinates (x, y) in [-1, 1]^2 of directions d [..., 3]."""
    d = np.asarray(d, F64)
    n = d / np.abs(d).sum(axis=-1, keepdims=True)
    return _octa(n[..., 0], n[..., 1], n[..., 2], 1.0)


def xy_to_dir64(x, y):
    """The unit direction of octahedral coordinates: the inverse of dir_to_xy64 up to the length."""
    x, y = np.asarray(x, F64), np.asarray(y, F64)
    z = 1.0 - np.abs(x) - np.abs(y)
    sg = lambda t: np.where(t >= 0, 1.0, -1.0)
    low = z < 0
    n0 = np.where(low, (1.0 - np.abs(y)) * sg(x), x)
    n1 = np.where(low, (1.0 - np.abs(x)) * sg(y), y)
    d = np.stack([n0, n1, z], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def taps64_xy(x, y, res, wrap="fold"):
    sx, sy = x * (0.5 * res) + (0.5 * res - 0.5), y * (0.5 * res) + (0.5 * res - 0.5)
    fx0, fy0 = np.clip(np.floor(sx), -1, res - 1), np.clip(np.floor(sy), -1, res - 1)
    i0, j0 = fx0.astype(I64), fy0.astype(I64)
    idx = np.stack([fold(i0, j0, res, wrap), fold(i0 + 1, j0, res, wrap), fold(i0, j0 + 1, res, wrap),
                    fold(i0 + 1, j0 + 1, res, wrap)], axis=-1)
    return idx, sx - fx0, sy - fy0


def pixel_dirs64(cam, orientation=None):
    """Map-space ray directions [H W, 3] from the float32 view block, evaluated in fp64."""
    m = view_matrix(cam["R"], orientation).astype(F64).reshape(3, 3)
    h, w = cam["height"], cam["width"]
    u = np.tile(np.arange(w, dtype=F64), h)
    v = np.repeat(np.arange(h, dtype=F64), w)
    ax = ((u + 0.5) - float(F32(cam["cx"]))) / float(F32(cam["fx"]))
    ay = ((v + 0.5) - float(F32(cam["cy"]))) / float(F32(cam["fy"]))
    return np.stack([ax, ay, np.ones_like(ax)], axis=1) @ m.T


def taps64(cam, res, orientation=None, wrap="fold"):
    x, y = dir_to_xy64(pixel_dirs64(cam, orientation))
    return taps64_xy(x, y, res, wrap)


def weights64(a, b):
    return np.stack([(1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b], axis=-1)


def sample64(E, taps):
    """B [..., 3] fp64 at the taps."""
    idx, a, b = taps
    E = np.asarray(E, F64)
    res = E.shape[1]
    wk = weights64(a, b)
    return np.stack([(E[c].reshape(res * res)[idx] * wk).sum(axis=-1) for c in range(3)], axis=-1)


def sample_dirs64(E, d, wrap="fold"):
    x, y = dir_to_xy64(d)
    return sample64(E, taps64_xy(x, y, np.asarray(E).shape[1], wrap))


def backward64(E, taps, g, T):
    """(dL_dalpha [H W], dL_denv [3,R,R]) of L = sum g (C + T B), analytic, fp64; g [H W, 3], T [H W]."""
    idx, a, b = taps
    E = np.asarray(E, F64)
    res = E.shape[1]
    B = sample64(E, taps)
    d_alpha = -(g * B).sum(axis=-1)
    wk = weights64(a, b)
    d_env = np.zeros((3, res * res))
    for c in range(3):
        np.add.at(d_env[c], idx, wk * (T * g[:, c])[:, None])
    return d_alpha, d_env.reshape(3, res, res)
