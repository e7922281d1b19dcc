"""numpy mirror of csrc/cugs_tsdf.h + tsdf.hip: TSDF fusion and surface-net extraction in the kernels'
operation and summation order, every step an explicit float32 operation, so that the GPU results can be compared byte
for byte.  integrate(..., dtype=np.float64) restates the same rule in float64 (for tests/test_tsdf_ref.py).
Also two analytic scenes: a sphere volume, and sphere depth / alpha maps seen from a pinhole camera."""
import numpy as np

f32 = np.float32
MIN_DEPTH, MIN_ALPHA, MAX_WEIGHT = 0.05, 0.5, 64.0


# ---- scenes ------------------------------------------------------------------------------------------------------------
def look_at(eye, target=(0.0, 0.0, 0.0)):
    """World-to-camera (R, t) float32 of a camera at `eye` looking at `target` (x right, y down, z forward)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.05]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R.astype(f32), (-R @ eye).astype(f32)


def make_view(R, t, fx, fy, cx, cy, W, H, depth, alpha, color=None, weight=None):
    """One view of integrate(): the first three rows of the row-major view matrix, the pinhole, the maps (float32)."""
    m = np.concatenate([np.asarray(R, f32), np.asarray(t, f32).reshape(3, 1)], axis=1)
    return dict(m=m, fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy), W=int(W), H=int(H),
                D=np.ascontiguousarray(depth, f32).reshape(H, W), A=np.ascontiguousarray(alpha, f32).reshape(H, W),
                color=None if color is None else np.ascontiguousarray(color, f32).reshape(H, W, 3),
                weight=None if weight is None else np.ascontiguousarray(weight, f32).reshape(H, W))


def sphere_maps(R, t, fx, fy, cx, cy, W, H, centre, radius):
    """Camera-space z of the first hit of the sphere through each pixel centre, and the hit mask: (D, A) float32 [H,W]."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    u = (np.arange(W) + 0.5 - float(cx)) / float(fx)
    v = (np.arange(H) + 0.5 - float(cy)) / float(fy)
    U, V = np.meshgrid(u, v)
    d = np.stack([U, V, np.ones_like(U)], -1)
    cc = R @ np.asarray(centre, np.float64) + t
    a, b, k = (d * d).sum(-1), -2.0 * (d @ cc), cc @ cc - radius * radius
    disc = b * b - 4.0 * a * k
    hit = disc > 0
    s = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * a), 0.0)
    hit &= s > 0
    return (s * hit).astype(f32), hit.astype(f32)


def sphere_volume(dims, origin, vs, trunc, centre, radius):
    """Planes [2, nz, ny, nx]: the sphere's signed distance / trunc clipped to [-1, 1], and weight 1."""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    o = np.asarray(origin, np.float64)
    P = np.stack([o[0] + x * float(vs), o[1] + y * float(vs), o[2] + z * float(vs)], -1)
    sd = np.linalg.norm(P - np.asarray(centre, np.float64), axis=-1) - radius
    return np.stack([np.clip(sd / float(trunc), -1.0, 1.0).astype(f32), np.ones((nz, ny, nx), f32)])


def new_planes(dims, color):
    nx, ny, nz = dims
    p = np.zeros((5 if color else 2, nz, ny, nx), f32)
    p[0] = 1.0
    return p


# ---- fusion ------------------------------------------------------------------------------------------------------------
def sample(dims, origin, vs, trunc, view, min_depth=MIN_DEPTH, min_alpha=MIN_ALPHA, dtype=f32):
    """Steps 1-6 of the rule for every voxel and one view, in `dtype`.  Returns a dict: ok (touched), tn, w, pix (valid
    where ok), and the intermediate quantities and stage masks the tests look at."""
    T = dtype
    nx, ny, nz = dims
    o = [T(c) for c in np.asarray(origin, f32)]
    vs, trunc, min_depth, min_alpha = T(f32(vs)), T(f32(trunc)), T(f32(min_depth)), T(f32(min_alpha))
    m = view["m"].astype(T)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    px, py, pz = o[0] + ix.astype(T) * vs, o[1] + iy.astype(T) * vs, o[2] + iz.astype(T) * vs
    row = lambda r: ((m[r, 0] * px + m[r, 1] * py) + m[r, 2] * pz) + m[r, 3]
    xc, yc, zc = row(0), row(1), row(2)
    front = zc > min_depth
    zs = np.where(front, zc, T(1))
    u = (T(view["fx"]) * xc) / zs + T(view["cx"])
    v = (T(view["fy"]) * yc) / zs + T(view["cy"])
    fu, fv = np.floor(u), np.floor(v)
    W, H = view["W"], view["H"]
    inside = front & (fu >= 0) & (fu < T(W)) & (fv >= 0) & (fv < T(H))
    iu, iv = np.where(inside, fu, 0).astype(np.int64), np.where(inside, fv, 0).astype(np.int64)
    pix = iv * W + iu
    A = view["A"].astype(T)[iv, iu]
    seen = inside & (A > min_alpha)
    with np.errstate(all="ignore"):
        d = view["D"].astype(T)[iv, iu] / np.where(seen, A, T(1))
        w = np.ones(A.shape, T) if view["weight"] is None else view["weight"].astype(T)[iv, iu]
        weighted = seen & (w > 0)
        sdf = d - zc
        ok = weighted & (sdf >= -trunc)
        tn = np.minimum(np.where(ok, sdf, T(0)) / trunc, T(1))
    return dict(ok=ok, tn=tn, w=w, pix=pix, iu=iu, iv=iv, front=front, inside=inside, seen=seen, weighted=weighted,
                zc=zc, u=u, v=v, A=A, sdf=sdf)


def integrate(planes, origin, vs, trunc, views, min_depth=MIN_DEPTH, min_alpha=MIN_ALPHA, max_weight=MAX_WEIGHT, dtype=f32,
              samples=None):
    """Step 7 for the views in the order given, in place on planes [P, nz, ny, nx] (of `dtype`).  Returns the mask of
    touched voxels.  `samples`: a list that receives each view's sample() dict."""
    T = dtype
    P, nz, ny, nx = planes.shape
    touched = np.zeros((nz, ny, nx), bool)
    for view in views:
        s = sample((nx, ny, nz), origin, vs, trunc, view, min_depth, min_alpha, T)
        if samples is not None:
            samples.append(s)
        ok = s["ok"]
        wo = planes[1][ok]
        w = s["w"][ok]
        wn = wo + w
        planes[0][ok] = (wo * planes[0][ok] + w * s["tn"][ok]) / wn
        if P == 5:
            c = view["color"].astype(T)[s["iv"][ok], s["iu"][ok]]
            for ch in range(3):
                planes[2 + ch][ok] = (wo * planes[2 + ch][ok] + w * c[:, ch]) / wn
        planes[1][ok] = np.minimum(wn, T(f32(max_weight)))
        touched |= ok
    return touched


# ---- surface nets ------------------------------------------------------------------------------------------------------
EDGE_A = (0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3)      # corner a of the twelve edges; the axis is e // 4, b = a + (1 << axis)


def surface_nets(planes, origin, vs, min_weight=0.0):
    """(vertices [V,3] f32, colors [V,3] f32 or None, faces [F,3] i32) of the volume, in the kernels' order."""
    P, nz, ny, nx = planes.shape
    tsdf, wgt = planes[0], planes[1]
    o = np.asarray(origin, f32)
    vs = f32(vs)
    empty = (np.zeros((0, 3), f32), np.zeros((0, 3), f32) if P == 5 else None, np.zeros((0, 3), np.int32))
    if min(nx, ny, nz) < 2:
        return empty
    valid, neg = wgt > f32(min_weight), tsdf < 0
    cut = lambda a, k: a[(k >> 2):nz - 1 + (k >> 2), ((k >> 1) & 1):ny - 1 + ((k >> 1) & 1), (k & 1):nx - 1 + (k & 1)]
    allv = np.ones((nz - 1, ny - 1, nx - 1), bool)
    cnt = np.zeros((nz - 1, ny - 1, nx - 1), np.int32)
    for k in range(8):
        allv &= cut(valid, k)
        cnt += cut(neg, k)
    active = allv & (cnt > 0) & (cnt < 8)
    zz, yy, xx = np.nonzero(active)                  # ascending cell index, x fastest
    n = len(zz)
    if n == 0:
        return empty
    vid = np.full(active.shape, -1, np.int64)
    vid[active] = np.arange(n)
    corner = lambda k: (zz + (k >> 2), yy + ((k >> 1) & 1), xx + (k & 1))
    f = np.stack([tsdf[corner(k)] for k in range(8)], 1)
    col = None if P != 5 else np.stack([np.stack([planes[2 + ch][corner(k)] for k in range(8)], 1) for ch in range(3)], 2)
    s, sc, count = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for e in range(12):
            axis, a = e // 4, EDGE_A[e]
            b = a + (1 << axis)
            fa, fb = f[:, a], f[:, b]
            cross = (fa < 0) != (fb < 0)
            t = fa / np.where(cross, fa - fb, f32(1))
            for k in range(3):
                term = t if k == axis else np.full(n, f32((a >> k) & 1))
                s[:, k] = np.where(cross, s[:, k] + term, s[:, k])
            if col is not None:
                for ch in range(3):
                    ca, cb = col[:, a, ch], col[:, b, ch]
                    sc[:, ch] = np.where(cross, sc[:, ch] + (ca + t * (cb - ca)), sc[:, ch])
            count += cross
        nf = count.astype(f32)
        cell = np.stack([xx, yy, zz], 1).astype(f32)
        verts = (o[None, :] + (cell + s / nf[:, None]) * vs).astype(f32)
        colors = None if col is None else (sc / nf[:, None]).astype(f32)
    # faces: the edge from voxel (x, y, z) along each axis belongs to cell (x, y, z)
    p = [xx, yy, zz]
    quads = np.zeros((n, 3, 4), np.int64)
    has = np.zeros((n, 3), bool)
    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        q = [p[0].copy(), p[1].copy(), p[2].copy()]
        q[axis] = q[axis] + 1
        na, nb = tsdf[zz, yy, xx] < 0, tsdf[q[2], q[1], q[0]] < 0
        good = (p[b] >= 1) & (p[c] >= 1) & (na != nb)
        ids = []
        for ob, oc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            r = [p[0].copy(), p[1].copy(), p[2].copy()]
            r[b] = np.maximum(r[b] + ob, 0)
            r[c] = np.maximum(r[c] + oc, 0)
            ids.append(vid[r[2], r[1], r[0]])
        ids = np.stack(ids, 1)
        good &= (ids >= 0).all(1)
        quads[:, axis] = np.where(na[:, None], ids, ids[:, ::-1])
        has[:, axis] = good
    tris = np.stack([quads[:, :, [0, 1, 2]], quads[:, :, [0, 2, 3]]], 2)         # [n, 3, 2, 3]
    faces = tris[has].reshape(-1, 3).astype(np.int32)
    return verts, colors, faces


def mesh_stats(V, F):
    """Edge statistics of a triangle mesh: closed (every undirected edge in two faces), oriented (no directed edge
    twice), the Euler characteristic and the signed volume."""
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]).astype(np.int64)
    _, cnt = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    _, dcnt = np.unique(e, axis=0, return_counts=True)
    Vd = V.astype(np.float64)
    vol = np.einsum("ij,ij->i", Vd[F[:, 0]], np.cross(Vd[F[:, 1]], Vd[F[:, 2]])).sum() / 6.0
    return dict(V=len(V), F=len(F), E=len(cnt), euler=len(V) - len(cnt) + len(F), edge_counts=np.bincount(cnt).tolist(),
                directed_max=int(dcnt.max()) if len(dcnt) else 0, volume=float(vol))
