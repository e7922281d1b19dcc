"""References for the similarity transform of a model (include/cugs_hip.h; test infrastructure).

  sh_basis64 / fit_sh_rotation   the project's real SH basis in fp64 and an INDEPENDENT construction of the band matrices:
                                 a least-squares fit of Y_l(R d) = D_l Y_l(d) over a fixed set of directions
  abi_matrices                   the fp32 values of a filled CugsSimilarity as numpy arrays
  mirror32                       the kernel's arithmetic in numpy float32, operation for operation (every product and
                                 every sum one correctly rounded numpy operation, in the order the header states)
  exact64 / mirror_bound         the transform in fp64 from fp64 matrices, and the element-wise bound of the mirror on it
  random_rotation, similarity_cases, render_cases, transformed_arrays   scenes and transforms shared by the tests
"""
import math

import numpy as np

K1 = 0.4886025119029199
K2 = (1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
K3 = (0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 1.4453057213202769)
BANDS = ((1, 4), (4, 9), (9, 16))
PARAMS = ("positions", "sh_coeffs", "opacities", "rotations", "scales")


def sh_basis64(d):
    """[..., 3] unit directions -> [..., 16], the polynomials of sh_basis (cugs_gaussian_math.h) in fp64."""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    Y = [0.28209479177387814 + 0.0 * x, -K1 * y, K1 * z, -K1 * x,
         K2[0] * x * y, K2[0] * y * z, K2[1] * (2 * zz - xx - yy), K2[0] * x * z, K2[2] * (xx - yy),
         K3[0] * y * (3 * xx - yy), K3[1] * x * y * z, K3[2] * y * (4 * zz - xx - yy),
         K3[3] * z * (2 * zz - 3 * xx - 3 * yy), K3[2] * x * (4 * zz - xx - yy), K3[4] * z * (xx - yy),
         K3[0] * x * (xx - 3 * yy)]
    return np.stack(Y, axis=-1)


def fixed_directions(count=64):
    """A Fibonacci spiral: `count` well-spread unit vectors, no randomness."""
    k = np.arange(count) + 0.5
    z = 1.0 - 2.0 * k / count
    phi = k * math.pi * (3.0 - math.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def fit_sh_rotation(R):
    """[D1, D2, D3] fp64 with Y_l(R d) = D_l Y_l(d), by least squares over fixed_directions()."""
    R = np.asarray(R, dtype=np.float64)
    d = fixed_directions()
    Y, Yr = sh_basis64(d), sh_basis64(d @ R.T)
    out = []
    for a, b in BANDS:
        X, res, rank, _ = np.linalg.lstsq(Y[:, a:b], Yr[:, a:b], rcond=None)    # Y X = Yr, X = D^T
        assert rank == b - a
        out.append(X.T)
    return out


def abi_matrices(xf):
    """The fp32 fields of a filled cugs_amd._lib.Similarity."""
    f32 = np.float32
    return dict(m=np.array(xf.m, dtype=f32).reshape(3, 3), t=np.array(xf.t, dtype=f32), log_scale=f32(xf.log_scale),
                q=np.array(xf.q, dtype=f32), d=[np.array(xf.d1, dtype=f32).reshape(3, 3),
                                               np.array(xf.d2, dtype=f32).reshape(5, 5),
                                               np.array(xf.d3, dtype=f32).reshape(7, 7)], flags=int(xf.flags))


def _rows_times(A, x):
    """[..., L] -> [..., L]: out_i = A[i][0] x_0, then + A[i][j] x_j for j ascending; every operation fp32."""
    assert A.dtype == np.float32 and x.dtype == np.float32
    L = A.shape[0]
    out = np.empty_like(x)
    for i in range(L):
        acc = A[i, 0] * x[..., 0]
        for j in range(1, L):
            acc = acc + A[i, j] * x[..., j]
        out[..., i] = acc
    return out


def mirror32(arrays, xf, mask=None):
    """The five arrays after cugs_transform_gaussians, computed in numpy float32 in the kernel's order."""
    f = abi_matrices(xf)
    rot_id, scale_one = bool(f["flags"] & 1), bool(f["flags"] & 2)
    out = {k: np.array(v, dtype=np.float32, copy=True) for k, v in arrays.items()}
    if rot_id and scale_one and not f["t"].any():
        return out
    p, q, s, sh = (np.asarray(arrays[k], dtype=np.float32) for k in ("positions", "rotations", "scales", "sh_coeffs"))
    new = dict(positions=_rows_times(f["m"], p) + f["t"])
    if not scale_one:
        new["scales"] = s + f["log_scale"]
    if not rot_id:
        a, (bw, bx, by, bz) = f["q"], (q[:, 0], q[:, 1], q[:, 2], q[:, 3])
        nq = np.empty_like(q)
        nq[:, 0] = a[0] * bw - a[1] * bx - a[2] * by - a[3] * bz
        nq[:, 1] = a[0] * bx + a[1] * bw + a[2] * bz - a[3] * by
        nq[:, 2] = a[0] * by - a[1] * bz + a[2] * bw + a[3] * bx
        nq[:, 3] = a[0] * bz + a[1] * by - a[2] * bx + a[3] * bw
        new["rotations"] = nq
        nsh = sh.copy()
        for (lo, hi), D in zip(BANDS, f["d"]):
            if hi <= sh.shape[2]:
                nsh[:, :, lo:hi] = _rows_times(D, sh[:, :, lo:hi])
        new["sh_coeffs"] = nsh
    for k, v in new.items():
        if mask is None:
            out[k] = v.astype(np.float32)
        else:
            out[k][mask] = v[mask]
    return out


def quat_of_rotation64(R):
    """Unit quaternion (wxyz, w >= 0) of a rotation matrix, fp64, through the eigenvector of the largest eigenvalue of
    the symmetric 4x4 matrix of the rotation (independent of the C library's branch formulas)."""
    R = np.asarray(R, dtype=np.float64)
    K = np.array([[R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]],
                  [R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1]],
                  [R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1]]]) / 3.0
    w, v = np.linalg.eigh(K)
    q = v[:, -1]
    return q if q[0] >= 0 else -q


def exact64(arrays, scale, R, t, bands=None):
    """The transform of fp32 arrays in fp64 (nothing rounded), with the band matrices `bands` (default: the fit).
    Returns (outputs, magnitudes): magnitudes[k] = sum_j |A_ij| |x_j| (+ |t_i| for positions) of every output element,
    what the mirror's error bound multiplies."""
    R = np.asarray(R, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    bands = bands if bands is not None else fit_sh_rotation(R)
    p, q, s, sh = (np.asarray(arrays[k], dtype=np.float64) for k in ("positions", "rotations", "scales", "sh_coeffs"))
    M = scale * R
    out = dict(positions=p @ M.T + t, scales=s + math.log(scale), opacities=np.asarray(arrays["opacities"], np.float64))
    mag = dict(positions=np.abs(p) @ np.abs(M).T + np.abs(t), scales=np.abs(s) + abs(math.log(scale)))
    a = quat_of_rotation64(R)
    H = np.array([[a[0], -a[1], -a[2], -a[3]], [a[1], a[0], -a[3], a[2]], [a[2], a[3], a[0], -a[1]],
                  [a[3], -a[2], a[1], a[0]]])                          # q_R (x) q = H q
    out["rotations"] = q @ H.T
    mag["rotations"] = np.abs(q) @ np.abs(H).T
    nsh, msh = sh.copy(), np.abs(sh)
    for (lo, hi), D in zip(BANDS, bands):
        if hi <= sh.shape[2]:
            nsh[:, :, lo:hi] = sh[:, :, lo:hi] @ D.T
            msh[:, :, lo:hi] = np.abs(sh[:, :, lo:hi]) @ np.abs(D).T
    out["sh_coeffs"], mag["sh_coeffs"] = nsh, msh
    return out, mag


def propagate(err, scale, R):
    """An element-wise error `err` (dict of non-negative arrays) of the INPUT of the transform (scale, R, .), carried to
    its output: |A| err per tensor, no translation."""
    _, mag = exact64(dict(err, opacities=err["positions"][:, :1]), scale, R, np.zeros(3))
    mag["scales"] = np.asarray(err["scales"], dtype=np.float64)
    return mag


MIRROR_FACTOR = 4.0 * 2.0 ** -23    # eight half-ulps: the matrix entry, one per product, one per add; seven terms at most


def transformed_arrays(arrays, sim):
    """The model moved by `sim` in fp64 and rounded to float32 once (what the oracle's invariance is measured on)."""
    out, _ = exact64(arrays, sim.scale, sim.rotation, sim.translation)
    return {k: np.ascontiguousarray(out[k].astype(np.float32)) for k in PARAMS}


def random_rotation(seed):
    """A proper rotation from a Philox-seeded normal quaternion, fp64."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    w, x, y, z = (lambda q: q / np.linalg.norm(q))(rng.standard_normal(4))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


ROT_Z90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def similarity_cases(pkg):
    """The six transforms of the bit-for-bit tests: (name, Similarity)."""
    S = pkg.Similarity
    return [("identity", S()),
            ("translation", S(1.0, np.eye(3), [0.25, -1.5, 3.0])),
            ("scale", S(1.75, np.eye(3), np.zeros(3))),
            ("rot_z90", S(1.0, ROT_Z90, np.zeros(3))),
            ("random_2.5", S(2.5, random_rotation(11), [0.3, -0.2, 0.5])),
            ("random_0.4", S(0.4, random_rotation(12), [-1.0, 2.0, 0.7]))]


def make_arrays(pkg, n, coeffs=16, seed=31, mu_s=-3.0):
    degree = {1: 0, 4: 1, 9: 2, 16: 3}[coeffs]
    return pkg.scene.make_gaussians(n, 64, 48, sh_degree=degree, seed=seed, mu_s=mu_s)


W, H = 64, 48


def render_cases(pkg):
    """The render-invariance cases, shared by the CPU oracle test and the GPU test:
    (name, arrays, camera, Similarity, active_sh_degree).  64x48; n = 300 (mu_s = -2) and n = 2000 (mu_s = -3), degree 3;
    s in {1, 2.5, 0.4}; views 0 and 3 of make_camera; one case at active_sh_degree = 1.  Depths lie in [2, 10], so
    depth * min(1, s) >= 0.8, well above the projection's cull at 0.2."""
    S = pkg.Similarity
    scenes = {300: pkg.scene.make_gaussians(300, W, H, sh_degree=3, seed=41, mu_s=-2.0),
              2000: pkg.scene.make_gaussians(2000, W, H, sh_degree=3, seed=42, mu_s=-3.0)}
    cases = []
    k = 0
    for n in (300, 2000):
        for s in (1.0, 2.5, 0.4):
            view = (0, 3)[k % 2]
            sim = S(s, random_rotation(100 + k), np.array([0.4, -0.3, 0.6]) * (1 + k % 3))
            cases.append((f"n{n}_s{s}_v{view}", scenes[n], pkg.scene.make_camera(W, H, view), sim, 3))
            k += 1
    cases.append(("n300_s2.5_v3_deg1", scenes[300], pkg.scene.make_camera(W, H, 3), S(2.5, random_rotation(107), [0.1, 0.2, -0.3]), 1))
    return cases


def oracle_render(orc, arrays, cam, degree=3, bg=(0.1, 0.2, 0.3)):
    """The oracle's render plus `alpha` (1 - final_T) and `depth_map`: its blend of the depths as a colour channel over
    a zero background, which is what render(want_depth_map=True) computes (tests/test_gpu_depth_map.py)."""
    K = cam.intrinsics
    w, h = cam.width, cam.height
    ref = orc.render(arrays, cam.rotation, cam.translation, K.fx, K.fy, K.cx, K.cy, w, h, bg=list(bg), active_degree=degree)
    rgb = np.ascontiguousarray(np.repeat(np.asarray(ref["depths"], np.float32).reshape(-1, 1), 3, axis=1))
    f = orc.rasterize_forward(w, h, (0.0, 0.0, 0.0), ref["tile_ranges"], ref["values"], ref["means_2d"],
                              ref["cov_2d_inv"], rgb, ref["opacities_act"])
    ref["depth_map"] = f["color"][..., 0]
    ref["alpha"] = np.float32(1.0) - ref["final_T"]
    return ref


def oracle_gap(orc, arrays, cam, sim, pkg, degree=3):
    """The oracle's own invariance gap for one case: max |difference| of image, alpha and depth_map / s (relative to the
    depth scale max |depth_map|) between (model, camera) and (model moved in fp64 and rounded once, moved camera), and
    whether radii > 0 agrees on every Gaussian."""
    a = oracle_render(orc, arrays, cam, degree)
    b = oracle_render(orc, transformed_arrays(arrays, sim), pkg.transform_camera(cam, sim), degree)
    dscale = max(float(np.max(np.abs(a["depth_map"]))), 1e-30)
    return dict(color=float(np.max(np.abs(a["color"].astype(np.float64) - b["color"]))),
                alpha=float(np.max(np.abs(a["alpha"].astype(np.float64) - b["alpha"]))),
                depth=float(np.max(np.abs(a["depth_map"].astype(np.float64) - b["depth_map"].astype(np.float64) / sim.scale))) / dscale,
                same_visibility=bool(np.array_equal(a["radii"] > 0, b["radii"] > 0)), ref=a)
