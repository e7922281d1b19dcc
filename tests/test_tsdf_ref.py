"""tests/tsdf_ref.py, the numpy mirror of the TSDF fusion and surface-net kernels, checked on its own:
the mesh of an analytic sphere is a closed, consistently oriented surface of genus 0 within a cell of the sphere, and
the float32 fusion agrees with a float64 restatement of the same rule wherever float32 rounding cannot flip a decision.
No GPU, no library."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as cases      # noqa: E402
import tsdf_ref as R            # noqa: E402

f32 = np.float32
U = 2.0 ** -24                  # float32 unit roundoff


def test_analytic_sphere_mesh_is_a_closed_oriented_sphere():
    dims, origin = cases.BOXES["odd"]
    assert dims == (37, 29, 23) and origin == (-1.8, -1.4, -1.1)
    planes = R.sphere_volume(dims, origin, 0.1, 0.4, (0.03, -0.02, 0.01), 0.83)
    V, C, F = R.surface_nets(planes, origin, 0.1)
    st = R.mesh_stats(V, F)
    err = np.abs(np.linalg.norm(V.astype(np.float64) - np.array(cases.CENTRE), axis=1) - 0.83) / 0.1
    print(f"analytic sphere: {st}, true volume {4 / 3 * np.pi * 0.83 ** 3:.4f}, max |r - R| = {err.max():.4f} voxels")
    assert C is None and V.dtype == f32 and F.dtype == np.int32 and len(V) > 0
    assert st["edge_counts"] == [0, 0, st["E"]]             # closed: every undirected edge in exactly two faces
    assert st["directed_max"] == 1                           # consistently oriented: no directed edge twice
    assert st["euler"] == 2
    assert st["volume"] > 0                                  # normals out of the sphere
    assert err.max() <= np.sqrt(3.0)                         # a surface-net vertex lies inside its cell
    assert F.min() >= 0 and F.max() < len(V)


def _margins(dims, origin, vs, trunc, view, s64):
    """First-order bounds on the float32 rounding error of zc, u, v and sdf at every voxel, from the float64 values."""
    nx, ny, nz = dims
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    o = np.asarray(origin, f32).astype(np.float64)
    p = [o[0] + ix * float(f32(vs)), o[1] + iy * float(f32(vs)), o[2] + iz * float(f32(vs))]
    ep = [2 * U * (abs(o[k]) + np.abs(p[k] - o[k])) for k in range(3)]                 # a product and a sum
    m = view["m"].astype(np.float64)
    err_row = lambda r: (sum(abs(m[r, k]) * ep[k] for k in range(3))
                         + 4 * U * (sum(np.abs(m[r, k] * p[k]) for k in range(3)) + abs(m[r, 3])))
    ex, ey, ez = err_row(0), err_row(1), err_row(2)
    zc = np.where(s64["front"], s64["zc"], 1.0)
    fx, fy = float(view["fx"]), float(view["fy"])
    eu = fx * (ex + np.abs(s64["u"] - float(view["cx"])) / fx * ez) / zc + 3 * U * (np.abs(s64["u"]) + abs(float(view["cx"])))
    ev = fy * (ey + np.abs(s64["v"] - float(view["cy"])) / fy * ez) / zc + 3 * U * (np.abs(s64["v"]) + abs(float(view["cy"])))
    with np.errstate(all="ignore"):
        d = np.abs(s64["sdf"] + s64["zc"])
        esdf = ez + U * d + U * np.abs(s64["sdf"])
    return ez, eu, ev, esdf


def test_float32_fusion_against_float64_restatement():
    dims, origin = cases.BOXES["odd"]
    views = cases.sphere_views(color=True)
    p32 = R.new_planes(dims, True)
    p64 = R.new_planes(dims, True).astype(np.float64)
    s32, s64 = [], []
    t32 = R.integrate(p32, origin, cases.VS, cases.TRUNC, views, samples=s32)
    t64 = R.integrate(p64, origin, cases.VS, cases.TRUNC, views, dtype=np.float64, samples=s64)
    unsafe = np.zeros(t32.shape, bool)
    for view, a, b in zip(views, s32, s64):
        ez, eu, ev, esdf = _margins(dims, origin, cases.VS, cases.TRUNC, view, b)
        near = np.abs(b["zc"] - float(f32(R.MIN_DEPTH))) <= ez                           # zc - min_depth
        # u, v against the edges of every pixel of the image: where the projection lands outside by more than its
        # error, no edge can change the result
        fr = b["front"] & (b["u"] >= -eu) & (b["u"] <= view["W"] + eu) & (b["v"] >= -ev) & (b["v"] <= view["H"] + ev)
        near |= fr & (np.abs(b["u"] - np.rint(b["u"])) <= eu)
        near |= fr & (np.abs(b["v"] - np.rint(b["v"])) <= ev)
        # A - min_alpha: alpha is an input, exact in both precisions; the decision cannot differ
        with np.errstate(all="ignore"):
            near |= b["weighted"] & (np.abs(b["sdf"] + float(f32(cases.TRUNC))) <= esdf)  # sdf + trunc
        unsafe |= near
        for stage in ("front", "inside", "seen", "weighted", "ok"):                      # decisions equal where safe
            assert np.array_equal(a[stage][~near], b[stage][~near]), stage
        assert np.array_equal(a["pix"][~near & b["ok"]], b["pix"][~near & b["ok"]])
    scored = ~unsafe
    assert np.array_equal(t32[scored], t64[scored])
    touched = int((t32 | t64).sum())
    remaining = int(unsafe.sum())
    err = np.abs(p32.astype(np.float64) - p64)[:, scored]
    names = ("tsdf", "weight", "r", "g", "b")
    print(f"touched {touched} of {t32.size}, not scored {remaining} ({100.0 * remaining / touched:.4f} %)")
    print("max |float32 - float64| on the scored set: " + ", ".join(f"{n} {e:.3e}" for n, e in zip(names, err.max(1))))
    assert touched > 5000
    assert remaining <= 0.005 * touched                       # the cap, with the mirror alone
    # Tolerances: 4 x what this comparison measures with these cameras (the margin for other inputs) - tsdf 7.431e-07
    # (the error of sdf / trunc: a few roundings of zc ~ 3 over trunc = 0.4, averaged), weight 3.576e-07 (a sum of up to
    # eight weights in [0.5, 2)), colour 1.449e-07 (a weighted mean of values in [0, 1)).
    assert err[0].max() <= TOL_TSDF
    assert err[1].max() <= TOL_WEIGHT
    assert err[2:].max() <= TOL_COLOUR


TOL_TSDF, TOL_WEIGHT, TOL_COLOUR = 4 * 7.431e-07, 4 * 3.576e-07, 4 * 1.449e-07


def test_fused_sphere_mesh_in_the_mirror():
    """The fused volume gives an oriented surface near the sphere, with holes where no camera saw it."""
    planes, origin, _ = cases.fused_sphere("odd", True)
    V, C, F = R.surface_nets(planes, origin, cases.VS)
    st = R.mesh_stats(V, F)
    err = np.abs(np.linalg.norm(V.astype(np.float64) - np.array(cases.CENTRE), axis=1) - cases.RADIUS) / cases.VS
    print(f"fused sphere: {st}, median |r - R| = {np.median(err):.4f} voxels")
    assert len(V) > 1000 and len(F) > 1500 and C.shape == V.shape
    assert F.min() >= 0 and F.max() < len(V)
    assert np.median(err) < 0.5
    assert st["volume"] > 0
    assert (C >= 0).all() and (C < 1).all()                   # interpolated between colour means in [0, 1)
