"""Point-cloud initialisation on the device (csrc/knn.hip behind cugs_knn_mean_distances and
cugs_init_from_points, pkg.init_gaussians_from_sparse / pkg.knn_mean_distances) against the numpy restatement
tests/init_ref.py: mean distances, positions, coefficients, opacities and rotations bit for bit, the scales within 2 ulp of
the float64 logarithm, on every route (exhaustive, tree, automatic)."""
import numpy as np
import pytest
import torch

import init_ref as ir

pytestmark = pytest.mark.gpu
F = np.float32
ROUTES = ("exhaustive", "tree", "auto")
CLOUDS = ("uniform", "blobs", "plane")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    assert got.shape == want.shape and bad.size == 0, (
        f"{what}: {bad.size} of {want.size} differ, first at {bad[:5]}: got {got.ravel()[bad[:5]]} want {want.ravel()[bad[:5]]}")


def _lattice():
    g = np.arange(3, dtype=F)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def _small_cloud(n):
    if n == 27:
        return _lattice(), np.full((27, 3), 128, np.uint8)
    pos, col = ir.make_cloud("uniform", n, seed=n)
    if n >= 3:
        col[0], col[1], col[2] = 0, 128, 255
    return pos, col


def _check_model(model, ref, n, degree, what):
    for name in ("positions", "sh_coeffs", "opacities", "rotations"):
        _same(getattr(model, name), ref[name], f"{what} {name}")
    sh = model.sh_coeffs.cpu().numpy()
    assert sh.shape == (n, 3, (degree + 1) ** 2) and not sh[:, :, 1:].any()
    s = model.scales.cpu().numpy()
    assert s.shape == (n, 3)
    if n:
        assert np.array_equal(_bits(s[:, 0]), _bits(s[:, 1])) and np.array_equal(_bits(s[:, 0]), _bits(s[:, 2]))
        err = float(ir.scale_ulp_error(s, ref["mean_dist"]).max())
        print(f"{what}: worst scale error {err:.3f} ulp")
        assert err <= 2.0, (what, err)
    assert model.is_valid() and model.positions.device.type == "cuda"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n", (0, 1, 2, 3, 4, 27, 1000))
def test_small_clouds_match_the_restatement(pkg, dev, n, route):
    pos, col = _small_cloud(n)
    for k in (1, 3, 8, 16):
        want = ir.knn_mean_distances(pos, k)
        _same(pkg.knn_mean_distances(pos, k, route=route, device=dev), want, f"n={n} k={k} {route} mean_dist")
    for degree in (0, 1, 2, 3):
        ref = ir.init_model(pos, col, degree, 3)
        model = pkg.init_gaussians_from_sparse(pos, col, sh_degree=degree, k_neighbors=3, device=dev, route=route)
        _check_model(model, ref, n, degree, f"n={n} degree={degree} {route}")
    if n == 27:
        m = pkg.knn_mean_distances(pos, 3, route=route, device=dev).cpu().numpy()
        assert np.all(m == 1.0)                                                # ScaleIsReasonable: spacing 1
        model = pkg.init_gaussians_from_sparse(pos, col, 0, 3, device=dev, route=route)
        assert np.all(model.scales.cpu().numpy() == 0.0)


def test_colours_and_tensor_inputs(pkg, dev):
    pos, _ = ir.make_cloud("uniform", 300, seed=9)
    col = np.repeat(np.array([0, 128, 255] * 100, np.uint8)[:, None], 3, axis=1)
    col[:, 1] = col[::-1, 0]
    ref = ir.init_model(pos, col, 2, 3)
    a = pkg.init_gaussians_from_sparse(pos, col, 2, 3, device=dev)
    b = pkg.init_gaussians_from_sparse(torch.from_numpy(pos).to(dev), torch.from_numpy(col).to(dev), 2, 3)
    for m in (a, b):
        _check_model(m, ref, 300, 2, "colours")
    dc = a.sh_coeffs.cpu().numpy()[:, :, 0]
    assert np.all(dc[col == 0] == F(-0.5) / ir.SH_C0) and np.all(dc[col == 255] == F(0.5) / ir.SH_C0)
    for name in ("positions", "sh_coeffs", "opacities", "rotations", "scales"):
        assert torch.equal(getattr(a, name), getattr(b, name))


@pytest.mark.parametrize("kind", CLOUDS)
def test_every_point_of_20k_clouds(pkg, dev, kind):
    pos, col = ir.make_cloud(kind, 20000, seed=11)
    want = ir.knn_mean_distances(pos, 3)
    for route in ROUTES:
        _same(pkg.knn_mean_distances(pos, 3, route=route, device=dev), want, f"{kind} {route}")
    want8 = ir.knn_mean_distances(pos, 8)
    for route in ("exhaustive", "tree"):
        _same(pkg.knn_mean_distances(pos, 8, route=route, device=dev), want8, f"{kind} {route} k=8")
    model = pkg.init_gaussians_from_sparse(pos, col, 3, 3, device=dev)
    ref = ir.init_model(pos, col, 3, 3)
    _check_model(model, ref, 20000, 3, f"{kind} 20k")


@pytest.mark.parametrize("n", (136000, 1000000))
@pytest.mark.parametrize("kind", CLOUDS)
def test_tree_equals_exhaustive_on_large_clouds(pkg, dev, kind, n):
    pos, _ = ir.make_cloud(kind, n, seed=17)
    p = torch.from_numpy(pos).to(dev)
    tree = pkg.knn_mean_distances(p, 3, route="tree")
    full = pkg.knn_mean_distances(p, 3, route="exhaustive")
    auto = pkg.knn_mean_distances(p, 3, route="auto")
    assert torch.equal(tree.view(torch.int32), full.view(torch.int32)), f"{kind} {n}: tree differs from exhaustive"
    assert torch.equal(auto.view(torch.int32), full.view(torch.int32))
    m = tree.cpu().numpy()
    order = np.argsort(m, kind="stable")
    rng = np.random.default_rng(n)
    sample = np.unique(np.concatenate([order[:64], order[-64:], rng.choice(n, 384, replace=False)]))
    want = ir.knn_mean_distances(pos, 3, queries=sample)
    _same(m[sample], want, f"{kind} {n} sample (tree)")
    _same(full.cpu().numpy()[sample], want, f"{kind} {n} sample (exhaustive)")


def test_many_copies_of_one_point(pkg, dev):
    """The early stop at a k-th best of 0: without it every copy visits every bucket that holds the point."""
    pos, _ = ir.make_cloud("uniform", 100000, seed=23)
    pos[:50000] = pos[0]
    rng = np.random.default_rng(2)
    pos = pos[rng.permutation(100000)]
    want = ir.knn_mean_distances(pos, 3, queries=np.arange(0, 100000, 50))
    for route in ("tree", "exhaustive"):
        m = pkg.knn_mean_distances(pos, 3, route=route, device=dev).cpu().numpy()
        _same(m[::50], want, f"copies {route}")
    copies = np.all(pos == ir.make_cloud("uniform", 100000, seed=23)[0][0], axis=1)
    assert copies.sum() == 50000 and np.all(m[copies] == 0.0)
    model = pkg.init_gaussians_from_sparse(pos, np.zeros((100000, 3), np.uint8), 0, 3, device=dev, route="tree")
    s = model.scales.cpu().numpy()
    assert np.all(np.abs(s[copies] - np.log(np.float64(F(1e-7)))) <= 2 * np.spacing(np.abs(s[copies])))


@pytest.mark.parametrize("route", ROUTES)
def test_degenerate_clouds(pkg, dev, route):
    rng = np.random.default_rng(31)
    line = np.zeros((3000, 3), F)
    line[:, 0] = rng.uniform(-5, 5, 3000)
    line[:, 1] = F(2.0) * line[:, 0]                                            # collinear, not axis-aligned
    axis = np.zeros((3000, 3), F)
    axis[:, 2] = rng.uniform(0, 1, 3000)                                        # on one axis: two extents are 0
    two = np.repeat(np.array([[0.5, 1.0, 2.0], [0.5, 1.0, 2.25]], F), 1000, axis=0)[rng.permutation(2000)]
    one = np.full((500, 3), F(3.25))
    g = (np.arange(12, dtype=np.float64) * 0.1 + 1e6).astype(F)                # fp32 cancellation in dx
    far = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    for name, pos in (("line", line), ("axis", axis), ("two", two), ("one", one), ("far", far)):
        for k in (3, 16):
            _same(pkg.knn_mean_distances(pos, k, route=route, device=dev), ir.knn_mean_distances(pos, k),
                  f"{name} k={k} {route}")


@pytest.mark.parametrize("route", ROUTES)
def test_input_order_is_kept(pkg, dev, route):
    pos, col = ir.make_cloud("blobs", 30000, seed=41)
    perm = np.random.default_rng(42).permutation(30000)
    a = pkg.init_gaussians_from_sparse(pos, col, 1, 3, device=dev, route=route)
    b = pkg.init_gaussians_from_sparse(pos[perm], col[perm], 1, 3, device=dev, route=route)
    for name in ("positions", "sh_coeffs", "opacities", "rotations", "scales"):
        _same(getattr(b, name), getattr(a, name).cpu().numpy()[perm], f"{name} {route}")
    _same(a.positions, pos, "positions are the input")


def test_deterministic_and_stream_safe(pkg, dev):
    pa, _ = ir.make_cloud("blobs", 200000, seed=51)
    pb, _ = ir.make_cloud("uniform", 150000, seed=52)
    ta, tb = torch.from_numpy(pa).to(dev), torch.from_numpy(pb).to(dev)
    for route in ("tree", "exhaustive"):
        first = pkg.knn_mean_distances(ta, 3, route=route)
        again = pkg.knn_mean_distances(ta, 3, route=route)
        assert torch.equal(first.view(torch.int32), again.view(torch.int32)), route
    alone_a = pkg.knn_mean_distances(ta, 3, route="tree")
    alone_b = pkg.knn_mean_distances(tb, 3, route="tree")
    torch.cuda.synchronize(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    outs = []
    for _ in range(3):                                                          # two calls in flight, a workspace each
        with torch.cuda.stream(s1):
            ra = pkg.knn_mean_distances(ta, 3, route="tree")
        with torch.cuda.stream(s2):
            rb = pkg.knn_mean_distances(tb, 3, route="tree")
        outs.append((ra, rb))
    torch.cuda.synchronize(dev)
    from cugs_amd import gaussian_init
    keys = [k for k in gaussian_init._workspaces if k[1] in (s1.cuda_stream, s2.cuda_stream)]
    assert len(keys) == 2
    for ra, rb in outs:
        assert torch.equal(ra.view(torch.int32), alone_a.view(torch.int32))
        assert torch.equal(rb.view(torch.int32), alone_b.view(torch.int32))


def test_end_to_end_render_and_step(pkg, orc, dev):
    """A model made from a point cloud goes through render -> render_backward -> FusedAdam.step; the forward image is
    the oracle's on the same arrays, bit for bit."""
    w, h, n = 160, 120, 20000
    cam = pkg.scene.make_camera(w, h)
    rng = np.random.default_rng(61)
    pos = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3.0, 8.0, n)], -1).astype(F)
    assert np.array_equal(cam.rotation, np.eye(3)) and not np.any(cam.translation)      # view 0 looks down +z
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    model = pkg.init_gaussians_from_sparse(pos, col, sh_degree=3, k_neighbors=3, device=dev)
    settings = pkg.RenderSettings(background=[0.1, 0.2, 0.3], active_sh_degree=3)
    out = pkg.render(model, cam, settings)
    arrays = {k: getattr(model, k).cpu().numpy() for k in ("positions", "sh_coeffs", "opacities", "rotations", "scales")}
    K = cam.intrinsics
    ref = orc.render(arrays, cam.rotation, cam.translation, K.fx, K.fy, K.cx, K.cy, w, h, bg=settings.background)
    assert int((ref["radii"] > 0).sum()) > n // 2                               # the cloud is in front of the camera
    assert np.array_equal(out.radii.cpu().numpy(), ref["radii"])
    _same(out.color, ref["color"], "forward image")
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h)).to(dev)
    grads = pkg.render_backward(g, out, model, cam, settings)
    opt = pkg.FusedAdam(model)
    before = model.positions.clone()
    opt.apply_gradients(grads)
    opt.step()
    torch.cuda.synchronize(dev)
    assert bool((model.positions != before).any()) and bool(torch.isfinite(model.positions).all())
