"""Point-cloud initialisation without a GPU: the numpy restatement tests/init_ref.py on cases that can be
worked out by hand, the statement that any summation order of the k terms stays within k ulp of the ascending one, and the
argument checks of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import init_ref as ir

F = np.float32


@pytest.fixture(scope="module")
def api(pkg):
    """Every test here is about the new interface: none can pass without it."""
    assert callable(pkg.init_gaussians_from_sparse) and callable(pkg.knn_mean_distances)
    from cugs_amd import gaussian_init
    return gaussian_init


def _lattice():
    g = np.arange(3, dtype=F)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def test_lattice_centre_and_corners(api):
    pos = _lattice()                                               # the reference's ScaleIsReasonable: spacing 1
    col = np.full((27, 3), 128, np.uint8)
    ref = ir.init_model(pos, col, sh_degree=0, k_neighbors=3)
    centre = 13
    assert np.array_equal(pos[centre], [1, 1, 1])
    assert ref["mean_dist"][centre] == 1.0 and np.all(ref["scales"][centre] == 0.0)
    for corner in (0, 2, 6, 8, 18, 20, 24, 26):
        assert ref["mean_dist"][corner] == 1.0
    assert np.all(ref["mean_dist"] == 1.0)                          # every lattice point has three neighbours at 1
    assert ref["sh_coeffs"].shape == (27, 3, 1)
    assert np.all(ref["sh_coeffs"] == (F(128) / F(255) - F(0.5)) / ir.SH_C0)
    assert np.all(ref["rotations"] == [1, 0, 0, 0]) and np.all(ref["opacities"] == F(-2.1972245773362196))


def test_two_points_and_clamped_k(api):
    two = np.array([[0, 0, 0], [3, 4, 0]], F)
    assert np.array_equal(ir.knn_mean_distances(two, 3), [5, 5])   # k clamped to 1
    line = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]], F)
    assert np.array_equal(ir.knn_mean_distances(line, 3), [2, 1.5, 2.5])          # k = 3 clamped to 2
    assert np.array_equal(ir.knn_mean_distances(np.zeros((1, 3), F), 3), [1])
    assert ir.knn_mean_distances(np.zeros((0, 3), F), 3).shape == (0,)
    assert np.array_equal(ir.knn_mean_distances(line, 3, queries=[2, 0]), [2.5, 2])


def test_duplicates_are_neighbours_at_distance_zero(api):
    pos = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 3], [5, 1, 1]], F)
    m = ir.knn_mean_distances(pos, 2)
    assert np.array_equal(m, [1, 1, 2, 4])                          # (0 + 2) / 2, (0 + 2) / 2, (2 + 2) / 2, (4 + 4) / 2
    same = np.ones((5, 3), F) * F(0.25)
    ref = ir.init_model(same, np.zeros((5, 3), np.uint8), 1, 3)
    assert np.all(ref["mean_dist"] == 0.0)
    assert np.all(ref["scales"] == np.log(np.float64(F(1e-7))).astype(F))


def test_any_summation_order_is_within_k_ulp_of_ascending(api):
    """What the contract says about the reference, whose nth_element leaves the order of the k terms open."""
    pos, _ = ir.make_cloud("uniform", 10000, seed=3)
    rng = np.random.default_rng(4)
    for k in (3, 8, 16):
        best = ir.knn_sq_distances(pos, k)
        m = ir.mean_of_sorted(best)
        worst = 0.0
        for _ in range(20):
            perm = rng.permuted(best, axis=1)
            other = ir.mean_of_sorted(perm)
            worst = max(worst, float(np.max(np.abs(other.astype(np.float64) - m) / np.spacing(m))))
        print(f"k={k}: worst {worst} ulp")
        assert worst <= k


def test_clouds_have_the_stated_shape(api):
    for kind in ("uniform", "blobs", "plane"):
        pos, col = ir.make_cloud(kind, 5000, seed=1)
        pos2, col2 = ir.make_cloud(kind, 5000, seed=1)
        assert pos.dtype == F and pos.shape == (5000, 3) and col.dtype == np.uint8 and col.shape == (5000, 3)
        assert np.array_equal(pos, pos2) and np.array_equal(col, col2)
    assert np.all(ir.make_cloud("plane", 100)[0][:, 2] == F(1.5))
    far = np.abs(ir.make_cloud("blobs", 20000)[0] - 5.0).max(axis=1) > 20.0
    assert 0.005 < far.mean() < 0.015


def test_knn_abi_argument_validation_without_gpu(api):
    from cugs_amd._lib import lib
    null, fake = C.c_void_p(0), C.c_void_p(0x1000)
    knn = lambda n, k, p, m, ws, wsb, route: lib.cugs_knn_mean_distances(n, k, p, m, ws, wsb, route, null)
    big = 1 << 40
    for route in (0, 1, 2):
        assert knn(0, 3, null, null, null, 0, route) == 0          # n == 0: nothing queued
        assert knn(-1, 3, fake, fake, fake, big, route) == -1
        assert knn(10, 0, fake, fake, fake, big, route) == -1
        assert knn(10, 17, fake, fake, fake, big, route) == -1
        assert knn(10, 3, null, fake, fake, big, route) == -1
        assert knn(10, 3, fake, null, fake, big, route) == -1
    assert knn(10, 3, fake, fake, fake, big, 3) == -1 and knn(10, 3, fake, fake, fake, big, -1) == -1
    for route in (0, 2):                                            # a short workspace, before anything is queued
        assert knn(100000, 3, fake, fake, fake, 16, route) == -4
        assert knn(100000, 3, fake, fake, fake, lib.cugs_knn_workspace_bytes(100000, 3) - 1, route) == -4
        assert knn(100000, 3, fake, fake, null, big, route) == -1
    sizes = [lib.cugs_knn_workspace_bytes(n, 3) for n in (0, 1, 2, 100, 4096, 4097, 100000, 1 << 20, 6 << 20, 16 << 20)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[3]
    assert lib.cugs_knn_workspace_bytes(-1, 3) == 0 and lib.cugs_knn_workspace_bytes(10, 0) == 0
    assert lib.cugs_knn_workspace_bytes(10, 17) == 0
    fill = lambda n, c, p: lib.cugs_init_from_points(n, c, p, p, p, p, p, p, p, p, null)
    assert fill(0, 16, null) == 0
    assert fill(-1, 16, fake) == -1
    assert fill(10, 5, fake) == -1 and fill(0, 0, null) == -1
    assert fill(10, 16, null) == -1
    assert lib.cugs_init_from_points(10, 4, fake, fake, fake, fake, fake, fake, fake, null, null) == -1


def test_host_argument_checks_without_gpu(api):
    pos, col = np.zeros((4, 3), F), np.zeros((4, 3), np.uint8)
    with pytest.raises(RuntimeError, match=r"SH degree must be 0\.\.3, got 4"):
        api.init_gaussians_from_sparse(pos, col, sh_degree=4, device="cpu")
    with pytest.raises(RuntimeError, match=r"SH degree must be 0\.\.3, got -1"):
        api.init_gaussians_from_sparse(pos, col, sh_degree=-1, device="cpu")
    with pytest.raises(RuntimeError, match="positions must be"):
        api.knn_mean_distances(np.zeros((4, 2), F), device="cpu")
    with pytest.raises(RuntimeError, match="k_neighbors must be 1..16"):
        api.knn_mean_distances(pos, 17, device="cpu")
    with pytest.raises(RuntimeError, match="route must be"):
        api.knn_mean_distances(pos, 3, route="grid", device="cpu")
    with pytest.raises(RuntimeError, match="colors must be uint8"):
        api.init_gaussians_from_sparse(pos, col.astype(np.float32), device="cpu")
    with pytest.raises(RuntimeError, match=r"colors must be \[N, 3\]"):
        api.init_gaussians_from_sparse(pos, col[:3], device="cpu")
