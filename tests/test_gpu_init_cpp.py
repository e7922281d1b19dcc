"""The point-cloud initialisation through the C++ host (cuda-gaussian-splatting_amd/adapter: cugs_hip::
init_gaussians_from_sparse / knn_mean_distances) run as a native program (adapter/init_driver.bin) on the same raw inputs
as the Python host: identical bits, on every route."""
import numpy as np
import pytest

import init_ref as ir
from cpp_driver import run_driver

pytestmark = pytest.mark.gpu
NAMES = ("positions", "sh_coeffs", "opacities", "rotations", "scales")


@pytest.mark.parametrize("route", ("auto", "exhaustive", "tree"))
def test_cpp_init_matches_python_host(pkg, dev, tmp_path, route):
    from cugs_amd import gaussian_init
    n, degree, k = 30000, 2, 4
    pos, col = ir.make_cloud("blobs", n, seed=71)
    pos.tofile(tmp_path / "positions.bin")
    col.tofile(tmp_path / "colors.bin")
    res = run_driver("init_driver", tmp_path, n, degree, k, gaussian_init.ROUTES[route])
    assert f"init_driver ok n={n} coeffs=9 cuda=1 bad_degree_throws=1 empty=0" in res.stdout

    model = pkg.init_gaussians_from_sparse(pos, col, sh_degree=degree, k_neighbors=k, device=dev, route=route)
    mean = pkg.knn_mean_distances(pos, k, route=route, device=dev)
    rd = lambda name, shape: np.fromfile(tmp_path / name, np.float32).reshape(shape)
    assert rd("out_mean_dist.bin", (n,)).tobytes() == mean.cpu().numpy().tobytes()
    assert mean.cpu().numpy().tobytes() == ir.knn_mean_distances(pos, k).tobytes()
    for name in NAMES:
        want = getattr(model, name).cpu().numpy()
        assert rd(f"out_{name}.bin", want.shape).tobytes() == want.tobytes(), name
