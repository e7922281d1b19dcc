"""The depth and alpha maps through the C++ host (adapter/depth_driver.cpp: cugs_hip::render(..., want_depth_map) and
render_backward(..., dL_ddepth_map, dL_dalpha)) against the Python host on the same inputs."""
import numpy as np
import pytest
import torch

from cpp_driver import NO_LEGACY_IPC, read_f32, run_driver, write_camera, write_f32
from util import max_err_over_max, np_

pytestmark = pytest.mark.gpu


def test_cpp_depth_driver_matches_python_host(pkg, dev, tmp_path):
    w, h, n = 200, 150, 5000
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=3, seed=23, mu_s=-3.8)
    cam = pkg.scene.make_camera(w, h, view=2)
    rng = np.random.default_rng(3)
    g = pkg.scene.make_dl_dcolor(w, h)
    dD = (rng.standard_normal((h, w)) * 0.05).astype(np.float32)
    dA = (rng.standard_normal((h, w)) * 0.3).astype(np.float32)
    files = dict(positions=arrays["positions"], sh=arrays["sh_coeffs"], opacities=arrays["opacities"],
                 rotations=arrays["rotations"], scales=arrays["scales"], dl_dcolor=g, dl_ddepth=dD, dl_dalpha=dA)
    write_f32(tmp_path, **files)
    write_camera(tmp_path / "camera.f32", cam)
    run_driver("depth_driver", tmp_path, env=NO_LEGACY_IPC)

    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=3)
    out = pkg.render(model, cam, settings, want_depth_map=True)
    t = lambda a: torch.from_numpy(a).to(dev)
    grads = pkg.render_backward(t(g), out, model, cam, settings, dL_ddepth_map=t(dD), dL_dalpha=t(dA))
    rd = lambda name: read_f32(tmp_path, name)
    assert np.array_equal(rd("depth_map").view(np.uint32), np_(out.depth_map).reshape(-1).view(np.uint32))
    assert np.array_equal(rd("alpha").view(np.uint32), np_(out.alpha).reshape(-1).view(np.uint32))
    for name, k in (("d_positions", "dL_dpositions"), ("d_rotations", "dL_drotations"), ("d_scales", "dL_dscales"),
                    ("d_opacities", "dL_dopacities"), ("d_sh", "dL_dsh_coeffs")):
        assert max_err_over_max(rd(name), np_(getattr(grads, k)).reshape(-1)) <= 1e-5, name   # up to atomic order
