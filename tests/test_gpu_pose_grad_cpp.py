"""The camera-pose gradient through the C++ host (adapter/pose_driver.cpp: cugs_hip::render_backward(...,
want_camera_grad = true) with the depth and alpha map gradients) against the Python host on the same inputs."""
import numpy as np
import pytest
import torch

from cpp_driver import NO_LEGACY_IPC, read_f32, run_driver, write_camera, write_f32
from util import max_err_over_max, np_

pytestmark = pytest.mark.gpu


def test_cpp_pose_driver_matches_python_host(pkg, dev, tmp_path):
    w, h, n = 200, 150, 5000
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=3, seed=29, mu_s=-3.8)
    cam = pkg.pose.apply_se3(pkg.scene.make_camera(w, h, view=2), [0.05, -0.03, 0.1, 0.04, -0.06, 0.03])
    rng = np.random.default_rng(4)
    g = pkg.scene.make_dl_dcolor(w, h)
    dD = (rng.standard_normal((h, w)) * 1e-4).astype(np.float32)
    dA = (rng.standard_normal((h, w)) * 1e-4).astype(np.float32)
    files = dict(positions=arrays["positions"], sh=arrays["sh_coeffs"], opacities=arrays["opacities"],
                 rotations=arrays["rotations"], scales=arrays["scales"], dl_dcolor=g, dl_ddepth=dD, dl_dalpha=dA)
    write_f32(tmp_path, **files)
    write_camera(tmp_path / "camera.f32", cam)
    run_driver("pose_driver", tmp_path, env=NO_LEGACY_IPC)

    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=3)
    out = pkg.render(model, cam, settings, want_depth_map=True)
    t = lambda a: torch.from_numpy(a).to(dev)
    grads = pkg.render_backward(t(g), out, model, cam, settings, dL_ddepth_map=t(dD), dL_dalpha=t(dA),
                                want_camera_grad=True)
    rd = lambda name: read_f32(tmp_path, name)
    view = rd("d_view").reshape(4, 4)
    want = np_(grads.dL_dviewmat)
    assert (view[3] == 0.0).all() and np.abs(want).max() > 0.0
    # both hosts run the same kernels on the same inputs; the blend backward's scatter (float atomics) may order the
    # accumulator's additions differently from run to run, so the bits agree up to that order
    assert max_err_over_max(view, want) <= 1e-5
    assert max_err_over_max(rd("d_positions"), np_(grads.dL_dpositions).reshape(-1)) <= 1e-5
