"""The absolute 2-D mean gradients through the C++ host (adapter/absgrad_driver.cpp: cugs_hip::render_backward(...,
want_abs_grad) and DensificationController::accumulate_gradients on the strided view) against the Python host on the
same inputs."""
import pytest
import torch

from cpp_driver import NO_LEGACY_IPC, read_f32, run_driver, write_camera, write_f32
from util import max_err_over_max, np_

pytestmark = pytest.mark.gpu


def test_cpp_absgrad_driver_matches_python_host(pkg, dev, tmp_path):
    w, h, n = 200, 150, 5000
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=3, seed=23, mu_s=-3.8)
    cam = pkg.scene.make_camera(w, h, view=2)
    g = pkg.scene.make_dl_dcolor(w, h)
    files = dict(positions=arrays["positions"], sh=arrays["sh_coeffs"], opacities=arrays["opacities"],
                 rotations=arrays["rotations"], scales=arrays["scales"], dl_dcolor=g)
    write_f32(tmp_path, **files)
    write_camera(tmp_path / "camera.f32", cam)
    run_driver("absgrad_driver", tmp_path, env=NO_LEGACY_IPC)

    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=3)
    out = pkg.render(model, cam, settings)
    grads = pkg.render_backward(torch.from_numpy(g).to(dev), out, model, cam, settings, want_abs_grad=True)
    ctl = pkg.DensificationController(pkg.DensificationConfig(), 5.0)
    ctl.accumulate_gradients(grads.dL_dmeans_2d_abs, out.radii)
    rd = lambda name: read_f32(tmp_path, name)
    assert np_(grads.dL_dmeans_2d_abs).max() > 0
    for name, got in (("d_means_abs", grads.dL_dmeans_2d_abs), ("densify_accum", ctl.grad_accum_),
                      ("d_positions", grads.dL_dpositions), ("d_rotations", grads.dL_drotations),
                      ("d_scales", grads.dL_dscales), ("d_opacities", grads.dL_dopacities),
                      ("d_sh", grads.dL_dsh_coeffs)):
        assert max_err_over_max(rd(name), np_(got).reshape(-1)) <= 1e-5, name   # up to atomic order
