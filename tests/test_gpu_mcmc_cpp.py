"""N5 through the C++ host (cuda-gaussian-splatting_amd/adapter: cugs_hip::MCMCController and
render_backward(..., FusedAdam*, const MCMCController*, step)) run as a native program (adapter/mcmc_driver.bin) on
the same raw inputs as the Python mirror: regulariser + FusedAdam step + position noise + relocation give the same
bytes; the fused route through render_backward agrees up to the blend backward's atomic summation order."""
import numpy as np
import pytest
import torch

from cpp_driver import run_driver

pytestmark = pytest.mark.gpu
NAMES = ("positions", "sh_coeffs", "opacities", "rotations", "scales")


def test_cpp_mcmc_matches_python_host(pkg, dev, tmp_path):
    w, h, n, deg = 200, 150, 5000, 3
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=deg, seed=23, mu_s=-3.8)
    arrays["opacities"][::5] = -7.0                                  # a fifth dead: relocation has work
    cam = pkg.scene.make_camera(w, h, view=1)
    bg = [0.1, 0.2, 0.3]
    dl = pkg.scene.make_dl_dcolor(w, h) * 100.0
    rng = np.random.default_rng(5)
    grads = {k: (rng.standard_normal(v.shape) * 1e-4).astype(np.float32) for k, v in arrays.items()}
    for k, v in arrays.items():
        np.ascontiguousarray(v, np.float32).tofile(tmp_path / f"{k}.bin")
        grads[k].tofile(tmp_path / f"g_{k}.bin")
    dl.tofile(tmp_path / "dl_dcolor.bin")
    abi = cam.to_abi()
    np.array(list(abi.view) + [abi.fx, abi.fy, abi.cx, abi.cy] + list(abi.cam_center) + bg,
             np.float32).tofile(tmp_path / "camera.bin")
    res = run_driver("mcmc_driver", tmp_path, n, "16", w, h)
    assert "fused_grads_undefined=1 needs_fused=1" in res.stdout

    # the Python mirror of the same configuration (mcmc_driver.cpp); noise_lr_max_steps = 1 keeps the schedule at its
    # end point, so both hosts use the same learning rate whatever their libm's logf / expf
    cfg = pkg.MCMCConfig(relocate_cap=0.1, noise_lr_init=0.5, noise_lr_final=0.05, noise_lr_max_steps=1,
                         lambda_opacity=0.05, lambda_scale=0.05, seed=4242)
    ctrl = pkg.MCMCController(cfg, 5.0)
    m = pkg.scene.to_model(arrays, dev)
    opt = pkg.FusedAdam(m)
    value, r_o, r_s = ctrl.compute_regularization(m)
    G = {k: torch.from_numpy(v).to(dev) for k, v in grads.items()}
    opt.apply_gradients(pkg.BackwardOutput(G["positions"], G["rotations"], G["scales"] + r_s, G["opacities"] + r_o,
                                           G["sh_coeffs"], None))
    opt.step()
    ctrl.inject_noise(m, 3)
    st = ctrl.relocate(m, 3, optimizer=opt)
    assert st.num_relocated == int(np.float32(0.1) * np.float32(n)) and st.num_dead >= n // 5
    line = [l for l in res.stdout.splitlines() if l.startswith("relocate ")][0]
    assert line == f"relocate dead={st.num_dead} moved={st.num_relocated} total={n} should=1,0", line
    rd = lambda name, shape: np.fromfile(tmp_path / name, np.float32).reshape(shape)
    assert rd("out_value.bin", (1,))[0].tobytes() == value.cpu().numpy().tobytes()
    for k in NAMES:
        got = rd(f"out_{k}.bin", arrays[k].shape)
        assert got.tobytes() == getattr(m, k).cpu().numpy().tobytes(), k

    # the fused route: two processes ran two backward blends, whose float atomics may sum in different orders
    m2 = pkg.scene.to_model(arrays, dev)
    opt2 = pkg.FusedAdam(m2)
    settings = pkg.RenderSettings(background=bg, active_sh_degree=deg)
    out = pkg.render(m2, cam, settings)
    pkg.render_backward(torch.from_numpy(dl).to(dev), out, m2, cam, settings, fused_adam=opt2, mcmc=ctrl, mcmc_step=3)
    for k in ("positions", "opacities", "scales"):
        got = rd(f"out_fused_{k}.bin", arrays[k].shape).astype(np.float64)
        want = getattr(m2, k).cpu().numpy().astype(np.float64)
        close = np.abs(got - want) <= 1e-6 * np.maximum(np.abs(want), 1.0)
        assert close.mean() > 0.999, (k, close.mean())
        assert not np.array_equal(want, arrays[k])                   # the step moved them
