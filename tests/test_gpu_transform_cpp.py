"""The similarity transform and the merge through the C++ host (adapter/transform_driver.cpp: cugs_hip::Similarity,
transform_camera, transform_gaussians, merge_gaussians over ModelTensors / FusedAdam) against the Python host on the
same files: parameters bit for bit, moments zero in the same places."""
import numpy as np
import pytest
import torch

import transform_ref as tr
from cpp_driver import NO_LEGACY_IPC, read_f32, run_driver, write_camera
from util import max_err_over_max, np_

pytestmark = pytest.mark.gpu
FILES = dict(positions="positions", sh="sh_coeffs", opacities="opacities", rotations="rotations", scales="scales")


def test_cpp_transform_driver_matches_python_host(pkg, dev, tmp_path):
    w, h, n = tr.W, tr.H, 900
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=3, seed=81, mu_s=-3.0)
    other = pkg.scene.make_gaussians(250, w, h, sh_degree=1, seed=82, mu_s=-3.0)
    cam = pkg.scene.make_camera(w, h, 3)
    g = pkg.scene.make_dl_dcolor(w, h)
    mask = np.random.Generator(np.random.Philox(key=83)).uniform(size=n) < 0.5
    sim = pkg.Similarity(2.5, tr.random_rotation(84), [0.3, -0.4, 0.8])
    for name, key in FILES.items():
        np.ascontiguousarray(arrays[key], np.float32).tofile(tmp_path / f"{name}.f32")
        np.ascontiguousarray(other[key], np.float32).tofile(tmp_path / f"o_{name}.f32")
    g.tofile(tmp_path / "dl_dcolor.f32")
    mask.astype(np.float32).tofile(tmp_path / "mask.f32")
    np.concatenate([[sim.scale], sim.rotation.reshape(9), sim.translation]).astype(np.float64).tofile(tmp_path / "sim.f64")
    write_camera(tmp_path / "camera0.f32", cam)
    run_driver("transform_driver", tmp_path, env=NO_LEGACY_IPC)
    rd = lambda name: read_f32(tmp_path, name)

    moved = pkg.transform_camera(cam, sim)
    got_view = rd("camera_moved").reshape(4, 4)
    assert np.max(np.abs(got_view[:3, :3] - moved.rotation)) <= 2.0 ** -23
    assert np.max(np.abs(got_view[:3, 3] - moved.translation)) <= 2.0 ** -22 * np.max(np.abs(moved.translation))

    # the same in the Python host
    from cugs_amd.fused_adam import AdamConfig, PositionLRConfig
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=3)
    model = pkg.scene.to_model({k: v.copy() for k, v in arrays.items()}, dev)
    zero_lr = AdamConfig(position_lr_config=PositionLRConfig(lr_init=0.0, lr_final=0.0), lr_sh_coeffs=0.0,
                         lr_opacities=0.0, lr_scales=0.0, lr_rotations=0.0)
    opt = pkg.FusedAdam(model, zero_lr)
    out = pkg.render(model, cam, settings)
    opt.apply_gradients(pkg.render_backward(torch.from_numpy(g).to(dev), out, model, cam, settings))
    opt.step()

    def compare(prefix, mname, vname):
        for name, key in FILES.items():
            assert np.array_equal(rd(prefix + name).view(np.uint32),
                                  np_(getattr(model, key)).reshape(-1).view(np.uint32)), (prefix, name)   # bit for bit
        for k in range(5):
            for tag, mine in ((mname, opt.m_[k]), (vname, opt.v_[k])):
                theirs, mine = rd(f"{tag}{k}").reshape(mine.shape), np_(mine)
                if k in (0, 1, 4):                                    # positions, SH, rotations: the moved rows start over
                    assert not theirs[:n][mask].any() and not mine[:n][mask].any(), (tag, k)
                assert not theirs[n:].any() and not mine[n:].any(), (tag, k)               # merged rows: zero moments
                assert mine.any() and max_err_over_max(theirs, mine) <= 1e-5, (tag, k)     # up to atomic order

    pkg.transform_gaussians(model, sim, mask=torch.from_numpy(mask).to(dev), optimizer=opt)
    want = tr.mirror32(arrays, sim.to_abi(), mask)
    for key in tr.PARAMS:
        assert np.array_equal(np_(getattr(model, key)).view(np.uint32), want[key].view(np.uint32)), key
    assert not opt.m_[0][torch.from_numpy(mask).to(dev)].any()
    compare("t_", "tm_", "tv_")
    assert pkg.merge_gaussians(model, pkg.scene.to_model(other, dev), opt) == n + 250
    assert rd("p_sh").size == (n + 250) * 48
    compare("p_", "m_", "v_")
