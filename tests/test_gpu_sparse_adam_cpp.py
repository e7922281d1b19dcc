"""Sparse Adam through the C++ host (adapter/sparse_adam_driver.cpp: cugs_hip::FusedAdam::step(visible) and
render_backward(..., sparse_adam = true)) against the Python host on the same raw inputs.  The masked step on given
gradients gives the same bytes.  The fused route ran its own backward blend, whose float atomics may sum in another
order than the Python host's: there the rows the view does not see are compared bit for bit (they keep the bytes of
the input) and the stepped rows up to that order, as tests/test_gpu_mcmc_cpp.py does."""
import numpy as np
import pytest
import torch

from cpp_driver import NO_LEGACY_IPC, read_f32, run_driver, write_camera
from sparse_adam_ref import standard_invisible
from util import np_

pytestmark = pytest.mark.gpu
FILES = (("positions", "positions"), ("sh", "sh_coeffs"), ("opacities", "opacities"), ("rotations", "rotations"),
         ("scales", "scales"))
GROUPS = ("positions", "sh_coeffs", "opacities", "scales", "rotations")          # ParamGroup order


def test_cpp_sparse_adam_driver_matches_python_host(pkg, dev, tmp_path):
    n, w, h, deg = 1301, 128, 96, 3
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=deg, seed=31, mu_s=-3.7)
    inv = standard_invisible(n)
    arrays["positions"][inv, 2] *= -1.0
    cam = pkg.scene.make_camera(w, h)
    g = (pkg.scene.make_dl_dcolor(w, h, seed=32) * 3000.0).astype(np.float32)
    rng = np.random.default_rng(33)
    grads = {k: (rng.standard_normal(v.shape) * 1e-2).astype(np.float32) for k, v in arrays.items()}
    for f, k in FILES:
        np.ascontiguousarray(arrays[k], np.float32).tofile(tmp_path / f"{f}.f32")
        grads[k].tofile(tmp_path / f"g_{f}.f32")
    g.tofile(tmp_path / "dl_dcolor.f32")
    write_camera(tmp_path / "camera.f32", cam)
    res = run_driver("sparse_adam_driver", tmp_path, env=NO_LEGACY_IPC)
    assert "fused_grads_undefined=1 needs_fused=1 no_mcmc=1 untouched=1" in res.stdout, res.stdout
    rd = lambda name: read_f32(tmp_path, name)

    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=deg)
    model = pkg.scene.to_model({k: v.copy() for k, v in arrays.items()}, dev)
    out = pkg.render(model, cam, settings)
    radii = np_(out.radii)
    assert np.array_equal(rd("radii").astype(np.int32), radii)
    assert (radii[inv] == 0).all() and 0.25 <= float((radii <= 0).mean()) <= 0.75

    # (a) two masked steps on the given gradients: the same bytes
    opt = pkg.FusedAdam(model)
    G = {k: torch.from_numpy(v).to(dev) for k, v in grads.items()}
    for _ in range(2):
        opt.apply_gradients(pkg.BackwardOutput(G["positions"], G["rotations"], G["scales"], G["opacities"],
                                               G["sh_coeffs"], None))
        opt.step(visible=out.radii)
    for f, k in FILES:
        want = np_(getattr(model, k)).reshape(-1)
        assert np.array_equal(rd(f"a_{f}").view(np.uint32), want.view(np.uint32)), k
        assert not np.array_equal(want, arrays[k].reshape(-1)), k
    for i in range(5):
        assert np.array_equal(rd(f"a_m_{i}").view(np.uint32), np_(opt.m_[i]).reshape(-1).view(np.uint32)), i
        assert np.array_equal(rd(f"a_v_{i}").view(np.uint32), np_(opt.v_[i]).reshape(-1).view(np.uint32)), i

    # (b) the fused route
    m2 = pkg.scene.to_model({k: v.copy() for k, v in arrays.items()}, dev)
    opt2 = pkg.FusedAdam(m2)
    r2 = pkg.render_backward(torch.from_numpy(g).to(dev), pkg.render(m2, cam, settings), m2, cam, settings, fused_adam=opt2,
                             sparse_adam=True)
    unseen = radii <= 0
    dm = rd("b_means_2d").reshape(n, 2)
    assert (dm[unseen] == 0).all() and np.abs(dm - np_(r2.dL_dmeans_2d)).max() <= 1e-5 * np.abs(dm).max()
    for f, k in FILES:
        got = rd(f"b_{f}").reshape(arrays[k].shape)
        want = np_(getattr(m2, k))
        assert np.array_equal(got[unseen].view(np.uint32), arrays[k][unseen].view(np.uint32)), k       # bit for bit
        assert np.array_equal(want[unseen].view(np.uint32), arrays[k][unseen].view(np.uint32)), k
        close = np.abs(got.astype(np.float64) - want) <= 1e-6 * np.maximum(np.abs(want), 1.0)
        assert close.mean() > 0.999, (k, close.mean())
        assert not np.array_equal(want[~unseen], arrays[k][~unseen]), k                               # the step moved them
    for i, k in enumerate(GROUPS):
        for tag, mine in (("m", opt2.m_[i]), ("v", opt2.v_[i])):
            got = rd(f"b_{tag}_{i}").reshape(arrays[k].shape)
            assert not got[unseen].any() and not np_(mine)[unseen].any(), (tag, k)                    # still zero
