"""Contribution scores and score-based pruning through the C++ host (adapter/scores_driver.cpp:
cugs_hip::accumulate_contribution_scores, contribution_scores, prune_by_scores over ModelTensors / FusedAdam) against
the Python host on the same inputs, and against the reference of tests/scores_ref.py."""
import numpy as np
import pytest
import torch

from cpp_driver import NO_LEGACY_IPC, read_f32, run_driver, write_camera, write_f32
from scores_ref import combine, scene
from util import max_err_over_max, np_

pytestmark = pytest.mark.gpu
TINY = float(np.nextafter(np.float32(0.0), np.float32(1.0)))


def test_cpp_scores_driver_matches_python_host(pkg, dev, tmp_path):
    s0, s1 = scene("40x24", 0), scene("40x24", 1)
    arrays, n, w, h = s0["arrays"], s0["n"], s0["w"], s0["h"]
    cams = (s0["cam"], s1["cam"])
    g = pkg.scene.make_dl_dcolor(w, h)
    files = dict(positions=arrays["positions"], sh=arrays["sh_coeffs"], opacities=arrays["opacities"],
                 rotations=arrays["rotations"], scales=arrays["scales"], dl_dcolor=g)
    write_f32(tmp_path, **files)
    for i, cam in enumerate(cams):
        write_camera(tmp_path / f"camera{i}.f32", cam)
    res = run_driver("scores_driver", tmp_path, env=NO_LEGACY_IPC)
    rd = lambda name: read_f32(tmp_path, name)

    # the same in the Python host
    from cugs_amd.fused_adam import AdamConfig, PositionLRConfig
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=0)
    model = pkg.scene.to_model({k: v.copy() for k, v in arrays.items()}, dev)
    scores = pkg.contribution_scores(model, cams, settings)
    want = combine(s0["want"], s1["want"])
    for tag in ("a", "b"):
        assert np.array_equal(rd(f"{tag}_count").astype(np.int64), np_(scores.pixel_count)), tag
        assert np.array_equal(rd(f"{tag}_count").astype(np.int64), want["count"]), tag
        assert np.array_equal(rd(f"{tag}_max").view(np.uint32), np_(scores.weight_max).view(np.uint32)), tag
        assert np.array_equal(rd(f"{tag}_max").view(np.uint32), want["max"].view(np.uint32)), tag
        assert max_err_over_max(rd(f"{tag}_sum"), np_(scores.weight_sum)) <= 1e-5, tag      # up to atomic order
    zero_lr = AdamConfig(position_lr_config=PositionLRConfig(lr_init=0.0, lr_final=0.0), lr_sh_coeffs=0.0,
                         lr_opacities=0.0, lr_scales=0.0, lr_rotations=0.0)
    opt = pkg.FusedAdam(model, zero_lr)
    out = pkg.render(model, cams[0], settings)
    opt.apply_gradients(pkg.render_backward(torch.from_numpy(g).to(dev), out, model, cams[0], settings))
    opt.step()
    removed = pkg.prune_by_scores(model, scores, min_max_weight=TINY, optimizer=opt)
    assert removed == int((want["count"] == 0).sum()) and int(rd("removed")[0]) == removed
    for name, got in (("p_positions", model.positions), ("p_sh", model.sh_coeffs), ("p_opacities", model.opacities),
                      ("p_rotations", model.rotations), ("p_scales", model.scales)):
        assert np.array_equal(rd(name), np_(got).reshape(-1)), name                      # bit for bit
    for k in range(5):
        assert np_(opt.m_[k]).any()
        assert max_err_over_max(rd(f"m_{k}"), np_(opt.m_[k]).reshape(-1)) <= 1e-5, k       # up to atomic order
        assert max_err_over_max(rd(f"v_{k}"), np_(opt.v_[k]).reshape(-1)) <= 1e-5, k
