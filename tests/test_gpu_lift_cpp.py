"""Pixel maps lifted onto Gaussians through the C++ host (adapter/lift_driver.cpp: cugs_hip::lift_pixel_maps, lift_maps,
vote_labels, error_scores, select_gaussians over ModelTensors / FusedAdam) against the Python host on the same inputs,
and against the reference of tests/lift_ref.py."""
import numpy as np
import pytest
import torch

import lift_ref
from cpp_driver import NO_LEGACY_IPC, read_f32, run_driver, write_camera, write_f32
from scores_ref import scene
from util import max_err_over_max, np_

pytestmark = pytest.mark.gpu
KEY, IMAGE, KEEP = "40x24", "grid", 4


def test_cpp_lift_driver_matches_python_host(pkg, dev, tmp_path):
    s0, s1 = scene(KEY, 0), scene(KEY, 1)
    arrays, n, w, h = s0["arrays"], s0["n"], s0["w"], s0["h"]
    cams = (s0["cam"], s1["cam"])
    num = lift_ref.LABEL_IMAGES[IMAGE]
    g = pkg.scene.make_dl_dcolor(w, h)
    lab = lift_ref.label_image(KEY, IMAGE)
    files = dict(positions=arrays["positions"], sh=arrays["sh_coeffs"], opacities=arrays["opacities"],
                 rotations=arrays["rotations"], scales=arrays["scales"], dl_dcolor=g, labels=lab,
                 map0=lift_ref.float_map(KEY, 0, 4), map1=lift_ref.float_map(KEY, 1, 4),
                 err0=lift_ref.error_map(KEY, 0), err1=lift_ref.error_map(KEY, 1))
    write_f32(tmp_path, **files)
    for i, cam in enumerate(cams):
        write_camera(tmp_path / f"camera{i}.f32", cam)
    run_driver("lift_driver", tmp_path, num, KEEP, env=NO_LEGACY_IPC)
    rd = lambda name: read_f32(tmp_path, name)

    # the same in the Python host
    from cugs_amd.fused_adam import AdamConfig, PositionLRConfig
    t = lambda a: torch.tensor(np.asarray(a)).to(dev)
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=0)
    model = pkg.scene.to_model({k: v.copy() for k, v in arrays.items()}, dev)
    maps = [t(files["map0"]), t(files["map1"])]
    errs = [t(files["err0"]), t(files["err1"])]
    lifted = pkg.lift_maps(model, cams, maps, settings)
    want = lift_ref.combine(lift_ref.lifted(KEY, 0, 4), lift_ref.lifted(KEY, 1, 4))
    for tag in ("a", "b"):
        got = rd(f"{tag}_sums").reshape(n, 4)
        lift_ref.check(got, want, f"C++ {tag}")
        assert max_err_over_max(got, np_(lifted.sums)) <= 1e-5, tag                     # up to atomic order
    out = pkg.render(model, cams[0], settings, for_backward=False)
    window = pkg.lift_pixel_maps(pkg.LiftedMaps(n, dev, 2), out, cams[0], labels=t(lab), label_base=1)
    got = rd("c_sums").reshape(n, 2)
    lift_ref.check(got, lift_ref.wanted(s0["table"], lift_ref.one_hot(lab, num)[..., 1:3]), "C++ label window")
    assert max_err_over_max(got, np_(window.sums)) <= 1e-5
    labels, votes = pkg.vote_labels(model, cams, [t(lab), t(lab)], num, settings)
    ref_votes = lift_ref.votes(KEY, IMAGE, (0, 1))
    got_labels = rd("labels.out").astype(np.int64)
    assert np.array_equal(got_labels, np_(labels)) and np.array_equal(got_labels, ref_votes["label"])
    lift_ref.check(rd("votes").reshape(n, num), ref_votes, "C++ votes")
    assert max_err_over_max(rd("votes").reshape(n, num), np_(votes)) <= 1e-5
    for tag, reduce in (("err_max", "max"), ("err_sum", "sum")):
        assert max_err_over_max(rd(tag), np_(pkg.error_scores(model, cams, errs, settings, reduce=reduce))) <= 1e-5, tag
    e = lift_ref.errors(KEY)
    lift_ref.check(rd("err_max")[:, None], dict(sum=e["max"][:, None], bound=e["max_bound"][:, None],
                                                count=e["per_view"][0]["count"]), "C++ error_scores")

    zero_lr = AdamConfig(position_lr_config=PositionLRConfig(lr_init=0.0, lr_final=0.0), lr_sh_coeffs=0.0,
                         lr_opacities=0.0, lr_scales=0.0, lr_rotations=0.0)
    opt = pkg.FusedAdam(model, zero_lr)
    out = pkg.render(model, cams[0], settings)
    opt.apply_gradients(pkg.render_backward(torch.from_numpy(g).to(dev), out, model, cams[0], settings))
    opt.step()
    kept = pkg.select_gaussians(model, labels == KEEP, opt)
    assert 0 < kept < n and kept == int((ref_votes["label"] == KEEP).sum()) and int(rd("kept")[0]) == kept
    for name, got in (("p_positions", model.positions), ("p_sh", model.sh_coeffs), ("p_opacities", model.opacities),
                      ("p_rotations", model.rotations), ("p_scales", model.scales)):
        assert np.array_equal(rd(name), np_(got).reshape(-1)), name                      # bit for bit
    for k in range(5):
        assert np_(opt.m_[k]).any()
        assert max_err_over_max(rd(f"m_{k}"), np_(opt.m_[k]).reshape(-1)) <= 1e-5, k       # up to atomic order
        assert max_err_over_max(rd(f"v_{k}"), np_(opt.v_[k]).reshape(-1)) <= 1e-5, k
