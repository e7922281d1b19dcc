"""The adaptive-density training loop on the device, checked stage by stage against the CPU oracles
(tests/trainloop_ref.py; the scenario and what it reaches are pinned by tests/test_trainloop_ref.py).

The device runs all 48 steps and is the master trajectory.  After each stage the oracle recomputes that ONE stage from
the device's own inputs, downloaded, and the two are compared at the bars the stage tests use.  The trajectories are
not compared freely: Adam turns a last-bit difference in a near-zero gradient into a full lr step.

Four routes:
  step      zero_grad / apply_gradients / step(), densify(optimizer=opt)                          carried moments
  rebuilt   the same step, densify() alone and a new FusedAdam + update_lr(step) after a change   the reference's trainer
  fused     render_backward(..., fused_adam=opt), densify(optimizer=opt)                          carried
  sparse    render_backward(..., fused_adam=opt, sparse_adam=True), densify(optimizer=opt)        carried
"""
import numpy as np
import pytest
import torch

import trainloop_ref as tl
from util import max_err_over_max, np_

pytestmark = pytest.mark.gpu

ROUTES = ("step", "rebuilt", "fused", "sparse")


@pytest.fixture(scope="module")
def ctx(pkg, orc):
    import __graft_entry__ as ge
    return tl.Ctx(orc, ge.load_oracle_module("loss_oracle"), ge.load_oracle_module("densify_oracle"), pkg.scene)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))


def _model(model):
    return {k: np_(getattr(model, k)).copy() for k in tl.MODEL_KEYS}


def _moments(opt):
    """(m, v) by parameter name; FusedAdam keeps them in ParamGroup order, which is tl.PARAMS."""
    assert tuple(opt._names) == tl.PARAMS
    return ({k: np_(opt.m_[i]).copy() for i, k in enumerate(tl.PARAMS)},
            {k: np_(opt.v_[i]).copy() for i, k in enumerate(tl.PARAMS)})


def _accumulators(ctrl, n):
    """The controller's three accumulators, or None where it would start afresh at `n` rows."""
    if ctrl.grad_accum_ is None or int(ctrl.grad_accum_.shape[0]) != n:
        return None
    return (np_(ctrl.grad_accum_).copy(), np_(ctrl.grad_count_).copy(), np_(ctrl.max_radii_2d_).copy())


def _adam_config(pkg):
    return pkg.AdamConfig(position_lr_config=pkg.PositionLRConfig(lr_init=tl.LRS[0], lr_final=tl.POS_LR_FINAL,
                                                                  max_steps=tl.POS_LR_MAX_STEPS),
                          lr_sh_coeffs=tl.LRS[1], lr_opacities=tl.LRS[2], lr_scales=tl.LRS[3], lr_rotations=tl.LRS[4],
                          beta1=tl.BETA1, beta2=tl.BETA2, eps=tl.EPS)


def _check_forward(out, ref, step):
    assert np.array_equal(np_(out.radii), ref["radii"]), step
    assert int(out.total_pairs) == int(ref["total_pairs"]), step
    assert np.array_equal(np_(out.gaussian_indices), ref["values"]), step
    assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"]), step
    assert np.array_equal(np_(out.n_contrib), ref["n_contrib"]), step
    _same_bits(np_(out.color), ref["color"], ("color", step))
    _same_bits(np_(out.final_T), ref["final_T"], ("final_T", step))


def _check_densify(ctx, pkg, ctrl, model, opt, carried, step, dev):
    """One event: the device's densify against the oracle controller on the device's accumulators and pre-event model,
    same noise.  Returns (stats, the optimizer to go on with, the oracle's accumulators after the event)."""
    n = model.num_gaussians()
    acc = _accumulators(ctrl, n)
    assert acc is not None, step
    pre = _model(model)
    pre_m, pre_v = _moments(opt)
    count = opt.step_count_
    noise = tl.split_noise(step, n)
    want, want_stats, info, want_acc = tl.densify_stage(ctx, pre, acc, step, noise)
    s = ctrl.densify(model, step, torch.from_numpy(noise).to(dev), optimizer=opt if carried else None)
    assert (s.num_before, s.num_cloned, s.num_split, s.num_pruned, s.num_after) == \
        (want_stats.num_before, want_stats.num_cloned, want_stats.num_split, want_stats.num_pruned,
         want_stats.num_after), step
    assert model.num_gaussians() == s.num_after and model.is_valid()
    got = _model(model)
    kids = s.num_after - 2 * s.num_split                  # survivors, then clones: copied rows; then the split children
    for k in tl.MODEL_KEYS:
        _same_bits(got[k][:kids], want[k][:kids], (k, "copied rows", step))
        if k == "positions":                              # parent + noise * exp(scale - log 1.6): the bars of test_gpu_densify.py
            assert np.max(np.abs(got[k][kids:] - want[k][kids:]), initial=0.0) <= 1e-6 * max(1.0, np.abs(want[k]).max()), step
        elif k == "scales":
            assert np.allclose(got[k][kids:], want[k][kids:], rtol=0, atol=1e-6), step
        else:
            _same_bits(got[k][kids:], want[k][kids:], (k, "children", step))
    for name in ("grad_accum_", "grad_count_", "max_radii_2d_"):
        t = getattr(ctrl, name)
        assert int(t.shape[0]) == s.num_after and not bool(t.any()), (name, step)
    if carried:
        want_m, want_v = tl.carry_moments(pre_m, pre_v, info["survivors"], s.num_after)
        got_m, got_v = _moments(opt)
        for k in tl.PARAMS:
            _same_bits(got_m[k], want_m[k], ("m", k, step))
            _same_bits(got_v[k], want_v[k], ("v", k, step))
        assert opt.step_count_ == count
    elif tl.changed(s):
        opt = pkg.FusedAdam(model, _adam_config(pkg))
        opt.update_lr(step)
        assert opt.step_count_ == 0
        assert all(not bool(t.any()) for t in opt.m_ + opt.v_)
        assert all(opt.m_[i].shape == getattr(model, k).shape == opt.v_[i].shape for i, k in enumerate(tl.PARAMS))
        assert opt.get_lr(pkg.ParamGroup.kPositions) == tl.learning_rates(ctx, step)[0]
    return s, opt, want_acc


@pytest.mark.parametrize("route", ROUTES)
def test_training_loop_stage_by_stage(pkg, ctx, dev, route):
    carried = route != "rebuilt"
    cams = [tl.camera(ctx, v) for v in range(tl.VIEWS)]
    target_t = [torch.from_numpy(np.array(t)).to(dev) for t in tl.targets(ctx)]
    model = pkg.scene.to_model(tl.start_model(ctx), dev)
    opt = pkg.FusedAdam(model, _adam_config(pkg))
    ctrl = pkg.DensificationController(tl.densify_config(pkg), tl.SCENE_EXTENT)
    losses, events, visible_rows_changed, acc_after_event = [], [], False, None
    for step in range(1, tl.STEPS + 1):
        # 1, 2: the schedules
        lrs = tl.learning_rates(ctx, step)
        opt.update_lr(step)
        assert opt.get_lr(pkg.ParamGroup.kPositions) == lrs[0], step
        assert [opt.get_lr(pkg.ParamGroup(i)) for i in range(1, 5)] == list(lrs[1:])
        view = tl.view_of(step)
        cam, settings = cams[view], pkg.RenderSettings(active_sh_degree=tl.active_degree(step))
        # 3: render
        pre = _model(model)
        n = model.num_gaussians()
        out = pkg.render(model, cam, settings)
        ref = tl.render_stage(ctx, pre, step)
        _check_forward(out, ref, step)
        radii = ref["radii"]
        assert (radii <= 0).any() and (radii > 0).any(), step
        # 4: loss and dL/dcolour
        loss, g = pkg.combined_loss_and_grad(out.color, target_t[view])
        want_loss, want_g = tl.loss_stage(ctx, np_(out.color), step)
        loss = float(loss)
        print(f"{route} step {step}: N {n} pairs {int(out.total_pairs)} loss {loss:.8f} oracle {want_loss:.8f}")
        assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), step
        assert max_err_over_max(np_(g), want_g) <= 1e-4, step
        losses.append(loss)
        # 5, 6: backward and Adam
        refb = tl.backward_stage(ctx, np_(g), ref, pre, step)
        pre_m, pre_v = _moments(opt)
        count = opt.step_count_
        if route in ("step", "rebuilt"):
            opt.zero_grad()
            res = pkg.render_backward(g, out, model, cam, settings)
            opt.apply_gradients(res)
            opt.step()
            grads = {k: np_(getattr(res, k)) for k in tl.GRADS}
            for k in tl.GRADS:
                assert max_err_over_max(grads[k].reshape(refb[k].shape), refb[k]) <= 1e-4, (k, step)
            assert opt.step_count_ == count + 1
            want, want_m, want_v = tl.adam_stage(ctx, pre, grads, pre_m, pre_v, lrs, opt.step_count_)
            got, (got_m, got_v) = _model(model), _moments(opt)
            for k in tl.PARAMS:
                _same_bits(got[k], want[k], (k, step))
                _same_bits(got_m[k], want_m[k], ("m", k, step))
                _same_bits(got_v[k], want_v[k], ("v", k, step))
        else:
            res = pkg.render_backward(g, out, model, cam, settings, fused_adam=opt, sparse_adam=route == "sparse")
            assert opt.step_count_ == count + 1
            got, (got_m, got_v) = _model(model), _moments(opt)
            for k in tl.PARAMS:
                assert np.isfinite(got[k]).all() and np.isfinite(got_m[k]).all() and np.isfinite(got_v[k]).all(), (k, step)
            if route == "sparse":
                culled = radii <= 0
                for k in tl.PARAMS:
                    _same_bits(got[k][culled], pre[k][culled], (k, "culled rows", step))
                    _same_bits(got_m[k][culled], pre_m[k][culled], ("m", k, "culled rows", step))
                    _same_bits(got_v[k][culled], pre_v[k][culled], ("v", k, "culled rows", step))
                assert (_bits(got["positions"][~culled]) != _bits(pre["positions"][~culled])).any(), step
                visible_rows_changed = True
        assert max_err_over_max(np_(res.dL_dmeans_2d), refb["dL_dmeans_2d"]) <= 1e-4, step
        # 7: the statistics, from the device's own dL_dmeans_2d and radii
        # (the step after an event starts from the ORACLE's reset accumulators: stale sums at an unchanged N show here)
        acc, acc_after_event = (acc_after_event if acc_after_event is not None else _accumulators(ctrl, n)), None
        ctrl.accumulate_gradients(res.dL_dmeans_2d, out.radii)
        want_acc = tl.accumulate_stage(ctx, acc, np_(res.dL_dmeans_2d), np_(out.radii))
        assert np.allclose(np_(ctrl.grad_accum_), want_acc[0], rtol=1e-6, atol=0), step
        assert np.array_equal(np_(ctrl.grad_count_), want_acc[1]), step
        assert np.array_equal(np_(ctrl.max_radii_2d_), want_acc[2]), step
        # 8: densify on schedule
        if ctrl.should_densify(step):
            assert tl.should_densify(step)
            s, opt, acc_after_event = _check_densify(ctx, pkg, ctrl, model, opt, carried, step, dev)
            events.append(s)
            print(f"{route} event {step}: {s.num_before} -> {s.num_after} cloned {s.num_cloned} split {s.num_split} "
                  f"pruned {s.num_pruned}")
        else:
            assert not tl.should_densify(step)
        # 9: opacity reset on schedule
        if ctrl.should_reset_opacity(step):
            assert tl.should_reset_opacity(step)
            before_m, before_v = _moments(opt)
            want = tl.reset_opacity_stage(ctx, _model(model))
            ctrl.reset_opacity(model)
            _same_bits(np_(model.opacities), want["opacities"], ("reset opacities", step))
            assert (np_(model.opacities) == np.float32(ctx.densify_oracle.K_RESET_OPACITY)).all()
            after_m, after_v = _moments(opt)
            for k in tl.PARAMS:
                _same_bits(after_m[k], before_m[k], ("m after the reset", k, step))
                _same_bits(after_v[k], before_v[k], ("v after the reset", k, step))
        else:
            assert not tl.should_reset_opacity(step)
    # the device's own trajectory got everywhere too
    assert len(events) == len(tl.EVENT_STEPS)
    assert any(s.num_cloned > 0 for s in events) and any(s.num_split > 0 for s in events)
    assert any(s.num_pruned > s.num_split for s in events)
    assert route != "sparse" or visible_rows_changed
    # and it learns: at least half the drop of the oracle's own loop with the same optimizer semantics
    drop = tl.loss_drop(losses)
    d_ref = tl.D_REF["carried" if carried else "rebuilt"]
    print(f"{route}: loss drop {drop:.6f}, oracle loop {d_ref:.6f}")
    assert drop >= 0.5 * d_ref
