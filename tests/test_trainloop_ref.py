"""The scenario of the training-loop tests (tests/trainloop_ref.py) on the CPU oracles alone: run() for both optimizer
semantics must reach every case the scenario exists for, so that tests/test_gpu_trainloop.py cannot pass by never
getting there.  No GPU; nothing under oracle/_ref is used (the stage oracles are the project's own C and libtorch
restatements), so there is nothing to skip for.

Measured (recorded here, asserted below through trainloop_ref.D_REF and the conditions):

  carried   event step        8     16     24     32     40     48
            N before       1500   1695   2165   3110   2414   3028
            cloned           37    236    773      2    361    840
            split           158    234    172      1    330    344
            pruned          158    234    172    700    407    423
            N after        1695   2165   3110   2414   3028   4133
            size rules only   0      0      0    699     57     45
            loss, mean of steps 1-6: 0.288903, of steps 43-48: 0.207985, drop d_ref = 0.080918

  rebuilt   event step        8     16     24     32     40     48
            N before       1500   1695   2163   3097   2346   2999
            cloned           37    237    772      4    409    766
            split           158    231    162      0    335    335
            pruned          158    231    162    755    426    367
            N after        1695   2163   3097   2346   2999   4068
            size rules only   0      0      0    754     73     24
            loss, mean of steps 1-6: 0.288903, of steps 43-48: 0.190261, drop d_ref = 0.098642

  both      at least 152 of the rows are culled (radii <= 0) in each of the three views at every step; the render of
            step 25, right after the opacity reset, has more than 23,000 pairs; active degrees 0, 1, 2, 3 from steps
            1, 12, 24, 36.  The reset at step 24 doubles the loss (0.31 -> 0.57); it is back under its start by step 35.
"""
import numpy as np
import pytest

import trainloop_ref as tl


@pytest.fixture(scope="module")
def ctx(pkg, orc):
    import __graft_entry__ as ge
    return tl.Ctx(orc, ge.load_oracle_module("loss_oracle"), ge.load_oracle_module("densify_oracle"), pkg.scene)


_runs = {}


def _run(ctx, semantics):
    if semantics not in _runs:
        _runs[semantics] = tl.run(ctx, semantics)
    return _runs[semantics]


def test_scenario_is_the_one_the_issue_sets(ctx):
    assert (tl.W, tl.H, tl.VIEWS, tl.STEPS) == (100, 72, 3, 48)
    assert ((tl.W + 15) // 16, (tl.H + 15) // 16) == (7, 5) and tl.W % 16 and tl.H % 16
    assert tl.SCHEDULE == dict(densify_from=8, densify_every=8, opacity_reset_every=24, densify_until=48)
    assert [s for s in range(1, 49) if tl.should_densify(s)] == list(tl.EVENT_STEPS) == [8, 16, 24, 32, 40, 48]
    assert [s for s in range(1, 49) if tl.should_reset_opacity(s)] == list(tl.RESET_STEPS) == [24, 48]
    assert [tl.active_degree(s) for s in (1, 11, 12, 23, 24, 35, 36, 48)] == [0, 0, 1, 1, 2, 2, 3, 3]
    assert [tl.view_of(s) for s in (1, 2, 3, 4, 48)] == [0, 1, 2, 0, 2]
    truth, start = tl.truth_model(ctx), tl.start_model(ctx)
    assert truth["sh_coeffs"].shape == (tl.N_TRUTH, 3, 16) and start["sh_coeffs"].shape == (tl.N_START, 3, 16)
    # coarser than the truth, with both clone and split candidates by size
    assert np.median(start["scales"].max(axis=1)) > np.median(truth["scales"].max(axis=1)) + 0.5
    big = np.exp(start["scales"]).max(axis=1) >= np.float32(tl.PERCENT_DENSE) * np.float32(tl.SCENE_EXTENT)
    assert 0.25 < big.mean() < 0.75
    # one rule for the split noise, a different draw per event
    a, b = tl.split_noise(8, 10), tl.split_noise(16, 10)
    assert a.shape == (2, 10, 3) and a.dtype == np.float32 and np.array_equal(a, tl.split_noise(8, 10))
    assert not np.array_equal(a, b)
    lrs = [tl.learning_rates(ctx, s)[0] for s in range(1, 49)]
    assert all(x > y for x, y in zip(lrs, lrs[1:])) and lrs[0] < tl.LRS[0] and lrs[-1] > tl.POS_LR_FINAL
    targets = tl.targets(ctx)
    assert len(targets) == 3 and all(t.shape == (72, 100, 3) for t in targets)
    assert not np.array_equal(targets[0], targets[1]) and not np.array_equal(targets[1], targets[2])


@pytest.mark.parametrize("semantics", ["carried", "rebuilt"])
def test_oracle_loop_reaches_every_case(ctx, semantics):
    rec = _run(ctx, semantics)
    events = rec["events"]
    for step, s, size_only in events:
        print(f"{semantics} step {step}: {s.num_before} -> {s.num_after} cloned {s.num_cloned} split {s.num_split} "
              f"pruned {s.num_pruned} size-only {size_only}")
    assert len(events) >= 4 and [e[0] for e in events] == list(tl.EVENT_STEPS)
    assert any(s.num_cloned > 0 for _, s, _ in events)
    assert any(s.num_split > 0 for _, s, _ in events)
    assert any(s.num_pruned > 0 for _, s, _ in events)
    assert any(s.num_after > s.num_before for _, s, _ in events)
    assert any(s.num_after < s.num_before for _, s, _ in events)
    assert any(step > 24 and size_only > 0 for step, _, size_only in events)
    assert all(size_only == 0 for step, _, size_only in events if step <= 24)      # the size rules start after the reset
    # with room to spare: tens of rows per case, not one
    assert max(s.num_cloned for _, s, _ in events) >= 100 and max(s.num_split for _, s, _ in events) >= 100
    assert max(size_only for _, _, size_only in events) >= 100
    assert len(rec["culled"]) == tl.STEPS and min(rec["culled"]) >= 50             # in every view, at every step
    assert all(c < n for c, n in zip(rec["culled"], rec["n"]))
    assert rec["pairs"][24] > 1000                                                 # step 25: right after the reset
    assert min(rec["pairs"]) > 1000
    assert sorted(set(rec["degrees"])) == [0, 1, 2, 3]
    assert rec["degrees"] == [tl.active_degree(s) for s in range(1, tl.STEPS + 1)]
    first, last = float(np.mean(rec["losses"][:6])), float(np.mean(rec["losses"][-6:]))
    drop = tl.loss_drop(rec["losses"])
    print(f"{semantics}: first six {first:.6f} last six {last:.6f} drop {drop:.6f}")
    assert last < 0.85 * first
    # the recorded yardstick of the GPU test.  The loop is chaotic in the last bit (Adam turns it into lr steps), so
    # another libtorch build may move the figure a little: 10 % here, where the GPU test takes half of it as its bar
    assert abs(drop - tl.D_REF[semantics]) <= 0.1 * tl.D_REF[semantics]
    assert all(np.isfinite(rec["model"][k]).all() for k in tl.MODEL_KEYS)


def test_semantics_differ_only_from_the_first_event_on(ctx):
    """Until the first event both runs are the same loop; after it the rebuilt optimizer restarts its moments and bias
    corrections, and the trajectories part."""
    a, b = _run(ctx, "carried"), _run(ctx, "rebuilt")
    assert a["losses"][:8] == b["losses"][:8]
    assert a["losses"][8:] != b["losses"][8:]
    assert a["events"][0][1] == b["events"][0][1]


def test_stage_functions_keep_no_state(ctx):
    """The stages return new arrays and leave their inputs alone: the GPU test hands them the device's data."""
    model = tl.copy_model(tl.start_model(ctx))
    keep = tl.copy_model(model)
    fwd = tl.render_stage(ctx, model, 13)
    loss, g = tl.loss_stage(ctx, fwd["color"], 13)
    grads = tl.backward_stage(ctx, g, fwd, model, 13)
    m, v = tl.zero_moments(model)
    stepped, m1, v1 = tl.adam_stage(ctx, model, grads, m, v, tl.learning_rates(ctx, 13), 1)
    acc = tl.accumulate_stage(ctx, None, grads["dL_dmeans_2d"], fwd["radii"])
    acc2 = tl.accumulate_stage(ctx, acc, grads["dL_dmeans_2d"], fwd["radii"])
    out, stats, info, zeroed = tl.densify_stage(ctx, model, acc2, 16)
    reset = tl.reset_opacity_stage(ctx, model)
    for k in tl.MODEL_KEYS:
        assert np.array_equal(model[k], keep[k]), k
    assert not any(m[k].any() or v[k].any() for k in tl.PARAMS)
    assert any(not np.array_equal(stepped[k], model[k]) for k in tl.PARAMS) and m1["positions"].any()
    assert np.array_equal(acc2[1], 2 * acc[1]) and np.allclose(acc2[0], 2 * acc[0], rtol=1e-6)
    assert acc[1].max() == 1 and (acc[1] == 0).any()                               # culled rows are not counted
    assert stats.num_cloned > 0 and stats.num_split > 0
    assert out["positions"].shape[0] == stats.num_after == zeroed[0].shape[0] and not any(z.any() for z in zeroed)
    kept = int(info["survivors"].sum())
    assert np.array_equal(out["positions"][:kept], model["positions"][info["survivors"]])
    cm, cv = tl.carry_moments(m1, v1, info["survivors"], stats.num_after)
    assert np.array_equal(cm["sh_coeffs"][:kept], m1["sh_coeffs"][info["survivors"]]) and not cm["sh_coeffs"][kept:].any()
    assert cv["scales"].shape == out["scales"].shape
    assert (reset["opacities"] == np.float32(ctx.densify_oracle.K_RESET_OPACITY)).all()
    assert np.array_equal(reset["positions"], model["positions"])
