"""The projection and its backward on the GPU with cameras and models as a capture has them (tests/camera_cases.py):
fx != fy, an off-centre principal point (C2: outside the image), all nine entries of W, Gaussians at and behind the near
plane (C3), quaternion norms from 1e-7 to 1e3 and exact zeros.  The rest of the suite runs on scene.make_camera /
make_gaussians, where a swapped fx / fy, W / 2 for cx, a transposed W or a wrong power of 1 / |q| all go unnoticed.

Yardsticks: the CPU oracle, bit for bit where the project claims "same operation order, no contraction" (every forward
output, the sort, n_contrib), and the fp64 models tests/projection_ref.py and test_oracle_autograd._render_autograd for
the gradients, each Gaussian judged against its own largest element (camera_cases.row_err): dL/dq scales as 1 / |q|, so a
tensor-wide scale sees only the rows with a small norm.  tests/test_projection_ref.py pins the oracle to those models
on the CPU (worst row 4.2e-5 at the log-scale spread of 0.5) and says what is ill-conditioned about the spread of 1.0.

Bars: ROW_TOL = 1e-4 per live row for the projection stage (the project's bar, applied per row), E2E_TOL = 2e-4 per row
for render_backward against the fp64 render model (the bar the oracle is held to there), culled rows exactly zero.

Measured on an MI355X (worst live row per tensor against fp64; -s prints them).  The four routes of a case - FACTORS,
the row tile with and without the gate bits, degrees 3 and 0 - give the same figures, and they are the oracle's own:
the stage is the oracle's bit for bit on these inputs too.
  stage      positions rotations scales   opacities sh(deg 3) sh(deg 0) dL/dW    dL/dtvec     (bar 1e-4)
  C0 Q1      9.2e-07   1.5e-05   5.4e-06  1.7e-06   4.3e-07   1.1e-07   9.2e-07  8.8e-07
  C0 Q2      9.2e-07   2.2e-05   5.3e-06  1.7e-06   4.3e-07   1.1e-07   9.2e-07  8.8e-07
  C1 Q1      1.1e-06   2.8e-05   1.3e-05  1.7e-06   4.3e-07   1.1e-07   1.3e-06  1.4e-06
  C1 Q2      9.7e-07   2.0e-05   1.1e-05  1.7e-06   4.3e-07   1.1e-07   1.2e-06  1.2e-06
  C2 Q1      8.9e-07   1.7e-05   3.8e-06  1.7e-06   3.9e-07   1.1e-07   7.4e-07  9.2e-07
  C2 Q2      1.3e-06   1.7e-05   5.6e-06  1.7e-06   3.9e-07   1.1e-07   7.6e-07  1.2e-06
  C3 Q1      1.2e-05   4.1e-05   3.5e-05  6.5e-07   2.6e-06   1.1e-07   1.2e-05  1.2e-05
  C3 Q2      1.2e-05   4.2e-05   1.7e-05  6.5e-07   2.6e-06   1.1e-07   1.2e-05  1.2e-05
  render     positions rotations scales   opacities sh                                        (bar 2e-4)
  C1 Q1      8.1e-06   1.8e-05   4.1e-05  1.5e-04   1.1e-05      (18 of 24 rows with a gradient; the same on every run)
  C2 Q1      4.4e-06   1.6e-05   1.2e-05  9.4e-06   9.1e-06      (7 of 24)
  A1 on C1   3.26 % of the live rows left out; kept rows 9.5e-06; left-out rows 4.5e-04 = 1.00 x the oracle's row error
The rotations column is the widest because dL/dq cancels for a nearly isotropic splat (Sigma does not depend on R when
the three scales are equal): the row's own largest element is then small against its terms.  It is a property of the
inputs, the same for any fp32 evaluation; tests/test_projection_ref.py records how the seeds were chosen for it.
"""
import functools

import numpy as np
import pytest
import torch

import camera_cases as cc
import pose_ref
import projection_ref as pref
from test_gpu_parity import _assert_projection_equal
from test_gpu_pose_grad import _check_reduction, _misaligned
from test_gpu_sparse_adam import _bits_equal, _state, shared_blend  # noqa: F401  (shared_blend is a fixture)
from test_projection_ref import GEOMETRY, oracle_row_errors, stage_case
from util import max_err_over_max, np_, oracle_forward

pytestmark = pytest.mark.gpu

ROW_TOL = 1e-4          # per live row against fp64: 5 x the oracle's own worst row
E2E_TOL = 2e-4          # render_backward per row against the fp64 render model
GRAD_TOL = 1e-4         # the existing bar: error relative to each tensor's scale, against the oracle
FWD_NAMES = ("means_2d", "depths", "cov_2d_inv", "radii", "tiles_touched", "rgb", "opacities_act", "packed", "colour_gate")
BOTH = [pytest.param(c, m, id=f"{c}-{m}") for c in cc.CAMERAS for m in cc.MODELS]


def _model(pkg, dev, arrays):
    return pkg.scene.to_model({k: np.array(v) for k, v in arrays.items()}, dev)        # the cached arrays are read-only


def _dev(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _camera_rows(pkg, orc, cam_name, model_name):
    case = stage_case(pkg, orc, cam_name, model_name)
    gm, gc, _, _ = case["grads"]
    arrays = {k: np.array(v) for k, v in case["arrays"].items()}                        # torch wants writable arrays
    rows = pose_ref.camera_rows(arrays, case["cam"], np.array(gm), np.array(gc), live=case["live"])
    rows.setflags(write=False)
    return rows


def _report(label, got, want, tol, expect_culled=None):
    """Every row of `got` against fp64 `want`: finite, culled rows exactly zero, live rows within tol; prints and
    returns the worst live row."""
    assert np.isfinite(got).all(), label
    err, culled = cc.row_err(got, want)
    if expect_culled is not None:
        assert (culled >= expect_culled).all(), label
    worst = cc.worst(err, culled)
    print(f"{label}: worst row {worst:.2e} (row {int(np.argmax(np.where(culled, 0.0, err)))}), "
          f"exactly zero {int(culled.sum())}")
    assert (err[culled] == 0.0).all(), (label, "a culled row is not exactly zero", np.flatnonzero(err == np.inf)[:8])
    assert (err <= tol).all(), (label, int(np.argmax(err)), float(err.max()))
    return worst


# ---- forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam_name,model_name", BOTH)
def test_forward_every_route_is_the_oracle_bit_for_bit(pkg, orc, dev, cam_name, model_name):
    """project_gaussians whole, in two halves, keyed, and on unaligned pointers: radii, tiles, means, depths, conic and
    activated opacity are the oracle's bits (rsqrt of a non-unit norm included), rgb within 1e-6; the routes are each
    other's bits in every output, the packed records and the gate bits included."""
    case = stage_case(pkg, orc, cam_name, model_name)
    ref, cam = case["fwd"], case["cam"]
    model = _model(pkg, dev, case["arrays"])
    R = pkg.rasterizer
    margs = (model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam, 3)
    whole = R.project_gaussians(*margs)
    halves = R.project_gaussians(*margs, key_sort=True, colour_on_side_stream=True)
    halves.wait_colour()
    keyed = R.project_gaussians(*margs, key_sort=True)
    loose = R.project_gaussians(model.positions, _misaligned(model.rotations), model.scales, model.opacities,
                                _misaligned(model.sh_coeffs), cam, 3)
    torch.cuda.synchronize(dev)
    _assert_projection_equal(whole, ref)
    for tag, out in (("halves", halves), ("keyed", keyed), ("unaligned", loose)):
        for name in FWD_NAMES:
            a, b = getattr(whole, name), getattr(out, name)
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (tag, name)
        _assert_projection_equal(out, ref)
    live = ref["radii"] > 0
    assert live.sum() > cc.N // 2
    if cam_name == "C3":
        assert cc.N / 5 <= (ref["depths"] == 0.0).sum() <= cc.N / 2


def test_two_halves_feed_the_sort_on_a_camera_with_the_principal_point_outside(pkg, orc, dev):
    """test_projection_in_two_halves_equals_the_whole's last step on C2: the sort that consumes the keys the geometry
    half left in the workspace gives the oracle's order."""
    case = stage_case(pkg, orc, "C2", "Q1")
    ref, cam = case["fwd"], case["cam"]
    model = _model(pkg, dev, case["arrays"])
    R = pkg.rasterizer
    key = R._skey(torch.device(dev))
    R._last_pairs[key] = ref["total_pairs"]
    R._held_capacity.pop(key, None)
    try:
        halves = R.project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam,
                                     3, key_sort=True, colour_on_side_stream=True)
        pend = R.sort_gaussians_predicted(halves.means_2d, halves.depths, halves.radii, halves.tiles_touched, cc.W, cc.H,
                                          want_keys=True, keyed_workspace=halves.sort_workspace)
        srt, valid = pend.finish() if isinstance(pend, R.PendingSort) else (pend, True)
        halves.wait_colour()
    finally:
        R._last_pairs.pop(key, None)
    assert valid and srt.total_pairs == ref["total_pairs"] > 0
    assert np.array_equal(np_(srt.gaussian_keys_sorted).view(np.uint64), ref["keys"])
    assert np.array_equal(np_(srt.gaussian_values_sorted), ref["values"])
    assert np.array_equal(np_(srt.tile_ranges), ref["tile_ranges"])


@pytest.mark.parametrize("cam_name,model_name", BOTH)
def test_sort_and_blend_on_these_views(pkg, orc, dev, cam_name, model_name):
    case = stage_case(pkg, orc, cam_name, model_name)
    ref, cam = case["fwd"], case["cam"]
    off_screen = (ref["radii"] > 0) & (ref["tiles_touched"] == 0)
    if cam_name in ("C2", "C3"):
        assert off_screen.any()                            # a live splat that touches no tile: the case cannot vanish
    assert ref["total_pairs"] > 0 and ref["n_contrib"].max() > 0
    model = _model(pkg, dev, case["arrays"])
    out = pkg.render(model, cam, pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=3))
    srt = pkg.sort_gaussians(out.means_2d, out.depths, out.radii, _dev(dev, ref["tiles_touched"]), cc.W, cc.H)
    assert out.total_pairs == srt.total_pairs == ref["total_pairs"]
    assert np.array_equal(np_(out.radii), ref["radii"])
    assert np.array_equal(np_(srt.gaussian_keys_sorted).view(np.uint64), ref["keys"])
    assert np.array_equal(np_(srt.gaussian_values_sorted), ref["values"])
    assert np.array_equal(np_(out.gaussian_indices), ref["values"])
    assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"])
    assert np.array_equal(np_(out.n_contrib), ref["n_contrib"])
    assert max_err_over_max(np_(out.color), ref["color"]) <= 1e-4


# ---- backward stage ------------------------------------------------------------------------------------------------
def _stage(pkg, dev, case, degree, gate, rows=True):
    """project_backward with the camera gradient on the case's incoming gradients: (output, rows [n,12] numpy)."""
    arrays, cam = case["arrays"], case["cam"]
    n = arrays["positions"].shape[0]
    model = _model(pkg, dev, arrays)
    gm, gc, gr, go = (_dev(dev, g) for g in case["grads"])
    bits = None
    if gate:
        bits = pkg.project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam,
                                     degree).colour_gate
        assert bits is not None
    view_rows = torch.full((n, 12), float("nan"), device=dev)
    out = pkg.project_backward(gm, gc, gr, go, model.positions, model.rotations, model.scales, model.opacities,
                               model.sh_coeffs, _dev(dev, case["fwd"]["radii"]), cam, degree, colour_gate=bits,
                               want_camera_grad=True, dL_dview_rows=view_rows)
    torch.cuda.synchronize(dev)
    return out, np_(view_rows).astype(np.float64)


# degree 3 stores 16 coefficients: with the gate bits that is the FACTORS route, without them the row tile with the gate
# recomputed; degree 0 stores one coefficient: the row tile, gate bits given and recomputed
@pytest.mark.parametrize("degree,gate", [(3, True), (3, False), (0, True), (0, False)])
@pytest.mark.parametrize("cam_name,model_name", BOTH)
def test_backward_stage_rows_match_fp64(pkg, orc, dev, cam_name, model_name, degree, gate):
    case = stage_case(pkg, orc, cam_name, model_name, degree)
    live = case["live"]
    out, rows = _stage(pkg, dev, case, degree, gate)
    label = f"{cam_name} {model_name} deg {degree} {'gate' if gate else 'no gate'}"
    for name in pref.NAMES:
        got = np_(getattr(out, name))
        _report(f"{label} {name}", got, case["want_bwd"][name], ROW_TOL, None if name == "dL_dsh_coeffs" else ~live)
        # the existing bar, against the oracle's own backward
        assert max_err_over_max(got, case["bwd"][name]) <= GRAD_TOL, name
    want_rows = _camera_rows(pkg, orc, cam_name, model_name)
    _report(f"{label} dL_dW rows", rows[:, :9], want_rows[:, :9], ROW_TOL, ~live)
    _report(f"{label} dL_dtvec rows", rows[:, 9:], want_rows[:, 9:], ROW_TOL, ~live)
    _check_reduction(np_(out.dL_dviewmat), rows)


def test_anisotropic_rows_by_the_conditioning_rule(pkg, orc, dev):
    """A1 (log-scale spread 1.0) on C1.  A Gaussian is compared at ROW_TOL when the ORACLE's own row error against fp64
    is <= 1e-5 on every geometry gradient; fewer than 5 % may be left out, and a left-out row must still be finite and
    within max(1e-4, 16 x the oracle's row error): two fp32 orderings of one cancelling sum."""
    case = stage_case(pkg, orc, "C1", "A1")
    live = case["live"]
    orc_err = oracle_row_errors(case)
    per_row = np.max([orc_err[k][0] for k in GEOMETRY], axis=0)
    kept = per_row <= 1e-5
    share = float((~kept[live]).mean())
    out, _ = _stage(pkg, dev, case, 3, True)
    worst_kept = worst_left = worst_ratio = 0.0
    for name in GEOMETRY:
        got = np_(getattr(out, name))
        assert np.isfinite(got).all(), name
        err, culled = cc.row_err(got, case["want_bwd"][name])
        assert (culled >= ~live).all() and (err[culled] == 0.0).all(), name
        bound = np.where(kept, ROW_TOL, np.maximum(1e-4, 16.0 * orc_err[name][0]))
        worst_kept = max(worst_kept, float(err[kept].max()))
        if (~kept).any():
            worst_left = max(worst_left, float(err[~kept].max()))
            worst_ratio = max(worst_ratio, float((err[~kept] / np.maximum(orc_err[name][0][~kept], 1e-300)).max()))
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, (name, bad[:8], err[bad[:8]], orc_err[name][0][bad[:8]])
    print(f"A1 on C1: {100 * share:.2f} % left out; kept rows worst {worst_kept:.2e}; left-out rows worst {worst_left:.2e}, "
          f"at most {worst_ratio:.2f} x the oracle's row error")
    assert share < 0.05


# ---- end to end ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_case(pkg, orc, cam_name):
    w, h, n = cc.SMALL
    arrays, bg = cc.small_scene(pkg, "Q1")
    cam = cc.camera(pkg, cam_name, w, h)
    fwd = oracle_forward(orc, arrays, cam, bg=bg)
    rng = np.random.default_rng(3)
    g = rng.standard_normal((h, w, 3)).astype(np.float32)
    g_depth = (0.2 * rng.standard_normal((h, w))).astype(np.float32)
    g_alpha = rng.standard_normal((h, w)).astype(np.float32)
    maps, want = pref.render_backward(arrays, cam, fwd, bg, g, g_depth, g_alpha)
    return arrays, bg, cam, fwd, (g, g_depth, g_alpha), maps, want


@pytest.mark.parametrize("cam_name", ["C1", "C2"])
def test_render_backward_end_to_end_matches_fp64(pkg, orc, dev, cam_name):
    """The 48 x 32, n = 24 scene of test_oracle_autograd (nothing saturates, nothing clamps) with the depth-map and alpha
    gradients, so that W[2, :] enters through dL/dz: GPU render_backward against the fp64 render model, per row."""
    arrays, bg, cam, fwd, (g, g_depth, g_alpha), maps, want = _small_case(pkg, orc, cam_name)
    assert fwd["final_T"].min() > 1.5 / 255.0
    assert (np.abs(want["dL_dpositions"]).max(1) > 0).sum() >= (12 if cam_name == "C1" else 6)    # rows with a gradient
    model = _model(pkg, dev, arrays)
    settings = pkg.RenderSettings(background=list(bg), active_sh_degree=3)
    out = pkg.render(model, cam, settings, want_depth_map=True)
    assert np.array_equal(np_(out.gaussian_indices), fwd["values"])
    assert np.array_equal(np_(out.tile_ranges), fwd["tile_ranges"])
    assert np.allclose(np_(out.color), maps["color"], atol=2e-5)
    assert np.allclose(np_(out.depth_map), maps["depth_map"], atol=2e-5 * max(1.0, float(np.abs(maps["depth_map"]).max())))
    assert np.allclose(1.0 - np_(out.final_T), maps["alpha"], atol=2e-5)
    grads = pkg.render_backward(_dev(dev, g), out, model, cam, settings, dL_ddepth_map=_dev(dev, g_depth),
                                dL_dalpha=_dev(dev, g_alpha))
    torch.cuda.synchronize(dev)
    for name in pref.NAMES:
        got = np_(getattr(grads, name)).reshape(want[name].shape)
        _report(f"{cam_name} Q1 render {name}", got, want[name], E2E_TOL)


# ---- fused routes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse,pose,mcmc", [(False, False, False), (True, False, False), (False, True, False),
                                              (True, True, False), (False, False, True)],
                         ids=["adam", "adam-sparse", "adam-pose", "adam-sparse-pose", "adam-mcmc"])
def test_fused_routes_equal_backward_then_step(pkg, dev, shared_blend, sparse, pose, mcmc):
    """C1 and Q1: render_backward(fused_adam=...) in its five combinations against render_backward -> apply_gradients ->
    step (with step(visible=radii) for sparse_adam; + the regulariser's gradients and inject_noise for mcmc), two steps,
    the model, the moments and dL_dmeans_2d bit for bit - and dL_dviewmat with want_camera_grad.  Both paths consume one
    backward blend (shared_blend: its float atomics may order sums differently from run to run).  Every fifth Gaussian
    is mirrored through the camera centre, so that the view culls a real share."""
    w, h, n = 124, 92, cc.N
    arrays = cc.model(pkg, "Q1", w=w, h=h)
    cam = cc.camera(pkg, "C1", w, h)
    hidden = np.arange(n) % 5 == 0
    centre = cam.camera_center().astype(np.float64)
    arrays["positions"][hidden] = (2.0 * centre - arrays["positions"][hidden]).astype(np.float32)
    settings = pkg.RenderSettings(background=[0.2, 0.1, 0.3], active_sh_degree=3)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=31) * 3000.0).to(dev)
    ma, mb = pkg.scene.to_model(arrays, dev), pkg.scene.to_model(arrays, dev)
    oa, ob = pkg.FusedAdam(ma), pkg.FusedAdam(mb)
    ctrl = pkg.MCMCController(pkg.MCMCConfig(noise_lr_init=5.0, noise_lr_final=0.5, noise_lr_max_steps=10,
                                             lambda_opacity=0.05, lambda_scale=0.05, seed=77), 5.0) if mcmc else None
    gen = torch.Generator(device="cpu").manual_seed(5)
    for step in (1, 2):
        out = pkg.render(ma, cam, settings)
        assert all(_bits_equal(a, b) for a, b in zip(_state(ma, oa), _state(mb, ob))), step
        radii = np_(out.radii)
        assert (radii[hidden] == 0).all() and (radii[~hidden] > 0).mean() > 0.9
        noise = torch.randn((n, 3), generator=gen).to(dev) if mcmc else None
        plain = pkg.render_backward(g, out, ma, cam, settings, want_camera_grad=pose)
        grads = plain
        if mcmc:
            _, r_o, r_s = ctrl.compute_regularization(ma)
            grads = pkg.BackwardOutput(plain.dL_dpositions, plain.dL_drotations, plain.dL_dscales + r_s,
                                       plain.dL_dopacities + r_o, plain.dL_dsh_coeffs, plain.dL_dmeans_2d)
        oa.apply_gradients(grads)
        oa.step(visible=out.radii if sparse else None)
        if mcmc:
            ctrl.inject_noise(ma, step, noise=noise)
        fused = pkg.render_backward(g, out, mb, cam, settings, fused_adam=ob, sparse_adam=sparse, want_camera_grad=pose,
                                    mcmc=ctrl, mcmc_step=step, mcmc_noise=noise)
        torch.cuda.synchronize(dev)
        assert len(shared_blend) == step                     # one blend per step fed both paths
        assert fused.dL_dpositions is None and _bits_equal(fused.dL_dmeans_2d, plain.dL_dmeans_2d)
        for i, (a, b) in enumerate(zip(_state(ma, oa), _state(mb, ob))):
            assert _bits_equal(a, b), (step, i)
        if pose:
            assert _bits_equal(fused.dL_dviewmat, plain.dL_dviewmat)
            assert bool((fused.dL_dviewmat[:3] != 0).all()) and bool(torch.isfinite(fused.dL_dviewmat).all())
        else:
            assert fused.dL_dviewmat is None
    assert oa.step_count_ == ob.step_count_ == 2
    start = pkg.scene.to_model(arrays, dev)
    assert not torch.equal(mb.rotations, start.rotations) and not torch.equal(mb.positions, start.positions)
    if sparse:                                               # never seen, never touched
        rows = torch.from_numpy(hidden).to(dev)
        for k in ("positions", "rotations", "scales", "opacities", "sh_coeffs"):
            assert _bits_equal(getattr(mb, k)[rows], getattr(start, k)[rows]), k
