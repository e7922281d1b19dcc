"""The all-element blend-backward check (oracle/parity.py: blend_bound_report) is stronger than the checks it joins:
errors the tensor-scale bar and the over-the-bar rule (blend_accumulator_report) let through must fail it.  Oracle
only, no GPU: a hand-made 2-D scene of three Gaussians in three tiles of one 48x16 image, each alone in its tile list
(no overlap, so the colour and opacity sums do not cancel), and a fourth that stands in no list (no terms at all)."""
import numpy as np

from util import check_blend_bounds, load_parity

W, H, N = 48, 16, 4
BG = (0.0, 0.0, 0.0)
P = (24, 8)                                 # the pixel whose centre is the mean of Gaussian 1


def _scene():
    means = np.array([[8.5, 8.5], [24.5, 8.5], [40.5, 8.5], [-100.0, -100.0]], np.float32)
    cov = np.tile(np.array([[0.25, 0.0, 0.25]], np.float32), (N, 1))            # sigma 2 px, radius 6: one tile
    rgb = np.full((N, 3), 0.5, np.float32)
    # Gaussians 0 and 2 are the same splat 32 px apart; their sums differ by the opacity ratio, 8e-6
    opa = np.array([0.8, 0.7, 0.8 * (1.0 + 8e-6), 0.6], np.float32)
    tile_ranges = np.array([[0, 1], [1, 2], [2, 3]], np.int32)
    values = np.array([0, 1, 2], np.int32)
    return means, cov, rgb, opa, tile_ranges, values


def _backward(orc, scene, fwd, g):
    means, cov, rgb, opa, tr, vals = scene
    return orc.rasterize_backward_magnitudes(W, H, BG, tr, vals, means, cov, rgb, opa, g, fwd["final_T"],
                                             fwd["n_contrib"], N, depth_weighted=True)


def _reports(orc, scene, got, want):
    par = load_parity()
    entries = np.bincount(scene[5], minlength=N)
    acc = {k: want[k] for k in par.ACCUMULATORS}
    old = par.blend_accumulator_report(got, acc, want["mag"], scene[1], entries)
    new = par.blend_bound_report(got, {k: v.astype(np.float64) for k, v in acc.items()}, {"colour": want},
                                 scene[1], entries)
    return old, new, entries


def _old_checks_pass(old):
    for name, v in old.items():
        assert v["over_scale"] <= 1e-4, (name, v)
        assert v["over_bar_beyond_term_bound"] == 0, (name, v)


def test_a_dropped_pixel_passes_the_old_checks_and_fails_the_new(orc):
    scene = _scene()
    means, cov, rgb, opa, tr, vals = scene
    fwd = orc.rasterize_forward(W, H, BG, tr, vals, means, cov, rgb, opa)
    assert fwd["n_contrib"][P[1], P[0]] == 1
    g = np.ones((H, W, 3), np.float32)
    g[P[1], P[0]] = 5e-4                    # small enough for the old bar, large against the fp32 bound of the terms
    want = _backward(orc, scene, fwd, g)
    g_drop = g.copy()
    g_drop[P[1], P[0]] = 0.0                # exactly "this pixel's contributions were lost"
    dropped = _backward(orc, scene, fwd, g_drop)
    par = load_parity()
    got = {k: dropped[k] for k in par.ACCUMULATORS}
    old, new, entries = _reports(orc, scene, got, want)
    _old_checks_pass(old)
    print(par.format_bound_report(new, "one pixel dropped:"))
    failed = {k: v for k, v in new.items() if not v["ok"]}
    assert failed, "the all-element rule missed a dropped pixel"
    for v in failed.values():
        who = v["worst"]["gaussian"]
        assert who == 1, v                  # the Gaussian that covers the pixel
        assert v["worst_diff_over_bound"] > 2.0


def test_swapped_rows_pass_the_old_checks_and_fail_the_new(orc):
    scene = _scene()
    means, cov, rgb, opa, tr, vals = scene
    fwd = orc.rasterize_forward(W, H, BG, tr, vals, means, cov, rgb, opa)
    want = _backward(orc, scene, fwd, np.ones((H, W, 3), np.float32))
    par = load_parity()
    got = {k: want[k].copy() for k in par.ACCUMULATORS}
    for k in par.ACCUMULATORS:              # a slot mix-up: the two near-twins trade their rows
        got[k][[0, 2]] = got[k][[2, 0]]
    r0, r2 = want["dL_drgb"][0].astype(np.float64), want["dL_drgb"][2].astype(np.float64)
    assert 1e-6 < np.max(np.abs(r0 - r2) / np.abs(r0)) <= 1e-5          # the values agree to 1e-5
    old, new, entries = _reports(orc, scene, got, want)
    _old_checks_pass(old)
    print(par.format_bound_report(new, "two rows swapped:"))
    failed = {k: v for k, v in new.items() if not v["ok"]}
    assert "dL_drgb" in failed
    for v in failed.values():
        assert v["worst"]["gaussian"] in (0, 2), v


def test_a_sum_in_a_row_without_terms_fails_the_new_check(orc):
    """Gaussian 3 stands in no tile list: its row must be exactly zero, however small the stray value."""
    scene = _scene()
    means, cov, rgb, opa, tr, vals = scene
    fwd = orc.rasterize_forward(W, H, BG, tr, vals, means, cov, rgb, opa)
    want = _backward(orc, scene, fwd, np.ones((H, W, 3), np.float32))
    par = load_parity()
    assert not want["mag"][3].any()
    got = {k: want[k].copy() for k in par.ACCUMULATORS}
    got["dL_dcov_2d_inv"][3, 1] = 1e-38
    old, new, entries = _reports(orc, scene, got, want)
    _old_checks_pass(old)
    assert new["dL_dcov_2d_inv"]["nonzero_without_terms"] == 1 and not new["dL_dcov_2d_inv"]["ok"]
    assert new["dL_dcov_2d_inv"]["worst"]["gaussian"] == 3
    # and the unmodified sums pass, through the test helper that prints the table
    exact = {k: want[k] for k in par.ACCUMULATORS}
    check_blend_bounds(exact, {k: v.astype(np.float64) for k, v in exact.items()}, {"colour": want}, cov,
                       entries, "oracle against itself")


def test_depth_weighted_magnitudes(orc):
    """mag_depth weights each term by its depth j >= 1 in its pixel's replay: at least mag, exactly mag for a Gaussian
    that is always first (the lone splats here), the same for every thread count, and the plain call is unchanged."""
    scene = _scene()
    means, cov, rgb, opa, tr, vals = scene
    fwd = orc.rasterize_forward(W, H, BG, tr, vals, means, cov, rgb, opa)
    g = np.ones((H, W, 3), np.float32)
    plain = orc.rasterize_backward_magnitudes(W, H, BG, tr, vals, means, cov, rgb, opa, g, fwd["final_T"],
                                              fwd["n_contrib"], N)
    assert "mag_depth" not in plain
    one = _backward(orc, scene, fwd, g)
    three = orc.rasterize_backward_magnitudes(W, H, BG, tr, vals, means, cov, rgb, opa, g, fwd["final_T"],
                                              fwd["n_contrib"], N, threads=3, depth_weighted=True)
    assert np.array_equal(plain["mag"], one["mag"])
    assert np.array_equal(one["mag_depth"], one["mag"])                 # alone in its list: j = 1 everywhere
    assert np.allclose(three["mag_depth"], one["mag_depth"], rtol=1e-12, atol=0)
    # two splats on one pixel: the one behind is replayed first (j = 1), the front one second (j = 2)
    m2 = np.array([[8.5, 8.5], [8.5, 8.5]], np.float32)
    c2 = np.tile(np.array([[0.25, 0.0, 0.25]], np.float32), (2, 1))
    r2 = np.full((2, 3), 0.5, np.float32)
    o2 = np.array([0.5, 0.5], np.float32)
    tr2, v2 = np.array([[0, 2]], np.int32), np.array([0, 1], np.int32)
    f2 = orc.rasterize_forward(16, 16, BG, tr2, v2, m2, c2, r2, o2)
    b2 = orc.rasterize_backward_magnitudes(16, 16, BG, tr2, v2, m2, c2, r2, o2, np.ones((16, 16, 3), np.float32),
                                           f2["final_T"], f2["n_contrib"], 2, depth_weighted=True)
    assert np.allclose(b2["mag_depth"][1, :3], b2["mag"][1, :3], rtol=1e-12)
    assert np.allclose(b2["mag_depth"][0, :3], 2.0 * b2["mag"][0, :3], rtol=1e-12)
