"""tests/multiview_ref.py, the CPU-side expectation of the multi-view exchange path, checked on its own: the fp32
restatement against the float64 sum (standard rounding bound), against the oracle's single-view SH backward, at a
Gaussian on a camera centre - and the reference's SyntheticConvergence loop on the oracle, which fixes the seed the GPU
convergence test (tests/test_gpu_multiview.py) uses."""
import numpy as np
import pytest

import multiview_ref as mv


@pytest.fixture(scope="module")
def loss_oracle():
    import __graft_entry__ as ge
    return ge.load_oracle_module("loss_oracle")


def _inputs(pkg, n, V, C, seed):
    arrays = pkg.scene.make_gaussians(n, 640, 360, sh_degree=int(np.sqrt(C)) - 1, seed=seed)
    arrays["sh_coeffs"] = (arrays["sh_coeffs"] * np.float32(4.0)).astype(np.float32)    # closed gates at every degree
    centres = np.stack([pkg.scene.make_camera(640, 360, view=v).camera_center() for v in range(V)])
    rng = np.random.Generator(np.random.Philox(key=seed + 1))
    gated = rng.standard_normal((V, n, 3)).astype(np.float32)
    return arrays, centres, gated


@pytest.mark.parametrize("degree,C", [(0, 1), (1, 4), (2, 9), (3, 16), (1, 16), (0, 9)])
@pytest.mark.parametrize("V", [1, 2, 8, 16])
def test_fp32_restatement_is_within_the_rounding_bound_of_the_fp64_sum(pkg, orc, degree, C, V):
    """V products and V ordered additions in fp32: |fl - exact| <= (V + 1) 2^-24 sum_v |g_v Y_v|, element by element
    (first order: every product and every partial sum carries one relative error of at most 2^-24)."""
    n = 3001
    arrays, centres, gated = _inputs(pkg, n, V, C, seed=31 + V)
    got = mv.sh_views_fp32(orc, degree, arrays["positions"], centres, gated, C)
    want, mag = mv.sh_views_fp64(orc, degree, arrays["positions"], centres, gated, C, want_abs=True)
    assert got.dtype == np.float32 and got.shape == (n, 3, C)
    bound = (V + 1) * 2.0 ** -24 * mag
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    active = (degree + 1) ** 2
    assert (got[:, :, active:] == 0.0).all() and (mag[:, :, active:] == 0.0).all()
    assert (mag[:, :, :active] > 0.0).mean() > 0.99                       # the bound is over real terms
    if V > 1:
        assert (got.astype(np.float64) != want).any()                        # and is not met trivially


@pytest.mark.parametrize("degree,stored", [(0, 0), (1, 1), (2, 2), (3, 3), (1, 3), (0, 2)])
def test_one_view_with_the_gate_is_the_oracle_sh_backward(pkg, orc, degree, stored):
    """V = 1, the model's real coefficients, an all-ones gradient: products x gate == orc.sh_backward; both gate values
    occur."""
    n, C = 4000, (stored + 1) ** 2
    arrays, centres, _ = _inputs(pkg, n, 1, C, seed=7 + degree)
    ones = np.ones((1, n, 3), np.float32)
    got = mv.sh_views_fp32(orc, degree, arrays["positions"], centres, ones, C)
    gate = mv.colour_gate(orc, degree, arrays["sh_coeffs"], arrays["positions"], centres[0])
    assert gate.shape == (n, 3) and gate.dtype == np.bool_
    for ch in range(3):
        assert gate[:, ch].any() and (~gate[:, ch]).any()
    want = orc.sh_backward(degree, arrays["sh_coeffs"], orc.directions(arrays["positions"], centres[0]), ones[0])
    assert np.array_equal((got * gate[:, :, None].astype(np.float32)).view(np.uint32), want.view(np.uint32))
    # the gate is the oracle's own raw > 0 test, restated in plain numpy on the forward's raw colour where that is
    # not within rounding of zero
    raw = orc.sh_forward(degree, arrays["sh_coeffs"], orc.directions(arrays["positions"], centres[0]))
    clear = np.abs(raw) > 1e-4
    assert np.array_equal(gate[clear], (raw > 0)[clear])


def test_a_gaussian_on_a_camera_centre_has_direction_zero_and_finite_results(pkg, orc):
    n, V, C = 300, 3, 16
    arrays, centres, gated = _inputs(pkg, n, V, C, seed=3)
    pos = arrays["positions"].copy()
    pos[5] = centres[1]                                                      # exactly on view 1's centre
    pos[6] = centres[0] + np.array([1e-9, 0.0, 0.0], np.float32)             # under the norm clamp (view 0 is at the origin)
    assert np.array_equal(orc.directions(pos, centres[1])[5], np.zeros(3, np.float32))
    d6 = orc.directions(pos, centres[0])[6]
    assert d6[0] == np.float32(np.float32(1e-9) / np.float32(1e-8)) and d6[1] == 0 and d6[2] == 0
    got = mv.sh_views_fp32(orc, 3, pos, centres, gated, C)
    assert np.isfinite(got).all()
    # on the centre only Y_0 survives for that view: column 0 still carries all three views
    one = mv.sh_views_fp32(orc, 3, pos[5:6], centres[1:2], gated[1:2, 5:6], C)
    assert (one[0, :, 1:] == 0.0).all() and (one[0, :, 0] != 0.0).all()


def test_synthetic_convergence_on_the_oracle(orc, loss_oracle):
    """The reference's SyntheticConvergence (tests/test_training.cpp:159-261) on orc.render, loss_oracle.
    combined_loss_and_grad, orc.render_backward and orc.fused_adam, with the seed the GPU test uses: the loss must drop
    by more than 10 % (the reference's threshold).  The committed seed drops by far more (see the GPU test's
    docstring), so the 10 % does not rest on a lucky draw; neighbouring seeds are checked too."""
    initial, final, model = mv.oracle_convergence(orc, loss_oracle)
    drop = (initial - final) / initial
    print(f"oracle convergence: initial {initial:.6f} final {final:.6f} drop {100 * drop:.1f} %")
    assert drop > 0.10
    assert drop > 0.30                                                       # comfortably past it
    assert all(np.isfinite(model[k]).all() for k in mv.CONV_PARAMS)
    for seed in (mv.CONV_SEED + 1, mv.CONV_SEED + 2):
        a, b, _ = mv.oracle_convergence(orc, loss_oracle, seed=seed)
        assert (a - b) / a > 0.10, seed
