"""The CPU reference of the normal-supervision loss (tests/normal_loss_ref.py) checked against independent arithmetic:
its gradients, normals, masks and loss against float64 torch autograd of the definition, the cases
that must give nothing, and a short gradient descent that a wrong sign in either gradient formula turns round.  No GPU."""
import numpy as np
import pytest

import normal_loss_ref as nr

WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (0.7, 0.3)]           # cos alone, L1 alone, both


@pytest.mark.parametrize("shape", nr.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_matches_float64_autograd(shape):
    """Bars: 1e-4 of each gradient's largest magnitude, 1e-4 absolute on the unit normals (a prototype of this
    definition measured 4e-6 and 6e-6: ~20 float32 roundings of 6e-8 each, amplified by 1 / |n| ~ W / d through the
    normalisation), and 1e-5 relative on the loss (each term is ~10 roundings from the inputs and the terms are summed
    in float64).  The masks must be EQUAL: the inputs keep |n|^2, |t|^2 and alpha far from their thresholds except
    where a value sits on one exactly (alpha == min_alpha, the zero and NaN prior vectors)."""
    case = nr.case(*shape)
    for weighted in (False, True):
        for cw, lw in WEIGHTS:
            ref = nr.reference(case, weighted, cos_weight=cw, l1_weight=lw)
            want = nr.autograd64(case, weighted, cos_weight=cw, l1_weight=lw)
            for m in ("depth_valid", "normal_valid", "valid"):
                assert np.array_equal(ref[m], want[m]), (m, int((ref[m] != want[m]).sum()))
            assert np.isfinite(ref["gD"]).all() and np.isfinite(ref["gA"]).all() and np.isfinite(ref["normals"]).all()
            for name in ("gD", "gA"):
                scale = np.abs(want[name]).max()
                err = np.abs(ref[name].astype(np.float64) - want[name]).max()
                print(shape, weighted, cw, lw, name, f"max err {err / scale if scale else err:.2e} of the tensor's max")
                assert err <= 1e-4 * scale, (name, err, scale)
            err_n = np.abs(ref["normals"].astype(np.float64) - want["normals"]).max()
            print(shape, weighted, cw, lw, f"normals max abs err {err_n:.2e}  loss {ref['loss64']:.9g} vs {want['loss']:.9g}")
            assert err_n <= 1e-4
            assert abs(ref["loss64"] - want["loss"]) <= 1e-5 * abs(want["loss"])
            if shape in nr.EMPTY:
                assert ref["n_valid"] == 0
            else:
                assert ref["n_valid"] > 0 and ref["loss64"] > 0 and ref["gD"].any() and ref["gA"].any()
                # mild surface: the normals point at the camera
                assert (ref["normals"][2][ref["normal_valid"]] < 0).all()
                unit = np.sqrt((ref["normals"].astype(np.float64) ** 2).sum(0))[ref["normal_valid"]]
                assert np.abs(unit - 1.0).max() <= 1e-6
            assert not ref["normals"][:, ~ref["normal_valid"]].any()


@pytest.mark.parametrize("shape", nr.EMPTY, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cases_without_a_valid_pixel_give_exactly_nothing(shape):
    """1x1 and 2x5 have no interior; the 3x4 alpha hole of 5x7 leaves no interior pixel with four valid neighbours."""
    case = nr.case(*shape)
    for weighted in (False, True):
        for cw, lw in WEIGHTS:
            ref = nr.reference(case, weighted, cos_weight=cw, l1_weight=lw)
            assert ref["n_valid"] == 0 and ref["loss64"] == 0.0 and ref["sw64"] == 0.0
            assert not ref["valid"].any() and not ref["normal_valid"].any()
            for k in ("gD", "gA", "normals"):
                assert not ref[k].view(np.uint32).any(), k            # +0.0 everywhere, not even a -0.0


def test_single_interior_pixel():
    """3x3: the centre is the one stencil; its four neighbours get a gradient, the centre and the corners none."""
    ref = nr.reference(nr.case(3, 3), True)
    assert ref["n_valid"] == 1 and ref["valid"][1, 1] and ref["loss64"] > 0
    cross = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], bool)
    assert (ref["gD"] != 0)[cross].all() and not ref["gD"][~cross].any() and not ref["gA"][~cross].any()


def test_no_prior_gives_the_normal_map_alone():
    case = nr.case(37, 53)
    ref, full = nr.reference(case, prior=False), nr.reference(case, True)
    assert ref["gD"] is None and ref["gA"] is None and ref["loss64"] == 0.0 and ref["n_valid"] == 0
    assert ref["normals"].tobytes() == full["normals"].tobytes()


DESCENT_LR, DESCENT_STEPS = 0.25, 30


@pytest.mark.parametrize("cw,lw", WEIGHTS)
def test_gradient_descent_on_the_depth_map_lowers_the_loss(cw, lw):
    """30 steps of D -= lr dL/dD with the mirror's gradient on 37x53.  lr = 0.25: |dL/dD| is at most 0.01 to 0.03 here (a mean
    over 1961 pixels of terms with d n^ / d d ~ W / (2 d) ~ 9, times up to three signs for L1), so a step moves a
    depth by less than 1e-2 where neighbouring depths differ by ~2e-2 - small enough for plain descent to descend.  A wrong sign in the gradient makes the loss grow."""
    case = nr.case(37, 53)
    D = case["D"].copy()
    losses = []
    for _ in range(DESCENT_STEPS + 1):
        ref = nr.reference(case, True, cos_weight=cw, l1_weight=lw, D=D)
        losses.append(ref["loss64"])
        D = (D - np.float32(DESCENT_LR) * ref["gD"]).astype(np.float32)
    print("loss every 5th step:", " ".join(f"{v:.6f}" for v in losses[::5]))
    assert losses[-1] < losses[0], losses
    assert losses[1] < losses[0], losses


def test_shapes_cover_the_kernel_paths():
    tiles = [(-(-h // nr.TILE_H), -(-w // nr.TILE_W)) for h, w in nr.SHAPES]
    assert (nr.TILE_H + 1, nr.TILE_W + 1) in nr.SHAPES
    assert any(ty >= 2 and tx >= 2 and h % nr.TILE_H and w % nr.TILE_W for (ty, tx), (h, w) in zip(tiles, nr.SHAPES))
    assert any(h % nr.TILE_H == 0 and w % nr.TILE_W == 0 for h, w in nr.SHAPES)
    h, w = nr.MANY_TILES                                   # the strided sum and the tree of the finalize kernel
    assert -(-h // nr.TILE_H) * -(-w // nr.TILE_W) > 256 and nr.reference(nr.case(h, w))["n_valid"] > 30000
