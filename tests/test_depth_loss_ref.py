"""The CPU reference of the depth-supervision loss (tests/depth_loss_ref.py) checked against independent arithmetic:
its gradients against float64 torch autograd of the same loss, its fit against numpy's least squares.  No GPU."""
import numpy as np
import pytest
import torch

import depth_loss_ref as dr

SPACES = [False, True]


def _autograd(case, weighted, s, b):
    """float64 autograd of sum_valid w |x - (s t + b)| / n with respect to D and A; r in float64."""
    D = torch.tensor(case["D"].astype(np.float64), requires_grad=True)
    A = torch.tensor(case["A"].astype(np.float64), requires_grad=True)
    wt = case["w"] if weighted else np.ones_like(case["A"])
    with np.errstate(all="ignore"):
        valid, _, _ = dr.expected_depth(case["D"], case["A"], case["t"], wt, case["inverse"])
    v = torch.tensor(valid)
    t = torch.tensor(np.where(valid, case["t"], 1.0).astype(np.float64))
    one = torch.ones_like(D)
    num, den = (A, D) if case["inverse"] else (D, A)
    x = torch.where(v, num, one) / torch.where(v, den, one)
    r = x - (float(np.float32(s)) * t + float(np.float32(b)))
    loss = (torch.tensor(wt.astype(np.float64)) * r.abs())[v].sum() / D.numel()
    loss.backward()
    return D.grad.numpy(), A.grad.numpy(), r.detach().numpy(), float(loss.detach())


@pytest.mark.parametrize("inverse", SPACES)
@pytest.mark.parametrize("shape", dr.SHAPES)
def test_reference_gradients_match_float64_autograd(shape, inverse):
    """Bar: max error <= 1e-6 of each tensor's max (four float32 roundings between the inputs and a gradient: the
    division for x, the two products of gx, the final division - 4 * 6e-8 relative; a prototype measured <= 1e-7).
    sgn is discontinuous at r = 0, so a pixel whose float32 residual does not have the sign of the float64 one - the
    hand-placed x == t' pixel, where the float32 r is exactly 0 and the float64 one is the rounding error of x - has
    no derivative to compare; there may be only a handful, and the exact pixel must have gradient 0."""
    case = dr.case(*shape, inverse)
    for weighted in (False, True):
        f = dr.fit(case, weighted)
        for s, b in ((1.0, 0.0), (f["s"], f["b"])):
            ref = dr.reference(case, weighted, s, b)
            gD, gA, r64, loss64 = _autograd(case, weighted, s, b)
            r32 = ref["r"].astype(np.float64)
            same = (np.sign(np.where(ref["valid"], r32, 0.0)) == np.sign(np.where(ref["valid"], r64, 0.0))) | ~ref["valid"]
            assert (~same).sum() <= 3, (~same).sum()
            for name, got, want in (("dL/dD", ref["gD"], gD), ("dL/dA", ref["gA"], gA)):
                err = np.abs(got.astype(np.float64) - want)[same].max() / np.abs(want).max()
                print(shape, inverse, weighted, name, f"max err {err:.2e} of the tensor's max")
                assert err <= 1e-6, (name, err)
            assert np.isfinite(ref["gD"]).all() and np.isfinite(ref["gA"]).all() and np.isfinite(ref["expected"]).all()
            assert not ref["gD"][~ref["valid"]].any() and not ref["gA"][~ref["valid"]].any()
            assert not ref["expected"][~ref["valid"]].any()
            assert abs(ref["loss64"] - loss64) <= 1e-6 * loss64
        # without alignment the hand-placed pixel has x == t': sgn = 0, no gradient, but it is counted
        ref = dr.reference(case, weighted)
        e = case["exact"]
        assert ref["r"].flat[e] == 0 and ref["valid"].flat[e] and ref["gD"].flat[e] == 0 and ref["gA"].flat[e] == 0


@pytest.mark.parametrize("inverse", SPACES)
@pytest.mark.parametrize("shape", dr.SHAPES)
def test_reference_fit_matches_numpy_lstsq(shape, inverse):
    case = dr.case(*shape, inverse)
    for weighted in (False, True):
        f = dr.fit(case, weighted)
        assert f["fit_ok"]
        wt = case["w"] if weighted else np.ones_like(case["A"])
        with np.errstate(all="ignore"):
            valid, x, _ = dr.expected_depth(case["D"], case["A"], case["t"], wt, inverse)
        rw = np.sqrt(wt[valid].astype(np.float64))
        M = np.stack([case["t"][valid].astype(np.float64), np.ones(int(valid.sum()))], 1) * rw[:, None]
        (s, b), *_ = np.linalg.lstsq(M, x[valid].astype(np.float64) * rw, rcond=None)
        scale = max(abs(s), abs(b))
        assert abs(f["s"] - s) <= 1e-6 * scale and abs(f["b"] - b) <= 1e-6 * scale, (f, s, b)
        # the fitted alignment is no worse than none
        assert dr.reference(case, weighted, f["s"], f["b"])["loss64"] <= dr.reference(case, weighted)["loss64"]


@pytest.mark.parametrize("inverse", SPACES)
def test_constant_target_is_rejected(inverse):
    case = dr.case(16, 16, inverse)
    const = np.full_like(case["t"], 0.25 if inverse else 4.0)
    for weighted in (False, True):
        f = dr.fit(case, weighted, target=const)
        assert not f["fit_ok"] and (f["s"], f["b"]) == (1.0, 0.0) and f["n_valid"] >= 2
    # fewer than two valid pixels
    one = np.zeros_like(case["t"])
    one.flat[dr.P_ABOVE] = case["t"].flat[dr.P_ABOVE]
    f = dr.fit(case, False, target=one)
    assert f["n_valid"] == 1 and not f["fit_ok"] and (f["s"], f["b"]) == (1.0, 0.0)


def test_shapes_cover_the_kernel_paths():
    rows = [-(-h * w // dr.CHUNK) for h, w in dr.SHAPES]
    assert max(rows) > 256 and max(h * w for h, w in dr.SHAPES) < 300_000    # strided sum and tree of the finalize
    assert any(h * w % 4 for h, w in dr.SHAPES) and any(h * w % 4 == 0 for h, w in dr.SHAPES)   # scalar tail, and none
    assert min(rows) == 1 and 2 in rows
