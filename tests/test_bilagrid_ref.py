"""tests/bilagrid_ref.py, the numpy mirror of csrc/bilagrid.hip in the header's fp32 operation order, against libtorch's
fp64 grid_sample + einsum + autograd on the CPU: the formulas of include/cugs_hip.h ARE that sequence, gradient through
the luminance guidance and border clamp included.  No GPU.

Tolerance: element-wise, 1e-5 of each tensor's largest magnitude.  libtorch's own fp32 evaluation of the sequence
measures at most 1.3e-6 against fp64 at the small shapes and 7.8e-6 for dL_dgrid at 270x480 / (4,4,2) (its fp32 sum of
32 k terms per vertex), which is why the mirror sums the grid gradient in fp64."""
import numpy as np
import pytest

import bilagrid_ref as br

TOL = 1e-5


@pytest.mark.parametrize("c", br.CASES, ids=br.case_id)
def test_mirror_matches_libtorch_fp64(c):
    grid, img, g = br.case(*c)
    ref = br.torch_reference(*c)
    out = br.mirror_slice(grid, img)
    d_img, d_grid = br.mirror_backward(grid, img, g)
    errs = {"corrected": br.err_of_scale(out, ref["corrected"]),
            "dL_drendered": br.err_of_scale(d_img, ref["dL_drendered"]),
            "dL_dgrid": br.err_of_scale(d_grid, ref["dL_dgrid"])}
    print(br.case_id(c), {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= TOL, (k, v)


def test_clamp_case_has_pixels_outside_the_range():
    """The extra case really exercises the clamp: it has pixels above and below the range, the mirror flags exactly
    those, and every other case has none."""
    grid, img, _ = br.case(*br.CLAMP_SHAPE, True)
    luma = img.astype(np.float64) @ np.array([0.299, 0.587, 0.114])
    over, under = luma > 1.0, luma < 0.0
    assert over.any() and under.any()
    _, _, inside = br._coords(img, grid.shape[1:])
    assert not inside[over | under].any() and inside[~(over | under)].all()
    for h, w, shape in br.SHAPES:
        grid, img, _ = br.case(h, w, shape)
        assert br._coords(img, grid.shape[1:])[2].all()


def test_identity_grid_is_exact_in_the_mirror():
    for h, w, shape in br.SHAPES[:4]:
        _, img, g = br.case(h, w, shape)
        eye = br.identity_grid(shape)
        assert br.mirror_slice(eye, img).tobytes() == img.tobytes()
        d_img, _ = br.mirror_backward(eye, img, g)
        assert d_img.tobytes() == g.tobytes()


@pytest.mark.parametrize("shape", [s for _, _, s in br.SHAPES], ids=str)
def test_tv_mirror_matches_libtorch_fp64(shape):
    grid, _, _ = br.case(7, 5, shape)
    import torch
    G = torch.from_numpy(grid.astype(np.float64)).requires_grad_(True)
    tv = br.torch_tv(G)
    (want,) = torch.autograd.grad(tv, G)
    tv = float(tv.detach())
    got_tv, got = br.mirror_tv(grid, weight=1.0)
    assert abs(float(got_tv) - tv) <= np.spacing(np.float32(tv))
    assert br.err_of_scale(got, want.numpy()) <= 1e-6
    _, scaled = br.mirror_tv(grid, weight=2.5)
    assert br.err_of_scale(scaled, 2.5 * want.numpy()) <= 1e-6
