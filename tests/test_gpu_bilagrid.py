"""The bilateral-grid kernels on the GPU (csrc/bilagrid.hip) against tests/bilagrid_ref.py: the numpy
mirror in the header's fp32 operation order (corrected and dL_drendered: the same bytes) and libtorch's fp64
grid_sample + autograd (dL_dgrid: 1e-5 of its largest magnitude, element-wise; the combine is fp64, so the measured
figure - printed - is near 1e-7); the TV regulariser; BilateralGridModel; and a short fit."""
import numpy as np
import pytest
import torch

import bilagrid_ref as br
from util import np_

pytestmark = pytest.mark.gpu


def _dev(dev, *arrays):
    return tuple(torch.from_numpy(np.array(a)).to(dev) for a in arrays)


@pytest.mark.parametrize("c", br.CASES, ids=br.case_id)
def test_slice_and_backward(pkg, dev, c):
    grid_h, img_h, g_h = br.case(*c)
    grid, img, g = _dev(dev, grid_h, img_h, g_h)
    ref = br.torch_reference(*c)
    want_img, _ = br.mirror_backward(grid_h, img_h, g_h)

    out = pkg.bilagrid_slice(grid, img)
    back = pkg.bilagrid_slice_backward(grid, img, g)
    assert np_(out).tobytes() == br.mirror_slice(grid_h, img_h).tobytes()
    assert np_(back.dL_drendered).tobytes() == want_img.tobytes()
    err = br.err_of_scale(np_(back.dL_dgrid), ref["dL_dgrid"])
    print(f"{br.case_id(c)}: dL_dgrid error {err:.2e} of scale against libtorch fp64")
    assert err <= 1e-5
    assert br.err_of_scale(np_(out), ref["corrected"]) <= 1e-5
    assert br.err_of_scale(np_(back.dL_drendered), ref["dL_drendered"]) <= 1e-5

    again, back2 = pkg.bilagrid_slice(grid, img), pkg.bilagrid_slice_backward(grid, img, g)      # the same bits every run
    assert np_(again).tobytes() == np_(out).tobytes()
    assert np_(back2.dL_drendered).tobytes() == np_(back.dL_drendered).tobytes()
    assert np_(back2.dL_dgrid).tobytes() == np_(back.dL_dgrid).tobytes()

    only_grid = pkg.bilagrid_slice_backward(grid, img, g, want_image_grad=False)                # either output may be absent
    only_img = pkg.bilagrid_slice_backward(grid, img, g, want_grid_grad=False)
    assert only_grid.dL_drendered is None and only_img.dL_dgrid is None
    assert np_(only_grid.dL_dgrid).tobytes() == np_(back.dL_dgrid).tobytes()
    assert np_(only_img.dL_drendered).tobytes() == np_(back.dL_drendered).tobytes()


def test_unaligned_image_views(pkg, dev):
    """Images whose bases are 4-byte but not 16-byte aligned: the same bytes."""
    h, w, shape = br.SHAPES[2]
    grid_h, img_h, g_h = br.case(h, w, shape)
    grid, = _dev(dev, grid_h)
    pad = lambda a: torch.cat([torch.zeros(1, device=dev), torch.from_numpy(np.array(a)).to(dev).reshape(-1)])[1:].reshape(h, w, 3)
    img, g = pad(img_h), pad(g_h)
    assert img.data_ptr() % 16 != 0 and img.is_contiguous()
    assert np_(pkg.bilagrid_slice(grid, img)).tobytes() == br.mirror_slice(grid_h, img_h).tobytes()
    back = pkg.bilagrid_slice_backward(grid, img, g)
    assert np_(back.dL_drendered).tobytes() == br.mirror_backward(grid_h, img_h, g_h)[0].tobytes()


@pytest.mark.parametrize("c", br.CASES[:4], ids=br.case_id)
def test_identity_grid_is_exact(pkg, dev, c):
    """The lerp form a + t (b - a) returns a lattice that is constant over a pixel's corners exactly, so the identity
    grid gives rendered and dL_drendered = g bit for bit (no input here is -0.0)."""
    h, w, shape, clamp = c
    _, img_h, g_h = br.case(*c)
    grid, img, g = _dev(dev, br.identity_grid(shape), img_h, g_h)
    assert np_(pkg.bilagrid_slice(grid, img)).tobytes() == img_h.tobytes()
    assert np_(pkg.bilagrid_slice_backward(grid, img, g, want_grid_grad=False).dL_drendered).tobytes() == g_h.tobytes()


@pytest.mark.parametrize("shape", [(4, 3, 2), (16, 16, 8), (5, 3, 4)], ids=str)
def test_tv(pkg, dev, shape):
    grid_h, _, _ = br.case(7, 5, shape)
    grid, = _dev(dev, grid_h)
    G = torch.from_numpy(grid_h.astype(np.float64)).requires_grad_(True)
    want_tv = br.torch_tv(G)
    (want,) = torch.autograd.grad(want_tv, G)
    want_tv, want = float(want_tv.detach()), want.numpy()

    tv, d = pkg.bilagrid_tv(grid, weight=1.0)
    assert tv.dim() == 0 and abs(float(tv) - want_tv) <= np.spacing(np.float32(want_tv))      # within 1 ulp
    assert br.err_of_scale(np_(d), want) <= 1e-6
    tv2, d2 = pkg.bilagrid_tv(grid, weight=2.5)                                               # tv stays unweighted
    assert np_(tv2).tobytes() == np_(tv).tobytes()
    assert br.err_of_scale(np_(d2), 2.5 * want) <= 1e-6

    base = torch.from_numpy(np.random.default_rng(3).standard_normal(grid_h.shape).astype(np.float32)).to(dev)
    buf = base.clone()
    tv3, d3 = pkg.bilagrid_tv(grid, weight=2.5, dL_dgrid=buf)                                 # accumulate: one fp32 add
    assert d3.data_ptr() == buf.data_ptr()
    assert np_(buf).tobytes() == (np_(base) + np_(d2)).tobytes()
    assert np_(tv3).tobytes() == np_(tv).tobytes()


def test_model_steps_one_view(pkg, dev):
    model = pkg.BilateralGridModel(3, dev, grid_shape=(4, 3, 2), lr_init=0.01, lr_final=0.01)
    assert tuple(model.params.shape) == (3, 12, 2, 3, 4)
    assert np_(model.params[1]).tobytes() == br.identity_grid((4, 3, 2)).tobytes()
    assert model.grid(1).data_ptr() == model.params[1].data_ptr()                             # zero-copy
    grad = torch.from_numpy(np.random.default_rng(5).standard_normal((12, 2, 3, 4)).astype(np.float32)).to(dev)
    before = {k: np_(t).copy() for k, t in (("p", model.params), ("m", model.m_), ("v", model.v_))}
    model.step(1, grad, 0)
    after = {k: np_(t) for k, t in (("p", model.params), ("m", model.m_), ("v", model.v_))}
    for k in before:
        for view in (0, 2):
            assert after[k][view].tobytes() == before[k][view].tobytes(), (k, view)
        assert (after[k][1] != before[k][1]).all(), k
    # the first Adam step moves every element by lr against the sign of its gradient
    np.testing.assert_allclose(after["p"][1] - before["p"][1], -0.01 * np.sign(np_(grad)), rtol=0, atol=1e-6)
    assert model.steps_ == [0, 1, 0]

    state = model.state_dict()
    other = pkg.BilateralGridModel(3, dev, grid_shape=(4, 3, 2), lr_init=0.01, lr_final=0.01)
    other.load_state_dict(state)
    for a, b in ((other.params, model.params), (other.m_, model.m_), (other.v_, model.v_)):
        assert np_(a).tobytes() == np_(b).tobytes()
    assert other.steps_ == model.steps_
    model.step(1, grad, 1)                                                                    # the copies are independent
    assert np_(other.params).tobytes() == np_(state["params"]).tobytes()
    other.step(1, grad, 1)                                                                    # and resume identically
    assert np_(other.params).tobytes() == np_(model.params).tobytes()
    with pytest.raises(RuntimeError):
        model.step(3, grad, 0)
    with pytest.raises(RuntimeError):
        pkg.BilateralGridModel(2, dev, grid_shape=(4, 4, 2)).load_state_dict(state)


def test_wrappers_check_arguments(pkg, dev):
    grid_h, img_h, g_h = br.case(7, 5, (4, 3, 2))
    grid, img, g = _dev(dev, grid_h, img_h, g_h)
    for bad_grid in (grid.cpu(), grid.double(), grid[:, :, :, ::2], grid[:11], torch.zeros((12, 1, 3, 4), device=dev)):
        with pytest.raises(RuntimeError):
            pkg.bilagrid_slice(bad_grid, img)
    for bad_img in (img.cpu(), img.double(), img[..., :2], img.reshape(-1, 3)):
        with pytest.raises(RuntimeError):
            pkg.bilagrid_slice(grid, bad_img)
    with pytest.raises(RuntimeError):
        pkg.bilagrid_slice_backward(grid, img, g[:3])
    with pytest.raises(RuntimeError):
        pkg.bilagrid_tv(grid, dL_dgrid=torch.zeros((12, 2, 3, 5), device=dev))


def test_short_fit_recovers_a_grid(pkg, dev):
    """32x48, target = slice(G_true, c) with G_true = identity + 0.2 normal on a (4,4,2) grid; the model starts at the
    identity and takes 50 Adam steps at lr 0.01 of slice -> L1 loss -> backward -> step.  The same loop in libtorch
    (fp64 and fp32 alike) brings the L1 from 0.1002 to 0.0091 = 0.091 x; the bar is 0.2 x.  A wrong sign in either
    gradient makes the loss rise."""
    rng = np.random.default_rng(11)
    shape = (4, 4, 2)
    c = torch.from_numpy(rng.uniform(0.0, 1.0, (32, 48, 3)).astype(np.float32)).to(dev)
    g_true = torch.from_numpy((br.identity_grid(shape) + 0.2 * rng.standard_normal((12, 2, 4, 4))).astype(np.float32)).to(dev)
    target = pkg.bilagrid_slice(g_true, c)
    model = pkg.BilateralGridModel(1, dev, grid_shape=shape, lr_init=0.01, lr_final=0.01)
    losses = []
    for it in range(51):
        corrected = pkg.bilagrid_slice(model.grid(0), c)
        loss, grad = pkg.combined_loss_and_grad(corrected, target, lambda_=0.0)
        losses.append(loss)
        if it < 50:
            back = pkg.bilagrid_slice_backward(model.grid(0), c, grad)
            assert back.dL_drendered is not None
            model.step(0, back.dL_dgrid, it)
    first, last = float(losses[0]), float(losses[-1])
    print(f"fit: L1 {first:.4f} -> {last:.4f} = {last / first:.3f} x")
    assert last <= 0.2 * first
