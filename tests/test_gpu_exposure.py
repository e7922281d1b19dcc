"""Per-view exposure compensation and pixel masks in the fused loss on the GPU (csrc/loss.hip EXPO kernels through
cugs_combined_loss_opts, cugs_amd.combined_loss_exposure, cugs_amd.ExposureModel) against the CPU
mirror of tests/exposure_ref.py: the reference's loss ops on x' = m (A c + b), y' = m y, plus autograd."""
import ctypes as C

import numpy as np
import pytest
import torch

import exposure_ref as er
from util import max_err_over_max, np_

pytestmark = pytest.mark.gpu


def _check_parity(pkg, dev, c, t, E, mask, want, lam=0.2, ws=11, label=""):
    got = pkg.combined_loss_exposure(c.to(dev), t.to(dev), lam, exposure=E.to(dev), mask=None if mask is None else mask.to(dev),
                                     want_corrected=True, window_size=ws)
    errs = {k: abs(float(getattr(got, k)) - want[k]) / max(1.0, abs(want[k])) for k in ("loss", "l1", "ssim_mean")}
    errs["dL_dcolor"] = max_err_over_max(np_(got.dL_dcolor), want["dL_dcolor"])
    errs["dL_dexposure"] = max_err_over_max(np_(got.dL_dexposure), want["dL_dexposure"])
    errs["corrected"] = float(np.max(np.abs(np_(got.corrected).astype(np.float64) - want["corrected"])))
    print(label, {k: f"{v:.1e}" for k, v in errs.items()})
    assert got.dL_dcolor.shape == c.shape and got.dL_dexposure.shape == (3, 4) and got.loss.dim() == 0
    for k in ("loss", "l1", "ssim_mean"):
        assert errs[k] <= 1e-5, (k, errs)
    # the project's gradient bar: 1e-4 of each tensor's scale (the mirror's own rounding is ~1e-6, test_exposure_ref.py)
    assert errs["dL_dcolor"] <= 1e-4 and errs["dL_dexposure"] <= 1e-4, errs
    assert errs["corrected"] <= 1e-6, errs


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("h,w,ws", [(7, 5, 11), (17, 33, 11), (37, 53, 7), (37, 53, 11), (64, 64, 11)])
def test_parity_against_the_mirror(pkg, dev, h, w, ws, masked):
    c, t, E, mask, want = er.case(h, w, masked, 0.2, ws)
    _check_parity(pkg, dev, c, t, E, mask, want, 0.2, ws, f"{(h, w)} window {ws} masked {masked}")


def test_parity_with_more_tiles_than_reduction_lanes(pkg, dev):
    """3 x 45 = 135 tiles: every lane of the final reduction (85 per entry) takes a tile, the first fifty take two."""
    c, t, E, mask, want = er.case(33, 720, True)
    _check_parity(pkg, dev, c, t, E, mask, want, 0.2, 11, "(33, 720) masked")


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_parity_at_the_ends_of_lambda(pkg, dev, lam):
    c, t, E, mask, want = er.case(17, 33, True, lam)
    _check_parity(pkg, dev, c, t, E, mask, want, lam, 11, f"lambda {lam}")


@pytest.mark.parametrize("ws", [11, 7])
def test_offset_at_the_image_edge(pkg, dev, ws):
    """b != 0: a halo pixel outside the image is 0, not b - a loader that pads with the corrected value of a zero
    pixel shifts every window that crosses the edge."""
    c, t, _, _ = er.make_case(17, 33)
    E = er.identity()
    E[:, 3] = 0.3
    want = er.mirror(c, t, E, None, 0.2, ws)
    _check_parity(pkg, dev, c, t, E, None, want, 0.2, ws, f"b = 0.3, window {ws}")


def _raw(pkg, dev, c, t, ws, opts, with_opts_entry):
    """One call of the C ABI: (loss_out[4], ssim_map, dL_dcolor) as numpy arrays."""
    from cugs_amd._lib import check, lib
    h, w = c.shape[:2]
    out = torch.full((4,), -7.0, device=dev)
    smap, grad = torch.full((h, w), -7.0, device=dev), torch.full((h, w, 3), -7.0, device=dev)
    work = torch.empty(lib.cugs_loss_opts_workspace_bytes(w, h), dtype=torch.uint8, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if with_opts_entry:
        check(lib.cugs_combined_loss_opts(w, h, p(c), p(t), 0.2, ws, opts, p(work), work.numel(), p(out), p(smap), p(grad),
                                          stream), "cugs_combined_loss_opts")
    else:
        check(lib.cugs_combined_loss(w, h, p(c), p(t), 0.2, ws, p(work), work.numel(), p(out), p(smap), p(grad), stream),
              "cugs_combined_loss")
    return np_(out), np_(smap), np_(grad)


@pytest.mark.parametrize("h,w,ws", [(37, 53, 11), (37, 53, 7), (7, 5, 11)])
def test_no_options_gives_the_plain_routes_bits(pkg, dev, h, w, ws):
    from cugs_amd._lib import LossOpts
    c, t, _, _ = er.make_case(h, w)
    c, t = c.to(dev), t.to(dev)
    plain = _raw(pkg, dev, c, t, ws, None, False)
    for opts in (None, C.byref(LossOpts())):
        got = _raw(pkg, dev, c, t, ws, opts, True)
        for a, b in zip(got, plain):
            assert np.array_equal(a, b)
    # the identity through the EXPO kernels, on finite inputs: still every bit (a -0.0 may come back as +0.0)
    eye = er.identity().to(dev)
    got = _raw(pkg, dev, c, t, ws, C.byref(LossOpts(exposure=eye.data_ptr())), True)
    for a, b in zip(got, plain):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("h,w", [(17, 33), (64, 64)])
def test_identity_and_unit_mask_are_exact(pkg, dev, h, w):
    c, t, E, _ = er.make_case(h, w)
    c, t, E = c.to(dev), t.to(dev), E.to(dev)
    loss, grad = pkg.combined_loss_and_grad(c, t)
    ident = pkg.combined_loss_exposure(c, t, exposure=er.identity().to(dev), want_corrected=True)
    assert np.array_equal(np_(ident.loss), np_(loss)) and np.array_equal(np_(ident.dL_dcolor), np_(grad))
    assert np.array_equal(np_(ident.corrected), np_(c))
    nothing = pkg.combined_loss_exposure(c, t)
    assert np.array_equal(np_(nothing.loss), np_(loss)) and np.array_equal(np_(nothing.dL_dcolor), np_(grad))
    assert nothing.dL_dexposure is None and nothing.corrected is None
    a = pkg.combined_loss_exposure(c, t, exposure=E, want_corrected=True)
    b = pkg.combined_loss_exposure(c, t, exposure=E, mask=torch.ones((h, w), device=dev), want_corrected=True)
    for k in ("loss", "l1", "ssim_mean", "dL_dcolor", "dL_dexposure", "corrected"):
        assert np.array_equal(np_(getattr(a, k)), np_(getattr(b, k))), k


def test_exposure_gradient_is_reproducible(pkg, dev):
    c, t, E, mask = er.make_case(64, 64)
    c, t, E, mask = c.to(dev), t.to(dev), E.to(dev), mask.to(dev)
    a = pkg.combined_loss_exposure(c, t, exposure=E, mask=mask)
    b = pkg.combined_loss_exposure(c, t, exposure=E, mask=mask)
    assert np_(a.dL_dexposure).tobytes() == np_(b.dL_dexposure).tobytes()
    assert np_(a.dL_dcolor).tobytes() == np_(b.dL_dcolor).tobytes() and np_(a.loss).tobytes() == np_(b.loss).tobytes()


@pytest.mark.parametrize("ws", [11, 7])
def test_all_zero_mask(pkg, dev, ws):
    c, t, E, _ = er.make_case(37, 53)
    got = pkg.combined_loss_exposure(c.to(dev), t.to(dev), exposure=E.to(dev), mask=torch.zeros((37, 53), device=dev),
                                     window_size=ws)
    assert not np_(got.dL_dcolor).any() and not np_(got.dL_dexposure).any()
    assert float(got.l1) == 0.0 and abs(float(got.ssim_mean) - 1.0) <= 1e-6


def test_loss_only_and_mask_only(pkg, dev):
    """want_grad=False takes the one-workgroup finalize; a mask without an exposure has no dL_dexposure."""
    c, t, E, mask, want = er.case(37, 53, True)
    cd, td, Ed, md = c.to(dev), t.to(dev), E.to(dev), mask.to(dev)
    got = pkg.combined_loss_exposure(cd, td, exposure=Ed, mask=md, want_grad=False)
    assert got.dL_dcolor is None and got.dL_dexposure is None and got.corrected is None
    assert abs(float(got.loss) - want["loss"]) <= 1e-5
    full = pkg.combined_loss_exposure(cd, td, exposure=Ed, mask=md)
    assert np.array_equal(np_(full.loss), np_(got.loss))
    only = pkg.combined_loss_exposure(cd, td, mask=md)
    ref = er.mirror(c, t, None, mask)
    assert only.dL_dexposure is None and abs(float(only.loss) - ref["loss"]) <= 1e-5
    assert max_err_over_max(np_(only.dL_dcolor), ref["dL_dcolor"]) <= 1e-4


def test_validation(pkg, dev):
    c, t, E, mask = er.make_case(17, 33)
    c, t, E, mask = c.to(dev), t.to(dev), E.to(dev), mask.to(dev)
    bad = [dict(exposure=E.T.contiguous()), dict(exposure=E[:2]), dict(exposure=E.double()), dict(exposure=E.cpu()),
           dict(exposure=E.T.contiguous().T),                                  # [3,4] but not contiguous
           dict(mask=mask[:5]), dict(mask=mask.T.contiguous()), dict(mask=mask.double()), dict(mask=mask.cpu()),
           dict(mask=mask.unsqueeze(-1)), dict(window_size=10)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            pkg.combined_loss_exposure(c, t, **kw)
    with pytest.raises(RuntimeError):
        pkg.combined_loss_exposure(c, t[:5], exposure=E)


def test_exposure_model(pkg, dev):
    model = pkg.ExposureModel(3, dev, lr_init=0.01, lr_final=0.001, max_steps=30)
    assert model.params.shape == (3, 3, 4) and model.m_.shape == (3, 3, 4) and model.v_.shape == (3, 3, 4)
    first = np_(model.params).copy()
    assert np.array_equal(first, np.broadcast_to(er.identity().numpy(), (3, 3, 4)))
    assert model.matrix(1).data_ptr() == model.params[1].data_ptr() and model.matrix(1).is_contiguous()
    g = torch.Generator().manual_seed(4)
    mirror = er.AdamMirror(er.identity())
    for it in range(10):
        grad = torch.randn((3, 4), generator=g) * (0.1 + it)
        lr = pkg.position_lr(it * 3, pkg.PositionLRConfig(lr_init=0.01, lr_final=0.001, max_steps=30))
        model.step(1, grad.to(dev), it * 3)
        want = mirror.step(grad, lr)
        assert float(np.max(np.abs(np_(model.matrix(1)) - want.numpy()))) <= 1e-6, it
    after = np_(model.params)
    assert after[0].tobytes() == first[0].tobytes() and after[2].tobytes() == first[2].tobytes()
    assert not np_(model.m_[0]).any() and not np_(model.v_[2]).any() and model.steps_ == [0, 10, 0]
    names = ["a.png", "b.png", "c.png"]
    back = pkg.ExposureModel.from_json(model.to_json(names), names, dev)
    assert np.array_equal(np_(back.params), after) and not np_(back.m_).any()
    swapped = pkg.ExposureModel.from_json(model.to_json(names), names[::-1], dev)
    assert np.array_equal(np_(swapped.params), after[::-1])
    with pytest.raises(RuntimeError):
        model.step(3, torch.zeros((3, 4), device=dev), 0)
    with pytest.raises(RuntimeError):
        model.step(0, torch.zeros((3, 3), device=dev), 0)


def test_exposure_pipeline(pkg, dev):
    """render -> combined_loss_exposure -> render_backward / ExposureModel.step: thirty iterations that optimise only
    the exposure lower the loss against a target made with a gain, on the unmasked half of the image."""
    w, h, n = 160, 120, 400
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=1, seed=12, mu_s=-2.6)
    cam = pkg.scene.make_camera(w, h)
    model = pkg.scene.to_model(arrays, dev)
    st = pkg.RenderSettings(active_sh_degree=1)
    out = pkg.render(model, cam, st)
    target = (1.3 * out.color + 0.05).contiguous()                       # E* = [1.3 I | 0.05]
    mask = torch.zeros((h, w), device=dev)
    mask[:, : w // 2] = 1.0
    expo = pkg.ExposureModel(2, dev, lr_init=0.01, lr_final=0.01, max_steps=30)
    losses = []
    for it in range(30):
        res = pkg.combined_loss_exposure(out.color, target, exposure=expo.matrix(0), mask=mask)
        losses.append(res.loss)
        expo.step(0, res.dL_dexposure, it)
    final = pkg.combined_loss_exposure(out.color, target, exposure=expo.matrix(0), mask=mask)
    losses = [float(x) for x in losses]
    assert float(final.loss) < losses[0], (losses[0], float(final.loss))
    assert not np_(final.dL_dcolor[:, w // 2:]).any()                    # nothing flows through masked pixels
    grads = pkg.render_backward(final.dL_dcolor, out, model, cam, st)
    assert bool(torch.isfinite(grads.dL_dsh_coeffs).all()) and float(grads.dL_dsh_coeffs.abs().max()) > 0.0
    assert np.array_equal(np_(expo.params[1]), er.identity().numpy())
