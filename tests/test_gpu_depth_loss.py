"""The fused depth-supervision loss (csrc/depth_loss.hip, cugs_amd.depth_loss) on the GPU against its
numpy mirror tests/depth_loss_ref.py: the same bytes in dL_ddepth_map, dL_dalpha and expected, the exact valid count,
the loss, the weight sum and the fitted (s, b) within one float32 ulp of the reference's fp64 results - on every shape,
in both spaces, with and without a weight map, over the three alignment routes - and two short fits through
render_backward that a wrong sign in either gradient formula turns around."""
import ctypes as C

import numpy as np
import pytest
import torch

import depth_loss_ref as dr
from util import np_

pytestmark = pytest.mark.gpu

CASES = [(shape, inverse, weighted) for shape in dr.SHAPES for inverse in (False, True) for weighted in (False, True)]
IDS = [f"{h}x{w}-{'inv' if i else 'depth'}-{'w' if wt else 'now'}" for (h, w), i, wt in CASES]
GIVEN = (np.float32(0.8), np.float32(0.3))           # an alignment that is neither the identity nor the fit


def _tensors(case, weighted, dev):
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(case["D"]), t(case["A"]), t(case["t"]), (t(case["w"]) if weighted else None)


def _host(res):
    """Every output of a DepthLoss on the host (one read-back)."""
    out = {k: np_(getattr(res, k)) for k in ("loss", "scale_shift", "valid_weight", "valid_count", "fit_ok")}
    for k in ("dL_ddepth_map", "dL_dalpha", "expected"):
        v = getattr(res, k)
        if v is not None:
            out[k] = np_(v)
    return out


def _same_bytes(a, b, what):
    assert a.keys() == b.keys(), (what, a.keys(), b.keys())
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _check_against_reference(got, ref, s, b, label):
    for k, r in (("dL_ddepth_map", "gD"), ("dL_dalpha", "gA"), ("expected", "expected")):
        assert np.isfinite(got[k]).all(), (label, k)
        diff = int((got[k].view(np.uint32) != ref[r].view(np.uint32)).sum())
        assert got[k].tobytes() == ref[r].tobytes(), (label, k, f"{diff} of {got[k].size} elements differ")
    assert float(got["valid_count"]) == ref["n_valid"], (label, got["valid_count"], ref["n_valid"])
    ulp_loss, ulp_sw = dr.ulp_distance(got["loss"], ref["loss"]), dr.ulp_distance(got["valid_weight"], ref["sw"])
    print(label, f"loss {float(got['loss']):.9g} ref {ref['loss64']:.9g} ({ulp_loss} ulp)  valid weight "
          f"{float(got['valid_weight']):.9g} ref {ref['sw64']:.9g} ({ulp_sw} ulp)  valid {ref['n_valid']}")
    assert ulp_loss <= 1 and ulp_sw <= 1, (label, ulp_loss, ulp_sw)
    assert got["scale_shift"].tobytes() == np.array([s, b], np.float32).tobytes(), (label, got["scale_shift"], s, b)


@pytest.mark.parametrize("shape,inverse,weighted", CASES, ids=IDS)
def test_depth_loss_matches_reference_on_every_route(pkg, dev, shape, inverse, weighted):
    case = dr.case(*shape, inverse)
    D, A, t, w = _tensors(case, weighted, dev)
    kw = dict(weight=w, inverse=inverse, want_expected=True)
    # no alignment
    none = _host(pkg.depth_loss(D, A, t, **kw))
    _check_against_reference(none, dr.reference(case, weighted), np.float32(1), np.float32(0), "none")
    assert float(none["fit_ok"]) == 1.0
    _same_bytes(none, _host(pkg.depth_loss(D, A, t, **kw)), "none, second call")
    # a given (s, b)
    ss = torch.tensor(GIVEN, dtype=torch.float32, device=dev)
    given = _host(pkg.depth_loss(D, A, t, align=ss, **kw))
    _check_against_reference(given, dr.reference(case, weighted, *GIVEN), *GIVEN, "given")
    assert float(given["fit_ok"]) == 1.0
    _same_bytes(given, _host(pkg.depth_loss(D, A, t, align=ss, **kw)), "given, second call")
    # fitted on the device: the reference gets the (s, b) read back, so a last-bit difference cannot flip a sign
    res = pkg.depth_loss(D, A, t, align="fit", **kw)
    fit = _host(res)
    s, b = fit["scale_shift"]
    f = dr.fit(case, weighted)
    us, ub = dr.ulp_distance(s, np.float32(f["s"])), dr.ulp_distance(b, np.float32(f["b"]))
    print(f"fit s {s:.9g} ref {f['s']:.12g} ({us} ulp)  b {b:.9g} ref {f['b']:.12g} ({ub} ulp)  relvar {f['relvar']:.3f}")
    assert us <= 1 and ub <= 1, (s, b, f)
    assert float(fit["fit_ok"]) == 1.0
    _check_against_reference(fit, dr.reference(case, weighted, s, b), s, b, "fit")
    _same_bytes(fit, _host(pkg.depth_loss(D, A, t, align="fit", **kw)), "fit, second call")
    # the given route with the fitted values is the fit route
    _same_bytes(fit, _host(pkg.depth_loss(D, A, t, align=res.scale_shift.clone(), **kw)), "given the fitted values")


@pytest.mark.parametrize("shape,inverse,weighted", CASES, ids=IDS)
def test_fit_is_equivariant_to_an_affine_change_of_the_target(pkg, dev, shape, inverse, weighted):
    """t -> c1 t + c0 on the pixels that carry data (elsewhere the "no data" marks stay: 0 would become c0): the fit
    undoes it, s' c1 = s and s' c0 + b' = b, and the loss stays.  Bar 1e-4 of max(|s|, |b|, 1): the float rounding of
    the new target is ~6e-8 per pixel, the condition number at most 50 (relvar >= 0.02), so ~1e-6 is expected."""
    c1, c0 = np.float32(0.5), np.float32(1.0)
    case = dr.case(*shape, inverse)
    D, A, t, w = _tensors(case, weighted, dev)
    tn = case["t"]
    with np.errstate(all="ignore"):
        t2 = np.where((tn > 0) & (tn < np.inf), (c1 * tn + c0).astype(np.float32), tn).astype(np.float32)
    a = _host(pkg.depth_loss(D, A, t, weight=w, inverse=inverse, align="fit", want_grad=False))
    b = _host(pkg.depth_loss(D, A, torch.from_numpy(t2).to(dev), weight=w, inverse=inverse, align="fit", want_grad=False))
    (s, sh), (s2, sh2) = a["scale_shift"].astype(np.float64), b["scale_shift"].astype(np.float64)
    bar = 1e-4 * max(abs(s), abs(sh), 1.0)
    print(f"s {s:.8g} s'c1 {s2 * c1:.8g}  b {sh:.8g} s'c0+b' {s2 * c0 + sh2:.8g}  loss {float(a['loss']):.8g} {float(b['loss']):.8g}")
    assert float(a["fit_ok"]) == 1.0 and float(b["fit_ok"]) == 1.0
    assert abs(s2 * c1 - s) <= bar and abs(s2 * c0 + sh2 - sh) <= bar
    assert abs(float(a["loss"]) - float(b["loss"])) <= bar
    assert a["valid_count"] == b["valid_count"]


def _raw(pkg, dev, D, A, t, w, inverse, fit, g_d, g_a, expected):
    """cugs_depth_loss through ctypes, with any of the three maps absent."""
    from cugs_amd._lib import DepthLossOpts, check, lib
    from cugs_amd.rasterizer import _ptr, _stream, _workspace
    h, wd = D.shape
    out = torch.empty(8, dtype=torch.float32, device=dev)
    opts = DepthLossOpts(weight=_ptr(w), scale_shift=None, fit=int(fit), inverse=int(inverse), min_alpha=dr.MIN_ALPHA,
                         expected=_ptr(expected))
    ws = _workspace(dev, lib.cugs_depth_loss_workspace_bytes(wd, h), "depth_loss")
    check(lib.cugs_depth_loss(wd, h, _ptr(D), _ptr(A), _ptr(t), C.byref(opts), _ptr(ws), ws.numel(), _ptr(out), _ptr(g_d),
                              _ptr(g_a), _stream(dev)), "cugs_depth_loss")
    return np_(out)


@pytest.mark.parametrize("shape,inverse,weighted", CASES, ids=IDS)
def test_optional_outputs_leave_the_others_unchanged(pkg, dev, shape, inverse, weighted):
    case = dr.case(*shape, inverse)
    D, A, t, w = _tensors(case, weighted, dev)
    for align in (None, "fit"):
        kw = dict(weight=w, inverse=inverse, align=align)
        full = _host(pkg.depth_loss(D, A, t, want_expected=True, **kw))
        scalars = ("loss", "scale_shift", "valid_weight", "valid_count", "fit_ok")
        no_grad = pkg.depth_loss(D, A, t, want_grad=False, want_expected=True, **kw)
        assert no_grad.dL_ddepth_map is None and no_grad.dL_dalpha is None
        _same_bytes({k: full[k] for k in scalars + ("expected",)}, _host(no_grad), "want_grad=False")
        no_exp = pkg.depth_loss(D, A, t, want_expected=False, **kw)
        assert no_exp.expected is None
        _same_bytes({k: v for k, v in full.items() if k != "expected"}, _host(no_exp), "want_expected=False")
        bare = pkg.depth_loss(D, A, t, want_grad=False, want_expected=False, **kw)
        _same_bytes({k: full[k] for k in scalars}, _host(bare), "scalars only")
        # either gradient pointer NULL through the C ABI
        head = np.concatenate([np.atleast_1d(full[k]).ravel() for k in scalars[:4]] + [full["fit_ok"].ravel()])
        for want_d, want_a in ((True, False), (False, True), (False, False)):
            g_d = torch.full_like(D, 7.0) if want_d else None
            g_a = torch.full_like(D, 7.0) if want_a else None
            out = _raw(pkg, dev, D, A, t, w, inverse, align == "fit", g_d, g_a, None)
            assert out[:6].tobytes() == head.astype(np.float32).tobytes() and not out[6:].any(), (want_d, want_a, out, head)
            if want_d:
                assert np_(g_d).tobytes() == full["dL_ddepth_map"].tobytes()
            if want_a:
                assert np_(g_a).tobytes() == full["dL_dalpha"].tobytes()


@pytest.mark.parametrize("shape", [(7, 5), (37, 53)])
def test_unaligned_maps_take_the_scalar_path_to_the_same_bytes(pkg, dev, shape):
    """Contiguous views that start 4 bytes past a 16-byte boundary: no 16-byte access is possible, the pixel-to-thread
    map stays, so every output - the sums included - keeps its bytes."""
    case = dr.case(*shape, False)
    D, A, t, w = _tensors(case, True, dev)
    n = D.numel()

    def shifted(x):
        buf = torch.empty(n + 1, dtype=torch.float32, device=dev)
        buf[1:].copy_(x.reshape(-1))
        v = buf[1:].view(x.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    for align in (None, "fit"):
        want = _host(pkg.depth_loss(D, A, t, weight=w, align=align, want_expected=True))
        got = _host(pkg.depth_loss(shifted(D), shifted(A), shifted(t), weight=shifted(w), align=align, want_expected=True))
        _same_bytes(want, got, f"unaligned, align={align}")


def test_rejected_fit_falls_back_to_the_identity(pkg, dev):
    """A constant target has no variance to fit a scale to: fit_ok = 0, (s, b) = (1, 0), the outputs of no alignment."""
    case = dr.case(16, 16, False)
    D, A, t, w = _tensors(case, True, dev)
    const = torch.full_like(t, 4.0)
    fit, none = _host(pkg.depth_loss(D, A, const, weight=w, align="fit")), _host(pkg.depth_loss(D, A, const, weight=w))
    assert float(fit["fit_ok"]) == 0.0 and float(none["fit_ok"]) == 1.0
    assert fit["scale_shift"].tolist() == [1.0, 0.0]
    _same_bytes({k: v for k, v in fit.items() if k != "fit_ok"}, {k: v for k, v in none.items() if k != "fit_ok"}, "rejected")
    # nothing valid at all: zero loss, zero gradients, nothing NaN
    dead = _host(pkg.depth_loss(D, A, torch.zeros_like(t), align="fit", want_expected=True))
    assert float(dead["loss"]) == 0.0 and float(dead["valid_count"]) == 0.0 and float(dead["fit_ok"]) == 0.0
    assert not dead["dL_ddepth_map"].any() and not dead["dL_dalpha"].any() and not dead["expected"].any()


def test_bad_arguments_raise(pkg, dev):
    from cugs_amd._lib import DepthLossOpts, check, lib
    from cugs_amd.rasterizer import _ptr
    z = torch.ones((8, 6), device=dev)
    ok = pkg.depth_loss(z, z, z)
    assert float(ok.loss) == 0.0 and float(ok.valid_count) == 48.0
    bad = [
        lambda: pkg.depth_loss(z.reshape(-1), z, z),                                   # shapes
        lambda: pkg.depth_loss(z.unsqueeze(-1), z, z),
        lambda: pkg.depth_loss(z, z[:4], z),
        lambda: pkg.depth_loss(z, z, z.t()),
        lambda: pkg.depth_loss(z, z, z, weight=z[:, :3]),
        lambda: pkg.depth_loss(z.double(), z, z),                                      # dtypes
        lambda: pkg.depth_loss(z, z.half(), z),
        lambda: pkg.depth_loss(z, z, z.to(torch.uint8)),
        lambda: pkg.depth_loss(z, z, z, weight=z > 0),
        lambda: pkg.depth_loss(z.cpu(), z, z),                                         # devices
        lambda: pkg.depth_loss(z, z.cpu(), z),
        lambda: pkg.depth_loss(z, z, z.cpu()),
        lambda: pkg.depth_loss(z, z, z, weight=z.cpu()),
        lambda: pkg.depth_loss(z, z, z, min_alpha=0.0),                                # min_alpha
        lambda: pkg.depth_loss(z, z, z, min_alpha=-1e-3),
        lambda: pkg.depth_loss(z, z, z, min_alpha=float("inf")),
        lambda: pkg.depth_loss(z, z, z, min_alpha=float("nan")),
        lambda: pkg.depth_loss(z, z, z, align="median"),                               # align
        lambda: pkg.depth_loss(z, z, z, align=torch.ones(3, device=dev)),
        lambda: pkg.depth_loss(z, z, z, align=torch.ones(2, device=dev, dtype=torch.float64)),
        lambda: pkg.depth_loss(z, z, z, align=torch.ones(2)),
        lambda: pkg.depth_loss(z, z, z, align=(1.0, 0.0)),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail(f"bad argument {i} was accepted")
    # a fit together with a given (s, b): the C ABI refuses it before anything is queued
    ss, out, ws = torch.ones(2, device=dev), torch.zeros(8, device=dev), torch.empty(4096, dtype=torch.uint8, device=dev)
    opts = DepthLossOpts(scale_shift=_ptr(ss), fit=1, min_alpha=1e-3)
    with pytest.raises(RuntimeError):
        check(lib.cugs_depth_loss(6, 8, _ptr(z), _ptr(z), _ptr(z), C.byref(opts), _ptr(ws), ws.numel(), _ptr(out), None,
                                  None, None), "cugs_depth_loss")
    assert not np_(out).any()


def _fit_scene(pkg, dev):
    """The scene of tests/test_gpu_depth_map.py's depth fit: 128x96, 1500 Gaussians, z-perturbed positions."""
    w, h, n = 128, 96, 1500
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=0, seed=8, mu_s=-3.0)
    cam = pkg.scene.make_camera(w, h, view=0)
    settings = pkg.RenderSettings(active_sh_degree=0)
    true = pkg.render(pkg.scene.to_model(arrays, dev), cam, settings, want_depth_map=True, for_backward=False)
    tD, tA = true.depth_map.clone(), true.alpha.clone()
    depth = torch.where(tA > 0.5, tD / tA.clamp_min(1e-6), torch.zeros_like(tD))       # 0: no data
    rng = np.random.default_rng(9)
    pert = dict(arrays)
    pert["positions"] = (arrays["positions"] + np.stack([np.zeros(n), np.zeros(n), rng.normal(0.0, 0.4, n)], 1)
                         ).astype(np.float32)
    model = pkg.scene.to_model(pert, dev)
    cfg = pkg.AdamConfig(position_lr_config=pkg.PositionLRConfig(lr_init=1e-2, lr_final=1e-2))
    return w, h, cam, settings, model, pkg.FusedAdam(model, cfg), depth, tA


def test_fitting_with_depth_loss_reduces_the_depth_loss(pkg, dev):
    """Perturbed positions pulled back by depth_loss on the expected depth of the true scene (where its alpha is above
    0.5) plus the torch L1 alpha term of the existing depth fit, with FusedAdam.  A sign test, not a measurement: a
    wrong sign in dL/dD or dL/dA makes the loss grow."""
    w, h, cam, settings, model, opt, target, tA = _fit_scene(pkg, dev)
    hw = float(w * h)
    zero_c = torch.zeros((h, w, 3), device=dev)
    losses = []
    for it in range(100):
        out = pkg.render(model, cam, settings, want_depth_map=True)
        d = pkg.depth_loss(out.depth_map, out.alpha, target)
        losses.append(float(d.loss))
        pkg.render_backward(zero_c, out, model, cam, settings, fused_adam=opt, dL_ddepth_map=d.dL_ddepth_map,
                            dL_dalpha=d.dL_dalpha + torch.sign(out.alpha - tA) / hw)
    curve = " ".join(f"{v:.4f}" for v in losses[::10]) + f" ... {losses[-1]:.4f}"
    print("expected-depth L1 loss curve (every 10th):", curve)
    # measured on one MI355X: 0.4153 -> 0.0244 over the 100 iterations (-94 %); the bar leaves a wide margin
    assert losses[-1] < 0.5 * losses[0], "expected-depth L1 loss curve (every 10th): " + curve


def test_fitting_in_inverse_space_with_a_fitted_alignment(pkg, dev):
    """A monocular-style prior: the inverse of an affinely distorted depth, 1 / (0.5 d + 1).  The fitted alignment
    starts below the unaligned loss, and a short run with align="fit" lowers the fitted loss."""
    w, h, cam, settings, model, opt, depth, tA = _fit_scene(pkg, dev)
    target = torch.where(depth > 0, 1.0 / (0.5 * depth + 1.0), torch.zeros_like(depth))
    zero_c = torch.zeros((h, w, 3), device=dev)
    out = pkg.render(model, cam, settings, want_depth_map=True, for_backward=False)
    plain = float(pkg.depth_loss(out.depth_map, out.alpha, target, inverse=True, want_grad=False).loss)
    losses = []
    for it in range(41):
        out = pkg.render(model, cam, settings, want_depth_map=True)
        d = pkg.depth_loss(out.depth_map, out.alpha, target, inverse=True, align="fit")
        losses.append(float(d.loss))
        assert float(d.fit_ok) == 1.0
        if it < 40:
            pkg.render_backward(zero_c, out, model, cam, settings, fused_adam=opt, dL_ddepth_map=d.dL_ddepth_map,
                                dL_dalpha=d.dL_dalpha)
    curve = " ".join(f"{v:.5f}" for v in losses[::5])
    print(f"inverse-space loss, unaligned {plain:.5f}; fitted (every 5th): {curve}")
    # measured on one MI355X: unaligned 0.04534, fitted 0.02512 at iteration 0 and 0.00212 after 40 iterations
    assert losses[0] < plain, (losses[0], plain)
    assert losses[-1] < losses[0], curve
