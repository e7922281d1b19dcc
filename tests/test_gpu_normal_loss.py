"""The fused normal-supervision loss (csrc/normal_loss.hip, cugs_amd.normal_loss) on the GPU against its
numpy mirror tests/normal_loss_ref.py: the same bytes in dL_ddepth_map, dL_dalpha and the normal map, the exact valid
count, the loss and the weight sum within one float32 ulp of the mirror's fp64 results - on every shape, with and
without a weight map, a prior and the normal map, with either distance alone and both - the same bytes from
non-contiguous and 4-byte-offset views and whatever the tiling, and two short fits through render_backward that a wrong
sign in either gradient formula turns round."""
import numpy as np
import pytest
import torch

import normal_loss_ref as nr
from util import np_

pytestmark = pytest.mark.gpu

SHAPES = nr.SHAPES + [nr.MANY_TILES]
CASES = [(shape, weighted) for shape in SHAPES for weighted in (False, True)]
IDS = [f"{h}x{w}-{'w' if wt else 'now'}" for (h, w), wt in CASES]
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (0.7, 0.3)]           # cos alone, L1 alone, both


def _camera(case):
    from cugs_amd.types import CameraInfo, CameraIntrinsics
    return CameraInfo(width=case["width"], height=case["h"],
                      intrinsics=CameraIntrinsics(fx=case["fx"], fy=case["fy"], cx=case["cx"], cy=case["cy"]))


def _tensors(case, weighted, dev):
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(case["D"]), t(case["A"]), t(case["t"]), (t(case["w"]) if weighted else None)


def _host(res):
    """Every output of a NormalLoss on the host (one read-back)."""
    out = {k: np_(getattr(res, k)) for k in ("loss", "valid_weight", "valid_count")}
    for k in ("dL_ddepth_map", "dL_dalpha", "normals"):
        v = getattr(res, k)
        if v is not None:
            out[k] = np_(v)
    return out


def _same_bytes(a, b, what):
    assert a.keys() == b.keys(), (what, a.keys(), b.keys())
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _check_against_reference(got, ref, label):
    for k, r in (("dL_ddepth_map", "gD"), ("dL_dalpha", "gA"), ("normals", "normals")):
        if k not in got:
            continue
        assert np.isfinite(got[k]).all(), (label, k)
        differ = got[k].view(np.uint32) != ref[r].view(np.uint32)
        dev_ = float(np.abs(got[k].astype(np.float64) - ref[r]).max()) if differ.any() else 0.0
        print(label, k, f"{int(differ.sum())} of {got[k].size} elements differ from the mirror, max deviation {dev_:.3e}")
        assert got[k].tobytes() == ref[r].tobytes(), (label, k, f"{int(differ.sum())} of {got[k].size} elements differ")
    assert float(got["valid_count"]) == ref["n_valid"], (label, got["valid_count"], ref["n_valid"])
    ulp_loss, ulp_sw = nr.ulp_distance(got["loss"], ref["loss"]), nr.ulp_distance(got["valid_weight"], ref["sw"])
    print(label, f"loss {float(got['loss']):.9g} ref {ref['loss64']:.9g} ({ulp_loss} ulp)  valid weight "
          f"{float(got['valid_weight']):.9g} ref {ref['sw64']:.9g} ({ulp_sw} ulp)  valid {ref['n_valid']}")
    assert ulp_loss <= 1 and ulp_sw <= 1, (label, ulp_loss, ulp_sw)


@pytest.mark.parametrize("shape,weighted", CASES, ids=IDS)
def test_normal_loss_matches_reference_on_every_route(pkg, dev, shape, weighted):
    case = nr.case(*shape)
    cam = _camera(case)
    D, A, t, w = _tensors(case, weighted, dev)
    for cw, lw in WEIGHTS:
        kw = dict(weight=w, cos_weight=cw, l1_weight=lw)
        ref = nr.reference(case, weighted, cos_weight=cw, l1_weight=lw)
        full = _host(pkg.normal_loss(D, A, cam, t, want_normals=True, **kw))
        _check_against_reference(full, ref, f"cos {cw} l1 {lw}")
        _same_bytes(full, _host(pkg.normal_loss(D, A, cam, t, want_normals=True, **kw)), "second call")
        if shape in nr.EMPTY:
            assert float(full["loss"]) == 0.0 and float(full["valid_count"]) == 0.0
            for k in ("dL_ddepth_map", "dL_dalpha", "normals"):
                assert not full[k].view(np.uint32).any(), k
        # without the normal map, without the gradients: the other outputs keep their bytes
        no_n = pkg.normal_loss(D, A, cam, t, **kw)
        assert no_n.normals is None
        _same_bytes({k: v for k, v in full.items() if k != "normals"}, _host(no_n), "want_normals=False")
        no_g = pkg.normal_loss(D, A, cam, t, want_grad=False, want_normals=True, **kw)
        assert no_g.dL_ddepth_map is None and no_g.dL_dalpha is None
        _same_bytes({k: v for k, v in full.items() if not k.startswith("dL_")}, _host(no_g), "want_grad=False")
        bare = pkg.normal_loss(D, A, cam, t, want_grad=False, **kw)
        _same_bytes({k: full[k] for k in ("loss", "valid_weight", "valid_count")}, _host(bare), "scalars only")
    if not weighted:
        # no prior: the normal map alone, loss 0, no gradients
        res = pkg.normal_loss(D, A, cam, None, want_normals=True)
        assert res.dL_ddepth_map is None and res.dL_dalpha is None
        got = _host(res)
        _check_against_reference(got, nr.reference(case, prior=False), "no prior")
        assert float(got["loss"]) == 0.0 and float(got["valid_weight"]) == 0.0 and float(got["valid_count"]) == 0.0
        assert np_(pkg.depth_to_normals(D, A, cam)).tobytes() == got["normals"].tobytes()


@pytest.mark.parametrize("shape", [(9, 11), (37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_views_give_the_bytes_of_the_contiguous_call(pkg, dev, shape):
    """Non-contiguous views (every second column of a wider buffer, a channel-last prior) and contiguous views that
    start 4 bytes past a 16-byte boundary."""
    case = nr.case(*shape)
    cam = _camera(case)
    D, A, t, w = _tensors(case, True, dev)
    kw = dict(cos_weight=0.7, l1_weight=0.3, want_normals=True)
    want = _host(pkg.normal_loss(D, A, cam, t, weight=w, **kw))

    def strided(x):
        buf = torch.full(x.shape[:-1] + (2 * x.shape[-1],), 7.0, dtype=torch.float32, device=dev)
        buf[..., ::2] = x
        v = buf[..., ::2]
        assert not v.is_contiguous()
        return v

    def shifted(x):
        buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=dev)
        buf[1:].copy_(x.reshape(-1))
        v = buf[1:].view(x.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    channel_last = t.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not channel_last.is_contiguous()
    _same_bytes(want, _host(pkg.normal_loss(strided(D), strided(A), cam, channel_last, weight=strided(w), **kw)), "strided")
    _same_bytes(want, _host(pkg.normal_loss(shifted(D), shifted(A), cam, shifted(t), weight=shifted(w), **kw)), "shifted")


@pytest.mark.parametrize("dv,du", [(0, 0), (3, 5)], ids=["top-left", "shifted"])
def test_a_pixel_does_not_depend_on_the_tiling(pkg, dev, dv, du):
    """The 37x53 case as a window at (dv, du) of a 74x106 image with other values around it.  A pixel's gradient
    reaches 2 pixels and its normal 1, so every pixel of the window at least that far from the cut keeps its bytes,
    although it now lies in another image, in a tile row of another workgroup count and - shifted - at other tile
    edges (64 k - 5 and 16 k - 3 in window coordinates).  What makes the comparison exact: the principal point moves
    with the window and sits on a quarter pixel, so ((u + 0.5) - cx) is the same float in both images; and the larger
    image has 4 x the pixels, so its 1 / (H W) - and with it every gradient - is the smaller one's times 2^-2."""
    from cugs_amd.types import CameraInfo, CameraIntrinsics
    small, large = nr.case(37, 53), nr.case(74, 106)
    h, w = 37, 53
    cam = lambda width, height, ox, oy: CameraInfo(width=width, height=height, intrinsics=CameraIntrinsics(
        fx=53.0, fy=53.0, cx=27.25 + ox, cy=18.75 + oy))

    def embed(key):
        a = large[key].copy()
        a[..., dv:dv + h, du:du + w] = small[key]
        return torch.from_numpy(a).to(dev)

    kw = dict(cos_weight=0.7, l1_weight=0.3, want_normals=True)
    D, A, t, wt = _tensors(small, True, dev)
    alone = _host(pkg.normal_loss(D, A, cam(w, h, 0, 0), t, weight=wt, **kw))
    inside = _host(pkg.normal_loss(embed("D"), embed("A"), cam(106, 74, du, dv), embed("t"), weight=embed("w"), **kw))
    assert float(alone["valid_count"]) > 1000
    win = inside["normals"][:, dv:dv + h, du:du + w]
    assert win[:, 1:-1, 1:-1].tobytes() == alone["normals"][:, 1:-1, 1:-1].tobytes()
    for k in ("dL_ddepth_map", "dL_dalpha"):
        win = inside[k][dv:dv + h, du:du + w][2:-2, 2:-2] * np.float32(4.0)
        assert win.any() and win.tobytes() == alone[k][2:-2, 2:-2].tobytes(), k


def test_bad_arguments_raise(pkg, dev):
    case = nr.case(9, 11)
    cam = _camera(case)
    D, A, t, w = _tensors(case, True, dev)
    ok = pkg.normal_loss(D, A, cam, t, weight=w)
    assert float(ok.valid_count) > 0
    from cugs_amd.types import CameraInfo, CameraIntrinsics
    flat = CameraInfo(width=11, height=9, intrinsics=CameraIntrinsics(fx=0.0, fy=11.0, cx=5.0, cy=4.0))
    bad = [
        lambda: pkg.normal_loss(D.reshape(-1), A, cam, t),                            # shapes
        lambda: pkg.normal_loss(D, A[:4], cam, t),
        lambda: pkg.normal_loss(D, A, cam, t[:2]),
        lambda: pkg.normal_loss(D, A, cam, t.permute(1, 2, 0)),
        lambda: pkg.normal_loss(D, A, cam, t, weight=w[:, :3]),
        lambda: pkg.normal_loss(D.double(), A, cam, t),                               # dtypes
        lambda: pkg.normal_loss(D, A.half(), cam, t),
        lambda: pkg.normal_loss(D, A, cam, t.double()),
        lambda: pkg.normal_loss(D, A, cam, t, weight=w > 0),
        lambda: pkg.normal_loss(D.cpu(), A, cam, t),                                  # devices
        lambda: pkg.normal_loss(D, A.cpu(), cam, t),
        lambda: pkg.normal_loss(D, A, cam, t.cpu()),
        lambda: pkg.normal_loss(D, A, cam, t, weight=w.cpu()),
        lambda: pkg.normal_loss(D, A, (11.0, 11.0, 5.0, 4.0), t),                     # camera
        lambda: pkg.normal_loss(D, A, flat, t),
        lambda: pkg.normal_loss(D, A, cam, t, min_alpha=0.0),                         # min_alpha
        lambda: pkg.normal_loss(D, A, cam, t, min_alpha=float("nan")),
        lambda: pkg.normal_loss(D, A, cam, t, cos_weight=-1.0),                       # loss weights
        lambda: pkg.normal_loss(D, A, cam, t, l1_weight=float("inf")),
        lambda: pkg.normal_loss(D, A, cam, t, cos_weight=0.0, l1_weight=0.0),
        lambda: pkg.normal_loss(D, A, cam, None),                                     # no prior: nothing to compute
        lambda: pkg.normal_loss(D, A, cam, None, weight=w, want_normals=True),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail(f"bad argument {i} was accepted")


def _plane_scene(pkg, dev):
    """A 20 x 20 grid of overlapping Gaussians on the plane z = 4 + 0.4 x - 0.2 y, seen at 96x72; the prior is the unit
    normal of another plane, z = 4 - 0.3 x + 0.3 y, at every pixel: n ~ (dz/dx, dz/dy, -1)."""
    w, h, side = 96, 72, 20
    n = side * side
    cam = pkg.scene.make_camera(w, h, view=0)
    K = cam.intrinsics
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=0, seed=11)
    gx, gy = np.meshgrid(np.linspace(-1.1, 1.1, side), np.linspace(-1.1, 1.1, side))
    x, y = gx.ravel() * 4.0 * (w / 2.0) / K.fx, gy.ravel() * 4.0 * (h / 2.0) / K.fy
    z = 4.0 + 0.4 * x - 0.2 * y
    arrays["positions"] = np.stack([x * z / 4.0, y * z / 4.0, z], 1).astype(np.float32)
    spacing = 2.2 * 4.0 * (w / 2.0) / K.fx / (side - 1)
    arrays["scales"] = np.full((n, 3), np.log(0.7 * spacing), np.float32)
    arrays["opacities"] = np.full((n, 1), 2.0, np.float32)
    arrays["rotations"] = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (n, 1))
    prior = np.array([-0.3, 0.3, -1.0], np.float32)
    target = torch.from_numpy(np.broadcast_to(prior[:, None, None], (3, h, w)).copy()).to(dev)
    model = pkg.scene.to_model(arrays, dev)
    cfg = pkg.AdamConfig(position_lr_config=pkg.PositionLRConfig(lr_init=1e-2, lr_final=1e-2))
    return w, h, cam, pkg.RenderSettings(active_sh_degree=0), model, pkg.FusedAdam(model, cfg), target


@pytest.mark.parametrize("cw,lw", [(1.0, 0.0), (0.0, 1.0)], ids=["cos", "l1"])
def test_fitting_with_normal_loss_reduces_the_normal_loss(pkg, dev, cw, lw):
    """20 fused-Adam steps driven by dL_ddepth_map and dL_dalpha of normal_loss alone (a zero colour gradient): the
    plane of Gaussians tilts towards the prior's plane.  A sign test, not a measurement: a wrong sign in dL/dD or dL/dA
    makes the loss grow."""
    w, h, cam, settings, model, opt, target = _plane_scene(pkg, dev)
    zero_c = torch.zeros((h, w, 3), device=dev)
    losses, counts = [], []
    for it in range(21):
        out = pkg.render(model, cam, settings, want_depth_map=True)
        r = pkg.normal_loss(out.depth_map, out.alpha, cam, target, cos_weight=cw, l1_weight=lw, min_alpha=0.5)
        losses.append(float(r.loss))
        counts.append(float(r.valid_count))
        if it < 20:
            pkg.render_backward(zero_c, out, model, cam, settings, fused_adam=opt, dL_ddepth_map=r.dL_ddepth_map,
                                dL_dalpha=r.dL_dalpha)
    curve = " ".join(f"{v:.5f}" for v in losses[::4])
    print(f"normal loss (every 4th step): {curve}; valid pixels {counts[0]:.0f} -> {counts[-1]:.0f} of {w * h}")
    assert counts[0] > 0.5 * w * h and counts[-1] > 0.5 * w * h, counts       # the plane fills the image and stays
    assert losses[-1] < losses[0], curve
