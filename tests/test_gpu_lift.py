"""Pixel maps lifted onto Gaussians: cugs_blend_lift on every route against the reference of
tests/lift_ref.py (the unchanged oracle's weights times the map, in fp64, with a derived tolerance), label votes, NaN
containment, accumulation, the empty cases, and the two applications: error-based densification and selection by a
voted label."""
import numpy as np
import pytest
import torch

import lift_ref
from scores_ref import SCENES, scene
from util import np_

pytestmark = pytest.mark.gpu

ROUTES = ("packed_ordered", "packed", "soa", "render")
PARAMS = ("positions", "sh_coeffs", "opacities", "rotations", "scales")


def _t(a, dev):
    return torch.tensor(np.asarray(a)).to(dev)                     # a copy: the shared arrays are read-only


def _settings(pkg):
    return pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=0)


def _lift(pkg, dev, s, route, channels, lifted=None, model=None, **maps):
    """One launch of view `s` into `lifted` (a fresh table when None) on `route`; maps=..., or labels=... with
    label_base=..."""
    n, w, h, ref = s["n"], s["w"], s["h"], s["ref"]
    lifted = lifted if lifted is not None else pkg.LiftedMaps(n, dev, channels)
    if route == "soa":
        return pkg.blend_lift(lifted, _t(ref["means_2d"], dev), _t(ref["cov_2d_inv"], dev),
                              _t(ref["opacities_act"], dev), _t(ref["tile_ranges"], dev), _t(ref["values"], dev), w, h,
                              **maps)
    model = model if model is not None else pkg.scene.to_model(s["arrays"], dev)
    out = pkg.render(model, s["cam"], _settings(pkg), for_backward=False)
    if route == "render":
        return pkg.lift_pixel_maps(lifted, out, s["cam"], **maps)
    order = pkg.rasterizer.tile_order_of(out.tile_ranges, w, h) if route == "packed_ordered" else None
    assert (order is not None) == (route == "packed_ordered")
    return pkg.blend_lift(lifted, None, None, None, out.tile_ranges, out.gaussian_indices, w, h, packed=out.packed,
                          tile_order=order, **maps)


def _padding_is_zero(lifted):
    pad = np_(lifted.table)[:, lifted.channels:]
    assert not pad.view(np.uint32).any()                            # words C..3: never written, bit-zero


# ---- 1. float maps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("key", list(SCENES))
def test_float_maps_match_the_reference_on_every_route(pkg, dev, key, channels, route):
    s = scene(key)
    m = _t(lift_ref.float_map(key, 0, channels), dev)
    if channels == 1 and route in ("packed", "render"):
        m = m[:, :, 0]                                              # [H,W] is accepted for one channel
    lifted = _lift(pkg, dev, s, route, channels, maps=m)
    assert lifted.num_views == 1 and lifted.table.shape == (s["n"], 4) and lifted.table.dtype == torch.float32
    assert lifted.sums.shape == (s["n"], channels)
    assert lifted.sums.data_ptr() == lifted.table.data_ptr() and lifted.sums.stride() == (4, 1)   # a view, no copy
    lift_ref.check(np_(lifted.sums), lift_ref.lifted(key, 0, channels), f"{key} C={channels} {route}")
    _padding_is_zero(lifted)


@pytest.mark.parametrize("channels", [2, 4])
def test_the_map_needs_no_alignment(pkg, dev, channels):
    """A map that starts 4 bytes past a 16-byte boundary (and a label image likewise): same sums."""
    key = "33x17"
    s = scene(key)
    m = lift_ref.float_map(key, 0, channels)
    buf = torch.zeros(m.size + 1, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    shifted = buf[1:].view(*m.shape)
    shifted.copy_(_t(m, dev))
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    lifted = _lift(pkg, dev, s, "packed_ordered", channels, maps=shifted)
    lift_ref.check(np_(lifted.sums), lift_ref.lifted(key, 0, channels), f"{key} C={channels} map at +4 bytes")
    lab_np = lift_ref.label_image(key, "grid")
    ibuf = torch.zeros(lab_np.size + 1, dtype=torch.int32, device=dev)
    lab = ibuf[1:].view(*lab_np.shape)
    lab.copy_(_t(lab_np, dev))
    assert lab.data_ptr() % 16 == 4
    lifted = _lift(pkg, dev, s, "packed_ordered", channels, labels=lab, label_base=1)
    hot = lift_ref.one_hot(lab_np, 6)[..., 1:1 + channels]
    lift_ref.check(np_(lifted.sums), lift_ref.wanted(s["table"], hot), f"{key} C={channels} labels at +4 bytes")


# ---- 2. a map of ones is the score kernel's weight sum ----------------------------------------------------------------
@pytest.mark.parametrize("key", list(SCENES))
def test_a_map_of_ones_agrees_with_the_contribution_scores(pkg, dev, key):
    s = scene(key)
    n, w, h = s["n"], s["w"], s["h"]
    model = pkg.scene.to_model(s["arrays"], dev)
    out = pkg.render(model, s["cam"], _settings(pkg), for_backward=False)
    ones = torch.ones((h, w), dtype=torch.float32, device=dev)
    lifted = pkg.blend_lift(pkg.LiftedMaps(n, dev, 1), None, None, None, out.tile_ranges, out.gaussian_indices, w, h,
                            maps=ones, packed=out.packed)
    scores = pkg.blend_scores(pkg.ContributionScores(n, dev), None, None, None, out.tile_ranges, out.gaussian_indices,
                              w, h, packed=out.packed)
    want = lift_ref.wanted(s["table"], np.ones((h, w), np.float32))
    got, other = np_(lifted.sums)[:, 0], np_(scores.weight_sum)
    lift_ref.check(got[:, None], want, f"{key} ones")
    diff = np.abs(got.astype(np.float64) - other.astype(np.float64))
    print(f"{key}: worst |lift - weight_sum| / (2 bound) = {float((diff / np.maximum(2 * want['bound'][:, 0], 1e-300)).max()):.3f}")
    assert np.all(diff <= 2.0 * want["bound"][:, 0])                # each within its bound of the same exact sum
    idle = want["count"] == 0
    assert idle.any() and not got[idle].view(np.uint32).any()
    assert np.array_equal(np_(scores.pixel_count) == 0, idle)


# ---- 3. labels --------------------------------------------------------------------------------------------------------
# the checker image is used per view only: summed over two views one Gaussian's lead is within the bound on 40x24
VOTE_CASES = [(name, views) for name in lift_ref.LABEL_IMAGES for views in ((0,), (1,), (0, 1))
              if not (name == "checker" and len(views) > 1)]


@pytest.mark.parametrize("name,views", VOTE_CASES)
@pytest.mark.parametrize("key", list(SCENES))
def test_vote_labels_gives_the_reference_votes_and_argmax(pkg, dev, key, name, views):
    num = lift_ref.LABEL_IMAGES[name]
    want = lift_ref.votes(key, name, views)
    model = pkg.scene.to_model(scene(key)["arrays"], dev)
    lab = _t(lift_ref.label_image(key, name), dev)
    labels, votes = pkg.vote_labels(model, [scene(key, v)["cam"] for v in views], [lab] * len(views), num,
                                    _settings(pkg))
    assert labels.dtype == torch.int64 and labels.shape == (scene(key)["n"],)
    assert votes.dtype == torch.float32 and votes.shape == (scene(key)["n"], num)
    lift_ref.check(np_(votes), want, f"{key} {name} views {views}")
    got = np_(labels)
    assert np.array_equal(got, want["label"])                       # every Gaussian, none left out
    assert np.array_equal(got == -1, want["voters"] == 0)
    if name != "checker":
        assert np.array_equal(got == -1, want["count"] == 0)        # -1 exactly where the pixel count is 0


@pytest.mark.parametrize("route", ["packed_ordered", "soa"])
@pytest.mark.parametrize("key", list(SCENES))
def test_label_windows(pkg, dev, key, route):
    """The stage function in labels mode: a window in the middle of the checker image's labels (its -1 pixels and the
    labels on either side of the window contribute nothing), and a window that holds none of them."""
    s = scene(key)
    lab_np = lift_ref.label_image(key, "checker")
    lab = _t(lab_np, dev)
    for base, channels in ((2, 3), (5, 2), (-1, 4), (6, 1)):
        # label_base -1: channel 0 is "label == -1", a value like any other to the kernel
        hot = (lab_np[..., None] == base + np.arange(channels)).astype(np.float64)
        lifted = _lift(pkg, dev, s, route, channels, labels=lab, label_base=base)
        lift_ref.check(np_(lifted.sums), lift_ref.wanted(s["table"], hot), f"{key} {route} window {base}+{channels}")
        _padding_is_zero(lifted)
    sentinel = 1.5
    for base in (7, 100, -9, 2 ** 31 - 4):
        lifted = pkg.LiftedMaps(s["n"], dev, 4)
        lifted.table.fill_(sentinel)
        _lift(pkg, dev, s, route, 4, lifted, labels=lab, label_base=base)
        assert bool((lifted.table == sentinel).all()), base        # untouched, bit for bit


# ---- 4. NaN -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["packed_ordered", "soa"])
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("key", list(SCENES))
def test_a_nan_reaches_only_the_gaussians_that_blend_onto_its_pixel(pkg, dev, key, channels, route):
    s = scene(key)
    w, table = s["w"], s["table"]
    p = int((table > 0.0).sum(axis=1).argmax())                    # the pixel with most contributors
    hit = table[p] > 0.0
    assert 1 <= int(hit.sum()) < int((s["want"]["count"] > 0).sum())
    ch = channels // 2                                             # one channel of that pixel only
    m = lift_ref.float_map(key, 0, channels).copy()
    m[p // w, p % w, ch] = np.nan
    want = lift_ref.wanted(table, m)                                # the NaN counts as 0 there
    got = np_(_lift(pkg, dev, s, route, channels, maps=_t(m, dev)).sums)
    assert np.array_equal(np.isnan(got[:, ch]), hit)                # exactly those Gaussians read NaN
    others = [c for c in range(channels) if c != ch]
    assert not np.isnan(got[:, others]).any()
    finite = np.where(np.isnan(got), want["sum"].astype(np.float32), got)
    lift_ref.check(finite, want, f"{key} C={channels} {route} NaN at pixel {p}")
    # an Inf at a pixel outside every Gaussian's reach would reach nobody; here: +Inf on the same pixel
    m[p // w, p % w, ch] = np.inf
    got = np_(_lift(pkg, dev, s, route, channels, maps=_t(m, dev)).sums)
    assert np.array_equal(np.isinf(got[:, ch]), hit) and not np.isnan(got).any()


# ---- 5. accumulation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["packed_ordered", "soa"])
@pytest.mark.parametrize("key", list(SCENES))
def test_a_second_launch_doubles_the_sums(pkg, dev, key, route):
    s = scene(key)
    m = _t(lift_ref.float_map(key, 0, 3), dev)
    lifted = _lift(pkg, dev, s, route, 3, maps=m)
    _lift(pkg, dev, s, route, 3, lifted, maps=m)
    assert lifted.num_views == 2
    one = lift_ref.lifted(key, 0, 3)
    lift_ref.check(np_(lifted.sums), lift_ref.combine(one, one), f"{key} {route} twice")
    _padding_is_zero(lifted)
    lifted.reset()
    assert lifted.num_views == 0 and not lifted.table.any()


@pytest.mark.parametrize("key", list(SCENES))
def test_two_views_add_and_lift_maps_gives_the_same(pkg, dev, key):
    s0, s1 = scene(key, 0), scene(key, 1)
    want = lift_ref.combine(lift_ref.lifted(key, 0, 4), lift_ref.lifted(key, 1, 4))
    m0, m1 = _t(lift_ref.float_map(key, 0, 4), dev), _t(lift_ref.float_map(key, 1, 4), dev)
    model = pkg.scene.to_model(s0["arrays"], dev)
    lifted = _lift(pkg, dev, s0, "render", 4, model=model, maps=m0)
    _lift(pkg, dev, s1, "render", 4, lifted, model=model, maps=m1)
    lift_ref.check(np_(lifted.sums), want, f"{key} two views")
    offline = pkg.lift_maps(model, [s0["cam"], s1["cam"]], [m0, m1], _settings(pkg))
    assert offline.num_views == 2 and offline.channels == 4
    lift_ref.check(np_(offline.sums), want, f"{key} lift_maps")
    single = pkg.lift_maps(model, [s0["cam"]], [m0[:, :, 0].contiguous()], _settings(pkg))
    assert single.channels == 1
    lift_ref.check(np_(single.sums), lift_ref.wanted(s0["table"], lift_ref.float_map(key, 0, 4)[:, :, 0]),
                   f"{key} lift_maps [H,W]")


# ---- 6. empty cases ---------------------------------------------------------------------------------------------------
def test_empty_cases_leave_the_table_alone(pkg, dev):
    s = scene("40x24")
    n, w, h = s["n"], s["w"], s["h"]
    settings = _settings(pkg)
    f = dict(dtype=torch.float32, device=dev)
    m = _t(lift_ref.float_map("40x24", 0, 3), dev)
    lab = _t(lift_ref.label_image("40x24", "stripes"), dev)
    # n == 0
    empty = pkg.GaussianModel(torch.zeros((0, 3), **f), torch.zeros((0, 3, 1), **f), torch.zeros((0, 1), **f),
                              torch.zeros((0, 4), **f), torch.zeros((0, 3), **f))
    lifted = pkg.lift_maps(empty, [s["cam"]], [m], settings)
    assert lifted.table.shape == (0, 4) and lifted.sums.shape == (0, 3) and lifted.num_views == 1
    pkg.lift_pixel_maps(lifted, pkg.render(empty, s["cam"], settings), s["cam"], maps=m)
    assert lifted.num_views == 2
    labels, votes = pkg.vote_labels(empty, [s["cam"]], [lab], 6, settings)
    assert labels.shape == (0,) and votes.shape == (0, 6)
    assert pkg.error_scores(empty, [s["cam"]], [m[:, :, 0].contiguous()], settings).shape == (0,)
    # a model wholly behind the camera: no pairs, no index list
    arrays = {k: v.copy() for k, v in s["arrays"].items()}
    arrays["positions"][:, 2] = -5.0
    model = pkg.scene.to_model(arrays, dev)
    sentinel = 1.5
    lifted = pkg.LiftedMaps(n, dev, 3)
    lifted.table.fill_(sentinel)
    out = pkg.render(model, s["cam"], settings, for_backward=False)
    assert out.total_pairs == 0 and out.gaussian_indices.numel() == 0
    pkg.lift_pixel_maps(lifted, out, s["cam"], maps=m)
    pkg.blend_lift(lifted, None, None, None, out.tile_ranges, out.gaussian_indices, w, h, maps=m, packed=out.packed)
    pkg.blend_lift(lifted, out.means_2d, out.cov_2d_inv, out.opacities_act, out.tile_ranges, out.gaussian_indices, w, h,
                   maps=m)
    assert bool((lifted.table == sentinel).all())
    assert not pkg.lift_maps(model, [s["cam"]], [m], settings).table.any()
    labels, votes = pkg.vote_labels(model, [s["cam"]], [lab], 4, settings)
    assert bool((labels == -1).all()) and not votes.any()
    # a zero-sized image
    none = torch.empty((0, 2), dtype=torch.int32, device=dev)
    for zw, zh in ((0, h), (w, 0), (0, 0)):
        pkg.blend_lift(lifted, None, None, None, none, out.gaussian_indices, zw, zh,
                       maps=torch.empty((zh, zw, 3), **f), packed=out.packed)
        pkg.blend_lift(lifted, None, None, None, none, out.gaussian_indices, zw, zh,
                       labels=torch.empty((zh, zw), dtype=torch.int32, device=dev), packed=out.packed)
    torch.cuda.synchronize()
    assert bool((lifted.table == sentinel).all())


def test_the_host_rejects_maps_that_do_not_fit(pkg, dev):
    s = scene("40x24")
    n, w, h = s["n"], s["w"], s["h"]
    model = pkg.scene.to_model(s["arrays"], dev)
    out = pkg.render(model, s["cam"], _settings(pkg), for_backward=False)
    m = _t(lift_ref.float_map("40x24", 0, 3), dev)
    lab = _t(lift_ref.label_image("40x24", "stripes"), dev)
    lifted = pkg.LiftedMaps(n, dev, 3)
    for bad in (dict(), dict(maps=m, labels=lab), dict(maps=m[:, :, :2]), dict(maps=m.double()), dict(maps=m.cpu()),
                dict(labels=lab.long()), dict(labels=lab[:, :-1])):
        with pytest.raises(RuntimeError):
            pkg.lift_pixel_maps(lifted, out, s["cam"], **bad)
    with pytest.raises(RuntimeError):
        pkg.lift_pixel_maps(pkg.LiftedMaps(n + 1, dev, 3), out, s["cam"], maps=m)
    with pytest.raises(RuntimeError):
        pkg.LiftedMaps(n, dev, 5)
    assert lifted.num_views == 0 and not lifted.table.any()


# ---- 7. error scores and densification ----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(SCENES))
def test_error_scores_and_the_densification_they_drive(pkg, dev, key):
    s0, s1 = scene(key, 0), scene(key, 1)
    n = s0["n"]
    e = lift_ref.errors(key)
    settings = _settings(pkg)
    model = pkg.scene.to_model(s0["arrays"], dev)
    cams = [s0["cam"], s1["cam"]]
    maps = [_t(lift_ref.error_map(key, v), dev) for v in (0, 1)]
    got = pkg.error_scores(model, cams, maps, settings)                         # reduce="max"
    assert got.dtype == torch.float32 and got.shape == (n,)
    want_max = dict(sum=e["max"][:, None], bound=e["max_bound"][:, None],
                    count=np.maximum(e["per_view"][0]["count"], e["per_view"][1]["count"]))
    lift_ref.check(np_(got)[:, None], want_max, f"{key} error_scores max")
    total = pkg.error_scores(model, cams, maps, settings, reduce="sum")
    lift_ref.check(np_(total)[:, None], lift_ref.combine(*e["per_view"]), f"{key} error_scores sum")
    with pytest.raises(RuntimeError):
        pkg.error_scores(model, cams, maps, settings, reduce="mean")
    # the training-loop form: per view, render, lift the error image, hand the scores to the controller
    cfg = pkg.DensificationConfig()
    cfg.grad_threshold = e["threshold"]
    ctl = pkg.DensificationController(cfg, 5.0)
    radii = []
    for cam, m in zip(cams, maps):
        out = pkg.render(model, cam, settings, for_backward=False)
        view = pkg.lift_pixel_maps(pkg.LiftedMaps(n, dev, 1), out, cam, maps=m)
        ctl.accumulate_error_scores(view.sums[:, 0], out.radii)
        radii.append(out.radii.to(torch.float32))
    assert not ctl.grad_count_.any()                                            # left at zero: accum / max(count, 1) = the maximum
    lift_ref.check(np_(ctl.grad_accum_)[:, None], want_max, f"{key} controller accumulator")
    assert torch.equal(ctl.max_radii_2d_, torch.maximum(radii[0], radii[1]).clamp_min(0.0))
    flags, avg = ctl._classify(model, 100)
    grows = np_((flags & 3) != 0)                                               # clone or split
    assert np.array_equal(grows, e["max"] >= e["threshold"])
    assert 0 < int(grows.sum()) < n


# ---- 8. selection by a voted label -------------------------------------------------------------------------------------
def _stepped_optimizer(pkg, dev, s, model):
    """A FusedAdam on `model` whose moments are those of one real step; the parameters are put back afterwards."""
    settings = _settings(pkg)
    original = {k: getattr(model, k).clone() for k in PARAMS}
    opt = pkg.FusedAdam(model)
    out = pkg.render(model, s["cam"], settings)
    grads = pkg.render_backward(_t(pkg.scene.make_dl_dcolor(s["w"], s["h"]), dev), out, model, s["cam"], settings)
    opt.apply_gradients(grads)
    opt.step()
    assert all(bool(m.any()) for m in opt.m_) and all(bool(v.any()) for v in opt.v_)
    for k, v in original.items():
        getattr(model, k).copy_(v)
    return opt, original


@pytest.mark.parametrize("key", list(SCENES))
def test_select_gaussians_extracts_one_voted_label(pkg, dev, key):
    s = scene(key)
    n = s["n"]
    want = lift_ref.votes(key, "stripes", (0, 1))
    model = pkg.scene.to_model(s["arrays"], dev)
    opt, original = _stepped_optimizer(pkg, dev, s, model)
    moments = [t.clone() for t in (*opt.m_, *opt.v_)]
    lab = _t(lift_ref.label_image(key, "stripes"), dev)
    labels, _ = pkg.vote_labels(model, [scene(key, 0)["cam"], scene(key, 1)["cam"]], [lab, lab], 4, _settings(pkg))
    keep = labels == 2
    ref_keep = want["label"] == 2
    assert 0 < int(ref_keep.sum()) < n
    assert pkg.select_gaussians(model, keep, opt) == int(ref_keep.sum()) == model.num_gaussians()
    sel = torch.from_numpy(ref_keep).to(dev)
    for k, v in original.items():
        assert torch.equal(getattr(model, k), v[sel]), k             # bit for bit and in order
    for got, old in zip((*opt.m_, *opt.v_), moments):
        assert got.shape[0] == int(ref_keep.sum()) and torch.equal(got, old[sel])
    # everything kept: nothing changes
    assert pkg.select_gaussians(model, torch.ones(model.num_gaussians(), dtype=torch.bool, device=dev)) == int(ref_keep.sum())
