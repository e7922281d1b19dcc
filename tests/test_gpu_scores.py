"""Per-Gaussian contribution scores: cugs_blend_scores on every route against the reference of
tests/scores_ref.py (the unchanged oracle's weights, one-hot colours), accumulation over launches and views, the empty
cases, and the pruning the scores exist for."""
import numpy as np
import pytest
import torch

from scores_ref import SCENES, combine, scene
from util import np_

pytestmark = pytest.mark.gpu

ROUTES = ("packed_ordered", "packed", "soa", "render")
TINY = float(np.nextafter(np.float32(0.0), np.float32(1.0)))      # the smallest positive float32


def _t(a, dev):
    return torch.tensor(np.asarray(a)).to(dev)                     # a copy: the shared arrays are read-only


def _settings(pkg):
    return pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=0)


def _score(pkg, dev, s, route, scores=None, model=None):
    """One launch of view `s` into `scores` (a fresh table when None) on `route`."""
    n, w, h, ref = s["n"], s["w"], s["h"], s["ref"]
    scores = scores if scores is not None else pkg.ContributionScores(n, dev)
    if route == "soa":
        return pkg.blend_scores(scores, _t(ref["means_2d"], dev), _t(ref["cov_2d_inv"], dev),
                                _t(ref["opacities_act"], dev), _t(ref["tile_ranges"], dev), _t(ref["values"], dev), w, h)
    model = model if model is not None else pkg.scene.to_model(s["arrays"], dev)
    out = pkg.render(model, s["cam"], _settings(pkg), for_backward=False)
    if route == "render":
        return pkg.accumulate_contribution_scores(scores, out, s["cam"])
    order = pkg.rasterizer.tile_order_of(out.tile_ranges, w, h) if route == "packed_ordered" else None
    assert (order is not None) == (route == "packed_ordered")
    return pkg.blend_scores(scores, None, None, None, out.tile_ranges, out.gaussian_indices, w, h, packed=out.packed,
                            tile_order=order)


def _check(scores, want, label):
    """Maximum and count bit for bit; the sum within k * 2^-23 * ref per Gaussian, k its pixel count: the first-order
    bound (k - 1) * 2^-24 * ref for k non-negative fp32 terms summed in any order, doubled."""
    got_sum, got_max, got_cnt = np_(scores.weight_sum), np_(scores.weight_max), np_(scores.pixel_count)
    assert got_sum.dtype == np.float32 and got_max.dtype == np.float32 and got_cnt.dtype == np.int64
    bound = want["count"].astype(np.float64) * 2.0 ** -23 * want["sum"]
    err = np.abs(got_sum.astype(np.float64) - want["sum"])
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"scores {label}: {int((want['count'] > 0).sum())} of {len(got_sum)} contribute, max count "
          f"{int(want['count'].max())}, worst sum error / bound = {worst:.3f}")
    assert np.array_equal(got_cnt, want["count"]), label
    assert np.array_equal(got_max.view(np.uint32), want["max"].view(np.uint32)), label
    assert np.all(err <= bound), (label, worst)
    assert not np_(scores.table)[:, 3].any(), label                 # the padding word is never written


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("key", list(SCENES))
def test_scores_match_the_reference_on_every_route(pkg, dev, key, route):
    s = scene(key)
    scores = _score(pkg, dev, s, route)
    assert scores.num_views == 1 and scores.table.shape == (s["n"], 4)
    _check(scores, s["want"], f"{key} {route}")
    assert scores.weight_sum.data_ptr() == scores.table.data_ptr()  # views of the table, no copies
    assert scores.weight_max.data_ptr() == scores.table.data_ptr() + 4


@pytest.mark.parametrize("route", ["packed_ordered", "soa"])
@pytest.mark.parametrize("key", list(SCENES))
def test_a_second_launch_accumulates(pkg, dev, key, route):
    s = scene(key)
    scores = _score(pkg, dev, s, route)
    _score(pkg, dev, s, route, scores)
    assert scores.num_views == 2
    _check(scores, combine(s["want"], s["want"]), f"{key} {route} twice")     # sum and count double, the max stays
    scores.reset()
    assert scores.num_views == 0 and not scores.table.any()


@pytest.mark.parametrize("key", list(SCENES))
def test_two_views_combine_and_contribution_scores_gives_the_same(pkg, dev, key):
    s0, s1 = scene(key, 0), scene(key, 1)
    want = combine(s0["want"], s1["want"])
    assert not np.array_equal(s0["want"]["count"], s1["want"]["count"])       # the views differ
    model = pkg.scene.to_model(s0["arrays"], dev)
    scores = _score(pkg, dev, s0, "render", model=model)
    _score(pkg, dev, s1, "render", scores, model=model)
    _check(scores, want, f"{key} two views")
    offline = pkg.contribution_scores(model, [s0["cam"], s1["cam"]], _settings(pkg))
    assert offline.num_views == 2
    _check(offline, want, f"{key} contribution_scores")
    assert torch.equal(offline.table[:, 1:], scores.table[:, 1:])


def test_empty_cases_leave_the_table_alone(pkg, dev):
    s = scene("40x24")
    n, w, h = s["n"], s["w"], s["h"]
    settings = _settings(pkg)
    f = dict(dtype=torch.float32, device=dev)
    # n == 0
    empty = pkg.GaussianModel(torch.zeros((0, 3), **f), torch.zeros((0, 3, 1), **f), torch.zeros((0, 1), **f),
                              torch.zeros((0, 4), **f), torch.zeros((0, 3), **f))
    sc = pkg.contribution_scores(empty, [s["cam"]], settings)
    assert sc.table.shape == (0, 4) and sc.num_views == 1 and sc.pixel_count.shape == (0,)
    pkg.accumulate_contribution_scores(sc, pkg.render(empty, s["cam"], settings), s["cam"])
    assert sc.num_views == 2
    # a model wholly behind the camera: no pairs, no index list
    arrays = {k: v.copy() for k, v in s["arrays"].items()}
    arrays["positions"][:, 2] = -5.0
    model = pkg.scene.to_model(arrays, dev)
    sentinel = 0x3F800000
    sc = pkg.ContributionScores(n, dev)
    sc.table.fill_(sentinel)
    out = pkg.render(model, s["cam"], settings, for_backward=False)
    assert out.total_pairs == 0 and out.gaussian_indices.numel() == 0
    pkg.accumulate_contribution_scores(sc, out, s["cam"])
    pkg.blend_scores(sc, None, None, None, out.tile_ranges, out.gaussian_indices, w, h, packed=out.packed)
    pkg.blend_scores(sc, out.means_2d, out.cov_2d_inv, out.opacities_act, out.tile_ranges, out.gaussian_indices, w, h)
    assert bool((sc.table == sentinel).all())
    assert not pkg.contribution_scores(model, [s["cam"]], settings).table.any()
    # a zero-sized image
    none = torch.empty((0, 2), dtype=torch.int32, device=dev)
    for zw, zh in ((0, h), (w, 0), (0, 0)):
        pkg.blend_scores(sc, None, None, None, none, out.gaussian_indices, zw, zh, packed=out.packed)
    torch.cuda.synchronize()
    assert bool((sc.table == sentinel).all())


def _stepped_optimizer(pkg, dev, s, model):
    """A FusedAdam on `model` whose moments are those of one real step; the parameters are put back afterwards, so that
    the model is still the scene the reference was made from."""
    settings = _settings(pkg)
    original = {k: getattr(model, k).clone() for k in ("positions", "sh_coeffs", "opacities", "rotations", "scales")}
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
def test_pruning_what_never_contributes_changes_no_pixel(pkg, dev, key):
    s0, s1 = scene(key, 0), scene(key, 1)
    n = s0["n"]
    settings = _settings(pkg)
    never = combine(s0["want"], s1["want"])["count"] == 0
    assert 0 < int(never.sum()) < n
    model = pkg.scene.to_model(s0["arrays"], dev)
    opt, original = _stepped_optimizer(pkg, dev, s0, model)
    moments = [t.clone() for t in (*opt.m_, *opt.v_)]
    views = (s0["cam"], s1["cam"])
    shot = lambda: [(o.color.clone(), o.final_T.clone(), o.n_contrib.clone())
                    for o in (pkg.render(model, c, settings, for_backward=False) for c in views)]
    before = shot()
    scores = pkg.contribution_scores(model, views, settings)
    removed = pkg.prune_by_scores(model, scores, min_max_weight=TINY, optimizer=opt)
    assert removed == int(never.sum()) and model.num_gaussians() == n - removed
    for a, b in zip(before, shot()):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    keep = torch.from_numpy(~never).to(dev)
    for k, v in original.items():
        assert torch.equal(getattr(model, k), v[keep]), k
    for got, old in zip((*opt.m_, *opt.v_), moments):
        assert got.shape[0] == n - removed and torch.equal(got, old[keep])
    assert all(g is None for g in opt.grads_)
    # nothing left to remove: the same call again is a no-op
    again = pkg.contribution_scores(model, views, settings)
    assert pkg.prune_by_scores(model, again, min_max_weight=TINY, optimizer=opt) == 0


def test_pruning_by_fraction_keeps_the_top_half_of_the_reference_sum(pkg, dev):
    s = scene("40x24")
    n, want = s["n"], s["want"]
    keep_n = n // 2
    order = np.argsort(-want["sum"], kind="stable")
    cut_hi, cut_lo = want["sum"][order[keep_n - 1]], want["sum"][order[keep_n]]
    bound = want["count"].astype(np.float64) * 2.0 ** -23 * want["sum"]
    # no tie at the cut, by more than the two sums' error bounds: the selection is determined
    assert cut_hi - cut_lo > bound[order[keep_n - 1]] + bound[order[keep_n]] and cut_lo > 0.0
    kept = np.sort(order[:keep_n])
    model = pkg.scene.to_model(s["arrays"], dev)
    original = model.positions.clone()
    scores = pkg.contribution_scores(model, [s["cam"]], _settings(pkg))
    assert pkg.prune_by_scores(model, scores, keep_fraction=0.5) == n - keep_n
    assert torch.equal(model.positions, original[torch.from_numpy(kept).to(dev)])
    # both criteria: the union of the two prunes
    model = pkg.scene.to_model(s["arrays"], dev)
    thr = 0.05
    both = np.zeros(n, bool)
    both[kept] = True
    both &= want["max"] >= np.float32(thr)
    assert 0 < int(both.sum()) < keep_n
    assert pkg.prune_by_scores(model, scores, min_max_weight=thr, keep_fraction=0.5) == n - int(both.sum())
    assert torch.equal(model.positions, original[torch.from_numpy(both).to(dev)])


def test_prune_gaussians_rejects_a_mask_that_does_not_fit(pkg, dev):
    s = scene("40x24")
    n = s["n"]
    model = pkg.scene.to_model(s["arrays"], dev)
    with pytest.raises(RuntimeError, match="prune_mask"):
        pkg.prune_gaussians(model, torch.zeros(n + 1, dtype=torch.bool, device=dev))
    with pytest.raises(RuntimeError, match="prune_mask"):
        pkg.prune_gaussians(model, torch.zeros(n, dtype=torch.bool))              # on the host
    with pytest.raises(RuntimeError, match="prune_mask"):
        pkg.prune_gaussians(model, torch.zeros(n, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError):
        pkg.prune_by_scores(model, pkg.ContributionScores(n, dev))                # no criterion
    assert model.num_gaussians() == n
    assert pkg.prune_gaussians(model, torch.zeros(n, dtype=torch.bool, device=dev)) == 0
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    mask[::3] = True
    first = model.positions[1].clone()
    assert pkg.prune_gaussians(model, mask) == int(mask.sum()) and model.num_gaussians() == n - int(mask.sum())
    assert torch.equal(model.positions[0], first)
