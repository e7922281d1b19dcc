"""The pixel-map lift's reference (tests/lift_ref.py) pinned against the unchanged oracle before the GPU is asked: the
adjoint identity with the oracle's forward blend, and the margins that make the label and densification tests of
tests/test_gpu_lift.py determined (CPU only)."""
import numpy as np
import pytest

import lift_ref
from scores_ref import SCENES, scene


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("key", list(SCENES))
def test_lift_is_the_adjoint_of_the_oracles_forward(pkg, orc, key, view):
    """sum_g S[g,c] x[g,c] = sum_p M[p,c] image_x[p,c], image_x the oracle's forward of rgb := x with background 0.
    Both sides are sum_p sum_g w[p,g] M[p,c] x[g,c]; the left one is formed in fp64 from the weight table, the right
    one from an image whose pixel the oracle accumulated in fp32 - k_p fused multiply-adds for a pixel with k_p
    contributors, so that pixel is within k_p 2^-23 sum_g w |x| (the bound of lift_ref, per pixel) of its exact value."""
    s = scene(key, view)
    n, w, h, ref, table = s["n"], s["w"], s["h"], s["ref"], s["table"]
    x = np.random.default_rng(11 + view).standard_normal((n, 3)).astype(np.float32)
    m = lift_ref.float_map(key, view, 3)
    img = orc.rasterize_forward(w, h, (0.0, 0.0, 0.0), ref["tile_ranges"], ref["values"], ref["means_2d"],
                                ref["cov_2d_inv"], x, ref["opacities_act"])["color"]
    want = lift_ref.lifted(key, view, 3)
    left = (want["sum"] * x.astype(np.float64)).sum(axis=0)
    m64 = m.astype(np.float64).reshape(h * w, 3)
    right = (m64 * img.astype(np.float64).reshape(h * w, 3)).sum(axis=0)
    k_p = (table > 0.0).sum(axis=1).astype(np.float64)
    pixel_bound = k_p[:, None] * 2.0 ** -23 * (table.astype(np.float64) @ np.abs(x.astype(np.float64)))
    bound = (np.abs(m64) * pixel_bound).sum(axis=0)
    print(f"{key} view {view}: adjoint identity, |left - right| / bound = {np.abs(left - right) / bound}")
    assert np.all(bound > 0.0) and np.all(np.abs(left - right) <= bound)
    # a reference with one Gaussian's row shifted by one breaks the identity: the check can fail
    wrong = (np.roll(want["sum"], 1, axis=0) * x.astype(np.float64)).sum(axis=0)
    assert np.all(np.abs(wrong - right) > bound)


@pytest.mark.parametrize("key", list(SCENES))
def test_a_map_of_ones_gives_the_weight_sum_and_the_bound_of_the_scores(pkg, orc, key):
    s = scene(key)
    want = lift_ref.wanted(s["table"], np.ones((s["h"], s["w"]), np.float32))
    assert np.array_equal(want["count"], s["want"]["count"])
    assert np.allclose(want["sum"][:, 0], s["want"]["sum"], rtol=1e-15, atol=0.0)
    assert np.allclose(want["bound"][:, 0], s["want"]["count"] * 2.0 ** -23 * s["want"]["sum"], rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("name", list(lift_ref.LABEL_IMAGES))
@pytest.mark.parametrize("key", list(SCENES))
def test_label_margins(pkg, orc, key, name):
    """Every Gaussian with a vote leads its runner-up by more than twice the bound (the two votes' bounds summed), so
    the argmax the GPU test demands is determined: per view for all three images, over two views for stripes and grid."""
    num = lift_ref.LABEL_IMAGES[name]
    lab = lift_ref.label_image(key, name)
    assert sorted(set(np.unique(lab)) - {-1}) == list(range(num))
    assert (name == "checker") == bool((lab < 0).any())
    cases = [(0,), (1,)] + ([(0, 1)] if name != "checker" else [])
    for views in cases:
        v = lift_ref.votes(key, name, views)
        has = v["label"] >= 0
        print(f"{key} {name} views {views}: {int(has.sum())} Gaussians vote, smallest margin / bound = "
              f"{float(v['margin'][has].min()):.2f}, labels used {sorted(set(v['label'][has]))}")
        assert has.sum() > 50 and len(set(v["label"][has])) == num
        assert np.all(v["margin"][has] > 2.0)
        assert np.array_equal(has, v["voters"] > 0)
        if name != "checker":                                # every pixel carries a label: voters = contributors
            assert np.array_equal(v["voters"], v["count"])


@pytest.mark.parametrize("key", list(SCENES))
def test_error_scores_leave_room_for_a_threshold(pkg, orc, key):
    e = lift_ref.errors(key)
    pos = e["max"][e["max"] > 0.0]
    print(f"{key}: reference error scores {pos.min():.3g} .. {pos.max():.3g}, threshold {e['threshold']:.6g}, "
          f"{int((e['max'] >= e['threshold']).sum())} of {len(e['max'])} above it")
    assert not np.array_equal(e["per_view"][0]["sum"], e["per_view"][1]["sum"])
    above = e["max"] >= e["threshold"]
    assert 10 < int(above.sum()) < int((e["max"] > 0.0).sum()) - 10
    # the threshold lies more than twice the bound from every reference score
    assert np.all(np.abs(e["max"] - e["threshold"]) > 2.0 * e["max_bound"])
