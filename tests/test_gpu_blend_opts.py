"""Every combination of the blend options through the one entry each direction has (cugs_rasterize_forward_opts /
cugs_rasterize_backward_opts, reached through rasterizer.rasterize_forward / rasterize_backward): an option changes what
it says it changes and nothing else.  The scene is small: 400 Gaussians in the middle of a 100 x 70 image (7 x 5 tiles,
neither side a multiple of the tile, the border tiles empty)."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, W, H = 400, 100, 70
BG = [0.2, 0.1, 0.3]


@pytest.fixture(scope="module")
def view(pkg, dev):
    arrays = pkg.scene.make_gaussians(N, W, H, sh_degree=1, seed=11, mu_s=-4.0, cluster=(1.0, 0.12))
    out = pkg.render(pkg.scene.to_model(arrays, dev), pkg.scene.make_camera(W, H),
                     pkg.RenderSettings(background=BG, active_sh_degree=1))
    lens = out.tile_ranges[:, 1] - out.tile_ranges[:, 0]
    assert out.tile_ranges.shape[0] == 35 and bool((lens == 0).any()) and int((lens > 0).sum()) > 1
    assert int(out.n_contrib.max()) > 1                            # splats overlap: the blend has something to order
    return out, pkg.rasterizer.tile_order_of(out.tile_ranges, W, H)


def _close(a, b, what):
    """The bound of test_forward_blend_clears_the_backward_accumulator (atomics reorder the sums), word by word: each
    column of the rows against its own largest entry."""
    for k in range(a.shape[1]):
        err, bound = float((a[:, k] - b[:, k]).abs().max()), 1e-5 * max(float(a[:, k].abs().max()), 1e-30)
        assert err <= bound, (what, k, err, bound)


def test_forward_options_change_nothing_but_their_own_output(pkg, dev, view):
    out, order = view
    args = (out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges, out.gaussian_indices, W, H, BG)
    off = pkg.rasterize_forward(*args, packed=out.packed)
    assert off.depth_map is None
    depth_maps = {}
    for zero, ordered, depth in itertools.product((False, True), repeat=3):
        dirty = torch.full((N * 16 + 4,), 7.0, device=dev)
        f = pkg.rasterize_forward(*args, packed=out.packed, zero_buf=dirty[:N * 16] if zero else None,
                                  tile_order=order if ordered else None, depths=out.depths if depth else None)
        what = (zero, ordered, depth)
        assert torch.equal(f.color, off.color) and torch.equal(f.final_T, off.final_T), what
        assert torch.equal(f.n_contrib, off.n_contrib), what
        assert bool((dirty[:N * 16] == (0.0 if zero else 7.0)).all()) and bool((dirty[N * 16:] == 7.0).all()), what
        assert (f.depth_map is not None) == depth, what
        if depth:
            depth_maps[what] = f.depth_map
    first = depth_maps[(False, False, True)]
    assert bool((first > 0).any())
    for what, d in depth_maps.items():                             # with and without tile_order (and zero_buf): one map
        assert torch.equal(d, first), what


def test_backward_options_change_nothing_but_their_own_words(pkg, dev, view):
    out, order = view
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(W, H, seed=12)).to(dev)
    gen = torch.Generator(device="cpu").manual_seed(13)
    dD = (torch.randn((H, W), generator=gen) / (W * H)).to(dev)
    dA = (torch.randn((H, W), generator=gen) / (W * H)).to(dev)
    args = (g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges, out.gaussian_indices,
            out.final_T, out.n_contrib, W, H, BG, N)

    def run(zeroed, ordered, depth, want_abs, unpack):
        kw = dict(depths=out.depths, dL_ddepth_map=dD, dL_dalpha=dA) if depth else {}
        return pkg.rasterize_backward(*args, packed=out.packed, unpack=unpack,
                                      zeroed_accum=torch.zeros((N, 16), device=dev) if zeroed else None,
                                      tile_order=order if ordered else None, want_abs_grad=want_abs, **kw)

    # the references: each option alone (and the two that write words together), nothing else on
    ref = {(depth, want_abs): run(False, False, depth, want_abs, False).grad_accum
           for depth in (False, True) for want_abs in (False, True)}
    assert bool(ref[(False, False)][:, :9].any()) and bool(ref[(True, False)][:, 9].any())
    assert bool(ref[(False, True)][:, 10:12].any())
    a, b, c = out.cov_2d_inv[:, 0], out.cov_2d_inv[:, 1], out.cov_2d_inv[:, 2]         # Sigma'^-1, as in the records
    for zeroed, ordered, depth, want_abs, unpack in itertools.product((False, True), repeat=5):
        what = dict(zeroed=zeroed, ordered=ordered, depth=depth, want_abs=want_abs, unpack=unpack)
        r = run(zeroed, ordered, depth, want_abs, unpack)
        rows = r.grad_accum
        assert rows.shape == (N, 16)
        words = 10 if depth else 9
        _close(ref[(depth, False)][:, :words], rows[:, :words], what)
        if want_abs:
            _close(ref[(depth, True)][:, 10:12], rows[:, 10:12], what)
        else:
            assert not rows[:, 10:12].any(), what
        assert (r.dL_ddepths is not None) == (unpack and depth), what
        assert (r.dL_dmeans_2d_abs is not None) == want_abs, what
        if not unpack:
            assert r.dL_drgb is None and r.dL_dopacity_act is None and r.dL_dmeans_2d is None, what
            assert r.dL_dcov_2d_inv is None, what
            if want_abs:                                           # the rows' own words: a view, not a copy
                assert r.dL_dmeans_2d_abs.data_ptr() == rows[:, 10:12].data_ptr(), what
                assert torch.equal(r.dL_dmeans_2d_abs, rows[:, 10:12]), what
            continue
        # unpacked: the rows, through the per-Gaussian map of include/cugs_hip.h (each product and sum rounded once)
        assert torch.equal(r.dL_drgb, rows[:, 0:3]) and torch.equal(r.dL_dopacity_act, rows[:, 3]), what
        m1x, m1y = rows[:, 4], rows[:, 5]
        assert torch.equal(r.dL_dmeans_2d, torch.stack([a * m1x + b * m1y, b * m1x + c * m1y], dim=1)), what
        assert torch.equal(r.dL_dcov_2d_inv, torch.stack([-0.5 * rows[:, 6], -rows[:, 7], -0.5 * rows[:, 8]], dim=1)), what
        if depth:
            assert torch.equal(r.dL_ddepths, rows[:, 9]), what
        if want_abs:
            assert torch.equal(r.dL_dmeans_2d_abs, rows[:, 10:12]), what
