"""The AbsGrad reference of tests/absgrad_ref.py pinned against the oracle's own full-frame backward (CPU only)."""
import numpy as np

from absgrad_ref import abs_and_signed, per_pixel_channels
from util import oracle_forward


def test_per_pixel_reference_sums_to_the_oracles_gradient_and_shows_cancellation(pkg, orc):
    w, h, n = 24, 20, 150
    bg = (0.2, 0.4, 0.6)
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=0, seed=1, mu_s=-1.5)
    cam = pkg.scene.make_camera(w, h)
    ref = oracle_forward(orc, arrays, cam, bg=bg, degree=0)
    g = pkg.scene.make_dl_dcolor(w, h)
    rng = np.random.default_rng(5)
    dD = (rng.standard_normal((h, w)) * 0.05 / (w * h)).astype(np.float32)
    dA = (rng.standard_normal((h, w)) * 0.3 / (w * h)).astype(np.float32)
    ch = per_pixel_channels(orc, ref, n, w, h, g=g, bg=bg, dD=dD, dA=dA, depths=ref["depths"])
    geo = (ref["tile_ranges"], ref["values"], ref["means_2d"], ref["cov_2d_inv"])
    tail = (ref["final_T"], ref["n_contrib"], n)
    red = lambda m: np.stack([m, 0 * m, 0 * m], axis=2).astype(np.float32)
    zr = np.zeros((n, 3), np.float32)
    zr[:, 0] = ref["depths"]
    full = {
        "colour": orc.rasterize_backward(w, h, bg, *geo, ref["rgb"], ref["opacities_act"], g, *tail),
        "depth": orc.rasterize_backward(w, h, (0.0, 0.0, 0.0), *geo, zr, ref["opacities_act"], red(dD), *tail),
        "alpha": orc.rasterize_backward(w, h, (-1.0, 0.0, 0.0), *geo, np.zeros((n, 3), np.float32),
                                        ref["opacities_act"], red(dA), *tail),
    }
    for name, table in ch.items():
        a, s = abs_and_signed(table)
        want = full[name]["dL_dmeans_2d"].astype(np.float64)
        scale = float(np.abs(want).max())
        assert scale > 0.0
        # each side is an fp32 rounding of an fp64 sum of the same terms
        assert float(np.abs(s - want).max()) <= 1e-6 * scale, name
        assert np.all(a >= np.abs(s)), name
        assert np.all(a >= 0.0)
    a, s = abs_and_signed(ch["colour"])
    assert np.any(a > 2.0 * np.abs(s)), "the scene shows no cancellation: a kernel without the fabs would pass"
    a3, s3 = abs_and_signed(ch["colour"], ch["depth"], ch["alpha"])
    assert np.all(a3 >= np.abs(s3)) and np.any(a3 > 2.0 * np.abs(s3))
    # Gaussians in no list get nothing
    listed = np.zeros(n, bool)
    listed[ref["values"]] = True
    assert not a3[~listed].any()
