"""The staged cull inside the blend kernels (csrc/cugs_blend_cull.h): word 6 of the LDS record holds the
cull's limit for the tile, made once when the record is staged, and every wave tests it against the select-free minimum
over its live rectangle.  A record the cull drops is lost for good, and one it keeps changes nothing - so every output
must still be the oracle's: image, final_T, n_contrib, depth map and scores bit for bit (of the scores the maximum and
the pixel count; the weight sum is a sum of float atomics and is held to tests/test_gpu_scores.py's bound), gradients
within the project's bar, on the forward and backward blend of {packed, unpacked} x {colour, depth + alpha maps,
AbsGrad} and k_blend_scores.

The scene is built in 2-D (the blend's own inputs; lists are made by hand, so a tile lists splats that are nowhere near
it): 40 x 24 pixels - partial tiles, quads outside the image - and 1500 splats, every one in each tile's list with
probability 0.45: about 675 entries per list, three record batches with a partial last one.  Among them
  * opacities below 1/255 (tau = -1), exactly 1/255, a few ulp above, and ordinary ones;
  * thin splats whose mean lies 200 .. 600 px outside the image and whose long axis points into it: q is small on the
    image while B ~ a X^2 is ~1e5, so the 4e-6 B term of the slack is several tenths;
  * thin diagonal ellipses whose alpha = 1/255 contour passes a quad's corner pixel, just inside and just outside;
  * conics with a = 0 or c = 0 (never culled: the edge parabolas need a, c > 0);
  * eight opaque splats in tile 0's list alone: its waves close, in both directions, with batches left."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from absgrad_ref import abs_and_signed, per_pixel_channels
from scores_ref import scores_of, weight_table
from util import check_blend_bounds, load_parity, max_err_over_max, np_, oracle_blend_terms

pytestmark = pytest.mark.gpu

W, H, N = 40, 24, 1500
BG = (0.3, 0.1, 0.6)
AMIN = np.float32(1.0 / 255.0)
N_FAR, N_DIAG, N_FLAT, N_OPAQUE = 60, 64, 8, 8
GRAD_TOL = 1e-4     # the project's bar: error relative to each tensor's scale


def _conic(s1, s2, th):
    """Inverse of R diag(s1^2, s2^2) R^T: (a, b, c)."""
    cs, sn = np.cos(th), np.sin(th)
    cxx, cyy = s1 * s1 * cs * cs + s2 * s2 * sn * sn, s1 * s1 * sn * sn + s2 * s2 * cs * cs
    cxy = (s1 * s1 - s2 * s2) * sn * cs
    det = cxx * cyy - cxy * cxy
    return cyy / det, -cxy / det, cxx / det


@functools.lru_cache(maxsize=None)
def _scene():
    """The 2-D scene, the oracle's forward and every reference table - computed once, shared, never modified."""
    import __graft_entry__ as ge
    orc = ge.load_oracle()
    rng = np.random.default_rng(20261020)
    mean = np.stack([rng.uniform(-6.0, W + 6.0, N), rng.uniform(-6.0, H + 6.0, N)], axis=1)
    a, b, c = _conic(rng.uniform(0.8, 3.0, N), rng.uniform(0.8, 3.0, N), rng.uniform(0.0, np.pi, N))
    opa = rng.uniform(0.005, 0.06, N).astype(np.float32)
    kind = rng.integers(0, 10, N)
    opa = np.where(kind == 0, rng.uniform(0.0005, float(AMIN) * 0.999, N).astype(np.float32), opa)      # below 1/255
    opa = np.where(kind == 1, AMIN, opa)                                                                 # exactly
    opa = np.where(kind == 2, AMIN + rng.integers(1, 16, N).astype(np.float32) * np.spacing(AMIN), opa)   # a few ulp above
    opa = opa.astype(np.float32)
    assert np.any(opa < AMIN) and np.any(opa == AMIN)
    i = 0
    # far thin splats: long axis through a point of the image
    k = N_FAR
    th, dist = rng.uniform(0.0, 2.0 * np.pi, k), rng.uniform(200.0, 600.0, k)
    tx, ty = rng.uniform(0.0, W, k), rng.uniform(0.0, H, k)
    mean[i:i + k] = np.stack([tx + dist * np.cos(th), ty + dist * np.sin(th)], axis=1)
    a[i:i + k], b[i:i + k], c[i:i + k] = _conic(dist / 1.2, rng.uniform(1.5, 4.0, k), th)
    opa[i:i + k] = rng.uniform(0.05, 0.3, k)
    far = slice(i, i + k)
    i += k
    # thin diagonal ellipses: the alpha = 1/255 contour passes a corner pixel of a quad
    k = N_DIAG
    th = np.where(rng.integers(0, 2, k) == 0, np.pi / 4, 3 * np.pi / 4) + rng.uniform(-0.1, 0.1, k)
    thin = rng.uniform(0.5, 0.9, k)
    o = rng.uniform(0.3, 0.9, k)
    corner_x = 8.0 * rng.integers(0, 5, k) + np.where(rng.integers(0, 2, k) == 0, 0.5, 7.5)
    corner_y = 8.0 * rng.integers(0, 3, k) + np.where(rng.integers(0, 2, k) == 0, 0.5, 7.5)
    off = thin * np.sqrt(2.0 * np.log(255.0 * o)) * rng.uniform(0.7, 1.3, k) * np.where(rng.integers(0, 2, k) == 0, 1, -1)
    along = rng.uniform(-4.0, 4.0, k)
    mean[i:i + k] = np.stack([corner_x - off * np.sin(th) + along * np.cos(th),
                              corner_y + off * np.cos(th) + along * np.sin(th)], axis=1)
    a[i:i + k], b[i:i + k], c[i:i + k] = _conic(rng.uniform(8.0, 14.0, k), thin, th)
    opa[i:i + k] = o
    i += k
    # a = 0 (a band of rows) and c = 0 (a band of columns)
    k = N_FLAT
    band = rng.uniform(0.05, 0.5, k)
    a[i:i + k] = np.where(np.arange(k) % 2 == 0, 0.0, band)
    c[i:i + k] = np.where(np.arange(k) % 2 == 0, band, 0.0)
    b[i:i + k] = 0.0
    mean[i:i + k] = np.stack([rng.uniform(0.0, W, k), rng.uniform(0.0, H, k)], axis=1)
    opa[i:i + k] = rng.uniform(0.02, 0.05, k)
    flat = slice(i, i + k)
    i += k
    # the opaque ones sit in the MIDDLE of the depth order (index = depth order), in tile 0's list only
    opaque = np.arange(N // 2, N // 2 + N_OPAQUE)
    mean[opaque] = (8.0, 8.0)
    a[opaque], b[opaque], c[opaque] = 1.0 / 900.0, 0.0, 1.0 / 900.0
    opa[opaque] = 0.95
    member = rng.random((6, N)) < 0.45
    member[:, flat] = True
    member[:, opaque] = False
    member[0, opaque] = True
    values = np.concatenate([np.flatnonzero(m) for m in member]).astype(np.int32)     # ascending index = depth order
    ends = np.cumsum(member.sum(axis=1))
    tile_ranges = np.stack([ends - member.sum(axis=1), ends], axis=1).astype(np.int32)
    ref = dict(tile_ranges=tile_ranges, values=values, means_2d=mean.astype(np.float32),
               cov_2d_inv=np.stack([a, b, c], axis=1).astype(np.float32),
               rgb=rng.uniform(0.0, 1.0, (N, 3)).astype(np.float32), opacities_act=opa.reshape(N, 1).astype(np.float32),
               depths=np.linspace(2.0, 10.0, N).astype(np.float32))
    ref = {k_: np.ascontiguousarray(v) for k_, v in ref.items()}
    geo = (ref["tile_ranges"], ref["values"], ref["means_2d"], ref["cov_2d_inv"])
    ref.update(orc.rasterize_forward(W, H, BG, *geo, ref["rgb"], ref["opacities_act"]))
    zrgb = np.ascontiguousarray(np.repeat(ref["depths"].reshape(-1, 1), 3, axis=1))
    depth_map = orc.rasterize_forward(W, H, (0.0, 0.0, 0.0), *geo, zrgb, ref["opacities_act"])["color"][..., 0]
    r = np.random.default_rng(7)
    dC = (r.standard_normal((H, W, 3)) / (W * H)).astype(np.float32)
    dD = (r.standard_normal((H, W)) * 0.05 / math.sqrt(W * H)).astype(np.float32)
    dA = (r.standard_normal((H, W)) * 0.3 / math.sqrt(W * H)).astype(np.float32)
    want_c, mags_c = oracle_blend_terms(orc, ref, dC, BG, N, W, H)
    want_d, mags_d = oracle_blend_terms(orc, ref, dC, BG, N, W, H, dD=dD, dA=dA, depth_route=True)
    want_abs, _ = abs_and_signed(per_pixel_channels(orc, ref, N, W, H, g=dC, bg=BG)["colour"])
    table = weight_table(orc, ref, N, W, H)
    s = dict(ref=ref, depth_map=np.ascontiguousarray(depth_map), dC=dC, dD=dD, dA=dA, want_c=want_c, mags_c=mags_c,
             want_d=want_d, mags_d=mags_d, want_abs=want_abs, table=table, scores=scores_of(table), far=far, flat=flat,
             opaque=opaque)
    for v in (dC, dD, dA, table, want_abs, s["depth_map"], *ref.values()):
        v.setflags(write=False)
    return s


def test_scene_is_what_it_claims():
    """CPU only, from the oracle's outputs: list lengths, open and closed tiles, and that the special splats matter."""
    s = _scene()
    ref = s["ref"]
    length = ref["tile_ranges"][:, 1] - ref["tile_ranges"][:, 0]
    assert np.all(length > 2 * 256) and np.all(length < 3 * 256) and np.all(length % 64 != 0)      # three batches, a partial last
    nc, fT = ref["n_contrib"], ref["final_T"]
    assert np.all(fT[:16, :16] < AMIN) and np.all(nc[:16, :16] > 0)            # tile 0 closes ...
    assert np.all(fT[:, 16:] >= AMIN)                                         # ... and no pixel of the other tiles does
    cnt = s["scores"]["count"]
    mean, cov = ref["means_2d"].astype(np.float64), ref["cov_2d_inv"].astype(np.float64)
    # far splats reach pixels, from means hundreds of pixels away, with a slack term 4e-6 B of 0.05 and more
    X = np.maximum(np.abs(mean[s["far"], 0]), np.abs(mean[s["far"], 0] - W))
    Y = np.maximum(np.abs(mean[s["far"], 1]), np.abs(mean[s["far"], 1] - H))
    B = cov[s["far"], 0] * X * X + 2.0 * np.abs(cov[s["far"], 1]) * X * Y + cov[s["far"], 2] * Y * Y
    assert np.count_nonzero(cnt[s["far"]]) > 20 and np.count_nonzero(4e-6 * B > 0.05) > 20
    assert np.all(np.hypot(mean[s["far"], 0] - W / 2, mean[s["far"], 1] - H / 2) > 150.0)
    assert np.all(cnt[s["flat"]] > 0)                                          # a = 0 / c = 0 bands contribute
    assert not cnt[ref["opacities_act"].reshape(-1) < AMIN].any()              # below 1/255: never
    above = (ref["opacities_act"].reshape(-1) > AMIN) & (ref["opacities_act"].reshape(-1) < AMIN * 1.0001)
    assert above.sum() > 50 and not cnt[above].any()                           # a few ulp above: tau ~ 1e-6, no pixel centre that close


def _t(a, dev):
    return torch.tensor(np.asarray(a)).to(dev)            # a copy: the shared arrays are read-only


def _bits(a):
    return np.ascontiguousarray(np_(a) if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def inputs(pkg, dev):
    """The scene on the device, with the packed records made by cugs_pack_projected (tau = ln(255 o) included)."""
    ref = _scene()["ref"]
    d = {k: _t(ref[k], dev) for k in ("means_2d", "cov_2d_inv", "rgb", "opacities_act", "tile_ranges", "values", "depths",
                                      "final_T", "n_contrib")}
    packed = torch.empty((N, 12), dtype=torch.float32, device=dev)
    P = lambda x: C.c_void_p(x.data_ptr())
    rc = pkg.rasterizer.lib.cugs_pack_projected(C.c_int64(N), P(d["means_2d"]), P(d["cov_2d_inv"]), P(d["rgb"]),
                                                P(d["opacities_act"]), P(packed),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    d["packed"] = packed
    d["order"] = pkg.rasterizer.tile_order_of(d["tile_ranges"], W, H)
    return d


@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
def test_forward_is_the_oracles_bit_for_bit(pkg, inputs, packed, depth):
    s, d = _scene(), inputs
    ref = s["ref"]
    for order in (None, d["order"]):
        f = pkg.rasterize_forward(d["means_2d"], d["cov_2d_inv"], d["rgb"], d["opacities_act"], d["tile_ranges"],
                                  d["values"], W, H, BG, packed=d["packed"] if packed else None, tile_order=order,
                                  depths=d["depths"] if depth else None)
        assert np.array_equal(_bits(f.color), _bits(ref["color"]))
        assert np.array_equal(_bits(f.final_T), _bits(ref["final_T"]))
        assert np.array_equal(np_(f.n_contrib), ref["n_contrib"])
        if depth:
            assert np.array_equal(_bits(f.depth_map), _bits(s["depth_map"]))


@pytest.mark.parametrize("route", ["colour", "depth", "absgrad"])
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
def test_backward_gradients_within_the_bar(pkg, dev, inputs, packed, route):
    s, d = _scene(), inputs
    ref = s["ref"]
    par = load_parity()
    depth = route == "depth"
    extra = dict(depths=d["depths"], dL_ddepth_map=_t(s["dD"], dev), dL_dalpha=_t(s["dA"], dev)) if depth else {}
    rb = pkg.rasterize_backward(_t(s["dC"], dev), d["means_2d"], d["cov_2d_inv"], d["rgb"], d["opacities_act"],
                                d["tile_ranges"], d["values"], d["final_T"], d["n_contrib"], W, H, BG, N,
                                packed=d["packed"] if packed else None, want_abs_grad=(route == "absgrad"), **extra)
    want, mags = (s["want_d"], s["mags_d"]) if depth else (s["want_c"], s["mags_c"])
    got = {k: np_(getattr(rb, k)) for k in par.ACCUMULATORS}
    if depth:
        got["dL_ddepths"] = np_(rb.dL_ddepths)
    label = f"{'packed' if packed else 'unpacked'}/{route}"
    check_blend_bounds(got, want, mags, ref["cov_2d_inv"], np.bincount(ref["values"], minlength=N), label)
    for k in par.ACCUMULATORS:
        assert par.over_scale(got[k], want[k]) <= GRAD_TOL, (label, k)
    if route == "absgrad":
        err = max_err_over_max(np_(rb.dL_dmeans_2d_abs), s["want_abs"])
        print(f"absgrad {label}: max err / max = {err:.3e}")
        assert err <= GRAD_TOL, (label, err)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
def test_scores_count_and_maximum_bit_for_bit(pkg, dev, inputs, packed):
    s, d = _scene(), inputs
    want = s["scores"]
    scores = pkg.ContributionScores(N, dev)
    if packed:
        pkg.blend_scores(scores, None, None, None, d["tile_ranges"], d["values"], W, H, packed=d["packed"],
                         tile_order=d["order"])
    else:
        pkg.blend_scores(scores, d["means_2d"], d["cov_2d_inv"], d["opacities_act"], d["tile_ranges"], d["values"], W, H)
    assert np.array_equal(np_(scores.pixel_count), want["count"])
    assert np.array_equal(np_(scores.weight_max).view(np.uint32), want["max"].view(np.uint32))
    # the sum: k non-negative fp32 terms in any order, first-order bound (k - 1) 2^-24 of the sum, doubled
    bound = want["count"].astype(np.float64) * 2.0 ** -23 * want["sum"]
    assert np.all(np.abs(np_(scores.weight_sum).astype(np.float64) - want["sum"]) <= bound)
