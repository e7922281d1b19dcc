"""GPU parity tests proper: the HIP path, called through the C ABI (libcugs_hip.so via the host
mirror), against the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): bit-exact for radii, tiles_touched, sort keys / order, tile
ranges (and, by construction of the deterministic blend math, n_contrib); <= 1e-4 relative on
rendered RGB and on every gradient.  Tolerances are written at each assert.

Equality is with the CPU restatement of the reference's CUDA source (oracle/cugs_oracle.c), not
with bits from an nvcc build.
"""
import os

import numpy as np
import pytest
import torch

from util import (blend_stage_check, check_blend_bounds, load_parity, max_err_over_max, max_rel_err, np_, oracle_backward,
                  oracle_blend_terms, oracle_forward)

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4      # north_star: "within 1e-4 relative on rendered RGB"
GRAD_TOL = 1e-4     # north_star: "... and all gradients"


def _scene(pkg, n, w, h, deg, seed=1234, mu_s=-4.6, view=0):
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=deg, seed=seed, mu_s=mu_s)
    cam = pkg.scene.make_camera(w, h, view=view)
    return arrays, cam


def _assert_projection_equal(out, ref):
    # integer outputs: bit-exact
    assert np.array_equal(np_(out.radii), ref["radii"])
    assert np.array_equal(np_(out.tiles_touched), ref["tiles_touched"])
    # the float outputs of the projection are computed with the same operation order and no
    # contraction, so they are bit-exact too (stronger than the 1e-6 the survey asked for)
    for name in ("means_2d", "depths", "cov_2d_inv", "opacities_act"):
        got, want = np_(getattr(out, name)), ref[name]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert max_rel_err(np_(out.rgb), ref["rgb"]) <= 1e-6


@pytest.mark.parametrize("deg,active", [(0, 0), (1, 1), (2, 2), (3, 3), (3, 0), (3, 2)])
def test_projection_parity(pkg, orc, dev, deg, active):
    w, h, n = 640, 360, 20000
    arrays, cam = _scene(pkg, n, w, h, deg, seed=11 + deg)
    arrays["positions"][:50, 2] = -5.0            # behind the camera (test_projection.cpp:109-125)
    arrays["positions"][50:60, 2] = 0.15          # inside the near plane
    model = pkg.scene.to_model(arrays, dev)
    out = pkg.project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs,
                                cam, active)
    ref = oracle_forward(orc, arrays, cam, degree=active)
    _assert_projection_equal(out, ref)
    assert int((ref["radii"][:60] == 0).all())


@pytest.mark.parametrize("scale_mod,view", [(2.0, 0), (0.5, 3), (1.0, 5)])
def test_projection_scale_modifier_and_pose(pkg, orc, dev, scale_mod, view):
    w, h, n = 320, 240, 5000
    arrays, cam = _scene(pkg, n, w, h, 3, seed=5, view=view)
    model = pkg.scene.to_model(arrays, dev)
    out = pkg.project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs,
                                cam, 3, scale_mod)
    ref = oracle_forward(orc, arrays, cam, scale_mod=scale_mod)
    _assert_projection_equal(out, ref)


@pytest.mark.parametrize("n,w,h,mu_s", [(20000, 640, 360, -4.6), (3000, 250, 130, -3.0), (1, 64, 48, -2.0),
                                         (70000, 1920, 1080, -4.6),
                                         (3000, 4112, 4112, -2.0),    # 66049 tiles: tile ids wider than 16 bits, 3 passes
                                         (3000, 4096, 64, -2.0),      # 256 tile columns: the widest column-ordered emission
                                         (3000, 4112, 160, -2.0),     # 257 columns: 16-bit tile ids, pairs emitted in depth order
                                         (3000, 160, 4112, -2.0),     # 257 rows: same
                                         (400, 1920, 1080, 0.5)])     # splats covering thousands of tiles each
def test_sort_parity_bit_exact(pkg, orc, dev, n, w, h, mu_s):
    arrays, cam = _scene(pkg, n, w, h, 0, seed=n, mu_s=mu_s)
    ref = oracle_forward(orc, arrays, cam, degree=0)
    t = lambda k: torch.from_numpy(ref[k]).to(dev)
    srt = pkg.sort_gaussians(t("means_2d"), t("depths"), t("radii"), t("tiles_touched"), w, h)
    assert srt.total_pairs == ref["total_pairs"]
    assert np.array_equal(np_(srt.gaussian_keys_sorted).view(np.uint64), ref["keys"])       # tile ids + depth bits
    assert np.array_equal(np_(srt.gaussian_values_sorted), ref["values"])                    # sort order
    assert np.array_equal(np_(srt.tile_ranges), ref["tile_ranges"])                          # per-tile spans


@pytest.mark.parametrize("n,expect", [(230_000, "16"), (300_000, "64"), (600_000, "64")])
def test_render_sort_routes_by_size(pkg, orc, dev, n, expect):
    """render()'s sort at the sizes where its radix passes change shape (sort_workspace.h: scan_free / sup_block): a pair level of
    ~470 workgroups (super-blocks of 16), of ~610 and ~1230 (super-blocks of 64); each with the packed rectangles riding
    through the depth passes (n <= 1 M, 120 x 68 tiles).  (Pair levels beyond 4096 workgroups - the classic three kernels
    per pass - are the dense full-size view and config 4.)  Pairs, order, ranges and the image against the
    oracle; the predicted (keyed) route is the one render() takes from its second frame on."""
    w, h = 1920, 1080
    arrays, cam = _scene(pkg, n, w, h, 0, seed=n, mu_s=-4.6)
    ref = oracle_forward(orc, arrays, cam, degree=0)
    blocks = (ref["total_pairs"] + 4095) // 4096
    assert {"16": blocks <= 512, "64": 512 < blocks <= 4096}[expect], blocks
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=0)
    for frame in range(3):                      # blocking route, then twice the keyed / predicted one
        out = pkg.render(model, cam, settings, for_backward=False)
        assert out.total_pairs == ref["total_pairs"], frame
        assert np.array_equal(np_(out.gaussian_indices), ref["values"]), frame
        assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"]), frame
        assert np.array_equal(np_(out.n_contrib), ref["n_contrib"]), frame
        assert np.array_equal(np_(out.color).view(np.uint32), ref["color"].view(np.uint32)), frame


@pytest.mark.parametrize("mu_s,dense", [(-4.6, False), (-3.2, True)])
def test_sort_both_pair_routes(pkg, orc, dev, mu_s, dense):
    """The pair-level sort has two routes to the same permutation: pairs emitted in depth order + two radix passes
    by tile id (sparse views), or pairs emitted in tile-column order + one pass by tile row (>= 13 pairs per
    Gaussian, sort_workspace.h column_path_pays).  The same 1080p scene at two splat scales takes one each - exact and
    predicted-capacity entry points - and both must give the oracle's keys, order and tile ranges."""
    n, w, h = 50000, 1920, 1080
    arrays, cam = _scene(pkg, n, w, h, 0, seed=17, mu_s=mu_s)
    ref = oracle_forward(orc, arrays, cam, degree=0)
    assert (ref["total_pairs"] >= 13 * n) == dense
    t = lambda k: torch.from_numpy(ref[k]).to(dev)
    args = (t("means_2d"), t("depths"), t("radii"), t("tiles_touched"), w, h)
    R = pkg.rasterizer
    srt = pkg.sort_gaussians(*args)
    R._last_pairs[R._skey(torch.device(dev))] = ref["total_pairs"]
    R._held_capacity.pop(R._skey(torch.device(dev)), None)
    try:
        pend = R.sort_gaussians_predicted(*args, want_keys=True)
        assert isinstance(pend, R.PendingSort)
        srt2, valid = pend.finish()
    finally:
        R._last_pairs.pop(R._skey(torch.device(dev)), None)
    assert valid
    for out in (srt, srt2):
        assert out.total_pairs == ref["total_pairs"]
        assert np.array_equal(np_(out.gaussian_keys_sorted).view(np.uint64), ref["keys"])
        assert np.array_equal(np_(out.gaussian_values_sorted), ref["values"])
        assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"])


_RANK_MODES_CHILD = r"""
import ctypes as C, json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
from util import oracle_forward, np_
pkg, orc = ge.load_package(), ge.load_oracle()
from cugs_amd._lib import lib
fn = lib.cugsdbg_sort_rank_mode
fn.restype, fn.argtypes = C.c_int, [C.c_int]
dev = torch.device("cuda:0")
n, w, h = 60000, 1280, 720
arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=0, seed=8, mu_s=-4.0)
cam = pkg.scene.make_camera(w, h)
ref = oracle_forward(orc, arrays, cam, degree=0)
t = lambda k: torch.from_numpy(ref[k]).to(dev)
pkg.sort_gaussians(t("means_2d"), t("depths"), t("radii"), t("tiles_touched"), w, h)      # runs the probe
res = {"chosen": fn(-2), "modes": {}}
for mode in (0, 1):
    assert fn(mode) == mode
    srt = pkg.sort_gaussians(t("means_2d"), t("depths"), t("radii"), t("tiles_touched"), w, h)
    res["modes"][mode] = bool(np.array_equal(np_(srt.gaussian_keys_sorted).view(np.uint64), ref["keys"])
                              and np.array_equal(np_(srt.gaussian_values_sorted), ref["values"])
                              and np.array_equal(np_(srt.tile_ranges), ref["tile_ranges"]))
print(json.dumps(res))
"""


def test_sort_ranking_modes_agree_in_the_development_build(pkg, dev):
    """The shipped library ranks with wave ballots only (no mode variable, no environment, no cugsdbg_* export).
    The development build also carries the ranking by one LDS atomic-with-return per item, which relies on an
    undocumented ordering of same-address LDS lanes and is selected there by an on-device probe: a child process
    that loads that build must get the oracle's order in both modes."""
    import ctypes as C
    import json
    import subprocess
    import sys
    assert not hasattr(C.CDLL(pkg.LIB_PATH), "cugsdbg_sort_rank_mode")
    dev_lib = os.path.join(os.path.dirname(pkg.LIB_PATH), "libcugs_hip_dev.so")
    if not os.path.exists(dev_lib):
        pytest.skip("development library not built")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _RANK_MODES_CHILD, root], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, CUGS_HIP_LIBRARY=dev_lib))
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert out["chosen"] in (0, 1) and out["modes"] == {"0": True, "1": True}


def test_sort_predicted_capacity_path(pkg, orc, dev):
    """cugs_sort_pairs_predicted: same result as the exact two-call path when the capacity suffices (also with
    keys and with spare capacity), a detectable miss when it does not, and a clean empty case."""
    R = pkg.rasterizer
    n, w, h = 30000, 640, 360
    arrays, cam = _scene(pkg, n, w, h, 0, seed=5, mu_s=-4.2)
    ref = oracle_forward(orc, arrays, cam, degree=0)
    t = lambda k: torch.from_numpy(ref[k]).to(dev)
    args = (t("means_2d"), t("depths"), t("radii"), t("tiles_touched"), w, h)
    margin = R.PREDICT_MARGIN
    try:
        for last, mg, expect_valid in ((ref["total_pairs"], (1.0, 0), True),          # exact capacity
                                       (ref["total_pairs"], (1.5, 4096), True),       # spare capacity
                                       (ref["total_pairs"] - 1, (1.0, 0), False),     # one short: must be detected
                                       (7, (1.0, 0), False)):
            R._last_pairs[R._skey(torch.device(dev))] = last
            R._held_capacity.pop(R._skey(torch.device(dev)), None)            # the capacity of THIS estimate, not one held over
            R.PREDICT_MARGIN = mg
            pend = R.sort_gaussians_predicted(*args, want_keys=True)
            assert isinstance(pend, R.PendingSort)
            srt, valid = pend.finish()
            assert valid == expect_valid and srt.total_pairs == ref["total_pairs"]
            assert np.array_equal(np_(srt.gaussian_keys_sorted).view(np.uint64), ref["keys"])
            assert np.array_equal(np_(srt.gaussian_values_sorted), ref["values"])
            assert np.array_equal(np_(srt.tile_ranges), ref["tile_ranges"])
            assert R._last_pairs[R._skey(torch.device(dev))] >= ref["total_pairs"]          # running maximum, slow decay
        # nothing visible: the predicted path must leave every tile {0,0} and report zero pairs
        R._last_pairs[R._skey(torch.device(dev))] = 1000
        R._held_capacity.pop(R._skey(torch.device(dev)), None)
        z = torch.zeros(50, dtype=torch.int32, device=dev)
        pend = R.sort_gaussians_predicted(torch.zeros((50, 2), device=dev), torch.ones(50, device=dev), z, z, w, h)
        srt, valid = pend.finish()
        assert valid and srt.total_pairs == 0 and not bool(srt.tile_ranges.any()) and srt.gaussian_values_sorted.numel() == 0
    finally:
        R.PREDICT_MARGIN = margin
        R._last_pairs.pop(R._skey(torch.device(dev)), None)


def test_render_recovers_from_a_wrong_pair_prediction(pkg, orc, dev):
    """render() sorts on the pair count predicted from earlier frames; a scene with ten times more pairs than the
    previous one (a new view, a densification) must come out identical through the exact-path fallback, and a
    much smaller one through the spare capacity."""
    R = pkg.rasterizer
    small = _forward_both(pkg, orc, dev, 1500, 320, 240, 1, -4.0, (0.0, 0.0, 0.0), seed=5)
    assert R._last_pairs[R._skey(torch.device(dev))] < 60000
    R._last_pairs[R._skey(torch.device(dev))] = 100                       # force a gross under-prediction for the next frame
    R._held_capacity.pop(R._skey(torch.device(dev)), None)
    for n, mu_s in ((40000, -3.6), (1500, -4.0)):                # far above the prediction, then far below it
        arrays, cam, model, settings, out, ref = _forward_both(pkg, orc, dev, n, 320, 240, 1, mu_s, (0.1, 0.2, 0.3), seed=n)
        assert out.total_pairs == ref["total_pairs"]
        assert np.array_equal(np_(out.gaussian_indices), ref["values"])
        assert np.array_equal(np_(out.color).view(np.uint32), ref["color"].view(np.uint32))
    assert small[4].total_pairs == small[5]["total_pairs"]


@pytest.mark.parametrize("n,w,h,mu_s,ties", [
    (4000, 128, 96, -2.5, True),        # every depth identical (stability across workgroups and waves) + quirk Q12 zero pairs
    (300, 640, 360, 0.5, False),        # screen-filling splats: rectangles over 16 tiles tall (several owned rows per wave)
    (30000, 1600, 1063, -4.2, False),   # config 4's image: 100 x 67 tiles
    (5000, 2032, 2032, -3.0, False),    # 127 x 127 tiles: packable rectangles, but over the direct route's tile limit
    (3000, 3840, 2160, -3.5, False),    # 4K: neither packable nor direct
    (20000, 2032, 1280, -3.2, False),   # 127 x 80 = 10 160 tiles: 159 chunks of 64 tiles (three scans per wave), 16 block columns
    (20000, 1280, 2032, -3.2, False),   # 80 x 127: 16 block rows, 10 block columns
    (1_200_000, 640, 360, -5.8, False), # over 1 M Gaussians: the rectangles do not ride through the depth passes,
                                        # k_bin_count gathers and packs them (and writes them out for the scatter)
])
def test_render_sort_by_direct_binning(pkg, orc, dev, n, w, h, mu_s, ties):
    """render()'s second and later frames on a stream sort through cugs_sort_pairs_predicted_keyed, which - on images of
    up to ~10 000 tiles - bins every pair straight into its tile's list (k_bin_count / k_bin_scan / k_bin_scatter)
    instead of carrying the pairs through two radix passes.  Same permutation, bit for bit: the oracle's order
    (ascending index among equal depths), the Q12 zero pairs at the head of tile 0, {0,0} for untouched tiles; and a
    frame whose prediction was too small (the first after a ten times smaller scene) is recovered as before."""
    R = pkg.rasterizer
    arrays, cam = _scene(pkg, n, w, h, 0, seed=n + w, mu_s=mu_s)
    if ties:
        arrays["positions"][:, 2] = np.float32(4.0)
    K = cam.intrinsics
    ref = orc.render(arrays, cam.rotation, cam.translation, K.fx, K.fy, K.cx, K.cy, w, h, active_degree=0,
                     threads=orc.host_threads())
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=0)
    key = R._skey(torch.device(dev))
    for attempt, forced in enumerate((None, None, 100, None)):          # exact sort, predicted, predicted miss, predicted
        if forced is not None:
            R._last_pairs[key] = forced
            R._held_capacity.pop(key, None)
        out = pkg.render(model, cam, settings)
        assert out.total_pairs == ref["total_pairs"], attempt
        assert np.array_equal(np_(out.gaussian_indices), ref["values"]), attempt
        assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"]), attempt
        assert np.array_equal(np_(out.n_contrib), ref["n_contrib"]), attempt
    if ties:
        nzero = int((ref["keys"] == 0).sum())
        assert nzero > 0 and not np_(out.gaussian_indices)[:nzero].any()
    # the keys of the reference's SortingOutput, rebuilt from the tile starts on this route
    keyed = R.project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam, 0,
                                key_sort=True)
    pend = R.sort_gaussians_predicted(keyed.means_2d, keyed.depths, keyed.radii, keyed.tiles_touched, w, h,
                                      want_keys=True, keyed_workspace=keyed.sort_workspace)
    srt, valid = pend.finish()
    assert valid and np.array_equal(np_(srt.gaussian_keys_sorted).view(np.uint64), ref["keys"])
    assert np.array_equal(np_(srt.gaussian_values_sorted), ref["values"])


def test_sort_routes_agree_in_the_development_build(pkg, dev):
    """The development library can switch the direct-binning route off (cugsdbg_sort_direct_route): a sequence of
    scenes of changing size on one stream - predictions from the previous scene: hits and misses - must give the same
    pairs, ranges and image with the route on and off (tools/direct_route_check.py; the shipped library has no switch)."""
    import ctypes as C
    import subprocess
    import sys
    assert not hasattr(C.CDLL(pkg.LIB_PATH), "cugsdbg_sort_direct_route")
    dev_lib = os.path.join(os.path.dirname(pkg.LIB_PATH), "libcugs_hip_dev.so")
    if not os.path.exists(dev_lib):
        pytest.skip("development library not built")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "direct_route_check.py")], capture_output=True, text=True,
                         timeout=600, env=dict(os.environ, CUGS_HIP_LIBRARY=dev_lib))
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    assert "bad 0" in res.stdout and res.stdout.count(" same") >= 12


def test_sort_equal_depth_ties_keep_index_order(pkg, orc, dev):
    """CUB's stability contract: equal (tile, depth) keys stay in ascending Gaussian index."""
    w, h, n = 128, 96, 4000
    arrays, cam = _scene(pkg, n, w, h, 0, seed=3, mu_s=-2.5)
    arrays["positions"][:, 2] = np.float32(4.0)          # every depth identical
    ref = oracle_forward(orc, arrays, cam, degree=0)
    t = lambda k: torch.from_numpy(ref[k]).to(dev)
    srt = pkg.sort_gaussians(t("means_2d"), t("depths"), t("radii"), t("tiles_touched"), w, h)
    vals = np_(srt.gaussian_values_sorted)
    assert np.array_equal(vals, ref["values"])
    tr = ref["tile_ranges"]
    nzero = int((ref["keys"] == 0).sum())               # quirk Q12: leading (tile 0, Gaussian 0) pairs
    assert nzero > 0 and not vals[:nzero].any()          # this scene has them: they must be reproduced
    for s, e in tr[tr[:, 1] > tr[:, 0]][:50]:
        assert np.all(np.diff(vals[max(s, nzero):e]) > 0)


def _forward_both(pkg, orc, dev, n, w, h, deg, mu_s, bg, seed=1234, view=0):
    arrays, cam = _scene(pkg, n, w, h, deg, seed=seed, mu_s=mu_s, view=view)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=list(bg), active_sh_degree=deg)
    out = pkg.render(model, cam, settings)
    ref = oracle_forward(orc, arrays, cam, bg=bg, degree=deg)
    return arrays, cam, model, settings, out, ref


@pytest.mark.parametrize("n,w,h,deg,mu_s,bg", [
    (20000, 640, 360, 3, -4.6, (0.0, 0.0, 0.0)),
    (20000, 333, 211, 3, -3.5, (0.2, 0.4, 0.6)),       # dense: saturated pixels (Q1), ragged edge tiles
    (500, 320, 240, 0, -3.0, (1.0, 1.0, 1.0)),         # test_rasterizer.cpp:202-230 scale
    (100000, 1920, 1080, 0, -4.6, (0.0, 0.0, 0.0)),    # BASELINE config 2
])
def test_render_forward_parity(pkg, orc, dev, n, w, h, deg, mu_s, bg):
    arrays, cam, model, settings, out, ref = _forward_both(pkg, orc, dev, n, w, h, deg, mu_s, bg)
    assert out.total_pairs == ref["total_pairs"]
    assert np.array_equal(np_(out.gaussian_indices), ref["values"])
    assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"])
    assert np.array_equal(np_(out.n_contrib), ref["n_contrib"])          # every blend decision identical
    assert max_rel_err(np_(out.color), ref["color"]) <= RGB_TOL
    assert max_rel_err(np_(out.final_T), ref["final_T"]) <= RGB_TOL
    # in fact the blend is bit-identical to the oracle (same order, same explicit FMAs)
    assert np.array_equal(np_(out.color).view(np.uint32), ref["color"].view(np.uint32))


def test_rasterize_forward_unpacked_path(pkg, orc, dev):
    """rasterize_forward called with the reference's four arrays only (no packed scratch)."""
    w, h, n = 200, 120, 3000
    arrays, cam = _scene(pkg, n, w, h, 1, seed=9, mu_s=-3.2)
    ref = oracle_forward(orc, arrays, cam, degree=1, bg=(0.5, 0.1, 0.9))
    t = lambda k: torch.from_numpy(np.ascontiguousarray(ref[k])).to(dev)
    fwd = pkg.rasterize_forward(t("means_2d"), t("cov_2d_inv"), t("rgb"), t("opacities_act"), t("tile_ranges"),
                                t("values"), w, h, (0.5, 0.1, 0.9), packed=None)
    assert np.array_equal(np_(fwd.n_contrib), ref["n_contrib"])
    assert np.array_equal(np_(fwd.color).view(np.uint32), ref["color"].view(np.uint32))
    assert np.array_equal(np_(fwd.final_T).view(np.uint32), ref["final_T"].view(np.uint32))


@pytest.mark.parametrize("n,w,h,deg,mu_s,bg,view", [
    (20000, 640, 360, 3, -4.6, (0.0, 0.0, 0.0), 0),
    (20000, 333, 211, 3, -3.5, (0.2, 0.4, 0.6), 0),    # saturated pixels: the Q1 walk-from-the-end matters
    (6000, 320, 240, 2, -3.8, (0.0, 0.0, 0.0), 4),     # rotated + translated camera
    (2000, 160, 120, 0, -3.0, (0.3, 0.3, 0.3), 0),
])
def test_render_backward_parity(pkg, orc, dev, n, w, h, deg, mu_s, bg, view):
    arrays, cam, model, settings, out, ref = _forward_both(pkg, orc, dev, n, w, h, deg, mu_s, bg, seed=77, view=view)
    g = pkg.scene.make_dl_dcolor(w, h)
    grads = pkg.render_backward(torch.from_numpy(g).to(dev), out, model, cam, settings)
    refb = oracle_backward(orc, g, ref, arrays, cam, bg=bg)
    par = load_parity()
    names = ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs", "dL_dmeans_2d")
    rep = par.gradient_report({k: np_(getattr(grads, k)) for k in names}, refb, names)
    print(par.format_report(rep, "render_backward vs oracle (SURVEY 8d element-wise | of the tensor's scale):"))
    for name, v in rep["per_tensor"].items():
        assert v["over_scale"] <= GRAD_TOL, (name, v)    # error relative to the tensor's scale
        got = np_(getattr(grads, name)).reshape(refb[name].shape)
        assert max_rel_err(got, refb[name], floor_frac=1e-3) <= 20 * GRAD_TOL, name   # element-wise, floor 1e-3 of scale
    # SURVEY 8d's own metric (floor 1e-6 of the scale) is printed above; where it exceeds 1e-4 the element must be a
    # cancelling sum: |diff| within the fp32 bound of the magnitudes of its own terms, shown per accumulator
    # ... and EVERY accumulator element within the fp32 bound of its own terms (exactly zero where it has none)
    stage = blend_stage_check(pkg, orc, dev, out, ref, g, bg, n, w, h, tile_order=out.tile_order,
                              label=f"render_backward_parity {w}x{h}")
    print(par.format_report(stage, "blend-backward accumulators, element-wise with the magnitude of their terms:"))
    for name, v in stage.items():
        assert v["over_scale"] <= GRAD_TOL, (name, v)
        assert v["over_bar_beyond_term_bound"] == 0, (name, v)


def test_rasterize_backward_stage_parity(pkg, orc, dev):
    """Stage function with the reference's own signature and the reference-layout outputs."""
    w, h, n = 320, 200, 8000
    arrays, cam = _scene(pkg, n, w, h, 0, seed=21, mu_s=-3.6)
    bg = (0.1, 0.0, 0.2)
    ref = oracle_forward(orc, arrays, cam, degree=0, bg=bg)
    g = pkg.scene.make_dl_dcolor(w, h)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rb = pkg.rasterize_backward(t(g), t(ref["means_2d"]), t(ref["cov_2d_inv"]), t(ref["rgb"]),
                                t(ref["opacities_act"]), t(ref["tile_ranges"]), t(ref["values"]),
                                t(ref["final_T"]), t(ref["n_contrib"]), w, h, bg, n)
    want = orc.rasterize_backward(w, h, bg, ref["tile_ranges"], ref["values"], ref["means_2d"], ref["cov_2d_inv"],
                                  ref["rgb"], ref["opacities_act"], g, ref["final_T"], ref["n_contrib"], n)
    for name in ("dL_drgb", "dL_dopacity_act", "dL_dmeans_2d", "dL_dcov_2d_inv"):
        assert max_err_over_max(np_(getattr(rb, name)), want[name]) <= GRAD_TOL, name
    # Gaussians that touch no pixel keep exactly zero gradients (test_backward.cpp:181-201)
    untouched = ref["radii"] == 0
    assert not np_(rb.dL_drgb)[untouched].any()


def test_blend_with_rows_beyond_32bit_byte_offsets(pkg, orc, dev):
    """More than 2^26 Gaussians: the accumulator is larger than 4 GiB, so the scatter takes 64-bit addresses
    (k_raster_backward<.., WIDE = true>), and the record gathers of both blend kernels index past 2^31 bytes.
    A small scene placed at rows 2^26 .. 2^26 + n of otherwise empty tables must give the small scene's own
    image (bit for bit) and gradients."""
    w, h, n = 160, 120, 3000
    base = (1 << 26) + 5
    big = base + n
    arrays, cam = _scene(pkg, n, w, h, 0, seed=5, mu_s=-3.3)
    bg = (0.2, 0.1, 0.0)
    ref = oracle_forward(orc, arrays, cam, degree=0, bg=bg)
    g = pkg.scene.make_dl_dcolor(w, h)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def table(a):
        full = torch.zeros((big,) + a.shape[1:], dtype=torch.float32, device=dev)
        full[base:] = t(a)
        return full
    means, cov, rgb, opa = (table(ref[k]) for k in ("means_2d", "cov_2d_inv", "rgb", "opacities_act"))
    idx = t(ref["values"]) + base
    ranges = t(ref["tile_ranges"])
    fwd = pkg.rasterize_forward(means, cov, rgb, opa, ranges, idx, w, h, bg)
    assert np.array_equal(np_(fwd.color), ref["color"])
    assert np.array_equal(np_(fwd.n_contrib), ref["n_contrib"])
    rb = pkg.rasterize_backward(t(g), means, cov, rgb, opa, ranges, idx, fwd.final_T, fwd.n_contrib, w, h, bg, big)
    want = orc.rasterize_backward(w, h, bg, ref["tile_ranges"], ref["values"], ref["means_2d"], ref["cov_2d_inv"],
                                  ref["rgb"], ref["opacities_act"], g, ref["final_T"], ref["n_contrib"], n)
    for name in ("dL_drgb", "dL_dopacity_act", "dL_dmeans_2d", "dL_dcov_2d_inv"):
        got = getattr(rb, name)
        assert max_err_over_max(np_(got[base:]), want[name]) <= GRAD_TOL, name
        assert not bool(got[:base].any()), name                  # nothing landed in a truncated address
    # every element within the fp32 bound of its own terms
    terms, mags = oracle_blend_terms(orc, ref, g, bg, n, w, h)
    check_blend_bounds({k: np_(getattr(rb, k)[base:]) for k in terms}, terms, mags, ref["cov_2d_inv"],
                       np.bincount(ref["values"], minlength=n), "rows beyond 2^26 (WIDE, unpacked, colour)")
    del means, cov, rgb, opa, rb
    torch.cuda.empty_cache()


@pytest.mark.parametrize("packed", [False, True])
def test_depth_blend_with_rows_beyond_32bit_byte_offsets(pkg, orc, dev, packed):
    """k_raster_backward<PACKED, WIDE = true, DEPTH = true>: the depth-map backward on an accumulator larger than 4 GiB.
    The small scene sits at rows 2^26 + 5 .. of otherwise empty tables: the unpacked route takes the oracle's four
    arrays and depths there, the packed route the projection's own packed records (render() of the small scene)
    placed there.  Every element of the four accumulators and of dL_ddepths within the fp32 bound of its terms (colour
    + depth + alpha channels), nothing in the rows below, each >4 GiB accumulator freed before the next."""
    w, h, n = 160, 120, 3000
    base = (1 << 26) + 5
    big = base + n
    arrays, cam = _scene(pkg, n, w, h, 0, seed=6, mu_s=-3.3)
    bg = (0.2, 0.1, 0.0)
    ref = oracle_forward(orc, arrays, cam, degree=0, bg=bg)
    g = pkg.scene.make_dl_dcolor(w, h)
    rng = np.random.default_rng(61)
    dD = (rng.standard_normal((h, w)) * 1e-3).astype(np.float32)
    dA = (rng.standard_normal((h, w)) * 1e-3).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def table(a):
        a = torch.as_tensor(a).to(dev)
        full = torch.zeros((big,) + tuple(a.shape[1:]), dtype=torch.float32, device=dev)
        full[base:] = a
        return full
    means, cov, rgb, opa, depths = (table(ref[k]) for k in ("means_2d", "cov_2d_inv", "rgb", "opacities_act", "depths"))
    pk = None
    if packed:
        small = pkg.render(pkg.scene.to_model(arrays, dev), cam, pkg.RenderSettings(background=list(bg), active_sh_degree=0),
                           for_backward=True)
        assert np.array_equal(np_(small.gaussian_indices), ref["values"])
        pk = table(small.packed)
        del small
    idx = t(ref["values"]) + base
    ranges = t(ref["tile_ranges"])
    fwd = pkg.rasterize_forward(means, cov, rgb, opa, ranges, idx, w, h, bg, packed=pk, depths=depths)
    assert np.array_equal(np_(fwd.color).view(np.uint32), ref["color"].view(np.uint32))
    assert np.array_equal(np_(fwd.n_contrib), ref["n_contrib"])
    rb = pkg.rasterize_backward(t(g), means, cov, rgb, opa, ranges, idx, fwd.final_T, fwd.n_contrib, w, h, bg, big,
                                packed=pk, depths=depths, dL_ddepth_map=t(dD), dL_dalpha=t(dA))
    names = ("dL_drgb", "dL_dopacity_act", "dL_dmeans_2d", "dL_dcov_2d_inv", "dL_ddepths")
    for name in names:
        assert not bool(getattr(rb, name)[:base].any()), name   # nothing landed in a truncated address
    assert not bool(rb.grad_accum[:base].any())
    got = {k: np_(getattr(rb, k)[base:]) for k in names}
    del means, cov, rgb, opa, depths, pk, rb, fwd
    torch.cuda.empty_cache()
    terms, mags = oracle_blend_terms(orc, ref, g, bg, n, w, h, dD=dD, dA=dA, depth_route=True)
    assert float(np.abs(terms["dL_ddepths"]).max()) > 0.0
    check_blend_bounds(got, terms, mags, ref["cov_2d_inv"], np.bincount(ref["values"], minlength=n),
                       f"rows beyond 2^26 (WIDE, DEPTH, {'packed' if packed else 'unpacked'})")


def test_render_with_more_than_2_26_gaussians(pkg, dev):
    """The whole path (projection, sort, both blends, projection backward) on a model of 2^26 + 17 + 3000
    Gaussians: all but the last 3000 sit behind the camera.  Image, contributor counts and pair list must be those
    of the 3000 alone (bit for bit, indices shifted), the gradients theirs within the summation-order noise of the
    atomics, and the culled rows must stay exactly zero.  Size-independent property at a size the oracle cannot
    reach; the 3000-Gaussian view itself is oracle-checked by the tests above."""
    w, h, n0 = 160, 120, 3000
    base = (1 << 26) + 17
    big = base + n0
    arrays, cam = _scene(pkg, n0, w, h, 3, seed=8, mu_s=-3.3)
    small = pkg.scene.to_model(arrays, dev)
    st = pkg.RenderSettings(background=[0.1, 0.2, 0.3], active_sh_degree=3)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h)).to(dev)
    out_s = pkg.render(small, cam, st)
    grads_s = pkg.render_backward(g, out_s, small, cam, st)

    def grow(t, fill):
        full = torch.empty((big,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        full[:base] = torch.tensor(fill, dtype=t.dtype, device=dev).reshape((1,) + (-1,) * (t.dim() > 1) + (1,) * (t.dim() - 2))
        full[base:] = t
        return full
    model = pkg.GaussianModel(positions=grow(small.positions, [0.0, 0.0, -10.0]), sh_coeffs=grow(small.sh_coeffs, [0.0]),
                              opacities=grow(small.opacities, [0.0]), rotations=grow(small.rotations, [1.0, 0.0, 0.0, 0.0]),
                              scales=grow(small.scales, [-4.0]))
    out = pkg.render(model, cam, st)
    assert out.total_pairs == out_s.total_pairs
    assert torch.equal(out.color, out_s.color)
    assert torch.equal(out.n_contrib, out_s.n_contrib)
    assert torch.equal(out.tile_ranges, out_s.tile_ranges)
    assert torch.equal(out.gaussian_indices[:out.total_pairs], out_s.gaussian_indices[:out.total_pairs] + base)
    assert not bool(out.radii[:base].any())
    grads = pkg.render_backward(g, out, model, cam, st)
    for name in ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs"):
        got, want = getattr(grads, name), getattr(grads_s, name)
        assert not bool(got[:base].any()), name
        scale = float(want.abs().max())
        assert float((got[base:] - want).abs().max()) <= 1e-5 * scale, name
    del model, out, grads
    torch.cuda.empty_cache()


def test_sh_gate_is_the_backwards_own_recomputation(pkg, orc, dev):
    """The ReLU gate of the SH backward is the sign of the colour AS THE BACKWARD RECOMPUTES IT (sh_backward.cu:92-99,
    constants folded into the basis), not of the forward's output (sh.cu:44-77, constant times coefficient first): the
    two round differently, and this scene (found by tools/fuzz_parity.py, sweep 4242 case 4559) holds a Gaussian whose
    blue is +2^-24 in the forward while the backward's recomputation is <= 0 - the reference passes no gradient there.
    The projection's colour_gate bits must be that test, and the gate recomputed inside the projection backward
    (no bits given) the same."""
    n, w, h, deg, who = 3000, 640, 1, 3, 1742
    arrays = pkg.scene.make_gaussians(n, w, 8, sh_degree=deg, seed=11090329, mu_s=-3.8)
    cam = pkg.scene.make_camera(w, h, view=0)
    bg = (0.8241434213650344, 0.044957994903048415, 0.8172446097541172)
    ref = oracle_forward(orc, arrays, cam, bg=bg, degree=deg, scale_mod=0.5)
    g = pkg.scene.make_dl_dcolor(w, h, seed=4559)
    refb = oracle_backward(orc, g, ref, arrays, cam, bg=bg, scale_mod=0.5)
    dirs = orc.directions(arrays["positions"], cam.camera_center())
    probe = orc.sh_backward(deg, arrays["sh_coeffs"], dirs, np.ones((n, 3), np.float32))
    want_gate = (probe[:, :, 0] != 0).astype(np.uint8)            # Y_0 is a non-zero constant: the gate itself
    assert ref["rgb"][who, 2] > 0 and want_gate[who, 2] == 0       # the straddling channel: forward open, gate closed
    assert not refb["dL_dsh_coeffs"][who, 2].any() and refb["dL_dsh_coeffs"][who, 0].any()

    model = pkg.scene.to_model(arrays, dev)
    st = pkg.RenderSettings(background=list(bg), active_sh_degree=deg, scale_modifier=0.5)
    out = pkg.render(model, cam, st)
    bits = np_(out.colour_gate)
    assert np.array_equal(np.stack([(bits >> c) & 1 for c in range(3)], axis=1), want_gate)
    grads = pkg.render_backward(torch.from_numpy(g).to(dev), out, model, cam, st)
    got = np_(grads.dL_dsh_coeffs)
    assert not got[who, 2].any()
    assert max_err_over_max(got, refb["dL_dsh_coeffs"]) <= GRAD_TOL
    # no bits: recomputed from the coefficients inside the kernel - identical
    out2 = pkg.render(model, cam, st)
    out2.colour_gate = None
    grads2 = pkg.render_backward(torch.from_numpy(g).to(dev), out2, model, cam, st)
    a, b = grads.dL_dsh_coeffs, grads2.dL_dsh_coeffs            # (two runs of the blend backward differ in summation order)
    assert torch.equal(a == 0, b == 0)
    assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())


def test_project_backward_stage_parity(pkg, orc, dev):
    """Per-Gaussian chain rule on identical incoming 2-D gradients: same operation order, no
    contraction -> bit-identical to the oracle."""
    w, h, n = 320, 200, 8000
    arrays, cam = _scene(pkg, n, w, h, 3, seed=31, mu_s=-3.6, view=2)
    ref = oracle_forward(orc, arrays, cam)
    rng = np.random.default_rng(0)
    gm = rng.standard_normal((n, 2)).astype(np.float32)
    gc = rng.standard_normal((n, 3)).astype(np.float32)
    gr = rng.standard_normal((n, 3)).astype(np.float32)
    go = rng.standard_normal(n).astype(np.float32)
    model = pkg.scene.to_model(arrays, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pb = pkg.project_backward(t(gm), t(gc), t(gr), t(go), model.positions, model.rotations, model.scales,
                              model.opacities, model.sh_coeffs, t(ref["radii"]), cam, 3)
    K = cam.intrinsics
    want = orc.project_backward(arrays["positions"], arrays["rotations"], arrays["scales"], arrays["opacities"],
                                ref["view"], K.fx, K.fy, K.cx, K.cy, 1.0, ref["radii"], gm, gc, go)
    want_sh = orc.sh_backward(3, arrays["sh_coeffs"], ref["dirs"], gr)
    for name in ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities"):
        got = np_(getattr(pb, name)).reshape(want[name].shape)
        assert np.array_equal(got.view(np.uint32), want[name].view(np.uint32)), name
    assert max_rel_err(np_(pb.dL_dsh_coeffs), want_sh) <= 1e-6


@pytest.mark.parametrize("n,active", [(8000, 3), (257, 3), (5003, 1), (64, 0)])
def test_project_backward_factor_tile_equals_the_row_tile(pkg, orc, dev, n, active):
    """With the projection's gate bits and degree-3 storage the kernel keeps the FACTORS of the SH gradient rows in LDS
    (16 basis values + 3 gated colour gradients per Gaussian) and the storing thread multiplies; without
    the bits it assembles the rows themselves in the 50 KB tile.  Same products, same selects: every output bit for bit
    the same - ragged last workgroup, fewer active coefficients than stored ones (zeros beyond) and the geometry
    gradients, whose inputs the factor route requests earlier, included - and both the oracle's."""
    w, h = 320, 200
    arrays, cam = _scene(pkg, n, w, h, 3, seed=100 + n, mu_s=-3.6, view=1)
    ref = oracle_forward(orc, arrays, cam, degree=active)
    rng = np.random.default_rng(n)
    gm = rng.standard_normal((n, 2)).astype(np.float32)
    gc = rng.standard_normal((n, 3)).astype(np.float32)
    gr = rng.standard_normal((n, 3)).astype(np.float32)
    go = rng.standard_normal(n).astype(np.float32)
    model = pkg.scene.to_model(arrays, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    proj = pkg.project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam, active)
    assert proj.colour_gate is not None
    args = (t(gm), t(gc), t(gr), t(go), model.positions, model.rotations, model.scales, model.opacities,
            model.sh_coeffs, t(ref["radii"]), cam, active)
    rows = pkg.project_backward(*args)                                    # gate recomputed, rows in the tile
    fac = pkg.project_backward(*args, colour_gate=proj.colour_gate)       # gate bits given: the factor tile
    for name in ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs"):
        a, b = np_(getattr(rows, name)), np_(getattr(fac, name))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    bare = pkg.project_backward(*args, colour_gate=proj.colour_gate, skip_sh_grad=True)   # the data-parallel route: no rows
    assert bare.dL_dsh_coeffs is None
    for name in ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities"):
        assert torch.equal(getattr(bare, name), getattr(fac, name)), name
    want_sh = orc.sh_backward(active, arrays["sh_coeffs"], ref["dirs"], gr)
    got_sh = np_(fac.dL_dsh_coeffs)
    assert max_rel_err(got_sh, want_sh) <= 1e-6
    assert not got_sh[:, :, (active + 1) ** 2:].any()
    K = cam.intrinsics
    want = orc.project_backward(arrays["positions"], arrays["rotations"], arrays["scales"], arrays["opacities"],
                                ref["view"], K.fx, K.fy, K.cx, K.cy, 1.0, ref["radii"], gm, gc, go)
    for name in ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities"):
        got = np_(getattr(fac, name)).reshape(want[name].shape)
        assert np.array_equal(got.view(np.uint32), want[name].view(np.uint32)), name


@pytest.mark.parametrize("deg,c", [(0, 1), (1, 4), (2, 9), (3, 16), (1, 16), (0, 9)])
def test_sh_forward_backward_parity(pkg, orc, dev, deg, c):
    """evaluate_sh_cuda / evaluate_sh_backward_cuda; the reference's bar is 1e-4 (test_sh.cpp:161-216)."""
    n = 10000
    rng = np.random.default_rng(deg * 31 + c)
    sh = rng.standard_normal((n, 3, c)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    g = rng.standard_normal((n, 3)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    got = np_(pkg.evaluate_sh_cuda(deg, t(sh), t(d)))
    want = orc.sh_forward(deg, sh, d)
    assert np.allclose(got, want, rtol=1e-6, atol=1e-6)
    got_b = np_(pkg.evaluate_sh_backward_cuda(deg, t(sh), t(d), t(g)))
    want_b = orc.sh_backward(deg, sh, d, g)
    assert np.allclose(got_b, want_b, rtol=1e-6, atol=1e-7)
    assert not got_b[:, :, (deg + 1) ** 2:].any()          # inactive coefficients zero-filled


def test_sh_input_validation(pkg, dev):
    """test_sh.cpp:127-143: invalid inputs raise."""
    sh = torch.zeros((4, 3, 4), device=dev)
    d = torch.zeros((4, 3), device=dev)
    with pytest.raises(RuntimeError):
        pkg.evaluate_sh_cuda(4, sh, d)
    with pytest.raises(RuntimeError):
        pkg.evaluate_sh_cuda(2, sh, d)                     # needs 9 coefficients
    with pytest.raises(RuntimeError):
        pkg.evaluate_sh_cuda(1, sh, d[:3])


def test_empty_model_and_no_pairs(pkg, dev):
    """rasterizer.cpp:36-55 and sorting.cu:154-160."""
    w, h = 70, 50
    f = dict(dtype=torch.float32, device=dev)
    empty = pkg.GaussianModel(torch.zeros((0, 3), **f), torch.zeros((0, 3, 16), **f), torch.zeros((0, 1), **f),
                              torch.zeros((0, 4), **f), torch.zeros((0, 3), **f))
    cam = pkg.scene.make_camera(w, h)
    settings = pkg.RenderSettings(background=[0.2, 0.5, 0.7])
    out = pkg.render(empty, cam, settings)
    assert out.color.shape == (h, w, 3) and out.tile_ranges.shape == (0, 2)
    assert torch.allclose(out.color[..., 1], torch.full((h, w), 0.5, **f))
    assert bool((out.final_T == 1).all()) and not bool(out.n_contrib.any())
    grads = pkg.render_backward(torch.ones((h, w, 3), **f), out, empty, cam, settings)
    assert grads.dL_dpositions.shape == (0, 3) and grads.dL_dsh_coeffs.shape == (0, 3, 16)

    # every Gaussian behind the camera: P == 0, image = background, all gradients exactly zero
    arrays = pkg.scene.make_gaussians(300, w, h, sh_degree=1, seed=2)
    arrays["positions"][:, 2] = -3.0
    model = pkg.scene.to_model(arrays, dev)
    out = pkg.render(model, cam, settings)
    assert out.total_pairs == 0 and not bool(out.tile_ranges.any())
    assert torch.allclose(out.color[..., 2], torch.full((h, w), 0.7, **f))
    grads = pkg.render_backward(torch.ones((h, w, 3), **f), out, model, cam, settings)
    for name in ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs", "dL_dmeans_2d"):
        assert not bool(getattr(grads, name).any()), name


def test_fused_adam_parity(pkg, orc, dev):
    """One launch for the five groups: bit-exact against the oracle's restatement of k_fused_adam,
    and within the reference's own bar (test_fused_adam.cpp:95-145) of torch.optim.Adam."""
    n = 1003                                        # not a multiple of 4: exercises the scalar tails
    g0 = torch.Generator().manual_seed(42)
    shapes = dict(positions=(n, 3), sh_coeffs=(n, 3, 16), opacities=(n, 1), scales=(n, 3), rotations=(n, 4))
    host = {k: torch.randn(s, generator=g0) for k, s in shapes.items()}
    model = pkg.GaussianModel(**{k: v.clone().to(dev) for k, v in host.items()})
    cfg = pkg.AdamConfig()
    opt = pkg.FusedAdam(model, cfg)
    lrs = dict(positions=cfg.position_lr_config.lr_init, sh_coeffs=cfg.lr_sh_coeffs, opacities=cfg.lr_opacities,
               scales=cfg.lr_scales, rotations=cfg.lr_rotations)
    tparams = {k: v.clone().requires_grad_(True) for k, v in host.items()}
    topt = torch.optim.Adam([dict(params=[tparams[k]], lr=lrs[k]) for k in shapes], betas=(cfg.beta1, cfg.beta2),
                            eps=cfg.eps)
    o_p = {k: v.numpy().copy() for k, v in host.items()}
    o_m = {k: np.zeros_like(v) for k, v in o_p.items()}
    o_v = {k: np.zeros_like(v) for k, v in o_p.items()}
    for step in range(1, 11):
        grads = {k: torch.randn(s, generator=g0) for k, s in shapes.items()}
        opt.apply_gradients(pkg.BackwardOutput(grads["positions"].to(dev), grads["rotations"].to(dev),
                                               grads["scales"].to(dev), grads["opacities"].to(dev),
                                               grads["sh_coeffs"].to(dev), None))
        opt.step()
        bc1, bc2 = orc.adam_bias_correction(cfg.beta1, cfg.beta2, step)
        for k in shapes:
            orc.fused_adam(o_p[k], grads[k].numpy(), o_m[k], o_v[k], lrs[k], cfg.beta1, cfg.beta2, cfg.eps, bc1, bc2)
            tparams[k].grad = grads[k].clone()
        topt.step()
        if step in (1, 10):
            for k in shapes:
                got = np_(getattr(model, k))
                assert np.array_equal(got.view(np.uint32), o_p[k].view(np.uint32)), (k, step)
                rtol, atol = (1e-5, 1e-6) if step == 1 else (1e-4, 1e-5)
                assert np.allclose(got, tparams[k].detach().numpy(), rtol=rtol, atol=atol), (k, step)


def test_fused_adam_zero_grad_is_identity_and_lr(pkg, dev):
    """test_fused_adam.cpp:151-231: LR getters, decay, zero gradient leaves params bit-identical."""
    n = 64
    f = dict(dtype=torch.float32, device=dev)
    model = pkg.GaussianModel(torch.randn((n, 3), **f), torch.randn((n, 3, 4), **f), torch.randn((n, 1), **f),
                              torch.randn((n, 4), **f), torch.randn((n, 3), **f))
    before = {k: getattr(model, k).clone() for k in ("positions", "sh_coeffs", "opacities", "rotations", "scales")}
    opt = pkg.FusedAdam(model)
    z = lambda t: torch.zeros_like(t)
    opt.apply_gradients(pkg.BackwardOutput(z(model.positions), z(model.rotations), z(model.scales),
                                           z(model.opacities), z(model.sh_coeffs), None))
    opt.step()
    for k, v in before.items():
        assert torch.equal(getattr(model, k), v), k
    assert opt.get_lr(pkg.ParamGroup.kSHCoeffs) == pytest.approx(2.5e-3)
    opt.update_lr(15000)
    assert opt.get_lr(pkg.ParamGroup.kPositions) == pytest.approx(pkg.position_lr(15000, pkg.PositionLRConfig()))
    assert opt.get_lr(pkg.ParamGroup.kPositions) == pytest.approx(1.6e-5, rel=1e-3)


def test_compact_exchange_equals_sum_of_views(pkg, orc, dev):
    """Data-parallel extension: rebuilding the SH gradient of a V-view batch from the gated colour gradients
    (cugs_sh_backward_views) equals the sum of the per-view render_backward results, and the per-view path
    with the SH gradient skipped leaves every other gradient unchanged."""
    w, h, n, deg, V = 200, 150, 4000, 3, 3
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=deg, seed=5, mu_s=-3.6)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=deg)
    full_sh = torch.zeros((n, 3, 16), device=dev)
    full_pos = torch.zeros((n, 3), device=dev)
    gated_all, centres, pos_sum = [], [], torch.zeros((n, 3), device=dev)
    for v in range(V):
        cam = pkg.scene.make_camera(w, h, view=v)
        g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=100 + v)).to(dev)
        out = pkg.render(model, cam, settings)
        ref = pkg.render_backward(g, out, model, cam, settings)                        # standard path
        full_sh += ref.dL_dsh_coeffs
        full_pos += ref.dL_dpositions
        gated = torch.empty((n, 3), device=dev)
        flat = torch.empty((11 * n,), device=dev)
        lean = pkg.render_backward(g, out, model, cam, settings, dL_drgb_gated_out=gated, geom_flat=flat)   # exchange path
        assert lean.dL_dsh_coeffs is None and lean.dL_drotations.data_ptr() == flat.data_ptr()
        assert max_err_over_max(np_(lean.dL_drotations), np_(ref.dL_drotations)) <= 1e-5
        assert max_err_over_max(np_(lean.dL_dopacities), np_(ref.dL_dopacities)) <= 1e-5
        assert max_err_over_max(np_(lean.dL_dpositions), np_(ref.dL_dpositions)) <= 1e-5     # atomics order only
        pos_sum += lean.dL_dpositions
        gated_all.append(gated)
        centres.append(cam.camera_center().tolist())
        # single view through the exchange entry point (no process group): identical to the standard path
        one = pkg.parallel.exchange_gradients(lean, gated, model.positions, cam.camera_center(), deg, 16)
        assert max_err_over_max(np_(one.dL_dsh_coeffs), np_(ref.dL_dsh_coeffs)) <= 1e-5
        assert one.dL_dopacities.shape == (n, 1) and one.dL_drotations.shape == (n, 4)
    got = pkg.sh_backward_views(deg, model.positions, torch.stack(gated_all), centres, 16)
    assert max_err_over_max(np_(got), np_(full_sh)) <= 1e-5
    assert max_err_over_max(np_(pos_sum), np_(full_pos)) <= 1e-5


@pytest.mark.parametrize("n,w,h,deg,stored", [(3000, 200, 150, 3, 3), (777, 96, 64, 1, 1), (1000, 128, 96, 0, 0),
                                              (1301, 128, 96, 1, 3)])
def test_fused_adam_backward_equals_backward_then_adam(pkg, dev, n, w, h, deg, stored):
    """cugs_project_backward_adam (a8 + a9 + a11 in one launch, single-GPU training): the model, the moments and
    dL_dmeans_2d after render_backward(..., fused_adam=opt) must equal render_backward + apply_gradients + step
    BIT FOR BIT over three steps (moments carried, bias corrections advancing) - same arithmetic, same order;
    only the blend backward's atomics may reorder sums, so both paths consume the SAME accumulator rows.
    With degree-3 storage both launches keep the FACTORS of the SH gradient rows in LDS; the last case
    has fewer active coefficients than stored ones and a ragged last workgroup.
    After the third step both twins densify (same statistics, same noise, densify(optimizer=) on their own optimizers)
    and run two more steps at the new N: everything stays bit for bit equal, exactly as before the event."""
    arrays, cam = _scene(pkg, n, w, h, stored, seed=n, mu_s=-3.7)
    settings = pkg.RenderSettings(background=[0.2, 0.1, 0.3], active_sh_degree=deg)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=n + 1) * 3000.0).to(dev)    # gradients large enough to move parameters
    ma, mb = pkg.scene.to_model(arrays, dev), pkg.scene.to_model(arrays, dev)
    oa, ob = pkg.FusedAdam(ma), pkg.FusedAdam(mb)
    R = pkg.rasterizer
    names = ("positions", "sh_coeffs", "opacities", "scales", "rotations")
    # the hand-off to densification: after step 2 both twins accumulate their (equal) dL_dmeans_2d, densify with the same
    # noise, each through its OWN optimizer, and go on for two more steps - the fused launch takes the moment pointers
    # afresh each step, so the carried rows, the zeroed new rows and the running step count must serve both paths alike
    dcfg = pkg.DensificationConfig(densify_from=0, densify_every=5, opacity_threshold=0.3, percent_dense=0.0376)
    ca, cb = pkg.DensificationController(dcfg, 1.0), pkg.DensificationController(dcfg, 1.0)
    for step in range(5):
        if step == 3:
            assert not torch.equal(ma.positions, torch.from_numpy(arrays["positions"]).to(dev))   # three steps moved the model
            for ctrl, dm in ((ca, dm_a), (cb, dm_b)):
                ctrl.accumulate_gradients(dm, out.radii)
            # half of the visible rows over the threshold; by size about half of them clone and half split
            dcfg.grad_threshold = float(dm_a.norm(2, dim=1)[out.radii > 0].median())
            noise = torch.randn((2, n, 3), generator=torch.Generator().manual_seed(n)).to(dev)
            sa = ca.densify(ma, 5, noise, optimizer=oa)
            sb = cb.densify(mb, 5, noise, optimizer=ob)
            assert sa == sb and sa.num_cloned > 0 and sa.num_split > 0 and sa.num_pruned > sa.num_split
            n = ma.num_gaussians()
            assert n == sa.num_after == mb.num_gaussians() and n != arrays["positions"].shape[0]
            for i, k in enumerate(names):
                assert torch.equal(getattr(ma, k), getattr(mb, k)), ("densify", k)
                assert torch.equal(oa.m_[i], ob.m_[i]) and torch.equal(oa.v_[i], ob.v_[i]), ("densify", k)
                assert oa.m_[i].shape == getattr(ma, k).shape and bool(oa.m_[i].any()) and not bool(oa.m_[i][-1].any())
        out = pkg.render(ma, cam, settings)
        assert all(torch.equal(getattr(ma, k), getattr(mb, k)) for k in names)
        rb = R.rasterize_backward(g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                  out.gaussian_indices, out.final_T, out.n_contrib, w, h, settings.background, n,
                                  packed=out.packed, unpack=False)
        # path A: projection backward -> five gradient tensors -> FusedAdam.step
        dm_a = torch.empty((n, 2), device=dev)
        pb = R.project_backward(None, None, None, None, ma.positions, ma.rotations, ma.scales, ma.opacities,
                                ma.sh_coeffs, out.radii, cam, deg, settings.scale_modifier, grad_accum=rb.grad_accum,
                                colour_gate=out.colour_gate, dL_dmeans_2d_out=dm_a)
        oa.apply_gradients(pkg.BackwardOutput(pb.dL_dpositions, pb.dL_drotations, pb.dL_dscales, pb.dL_dopacities,
                                              pb.dL_dsh_coeffs, dm_a))
        oa.step()
        # path B: the fused launch on the same accumulator rows
        import ctypes as C
        from cugs_amd._lib import check, lib
        adam = ob.begin_fused_step()
        dm_b = torch.empty((n, 2), device=dev)
        cam_abi = cam.to_abi()
        P = lambda t: C.c_void_p(t.data_ptr())
        check(lib.cugs_project_backward_adam(n, int(mb.sh_coeffs.shape[2]), deg, P(mb.positions), P(mb.rotations),
                                             P(mb.scales), P(mb.opacities), P(mb.sh_coeffs), P(out.radii), P(out.colour_gate),
                                             C.byref(cam_abi), float(settings.scale_modifier), P(rb.grad_accum),
                                             C.byref(adam), P(dm_b), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "cugs_project_backward_adam")
        assert torch.equal(dm_a, dm_b)
        for i, k in enumerate(names):
            assert torch.equal(getattr(ma, k), getattr(mb, k)), (step, k)
            assert torch.equal(oa.m_[i], ob.m_[i]) and torch.equal(oa.v_[i], ob.v_[i]), (step, k)
        assert oa.step_count_ == ob.step_count_ == step + 1
    assert not torch.equal(ma.positions, torch.from_numpy(arrays["positions"]).to(dev))       # the model moved
    # and through the host surface: render_backward(..., fused_adam=) returns only dL_dmeans_2d
    out = pkg.render(mb, cam, settings)
    res = pkg.render_backward(g, out, mb, cam, settings, fused_adam=ob)
    assert res.dL_dpositions is None and res.dL_dsh_coeffs is None and res.dL_dmeans_2d.shape == (n, 2)
    assert ob.step_count_ == 6


def test_backward_with_clamped_alphas_and_tiny_images(pkg, orc, dev):
    """Q2 (backward.cu:181-191): where opacity * e >= 0.99 the alpha is clamped, dL/dopacity and dL/dpower are zeroed
    and dL/drgb still flows.  The standard scenes (opacity logits ~ N(0,1)) never reach the clamp, so a third of the
    Gaussians here get logit +9 (sigmoid 0.99988): the clamp gate (`below_alpha_cap`) decides on thousands of
    contributions.  Also the backward on 1-pixel / sliver images (the forward of these is in test_gpu_fullsize.py)."""
    for n, w, h, mu_s, seed in ((6000, 320, 200, -3.4, 5), (60, 1, 1, -3.0, 6), (300, 17, 3, -1.5, 7)):
        arrays = pkg.scene.make_gaussians(n, max(w, 8), max(h, 8), sh_degree=1, seed=seed, mu_s=mu_s)
        arrays["opacities"][:: 3] = 9.0
        cam = pkg.scene.make_camera(w, h)
        model = pkg.scene.to_model(arrays, dev)
        st = pkg.RenderSettings(background=[0.3, 0.1, 0.2], active_sh_degree=1)
        out = pkg.render(model, cam, st)
        ref = oracle_forward(orc, arrays, cam, bg=(0.3, 0.1, 0.2), degree=1)
        assert np.array_equal(np_(out.n_contrib), ref["n_contrib"])
        assert np.array_equal(np_(out.color).view(np.uint32), ref["color"].view(np.uint32))
        if n == 6000:                                   # the clamp is really exercised: some pixel sees alpha == 0.99
            assert float(ref["final_T"].min()) < 0.011 and int((ref["n_contrib"] == 1).sum()) > 0
        g = pkg.scene.make_dl_dcolor(w, h, seed=seed)
        grads = pkg.render_backward(torch.from_numpy(g).to(dev), out, model, cam, st)
        refb = oracle_backward(orc, g, ref, arrays, cam, bg=(0.3, 0.1, 0.2))
        for name in ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs", "dL_dmeans_2d"):
            got = np_(getattr(grads, name)).reshape(refb[name].shape)
            assert max_err_over_max(got, refb[name]) <= GRAD_TOL, (n, name)


def test_forward_blend_clears_the_backward_accumulator(pkg, orc, dev):
    """cugs_blend_forward_opts::zero_buf / cugs_blend_backward_opts::prezeroed: the forward blend fills a DIRTY buffer with
    zeros while it renders (image bit-equal to the plain entry), the backward run on that buffer without its own
    fill gives the gradients of the filling path (<= 1e-5: atomics reorder sums), an odd-sized buffer is covered to
    its last 16 bytes, a misaligned one is refused, and a RenderOutput hands its cleared accumulator out ONCE - a
    second render_backward on the same output falls back to the filling path and is still right."""
    n, w, h, deg = 20000, 333, 217, 2
    arrays, cam = _scene(pkg, n, w, h, deg, seed=77, mu_s=-3.8)
    settings = pkg.RenderSettings(background=[0.3, 0.6, 0.1], active_sh_degree=deg)
    model = pkg.scene.to_model(arrays, dev)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=78)).to(dev)
    R = pkg.rasterizer
    out = pkg.render(model, cam, settings)
    assert out.zeroed_accum is not None and int(torch.count_nonzero(out.zeroed_accum)) == 0
    args = (out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges, out.gaussian_indices,
            w, h, settings.background)
    plain = R.rasterize_forward(*args, packed=out.packed)
    for numel in (4, 16 * n, 16 * n + 4, 1 << 22):             # smaller than the grid, exact, odd tail, large
        dirty = torch.full((numel + 4,), 7.0, device=dev)
        z = R.rasterize_forward(*args, packed=out.packed, zero_buf=dirty[:numel])
        assert torch.equal(z.color, plain.color) and torch.equal(z.n_contrib, plain.n_contrib)
        assert int(torch.count_nonzero(dirty[:numel])) == 0 and bool((dirty[numel:] == 7.0).all())
    with pytest.raises(RuntimeError):
        R.rasterize_forward(*args, packed=out.packed, zero_buf=torch.zeros(9, device=dev)[1:])     # misaligned
    bargs = (g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges, out.gaussian_indices,
             out.final_T, out.n_contrib, w, h, settings.background, n)
    filled = R.rasterize_backward(*bargs, packed=out.packed)
    pre = R.rasterize_backward(*bargs, packed=out.packed, zeroed_accum=out.zeroed_accum)
    for k in ("dL_drgb", "dL_dopacity_act", "dL_dmeans_2d", "dL_dcov_2d_inv"):
        a, b = getattr(filled, k), getattr(pre, k)
        assert float((a - b).abs().max()) <= 1e-5 * max(float(a.abs().max()), 1e-30), k
    # through render()/render_backward(): consumed once, then the filling path
    out2 = pkg.render(model, cam, settings)
    first = pkg.render_backward(g, out2, model, cam, settings)
    assert out2.zeroed_accum is None
    second = pkg.render_backward(g, out2, model, cam, settings)
    for k in ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs"):
        a, b = getattr(first, k), getattr(second, k)
        assert float((a - b).abs().max()) <= 1e-5 * max(float(a.abs().max()), 1e-30), k
    assert pkg.render(model, cam, settings, for_backward=False).zeroed_accum is None


def test_predicted_capacity_is_held_while_the_pair_count_drifts(pkg, dev):
    """The capacity the predicted sort sizes its buffers with stays put while the estimate drifts below it (down to
    80 %), grows with 5 % to spare, and follows a collapse: a capacity that tracked a slowly moving count would change
    the output buffer size - and fragment the caching allocator - on every step."""
    R = pkg.rasterizer
    d = torch.device(dev)
    R._held_capacity.pop(R._skey(d), None)
    try:
        need = lambda e: int(e * R.PREDICT_MARGIN[0]) + R.PREDICT_MARGIN[1]
        c0 = R._capacity_for(d, 10_000_000)
        assert c0 == need(10_000_000)
        assert R._capacity_for(d, 9_900_000) == c0 and R._capacity_for(d, 8_200_000) == c0      # drift: held
        c1 = R._capacity_for(d, 10_400_000)                                                       # growth: 5 % spare
        assert c1 == int(need(10_400_000) * 1.05) and R._capacity_for(d, 10_800_000) == c1
        c2 = R._capacity_for(d, 2_000_000)                                                        # collapse: follow
        assert c2 == need(2_000_000)
    finally:
        R._held_capacity.pop(R._skey(d), None)


@pytest.mark.parametrize("mu_s", [-4.6, -3.0])
def test_sort_is_memory_safe_on_inconsistent_tile_counts(pkg, orc, dev, mu_s):
    """tiles_touched is an INPUT of sort_gaussians (the reference takes its cumsum for the offsets and recomputes the
    rectangles for the fill, sorting.cu:145,52-57): a caller may hand over counts that do not match the rectangles.
    The result is then not defined by the reference (its fill would write into the neighbours' slots), but both pair
    routes must stay inside their buffers: total = sum of the counts, every index a valid Gaussian, every tile range
    inside [0, total]."""
    n, w, h = 30000, 1280, 720
    arrays, cam = _scene(pkg, n, w, h, 0, seed=23, mu_s=mu_s)
    ref = oracle_forward(orc, arrays, cam, degree=0)
    rng = np.random.default_rng(5)
    tiles = ref["tiles_touched"].astype(np.int64)
    bad = np.clip(tiles + rng.integers(-3, 4, size=n) * (rng.random(n) < 0.3), 0, None).astype(np.int32)
    t = lambda k: torch.from_numpy(ref[k]).to(dev)
    srt = pkg.sort_gaussians(t("means_2d"), t("depths"), t("radii"), torch.from_numpy(bad).to(dev), w, h)
    total = int(bad.astype(np.int64).sum())
    assert srt.total_pairs == total
    vals, tr = np_(srt.gaussian_values_sorted), np_(srt.tile_ranges)
    assert vals.shape[0] == total and vals.min() >= 0 and vals.max() < n
    assert tr.min() >= 0 and tr.max() <= total and np.all(tr[:, 1] >= tr[:, 0])


def test_sort_reports_a_pair_count_beyond_int32(pkg, dev):
    """The reference indexes pairs with int (sorting.cu:146-151): more than 2^31 - 1 pairs cannot be represented.
    40 000 splats covering 63 001 tiles each (2.52e9 pairs) must come back as an overflow error from the count - with
    the sums carried in 64 bits on the device - not as a wrapped count and a short allocation."""
    n, w, h = 40000, 4096, 4096
    means = torch.full((n, 2), 2048.0, device=dev)
    depths = torch.linspace(1.0, 9.0, n, device=dev)
    radii = torch.full((n,), 2000, dtype=torch.int32, device=dev)
    x0, x1 = (2048 - 2000) // 16, (2048 + 2000 + 1 + 15) // 16      # sorting.cu:52-57
    per = (x1 - x0) ** 2
    assert n * per > 2 ** 31
    tiles = torch.full((n,), per, dtype=torch.int32, device=dev)
    with pytest.raises(pkg.CugsError, match="does not fit int32"):
        pkg.sort_gaussians(means, depths, radii, tiles, w, h)
    # and the library is usable afterwards
    srt = pkg.sort_gaussians(means[:10], depths[:10], radii[:10], tiles[:10], w, h)
    assert srt.total_pairs == 10 * per


@pytest.mark.parametrize("side", [4096, 4112])        # 256 tile columns: column-ordered emission; 257: three tile passes
def test_sort_of_a_billion_pairs(pkg, dev, side):
    """1.26e9 pairs (59 % of the int32 range): 20 000 splats, each covering the same 251 x 251 tiles, depths
    increasing with the index.  The exact answer is known without an oracle: every covered tile lists 0 .. n-1 in
    order, the covered tiles follow each other in tile-id order, every other tile is empty."""
    n = 20000
    means = torch.full((n, 2), 2048.0, device=dev)
    depths = torch.linspace(1.0, 9.0, n, device=dev)
    radii = torch.full((n,), 2000, dtype=torch.int32, device=dev)
    x0, x1 = (2048 - 2000) // 16, (2048 + 2000 + 1 + 15) // 16      # sorting.cu:52-57
    per = (x1 - x0) ** 2
    tiles = torch.full((n,), per, dtype=torch.int32, device=dev)
    srt = pkg.sort_gaussians(means, depths, radii, tiles, side, side)
    total = n * per
    assert srt.total_pairs == total and total > 1.2e9
    vals = srt.gaussian_values_sorted
    assert vals.shape[0] == total
    assert torch.equal(vals.view(per, n), torch.arange(n, dtype=torch.int32, device=dev).expand(per, n))
    ntx = (side + 15) // 16
    covered = torch.zeros((ntx, ntx), dtype=torch.bool, device=dev)
    covered[x0:x1, x0:x1] = True
    rank = torch.cumsum(covered.reshape(-1).to(torch.int64), 0) - 1
    start = torch.where(covered.reshape(-1), rank * n, torch.zeros_like(rank))
    end = torch.where(covered.reshape(-1), (rank + 1) * n, torch.zeros_like(rank))
    tr = srt.tile_ranges.to(torch.int64)
    assert torch.equal(tr[:, 0], start) and torch.equal(tr[:, 1], end)
    del srt, vals
    torch.cuda.empty_cache()


def test_deferred_pair_count_render(pkg, orc, dev):
    """render(..., defer_count=True) returns before the host has read the sort's pair count (a training loop queues
    its loss kernels in that window); wait() / render_backward complete it.  Same image, indices and gradients as
    the blocking render; a capacity that turns out too small raises PredictionMiss instead of handing out an
    invalid frame, and the next render is right again."""
    n, w, h, deg = 20000, 640, 360, 2
    arrays, cam = _scene(pkg, n, w, h, deg, seed=31, mu_s=-3.9)
    settings = pkg.RenderSettings(background=[0.1, 0.4, 0.2], active_sh_degree=deg)
    model = pkg.scene.to_model(arrays, dev)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=32)).to(dev)
    R = pkg.rasterizer
    ref = pkg.render(model, cam, settings)                       # blocking; also seeds the prediction
    ref_g = pkg.render_backward(g, ref, model, cam, settings)
    out = pkg.render(model, cam, settings, defer_count=True)
    assert out.pending is not None and out.total_pairs == -1
    grads = pkg.render_backward(g, out, model, cam, settings)    # waits, trims, runs
    assert out.pending is None and out.total_pairs == ref.total_pairs
    assert torch.equal(out.gaussian_indices, ref.gaussian_indices) and torch.equal(out.color, ref.color)
    for k in ("dL_dpositions", "dL_dsh_coeffs", "dL_dscales"):
        a, b = getattr(ref_g, k), getattr(grads, k)
        assert float((a - b).abs().max()) <= 1e-5 * max(float(a.abs().max()), 1e-30), k
    # a prediction that is too small
    R._last_pairs[R._skey(torch.device(dev))] = 50
    R._held_capacity.pop(R._skey(torch.device(dev)), None)
    margin = R.PREDICT_MARGIN
    R.PREDICT_MARGIN = (1.0, 0)
    try:
        bad = pkg.render(model, cam, settings, defer_count=True)
        with pytest.raises(pkg.PredictionMiss):
            bad.wait()
    finally:
        R.PREDICT_MARGIN = margin
    again = pkg.render(model, cam, settings, defer_count=True).wait()
    assert again.total_pairs == ref.total_pairs and torch.equal(again.color, ref.color)


@pytest.mark.parametrize("n,deg,stored", [(30000, 3, 3), (1000, 0, 0), (777, 1, 2), (5000, 2, 3)])
def test_projection_in_two_halves_equals_the_whole(pkg, orc, dev, n, deg, stored):
    """cugs_project_forward_geometry + cugs_project_forward_colour (render()'s route: the colour half on a side stream
    underneath the sort) against cugs_project_forward_keyed: every output - the packed records, the gate bits and the
    sort keys in the workspace included - bit for bit; ragged sizes (a partial last workgroup), every SH degree."""
    w, h = 640, 360
    arrays, cam = _scene(pkg, n, w, h, stored, seed=n, mu_s=-4.0)
    model = pkg.scene.to_model(arrays, dev)
    R = pkg.rasterizer
    margs = (model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam, deg, 1.3)
    whole = R.project_gaussians(*margs, key_sort=True)
    halves = R.project_gaussians(*margs, key_sort=True, colour_on_side_stream=True)
    assert halves.colour_ready is not None
    halves.wait_colour()
    assert halves.colour_ready is None
    torch.cuda.synchronize(dev)
    for name in ("means_2d", "depths", "cov_2d_inv", "radii", "tiles_touched", "rgb", "opacities_act", "packed",
                 "colour_gate"):
        a, b = getattr(whole, name), getattr(halves, name)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    ref = oracle_forward(orc, arrays, cam, degree=deg, scale_mod=1.3)
    _assert_projection_equal(halves, ref)
    # and the sort that consumes the keys the geometry half left behind gives the oracle's order
    key = R._skey(torch.device(dev))
    R._last_pairs[key] = ref["total_pairs"]
    R._held_capacity.pop(key, None)
    try:
        halves2 = R.project_gaussians(*margs, key_sort=True, colour_on_side_stream=True)
        pend = R.sort_gaussians_predicted(halves2.means_2d, halves2.depths, halves2.radii, halves2.tiles_touched, w, h,
                                          want_keys=True, keyed_workspace=halves2.sort_workspace)
        srt, valid = pend.finish() if isinstance(pend, R.PendingSort) else (pend, True)
        halves2.wait_colour()
    finally:
        R._last_pairs.pop(key, None)
    assert valid and srt.total_pairs == ref["total_pairs"]
    assert np.array_equal(np_(srt.gaussian_values_sorted), ref["values"])
    assert np.array_equal(np_(srt.tile_ranges), ref["tile_ranges"])


def test_two_renders_in_flight_on_two_streams(pkg, orc, dev):
    """the host-side sort state (workspaces the projection keys, pair-count prediction, held capacity,
    pinned count word) is per (device, STREAM).  Two different scenes are rendered on two torch streams with both
    frames in flight at once (defer_count=True: neither call waits), several rounds; every frame must be the oracle's
    image bit for bit and its own pair count - with one workspace per device the second projection would overwrite the
    sort keys of the first while its sort is still running."""
    R = pkg.rasterizer
    scenes = []
    for n, w, h, deg, seed, mu_s in ((40000, 640, 360, 1, 71, -4.0), (25000, 512, 384, 2, 72, -3.6)):
        arrays, cam = _scene(pkg, n, w, h, deg, seed=seed, mu_s=mu_s)
        ref = oracle_forward(orc, arrays, cam, degree=deg)
        scenes.append((pkg.scene.to_model(arrays, dev), cam, pkg.RenderSettings(active_sh_degree=deg), ref))
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    torch.cuda.synchronize(dev)
    keys = []
    for st, (model, cam, settings, ref) in zip(streams, scenes):          # seed each stream's prediction (blocking)
        with torch.cuda.stream(st):
            out = pkg.render(model, cam, settings)
            keys.append(R._skey(torch.device(dev)))
            assert out.total_pairs == ref["total_pairs"]
    assert keys[0] != keys[1] and all(k in R._last_pairs for k in keys)
    assert R._workspaces[(keys[0], "n")].data_ptr() != R._workspaces[(keys[1], "n")].data_ptr()
    for _round in range(4):
        outs = []
        for st, (model, cam, settings, ref) in zip(streams, scenes):      # both queued before either is waited for
            with torch.cuda.stream(st):
                outs.append(pkg.render(model, cam, settings, defer_count=True))
        for st, out, (model, cam, settings, ref) in zip(streams, outs, scenes):
            with torch.cuda.stream(st):
                assert out.pending is not None
                out.wait()
                st.synchronize()
            assert out.total_pairs == ref["total_pairs"]
            assert np.array_equal(np_(out.gaussian_indices), ref["values"])
            assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"])
            assert np.array_equal(np_(out.n_contrib), ref["n_contrib"])
            assert np.array_equal(np_(out.color).view(np.uint32), ref["color"].view(np.uint32))
    for k in keys:                                                        # leave no state behind for dead streams
        R._last_pairs.pop(k, None); R._held_capacity.pop(k, None)
        R._workspaces.pop((k, "n"), None); R._workspaces.pop((k, "p"), None)


def test_deferred_render_of_a_view_outside_the_fast_depth_range(pkg, orc, dev):
    """a view whose depths leave [0.2, ~13 107) made every predicted sort report -1: a wasted sort and blend
    plus a blocking re-sort per frame, and render(defer_count=True).wait() raised PredictionMiss on EVERY call while
    telling the caller to render again.  Now the stream remembers (rasterizer._wide_depth): the first deferred render of
    such a view still misses - with a message that says why - and the retry completes on the general depth route with
    the oracle's image; a training loop that follows the message converges in one retry."""
    n, w, h, deg, scale = 20000, 640, 360, 1, 5000.0
    arrays, cam = _scene(pkg, n, w, h, deg, seed=43, mu_s=-4.0)
    arrays = dict(arrays)
    arrays["positions"] = (arrays["positions"] * np.float32(scale)).astype(np.float32)
    arrays["scales"] = (arrays["scales"] + np.float32(np.log(scale))).astype(np.float32)
    ref = oracle_forward(orc, arrays, cam, degree=deg)
    assert ref["depths"][ref["tiles_touched"] > 0].max() > 13107.0
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=deg)
    R = pkg.rasterizer
    key = R._skey(torch.device(dev))
    R._wide_depth.pop(key, None)
    first = pkg.render(model, cam, settings)                      # blocking: seeds the prediction; route not yet known
    assert first.total_pairs == ref["total_pairs"]
    miss = pkg.render(model, cam, settings, defer_count=True)
    with pytest.raises(pkg.PredictionMiss, match="general"):
        miss.wait()
    assert R._wide_depth.get(key, 0) > 0
    renders = 0
    while True:                                                   # what a training loop does with a PredictionMiss
        renders += 1
        assert renders <= 2
        out = pkg.render(model, cam, settings, defer_count=True)
        try:
            out.wait()
            break
        except pkg.PredictionMiss:
            continue
    assert renders == 1
    assert out.total_pairs == ref["total_pairs"]
    assert np.array_equal(np_(out.gaussian_indices), ref["values"])
    assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"])
    assert np.array_equal(np_(out.color).view(np.uint32), ref["color"].view(np.uint32))
    # the non-deferred render on the sticky route: no re-sort either (the pending sort it finishes is valid)
    again = pkg.render(model, cam, settings)
    assert np.array_equal(np_(again.color).view(np.uint32), ref["color"].view(np.uint32))
    # the bit expires: after WIDE_DEPTH_HOLD sorts the narrow route is probed again
    R._wide_depth[key] = 1
    pkg.render(model, cam, settings)                              # last sort on the general route
    assert R._wide_depth.get(key, 0) == 0
    probe = pkg.render(model, cam, settings)                      # probes the three-pass route: -1 again -> sticky again
    assert R._wide_depth.get(key, 0) == R.WIDE_DEPTH_HOLD
    assert np.array_equal(np_(probe.color).view(np.uint32), ref["color"].view(np.uint32))


def test_early_colour_gather_equals_compact_exchange(pkg, orc, dev):
    """Data-parallel exchange with the colour gather started before the projection backward
    (render_backward(..., on_gated_ready=...) + parallel.begin_colour_gather / finish_exchange): the gated colour
    gradient made by cugs_gated_colour_grad from the accumulator rows is the tensor the projection backward writes,
    bit for bit; geometry gradients and the rebuilt SH gradient equal the compact exchange's; the hook runs BEFORE
    the projection backward is queued (the geometry buffer is still untouched when it fires)."""
    n, w, h, deg = 30000, 640, 360, 3
    arrays, cam = _scene(pkg, n, w, h, deg, seed=61, mu_s=-4.0)
    settings = pkg.RenderSettings(background=[0.2, 0.1, 0.3], active_sh_degree=deg)
    model = pkg.scene.to_model(arrays, dev)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=62)).to(dev)
    centre = cam.camera_center().tolist()
    # compact exchange (gated gradient written by the projection backward)
    gated_a, flat_a = torch.empty((n, 3), device=dev), torch.empty((11 * n,), device=dev)
    ga = pkg.render_backward(g, pkg.render(model, cam, settings), model, cam, settings, dL_drgb_gated_out=gated_a,
                             geom_flat=flat_a)
    ga = pkg.parallel.exchange_gradients(ga, gated_a, model.positions, centre, deg, 16, all_cam_centers=[centre])
    # early gather
    gated_b = torch.full((n, 3), float("nan"), device=dev)
    flat_b = torch.full((11 * n,), float("nan"), device=dev)
    seen = {}
    def hook(t):
        seen["same_tensor"] = t.data_ptr() == gated_b.data_ptr()
        seen["flat_untouched"] = bool(torch.isnan(flat_b).all())          # synchronises: nothing queued behind yet
        seen["gated"] = t.clone()
        seen["gather"] = pkg.parallel.begin_colour_gather(t)
    gb = pkg.render_backward(g, pkg.render(model, cam, settings), model, cam, settings, dL_drgb_gated_out=gated_b,
                             geom_flat=flat_b, on_gated_ready=hook)
    assert seen["same_tensor"] and seen["flat_untouched"]
    assert gb.dL_dsh_coeffs is None
    gb = pkg.parallel.finish_exchange(gb, seen["gather"], model.positions, deg, 16, all_cam_centers=[centre])
    # two backward blends of the same frame differ in the last bits (atomic summation order): 1e-5 here, bit
    # equality on ONE accumulator below
    close = lambda a, b: float((a - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-30)
    assert torch.equal(seen["gated"], gated_b) and close(gated_b, gated_a)
    assert float(gated_a.abs().max()) > 0 and int((gated_a == 0).all(dim=1).sum()) > 0      # gates / culled rows present
    assert torch.equal((gated_b == 0), (gated_a == 0))
    assert close(flat_b, flat_a) and close(gb.dL_dsh_coeffs, ga.dL_dsh_coeffs) and close(gb.dL_dmeans_2d, ga.dL_dmeans_2d)
    # one accumulator, both producers of the gated gradient: the same bits; geometry gradients too
    out = pkg.render(model, cam, settings)
    rb = pkg.rasterizer.rasterize_backward(g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                           out.gaussian_indices, out.final_T, out.n_contrib, w, h, settings.background,
                                           n, packed=out.packed, unpack=False)
    early = pkg.rasterizer.gated_colour_grad(rb.grad_accum, out.colour_gate)
    outs = []
    for gated_out in (torch.empty((n, 3), device=dev), None):
        flat = torch.empty((11 * n,), device=dev)
        pkg.rasterizer.project_backward(None, None, None, None, model.positions, model.rotations, model.scales,
                                        model.opacities, model.sh_coeffs, out.radii, cam, deg, 1.0,
                                        grad_accum=rb.grad_accum, colour_gate=out.colour_gate,
                                        dL_drgb_gated_out=gated_out, skip_sh_grad=True, geom_flat=flat)
        outs.append((gated_out, flat))
    assert torch.equal(early, outs[0][0]) and torch.equal(outs[0][1], outs[1][1])
    # the stage function on its own, and its argument checks
    rb_acc = torch.randn((100, 16), device=dev)
    gate = torch.randint(0, 8, (100,), dtype=torch.uint8, device=dev)
    got = pkg.rasterizer.gated_colour_grad(rb_acc, gate)
    bits = torch.stack([(gate >> k) & 1 for k in range(3)], dim=1).to(torch.float32)
    assert torch.equal(got, rb_acc[:, :3] * bits)
    with pytest.raises(RuntimeError):
        pkg.rasterizer.gated_colour_grad(rb_acc, gate[:50])


def test_two_deferred_renders_in_flight(pkg, orc, dev):
    """Two render(defer_count=True) calls before the first render_backward (views accumulated before one optimizer
    step), with a blocking render in between: each sort's pair count arrives in a pinned word of its own, so every
    output is judged by, and trimmed to, its OWN count - with one word per device the later sort overwrote it."""
    w, h, deg = 640, 360, 1
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=deg)
    arr_a, cam = _scene(pkg, 20000, w, h, deg, seed=51, mu_s=-3.9)
    arr_b, _ = _scene(pkg, 12000, w, h, deg, seed=52, mu_s=-4.4)
    ma, mb = pkg.scene.to_model(arr_a, dev), pkg.scene.to_model(arr_b, dev)
    ref_a, ref_b = pkg.render(ma, cam, settings), pkg.render(mb, cam, settings)
    assert ref_a.total_pairs != ref_b.total_pairs
    pkg.render(ma, cam, settings)                                # the prediction covers the larger view
    out_a = pkg.render(ma, cam, settings, defer_count=True)
    out_b = pkg.render(mb, cam, settings, defer_count=True)
    mid = pkg.render(mb, cam, settings)                          # blocking, while both counts are unread
    assert out_a.pending is not None and out_b.pending is not None
    assert out_a.pending._slot.tensor.data_ptr() != out_b.pending._slot.tensor.data_ptr()
    out_a.wait(), out_b.wait()
    assert out_a.total_pairs == ref_a.total_pairs and out_b.total_pairs == ref_b.total_pairs
    assert mid.total_pairs == ref_b.total_pairs
    assert torch.equal(out_a.gaussian_indices, ref_a.gaussian_indices)
    assert torch.equal(out_b.gaussian_indices, ref_b.gaussian_indices)
    assert torch.equal(out_a.color, ref_a.color) and torch.equal(out_b.color, ref_b.color)
    # the words went back to the pool: a further render allocates none
    pool = pkg.rasterizer._pinned[torch.device(dev)]
    held = len(pool)
    pkg.render(ma, cam, settings, defer_count=True).wait()
    assert len(pool) == held


@pytest.mark.parametrize("scale", [1.0, 0.02, 5000.0])
def test_depth_sort_routes(pkg, orc, dev, scale):
    """The depth ordering runs three 9-bit passes on the key's offset from the near plane when every splat that emits
    pairs has its depth in [0.2, ~13 000), and falls back to four 8-bit passes on the raw float bits otherwise -
    decided on the device, reported through the pair count (-1).  Depths scaled below the near plane and beyond the
    range must come out in the oracle's order just the same, through the blocking and the predicted entry points."""
    n, w, h = 30000, 640, 360
    arrays, cam = _scene(pkg, n, w, h, 0, seed=41, mu_s=-4.0)
    ref = oracle_forward(orc, arrays, cam, degree=0)
    depths = (ref["depths"] * np.float32(scale)).astype(np.float32)
    srt_ref = orc.sort(ref["means_2d"], depths, ref["radii"], ref["tiles_touched"], w, h)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (t(ref["means_2d"]), t(depths), t(ref["radii"]), t(ref["tiles_touched"]), w, h)
    R = pkg.rasterizer
    srt = pkg.sort_gaussians(*args)
    R._last_pairs[R._skey(torch.device(dev))] = srt.total_pairs
    R._held_capacity.pop(R._skey(torch.device(dev)), None)
    try:
        pend = R.sort_gaussians_predicted(*args, want_keys=True)
        srt2, valid = pend.finish()
        in_range = depths[ref["tiles_touched"] > 0]
        narrow = bool(in_range.min() > 0.2 and in_range.max() < 13000.0)
        assert valid == narrow
        # a view outside the three-pass range is remembered (sticky per stream): the NEXT predicted sort takes the
        # general route at once - valid, no -1, no blocking re-sort - and the blocking entry skips the wasted attempt
        assert (R._wide_depth.get(R._skey(torch.device(dev)), 0) > 0) == (not narrow)
        pend3 = R.sort_gaussians_predicted(*args, want_keys=True)
        srt3, valid3 = pend3.finish()
        assert valid3
        srt4 = pkg.sort_gaussians(*args, wide_depth=True)
    finally:
        R._last_pairs.pop(R._skey(torch.device(dev)), None)
        R._wide_depth.pop(R._skey(torch.device(dev)), None)
    for out in (srt, srt2, srt3, srt4):
        assert out.total_pairs == srt_ref["total_pairs"]
        assert np.array_equal(np_(out.gaussian_keys_sorted).view(np.uint64), srt_ref["keys"])
        assert np.array_equal(np_(out.gaussian_values_sorted), srt_ref["values"])
        assert np.array_equal(np_(out.tile_ranges), srt_ref["tile_ranges"])


@pytest.mark.parametrize("scale", [1.0, 5000.0])
def test_projection_keys_the_sort(pkg, orc, dev, scale):
    """render()'s route: cugs_project_forward_keyed leaves the sort's depth keys / tile rectangles in the sort
    workspace and cugs_sort_pairs_predicted_keyed skips the key kernel.  The projection's own outputs must not change
    by a bit, the sort must give the oracle's keys, order and ranges, and a scene whose depths leave the range of the
    three-pass depth ordering (everything 5000 times farther and larger: the same image) must be reported through the
    pair count and recovered by the general route, exactly as on the unkeyed path."""
    n, w, h, deg = 30000, 640, 360, 1
    arrays, cam = _scene(pkg, n, w, h, deg, seed=43, mu_s=-4.0)
    arrays = dict(arrays)
    arrays["positions"] = (arrays["positions"] * np.float32(scale)).astype(np.float32)
    arrays["scales"] = (arrays["scales"] + np.float32(np.log(scale))).astype(np.float32)
    ref = oracle_forward(orc, arrays, cam, degree=deg)
    model = pkg.scene.to_model(arrays, dev)
    R = pkg.rasterizer
    margs = (model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam, deg)
    plain = R.project_gaussians(*margs)
    assert plain.sort_workspace is None
    d = torch.device(dev)
    R._last_pairs[R._skey(d)] = ref["total_pairs"]
    R._held_capacity.pop(R._skey(d), None)
    try:
        keyed = R.project_gaussians(*margs, key_sort=True)
        pend = R.sort_gaussians_predicted(keyed.means_2d, keyed.depths, keyed.radii, keyed.tiles_touched, w, h,
                                          want_keys=True, keyed_workspace=keyed.sort_workspace)
        assert isinstance(pend, R.PendingSort)
        srt, valid = pend.finish()
    finally:
        R._last_pairs.pop(R._skey(d), None)
        R._wide_depth.pop(R._skey(d), None)
    _assert_projection_equal(keyed, ref)
    for name in ("means_2d", "depths", "cov_2d_inv", "radii", "tiles_touched", "rgb", "opacities_act", "packed", "colour_gate"):
        assert torch.equal(getattr(keyed, name), getattr(plain, name)), name
    in_range = ref["depths"][ref["tiles_touched"] > 0]
    assert valid == bool(in_range.min() > 0.2 and in_range.max() < 13000.0) == (scale == 1.0)
    assert srt.total_pairs == ref["total_pairs"] > 0
    assert np.array_equal(np_(srt.gaussian_keys_sorted).view(np.uint64), ref["keys"])
    assert np.array_equal(np_(srt.gaussian_values_sorted), ref["values"])
    assert np.array_equal(np_(srt.tile_ranges), ref["tile_ranges"])
    # and the whole frame through render(), which takes this route from its second call on a device
    settings = pkg.RenderSettings(active_sh_degree=deg)
    for _ in range(2):
        out = pkg.render(model, cam, settings)
        assert out.total_pairs == ref["total_pairs"]
        assert np.array_equal(np_(out.gaussian_indices), ref["values"])
        assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"])
        assert np.array_equal(np_(out.color).view(np.uint32), ref["color"].view(np.uint32))
