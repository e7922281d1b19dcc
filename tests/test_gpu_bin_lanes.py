"""k_bin_scatter<false>'s walk (sort_bin.h): hits are buffered 64 at a time, lane = hit forms the cover mask of the wave's
8 x 8 tile block, a 64 x 64 bit transpose across the wave makes lane = tile, and every tile lane pops its own hits in
depth order.  The scenes below are the smallest at which that can go wrong - batches that fill exactly, batches that fill
across candidate lists and groups, rectangles clipped by block borders, partial blocks, full-block covers between
single-tile ones, records without a rectangle - each through render()'s keyed, predicted sort with a capacity of exactly
the pair count (below 13 pairs per Gaussian, so the direct and not the staged variant runs), against the oracle, bit for bit.

Splats are placed at chosen pixels: identity camera, x = (px - cx) z / fx, isotropic scale sigma_px z / fx.  A splat with
sigma_px = 0.5 has a 3-pixel radius: centred in a tile it covers that tile alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from util import np_

pytestmark = pytest.mark.gpu

T = 16                      # tile edge in pixels
STAGE_RATIO = 13            # sort_workspace.h BIN_STAGE_RATIO: the staged variant runs from this many pairs per Gaussian


def _scene(px, py, sigma_px, z, w, h, opacity=-4.0):
    """Arrays of make_gaussians' layout (SH degree 0) for splats centred at pixel (px, py), depth z, footprint sigma_px."""
    px, py, sigma_px, z = (np.asarray(a, np.float64) for a in np.broadcast_arrays(px, py, sigma_px, z))
    n = px.shape[0]
    fx = 0.78 * w                                                   # scene.FOCAL_RATIO
    pos = np.stack([(px - w / 2.0) * z / fx, (py - h / 2.0) * z / fx, z], axis=1).astype(np.float32)
    scales = np.repeat(np.log(sigma_px * np.abs(z) / fx)[:, None], 3, axis=1).astype(np.float32)
    rot = np.zeros((n, 4), np.float32); rot[:, 0] = 1.0
    rng = np.random.Generator(np.random.Philox(key=n + w))
    sh = (0.5 * rng.standard_normal((n, 3, 1))).astype(np.float32)
    return dict(positions=pos, sh_coeffs=sh, opacities=np.full((n, 1), opacity, np.float32), rotations=rot, scales=scales)


def _depths(n, seed):
    """n distinct depths in [2, 6) in a shuffled order: depth order is not index order."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    return 2.0 + 4.0 * rng.permutation(n) / n


def _centre(tx, ty):
    return np.asarray(tx) * T + T / 2, np.asarray(ty) * T + T / 2


def same_tile(n):
    px, py = _centre(np.full(n, 3), np.full(n, 5))
    return _scene(px, py, 0.5, _depths(n, n), 128, 128), 128, 128


def all_tiles(n):
    rng = np.random.Generator(np.random.Philox(key=1000 + n))
    t = np.concatenate([rng.permutation(64) for _ in range((n + 63) // 64)])[:n]
    px, py = _centre(t % 8, t // 8)
    return _scene(px, py, 0.5, _depths(n, n + 1), 128, 128), 128, 128


def carry_over(n):
    """200 x 136: 13 x 9 tiles, one window of two blocks.  Every 29th to 31st splat lies in the second block (5 tile columns), the
    others in the first: the second block's wave finds 1-3 hits per 64 candidates and fills a batch across slice lists and
    groups; the first block's wave overflows its batch on nearly every iteration."""
    rng = np.random.Generator(np.random.Philox(key=2000 + n))
    second = np.zeros(n, bool)
    second[np.cumsum(rng.integers(29, 32, n // 28))[:n // 31]] = True
    tx = np.where(second, rng.integers(8, 13, n), rng.integers(0, 8, n))
    ty = rng.integers(0, 8, n)
    px, py = _centre(tx, ty)
    return _scene(px, py, 0.5, _depths(n, n + 2), 200, 136), 200, 136


def straddle():
    """Rectangles across the block borders of a 13 x 9-tile image (x = 128, y = 128) and its corner, between single-tile
    splats on both sides; sigma 0.5 and 4 = radius 3 and 13: two tiles across a border, four around the corner."""
    rng = np.random.Generator(np.random.Philox(key=3000))
    n = 300
    px, py = _centre(rng.integers(0, 13, n), rng.integers(0, 9, n))
    sig = np.full(n, 0.5)
    k = np.arange(0, n, 3)
    which = np.arange(k.shape[0]) % 3
    px[k] = np.where(which == 1, px[k], 128.0)                      # x border, y border, corner in turn
    py[k] = np.where(which == 0, py[k], 128.0)
    sig[k] = np.where(np.arange(k.shape[0]) % 2 == 0, 0.5, 4.0)
    return _scene(px, py, sig, _depths(n, 3001), 200, 136), 200, 136


def ragged(w, h, n, seed):
    """Splats of one to a few tiles anywhere on an image whose last blocks are partial."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    px, py = rng.uniform(0, w, n), rng.uniform(0, h, n)
    sig = np.where(rng.uniform(0, 1, n) < 0.3, 5.0, 0.5)
    return _scene(px, py, sig, _depths(n, seed + 1), w, h), w, h


def mix(equal_depth):
    """Screen-filling splats (64 pairs per hit) every 31st in depth between single-tile ones; and, unless all depths are to
    be equal, records without a rectangle (inside the near plane) and quirk-Q12 splats (past the bottom-right corner)."""
    rng = np.random.Generator(np.random.Philox(key=4000 + equal_depth))
    n = 330
    px, py = _centre(rng.integers(0, 8, n), rng.integers(0, 8, n))
    sig = np.full(n, 0.5)
    z = np.full(n, 4.0) if equal_depth else _depths(n, 4002)
    big = np.arange(7, n, 31)
    sig[big] = 100.0
    if not equal_depth:
        z[np.arange(3, n, 11)] = 0.1                                # radius 0
        q12 = np.arange(5, n, 23)
        px[q12] = 128.0 + 40.0; py[q12] = 128.0 + 40.0; sig[q12] = 0.5
    return _scene(px, py, sig, z, 128, 128), 128, 128


def cluster():
    """4000 splats of one group inside one 8 x 8 tile block of a 8 x 24-tile image (three windows: the middle one holds
    nearly everything, so the workgroups run window-major), 100 more elsewhere."""
    rng = np.random.Generator(np.random.Philox(key=5000))
    n = 4100
    tx, ty = rng.integers(0, 8, n), rng.integers(8, 16, n)
    rest = rng.permutation(n)[:100]
    ty[rest] = rng.integers(0, 24, 100)
    px, py = _centre(tx, ty)
    return _scene(px, py, 0.5, _depths(n, 5001), 128, 384), 128, 384


CASES = {}
for _n in (63, 64, 65, 127, 128, 129):
    CASES[f"same_tile_{_n}"] = (same_tile, (_n,))
    CASES[f"all_tiles_{_n}"] = (all_tiles, (_n,))
for _n in (4095, 4096, 4097, 8193):
    CASES[f"carry_over_{_n}"] = (carry_over, (_n,))
CASES["straddle"] = (straddle, ())
CASES["ragged_1040x64"] = (ragged, (1040, 64, 600, 6000))          # 65 x 4 tiles: two windows, a last block one tile wide
CASES["ragged_200x136"] = (ragged, (200, 136, 500, 6100))          # 13 x 9 tiles
CASES["mix"] = (mix, (False,))
CASES["mix_equal_depth"] = (mix, (True,))
CASES["cluster"] = (cluster, ())


def _reference(pkg, orc, arrays, w, h):
    cam = pkg.scene.make_camera(w, h)
    K = cam.intrinsics
    ref = orc.render(arrays, cam.rotation, cam.translation, K.fx, K.fy, K.cx, K.cy, w, h, active_degree=0,
                     threads=orc.host_threads())
    return cam, ref


def check_design(name, arrays, w, h, ref):
    """What each scene was built to contain (host only: the oracle's numbers)."""
    n = arrays["positions"].shape[0]
    tr = ref["tile_ranges"]
    counts = tr[:, 1] - tr[:, 0]
    assert 0 < ref["total_pairs"] < STAGE_RATIO * n                 # the direct variant
    if name.startswith("same_tile"):
        assert counts.max() == n == ref["total_pairs"]              # one tile's bits fill whole batches
    if name.startswith("all_tiles"):
        assert (counts > 0).sum() == min(n, 64) and ref["total_pairs"] == n
    if name.startswith("carry_over"):
        ntx = 13
        second = sum(int(counts[ty * ntx + 8: ty * ntx + 13].sum()) for ty in range(8))
        assert ref["total_pairs"] == n and 64 < second < n // 25
    if name == "straddle":
        assert int((ref["tiles_touched"] == 4).sum()) >= 10 and int((ref["tiles_touched"] == 2).sum()) >= 20
    if name == "mix":
        assert int((ref["tiles_touched"] == 64).sum()) >= 10 and int((ref["radii"] == 0).sum()) >= 25
        assert int((ref["keys"] == 0).sum()) > 0                    # quirk Q12's zero pairs
    if name == "mix_equal_depth":
        assert int((ref["tiles_touched"] == 64).sum()) >= 10 and np.unique(ref["depths"]).shape[0] == 1
    if name == "cluster":
        mid = int(counts[8 * 8: 16 * 8].sum())
        assert mid >= 4000 and 3 * mid > 2 * ref["total_pairs"]     # the window-major order's condition


@pytest.mark.parametrize("name", list(CASES))
def test_direct_scatter_matches_the_oracle(pkg, orc, dev, name):
    fn, args = CASES[name]
    arrays, w, h = fn(*args)
    cam, ref = _reference(pkg, orc, arrays, w, h)
    check_design(name, arrays, w, h, ref)
    R = pkg.rasterizer
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=0)
    key = R._skey(torch.device(dev))
    margin = R.PREDICT_MARGIN
    R.PREDICT_MARGIN = (1.0, 0)                                     # capacity = the pair count: the variant follows the view
    try:
        for frame in range(2):
            R._last_pairs[key] = ref["total_pairs"]
            R._held_capacity.pop(key, None)
            out = pkg.render(model, cam, settings)
            assert out.total_pairs == ref["total_pairs"], frame
            assert np.array_equal(np_(out.gaussian_indices), ref["values"]), frame
            assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"]), frame
            assert np.array_equal(np_(out.n_contrib), ref["n_contrib"]), frame
    finally:
        R.PREDICT_MARGIN = margin
        R._last_pairs.pop(key, None)
        R._held_capacity.pop(key, None)


def test_a_miss_leaves_the_index_buffer_untouched(pkg, orc, dev):
    """A capacity below the pair count, through the stage-level entry with an index buffer of our own: the count is reported,
    every range is {0,0}, and not one word of the buffer - sentinel-filled, larger than the true count - is written."""
    R = pkg.rasterizer
    lib = R.lib
    arrays, w, h = ragged(200, 136, 500, 6100)
    cam, ref = _reference(pkg, orc, arrays, w, h)
    p = ref["total_pairs"]
    model = pkg.scene.to_model(arrays, dev)
    n, tiles = 500, ((w + T - 1) // T) * ((h + T - 1) // T)
    sentinel = 0x5A5A5A5A
    vals = torch.full((p + 256,), sentinel, dtype=torch.int32, device=dev)
    for cap, hit in ((p // 2, False), (p - 1, False), (p, True)):
        vals.fill_(sentinel)
        keyed = R.project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam, 0,
                                    key_sort=True)                  # (a sort consumes the keys the projection left: one each)
        tile_ranges = torch.full((tiles, 2), -1, dtype=torch.int32, device=dev)
        wp = R._workspace(dev, lib.cugs_sort_pair_workspace_bytes(cap), "p")
        slot = R._pinned_total(dev)
        tiles_c = keyed.tiles_touched.contiguous().to(torch.int32)
        R.check(lib.cugs_sort_pairs_predicted_keyed(
            n, cap, R._ptr(keyed.means_2d), R._ptr(keyed.depths), R._ptr(keyed.radii), R._ptr(tiles_c), w, h,
            R._ptr(keyed.sort_workspace), keyed.sort_workspace.numel(), R._ptr(wp), wp.numel(), C.c_void_p(0), R._ptr(vals),
            R._ptr(tile_ranges), C.cast(slot.tensor.data_ptr(), C.POINTER(C.c_int64)), R._stream(dev)),
            "cugs_sort_pairs_predicted_keyed")
        torch.cuda.synchronize(dev)
        total = int(slot.tensor[0])
        slot.release()
        assert total == p, cap
        got = np_(vals)
        if hit:
            assert np.array_equal(got[:p], ref["values"]) and np.array_equal(np_(tile_ranges), ref["tile_ranges"])
            assert (got[p:] == sentinel).all()
        else:
            assert (got == sentinel).all(), cap
            assert not np_(tile_ranges).any(), cap
