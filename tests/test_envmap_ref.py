"""tests/envmap_ref.py, the numpy mirrors of csrc/envmap.hip, checked against the mathematics (no GPU): the octahedral
map and its inverse, exactness on a uniform map, continuity across the fold lines (which a clamp breaks), the analytic
gradients against central differences, the float32 mirror against the fp64 one, and the order-independence of the
fixed-point sum."""
import numpy as np
import pytest

import envmap_ref as er

F32, F64 = np.float32, np.float64
# max |B32 - B64| measured over er.cases() on maps with values in [0, 1): 8.78e-7 (a float32 error of the texel
# coordinate times the texel-to-texel slope); the bar is 4x that
F32_VS_F64 = 4 * 8.78e-7


def test_direction_round_trip_on_both_hemispheres():
    rng = np.random.default_rng(1)
    d = rng.standard_normal((4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert (d[:, 2] > 0.1).sum() > 500 and (d[:, 2] < -0.1).sum() > 500
    x, y = er.dir_to_xy64(d)
    assert np.abs(x).max() <= 1.0 and np.abs(y).max() <= 1.0
    back = er.xy_to_dir64(x, y)
    assert np.abs(back - d).max() < 1e-12
    # and the other way round, from the square
    xs, ys = rng.uniform(-1, 1, 4000), rng.uniform(-1, 1, 4000)
    x2, y2 = er.dir_to_xy64(er.xy_to_dir64(xs, ys))
    assert np.abs(x2 - xs).max() < 1e-12 and np.abs(y2 - ys).max() < 1e-12
    # the poles: +z is the centre of the map, -z its corner (sgn(0) = +1)
    assert er.dir_to_xy64(np.array([0.0, 0.0, 2.0])) == (0.0, 0.0)
    assert er.dir_to_xy64(np.array([0.0, 0.0, -3.0])) == (1.0, 1.0)


def test_fold_stays_inside_and_is_an_involution_on_the_border():
    for res in (4, 16, 2048):
        i, j = np.meshgrid(np.arange(-1, res + 1), np.arange(-1, res + 1))
        i, j = i.reshape(-1), j.reshape(-1)
        idx = er.fold(i, j, res)
        assert idx.min() >= 0 and idx.max() < res * res
        inside = (i >= 0) & (i < res) & (j >= 0) & (j < res)
        assert (idx[inside] == (j * res + i)[inside]).all()
        # the texel beyond the left edge of row j is the edge texel of row R - 1 - j (the same point of the sphere)
        rows = np.arange(res)
        assert (er.fold(np.full(res, -1), rows, res) == (res - 1 - rows) * res).all()
        assert (er.fold(rows, np.full(res, res), res) == (res - 1) * res + (res - 1 - rows)).all()


def test_uniform_map_samples_to_exactly_its_colour():
    colour = np.array([0.1, 0.7, 0.3333333], F32)
    for label, h, w, res, cam, orient in er.cases():
        E = np.broadcast_to(colour.reshape(3, 1, 1), (3, res, res)).copy()
        B = er.sample32(E, er.taps32(cam, res, orient), h, w)
        assert (B == colour).all(), label


def _fold_line_pairs(delta):
    """(d_a, d_b): directions a hair either side of the four fold lines of the lower hemisphere (n_y = 0 with n_x < 0 and
    > 0: the edges x = -1, +1; n_x = 0: the edges y = -1, +1) and of the z = 0 diamond."""
    ts = np.linspace(0.07, 0.93, 23)
    a, b = [], []
    for t in ts:
        for sx in (-1.0, 1.0):
            a.append([sx * t, +delta, -(1 - t)]); b.append([sx * t, -delta, -(1 - t)])
            a.append([+delta, sx * t, -(1 - t)]); b.append([-delta, sx * t, -(1 - t)])
            for sy in (-1.0, 1.0):
                a.append([sx * t, sy * (1 - t), +delta]); b.append([sx * t, sy * (1 - t), -delta])
    return np.array(a), np.array(b)


@pytest.mark.parametrize("res", [4, 8, 16])
def test_sampling_is_continuous_across_the_fold_lines_and_a_clamp_is_not(res):
    rng = np.random.default_rng(res)
    E = rng.random((3, res, res))
    da, db = _fold_line_pairs(1e-7)
    na, nb = da / np.abs(da).sum(1, keepdims=True), db / np.abs(db).sum(1, keepdims=True)
    # B is bilinear with a slope of at most `variation` per texel along each axis; the octahedral map takes an L1 step
    # on the octahedron to at most that L1 step in (x, y), and a texel is 2 / R of the square
    texels = 0.5 * res * np.abs(na - nb).sum(1)
    variation = E.max() - E.min()
    bound = 2.0 * variation * texels[:, None] + 1e-12
    diff = np.abs(er.sample_dirs64(E, da) - er.sample_dirs64(E, db))
    assert (diff <= bound).all(), (diff.max(), bound.max())
    clamp = np.abs(er.sample_dirs64(E, da, "clamp") - er.sample_dirs64(E, db, "clamp"))
    assert (clamp > 1e3 * bound).any()                        # the clamp variant jumps at the fold lines


def test_fp64_gradients_equal_central_differences():
    h, w, res = er.SHAPES[0][0], er.SHAPES[0][1], 4
    for name in ("-z", "oblique"):
        cam = er.cameras(h, w)[name]
        E32, C32, T32, g32 = er.case_data(h, w, res)
        E, C, T, g = E32.astype(F64), C32.astype(F64).reshape(-1, 3), T32.astype(F64).reshape(-1), g32.astype(F64).reshape(-1, 3)
        taps = er.taps64(cam, res)
        per_pixel = lambda E_, T_: (g * (C + T_[:, None] * er.sample64(E_, taps))).sum(axis=1)
        d_alpha, d_env = er.backward64(E, taps, g, T)
        # alpha = 1 - T: every pixel's loss depends on its own T only, so one perturbation serves all pixels
        step = 0.25
        num_alpha = -(per_pixel(E, T + step) - per_pixel(E, T - step)) / (2 * step)
        assert np.abs(num_alpha - d_alpha).max() <= 1e-9 * np.abs(d_alpha).max()
        num_env = np.empty_like(d_env)
        for c in range(3):
            for j in range(res):
                for i in range(res):
                    hi, lo = E.copy(), E.copy()
                    hi[c, j, i] += step
                    lo[c, j, i] -= step
                    num_env[c, j, i] = (per_pixel(hi, T).sum() - per_pixel(lo, T).sum()) / (2 * step)
        assert np.abs(num_env - d_env).max() <= 1e-9 * np.abs(d_env).max()
        assert (d_env != 0).sum() > res * res                # the view reaches a good part of the map


def test_float32_mirror_stays_near_the_fp64_one():
    worst = 0.0
    for label, h, w, res, cam, orient in er.cases():
        E, C, T, g = er.case_data(h, w, res)
        B32 = er.sample32(E, er.taps32(cam, res, orient), h, w)
        B64 = er.sample64(E, er.taps64(cam, res, orient)).reshape(h, w, 3)
        worst = max(worst, float(np.abs(B32.astype(F64) - B64).max()))
    print(f"max |B32 - B64| = {worst:.3e}")
    assert worst <= F32_VS_F64


def test_fixed_point_sum_does_not_depend_on_the_pixel_order():
    h, w, res = er.SHAPES[1][0], er.SHAPES[1][1], 4
    cam = er.cameras(h, w)["oblique"]
    E, C, T, g = er.case_data(h, w, res)
    taps = er.taps32(cam, res)
    grad, table, clamped = er.denv32(taps, g, T, res, grad_bound=1.0)
    assert clamped == 0 and (table != 0).any()
    rng = np.random.default_rng(5)
    for _ in range(3):
        grad2, table2, _ = er.denv32(taps, g, T, res, grad_bound=1.0, order=rng.permutation(h * w))
        assert (table2 == table).all() and grad2.tobytes() == grad.tobytes()
    # against the fp64 sum: each share carries one float32 rounding and 2^-F of quantisation
    ref = er.backward64(E.astype(F64), er.taps64(cam, res), g.astype(F64).reshape(-1, 3), T.astype(F64).reshape(-1))[1]
    assert np.abs(grad - ref).max() <= 1e-5 * np.abs(ref).max()
    # a bound below max |T g|: shares are clamped, the flag is raised and every sum stays far from overflow
    grad3, table3, clamped3 = er.denv32(taps, g, T, res, grad_bound=2.0 ** -6)
    assert clamped3 == 1 and np.abs(table3).max() < 2 ** 61 and np.isfinite(grad3).all()


def test_frac_bits_leave_room_for_every_sum():
    assert er.frac_bits(1080, 1920, 1.0) == (61 - 23 - 0, 0)
    assert er.frac_bits(17, 33, 0.3) == (61 - 12 + 1, -1)
    assert er.frac_bits(17, 33, 0.5) == (61 - 12 + 1, -1) and er.frac_bits(17, 33, 0.51)[1] == 0
    for h, w, bound in ((17, 33, 1.0), (1080, 1920, 4.0 / (3 * 1080 * 1920)), (4096, 4096, 100.0)):
        fb, e = er.frac_bits(h, w, bound)
        assert 2.0 ** e >= bound > 2.0 ** (e - 1)
        assert 4 * h * w * 2.0 ** e * 2.0 ** fb < 2.0 ** 61
