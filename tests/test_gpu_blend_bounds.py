"""Every live route of the blend backward (k_raster_backward) checked ELEMENT by element against the fp32 bound of each
gradient's own terms (oracle/parity.py: blend_bound_report): |g - r| <= (32 + 4 entries) 2^-24 sum|terms| +
3 2^-24 sum j |terms| (j: the term's depth in its pixel's replay) for every element of the four accumulators (and of
dL_ddepths on the depth-map route), and exactly zero where there are no terms.

Routes: {packed, unpacked} x {colour, depth + alpha maps} x {spatial order, longest-list-first order, a random order of
the tile records} x {accumulator filled by the backward, accumulator cleared by the forward's zero_buf}.
Scenes are built in 3-D (the projection makes the packed records; its outputs are the unpacked inputs) to reach the
kernel's structural edges: list lengths around the flush (1, 2, 3 pending), 64-record sub-batch and 256-record batch
boundaries; opaque stacks whose quads finish at different steps; ragged image edges; clamped alphas; thin needles with
opacities just above 1/255; Gaussians in more than 64 tile lists; and half of each image with zero incoming gradients.
The forward is bit-exact against the oracle on every route (precondition).  Then the chain from the accumulator rows
to the parameters (k_project_backward reading the rows, as render_backward does) against the oracle's projection
backward on the GPU's own unpacked accumulators."""
import math

import numpy as np
import pytest
import torch

from util import check_blend_bounds, load_parity, np_, oracle_blend_terms, oracle_forward

pytestmark = pytest.mark.gpu

STACK_K = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513)
BG = (0.3, 0.1, 0.6)


def _logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p / (1.0 - p))


def _at_pixels(cam, u, v, z, sigma_px, opacity, rng, needle=None):
    """Gaussians whose means project to pixel coordinates (u, v) at depths z with screen sigma ~ sigma_px (SH degree 0).
    needle: (long, short) screen sigmas of randomly rotated needles for those rows where it is not None."""
    K = cam.intrinsics
    n = len(u)
    z = np.asarray(z, np.float64)
    pos = np.stack([(np.asarray(u) - K.cx) * z / K.fx, (np.asarray(v) - K.cy) * z / K.fy, z], axis=1)
    if needle is None:
        s = np.log(np.asarray(sigma_px, np.float64) * z / K.fx)
        scales = np.repeat(s[:, None], 3, axis=1)
        q = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    else:
        long_, short = needle
        scales = np.stack([np.log(long_ * z / K.fx), np.log(short * z / K.fx), np.log(short * z / K.fx)], axis=1)
        q = rng.standard_normal((n, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    return dict(positions=pos.astype(np.float32), sh_coeffs=rng.uniform(-1.0, 1.0, (n, 3, 1)).astype(np.float32),
                opacities=_logit(opacity).reshape(n, 1).astype(np.float32), rotations=q.astype(np.float32),
                scales=scales.astype(np.float32))


def _cat(*parts):
    return {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts], axis=0)) for k in parts[0]}


def _scene(name, pkg):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "stacks":
        # K faint splats on one line of sight in tile i: the four quads of the tile see all K (flush(cnt) with
        # cnt = K mod 4, sub-batches of 64, re-staging at 256); opacity ~0.01 keeps the pixels open through K = 513
        w, h = 16 * len(STACK_K), 16
        cam = pkg.scene.make_camera(w, h)
        parts = []
        for i, k in enumerate(STACK_K):
            u = 16 * i + 8 + rng.uniform(-0.4, 0.4, k)
            v = 8 + rng.uniform(-0.4, 0.4, k)
            parts.append(_at_pixels(cam, u, v, rng.uniform(2.0, 10.0, k), rng.uniform(1.0, 1.3, k),
                                    rng.uniform(0.008, 0.012, k), rng))
        return _cat(*parts), cam
    if name == "early_exit":
        # opaque splats around the tile's central quad corner: pixels finish at different steps, each wave votes
        # itself done at its own step and active_rect shrinks mid-list; a third clamp at alpha = 0.99 (logit +9)
        w, h = 16 * 8, 32
        cam = pkg.scene.make_camera(w, h)
        parts = []
        for i, k in enumerate((3, 6, 17, 40, 64, 65, 90, 130, 5, 9, 33, 70, 100, 129, 12, 1)):
            tx, ty = i % 8, i // 8
            u = 16 * tx + 8 + rng.normal(0.0, 2.5, k)
            v = 16 * ty + 8 + rng.normal(0.0, 2.5, k)
            op = rng.uniform(0.4, 0.9, k)
            op[rng.random(k) < 1.0 / 3.0] = 1.0 / (1.0 + math.exp(-9.0))
            parts.append(_at_pixels(cam, u, v, rng.uniform(2.0, 10.0, k), rng.uniform(0.8, 2.5, k), op, rng))
        return _cat(*parts), cam
    # ragged images: widths 1, 2, 3 (mod 4), heights not a multiple of 8, with needles, faint splats and one splat in
    # more than 64 tile lists where the image has that many tiles
    size = {"ragged_1x1": (1, 1), "ragged_17x3": (17, 3), "ragged_50x21": (50, 21), "ragged_203x131": (203, 131),
            "ragged_129x45": (129, 45)}[name]
    w, h = size
    cam = pkg.scene.make_camera(w, h)
    n = max(60, int(w * h / 12))
    base = pkg.scene.make_gaussians(n, max(w, 8), max(h, 8), sh_degree=0, seed=w * 1000 + h, mu_s=-3.6)
    base["opacities"][rng.random(n) < 1.0 / 3.0] = 9.0                               # clamped alphas
    m = max(8, n // 4)
    needles = _at_pixels(cam, rng.uniform(-2.0, w + 2.0, m), rng.uniform(-2.0, h + 2.0, m), rng.uniform(2.0, 10.0, m),
                         None, (1.0 / 255.0) * (1.0 + 10.0 ** rng.uniform(-4.0, -0.5, m)), rng,
                         needle=(rng.uniform(6.0, 40.0), rng.uniform(0.02, 0.2)))
    parts = [base, needles]
    if w * h > 64 * 256:
        parts.append(_at_pixels(cam, [w / 2.0], [h / 2.0], [3.0], [45.0], [0.05], rng))
    return _cat(*parts), cam


def _incoming(w, h, n_seed, zero_half="left"):
    """dL/dcolour, dL/dD, dL/dA; all three zero on half the image: the left half (whole rows of Gaussians there must
    stay 0.0), or the top half (every stack of the "stacks" scene keeps gradients in its lower quads)."""
    rng = np.random.default_rng(n_seed)
    dC = (rng.standard_normal((h, w, 3)) / (w * h)).astype(np.float32)
    dD = (rng.standard_normal((h, w)) * 0.05 / math.sqrt(w * h)).astype(np.float32)
    dA = (rng.standard_normal((h, w)) * 0.3 / math.sqrt(w * h)).astype(np.float32)
    zero = (slice(None), slice(0, w // 2)) if zero_half == "left" else (slice(0, h // 2), slice(None))
    dC[zero] = 0.0
    dD[zero] = 0.0
    dA[zero] = 0.0
    return dC, dD, dA


def _bits(a):
    return np.ascontiguousarray(np_(a) if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


SCENES = ("stacks", "early_exit", "ragged_1x1", "ragged_17x3", "ragged_50x21", "ragged_129x45", "ragged_203x131")


@pytest.mark.parametrize("scene", SCENES)
def test_blend_backward_routes_element_wise(pkg, orc, dev, scene):
    arrays, cam = _scene(scene, pkg)
    w, h = cam.width, cam.height
    n = arrays["positions"].shape[0]
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=list(BG), active_sh_degree=0)
    out = pkg.render(model, cam, settings, want_depth_map=True)
    ref = oracle_forward(orc, arrays, cam, bg=BG, degree=0)
    assert np.array_equal(np_(out.gaussian_indices), ref["values"])
    assert np.array_equal(np_(out.n_contrib), ref["n_contrib"])
    assert np.array_equal(_bits(out.color), _bits(ref["color"]))
    assert np.array_equal(_bits(out.final_T), _bits(ref["final_T"]))
    entries = np.bincount(ref["values"], minlength=n)
    lists = np.diff(ref["tile_ranges"], axis=1)[:, 0]
    if scene == "stacks":
        assert lists.tolist() == list(STACK_K)                           # each stack alone in its tile list
    if scene == "ragged_203x131":
        assert entries.max() >= 64
    print(f"\n{scene}: {n} Gaussians, {w}x{h}, {int(ref['values'].size)} pairs, max entries {int(entries.max())}")

    dC, dD, dA = _incoming(w, h, n, "top" if scene == "stacks" else "left")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    want_c, mags_c = oracle_blend_terms(orc, ref, dC, BG, n, w, h)
    want_d, mags_d = oracle_blend_terms(orc, ref, dC, BG, n, w, h, dD=dD, dA=dA, depth_route=True)
    silent = (entries > 0) & ~np.any([m["mag"].any(axis=1) for m in mags_d.values()], axis=0)
    print(f"  {int(silent.sum())} listed Gaussians without a single term (their rows must be exactly 0)")
    if scene in ("early_exit", "ragged_203x131"):
        assert silent.sum() > 0
    longest = pkg.rasterizer.tile_order_of(out.tile_ranges, w, h)
    perm = torch.from_numpy(np.random.default_rng(n).permutation(int(longest.shape[0]))).to(dev)
    orders = {"spatial": None, "longest_first": longest, "random": longest[perm].contiguous()}
    assert int(lists.max()) == int(np_(longest)[0, 2] - np_(longest)[0, 1])

    par = load_parity()
    worst, failures = {}, []
    for packed in (True, False):
        src = dict(packed=out.packed) if packed else dict(packed=None)
        for depth in (False, True):
            want, mags = (want_d, mags_d) if depth else (want_c, mags_c)
            for oname, order in orders.items():
                for prezeroed in (False, True):
                    route = f"{'packed' if packed else 'unpacked'}/{'depth' if depth else 'colour'}/{oname}/" \
                            f"{'zero_buf' if prezeroed else 'fresh'}"
                    dk = dict(depths=out.depths) if depth else {}
                    accum = None
                    if prezeroed:                       # the forward clears it: start from garbage
                        accum = torch.full((n, 16), float("nan"), dtype=torch.float32, device=dev)
                        fwd = pkg.rasterize_forward(out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act,
                                                    out.tile_ranges, out.gaussian_indices, w, h, BG, zero_buf=accum,
                                                    tile_order=order, **src, **dk)
                        assert np.array_equal(_bits(fwd.color), _bits(ref["color"])), route
                        assert np.array_equal(np_(fwd.n_contrib), ref["n_contrib"]), route
                        assert not bool(accum.any()), route
                    extra = dict(depths=out.depths, dL_ddepth_map=t(dD), dL_dalpha=t(dA)) if depth else {}
                    rb = pkg.rasterize_backward(t(dC), out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act,
                                                out.tile_ranges, out.gaussian_indices, out.final_T, out.n_contrib, w,
                                                h, BG, n, tile_order=order, zeroed_accum=accum, **src, **extra)
                    got = {k: np_(getattr(rb, k)) for k in par.ACCUMULATORS}
                    if depth:
                        got["dL_ddepths"] = np_(rb.dL_ddepths)
                    rep = par.blend_bound_report(got, want, mags, ref["cov_2d_inv"], entries)
                    for k, v in rep.items():
                        worst[(route, k)] = v["worst_diff_over_bound"]
                        if not v["ok"]:
                            failures.append(par.format_bound_report({k: v}, route))
                    # the tensor-scale bar as before
                    for k in par.ACCUMULATORS:
                        assert par.over_scale(got[k], want[k]) <= 1e-4, (route, k)
    routes = sorted({r for r, _ in worst})
    names = list(par.ACCUMULATORS) + ["dL_ddepths"]
    print("  worst diff/bound per route:" + "".join(f"  {k[3:]}" for k in names))
    for r in routes:
        print(f"  {r:36s}" + "".join(f"  {worst.get((r, k), float('nan')):.3g}" for k in names))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("depth_maps", [False, True])
def test_accumulator_rows_to_parameter_gradients(pkg, orc, dev, depth_maps):
    """The production chain: k_project_backward reading the accumulator rows (grads_from_moments inside, as
    render_backward does) against the oracle's project_backward and sh_backward applied to the GPU's OWN unpacked
    accumulators of the same rows (k_unpack_grads: the same grads_from_moments).  Positions, rotations, scales,
    opacities and the 2-D mean gradient are bit-exact; dL_dsh_coeffs within 1e-6 of its scale; with a depth map the
    positions gain dL/dz W[2,:] per row (test_projection_backward_adds_dz_times_the_third_row's rule).  With the
    all-element bound on the accumulators, every parameter-gradient element is accounted for."""
    w, h, n, deg = 203, 131, 6000, 3
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=deg, seed=4242, mu_s=-3.7)
    arrays["positions"][:30, 2] = -5.0                                    # behind the camera: no row, no gradient
    cam = pkg.scene.make_camera(w, h, view=3)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=list(BG), active_sh_degree=deg)
    out = pkg.render(model, cam, settings, want_depth_map=depth_maps)
    ref = oracle_forward(orc, arrays, cam, bg=BG, degree=deg)
    assert np.array_equal(_bits(out.color), _bits(ref["color"]))
    dC, dD, dA = _incoming(w, h, 11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    extra = dict(depths=out.depths, dL_ddepth_map=t(dD), dL_dalpha=t(dA)) if depth_maps else {}
    R = pkg.rasterizer
    # the launch render_backward makes (render()'s order and cleared accumulator), unpacked as well
    rb = R.rasterize_backward(t(dC), out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                              out.gaussian_indices, out.final_T, out.n_contrib, w, h, BG, n, packed=out.packed,
                              zeroed_accum=out.zeroed_accum, tile_order=out.tile_order, **extra)
    out.zeroed_accum = None
    par = load_parity()
    want, mags = oracle_blend_terms(orc, ref, dC, BG, n, w, h, dD=dD, dA=dA, depth_route=depth_maps)
    got = {k: np_(getattr(rb, k)) for k in par.ACCUMULATORS}
    if depth_maps:
        got["dL_ddepths"] = np_(rb.dL_ddepths)
    check_blend_bounds(got, want, mags, ref["cov_2d_inv"], np.bincount(ref["values"], minlength=n),
                       f"rows for the chain test (depth maps: {depth_maps})")
    dm = torch.empty((n, 2), device=dev)
    pb = R.project_backward(None, None, None, None, model.positions, model.rotations, model.scales, model.opacities,
                            model.sh_coeffs, out.radii, cam, deg, 1.0, grad_accum=rb.grad_accum,
                            colour_gate=out.colour_gate, dL_dmeans_2d_out=dm)
    K = cam.intrinsics
    ob = orc.project_backward(arrays["positions"], arrays["rotations"], arrays["scales"], arrays["opacities"],
                              ref["view"], K.fx, K.fy, K.cx, K.cy, 1.0, ref["radii"], got["dL_dmeans_2d"],
                              got["dL_dcov_2d_inv"], got["dL_dopacity_act"])
    osh = orc.sh_backward(deg, arrays["sh_coeffs"], ref["dirs"], got["dL_drgb"])
    radii = ref["radii"]
    live = radii > 0
    assert (~live).sum() >= 30 and live.sum() > 1000
    for k in ("dL_drotations", "dL_dscales", "dL_dopacities"):
        assert np.array_equal(_bits(getattr(pb, k)), _bits(ob[k])), k
    assert np.array_equal(_bits(np_(dm)[live]), _bits(got["dL_dmeans_2d"][live]))
    pos, opos = np_(pb.dL_dpositions).astype(np.float64), ob["dL_dpositions"].astype(np.float64)
    if depth_maps:
        W = np.asarray(cam.rotation, np.float64)
        dz = got["dL_ddepths"].astype(np.float64)
        zterm = np.where(live[:, None], dz[:, None] * W[2][None, :], 0.0)
        assert float(np.abs(zterm).max()) > 0.0
        scale = np.linalg.norm(opos, axis=1, keepdims=True) + np.abs(dz)[:, None]
        assert np.all(np.abs(pos - opos - zterm) <= 1e-6 * scale + 1e-30)
        assert np.array_equal(pos[~live], opos[~live])
    else:
        assert np.array_equal(_bits(pb.dL_dpositions), _bits(ob["dL_dpositions"]))
    sh = np_(pb.dL_dsh_coeffs).astype(np.float64)
    assert float(np.abs(sh - osh).max()) <= 1e-6 * float(np.abs(osh).max())
