"""Depth and alpha maps: render(..., want_depth_map=True) and render_backward(..., dL_ddepth_map=,
dL_dalpha=) against the CPU oracle, WITHOUT a depth-aware oracle: the blend is linear in the per-Gaussian colour, so

  * the depth map is the red channel of a blend with rgb := (z, z, z) and background 0 - bit for bit;
  * its gradients are those of that channel: dL/dz = dL_drgb[:, 0] of the oracle's backward with rgb := z,
    dL_dcolor := (dL/dD, 0, 0), background 0; opacity and 2-D gradients likewise;
  * the alpha map 1 - final_T is the channel rgb := 1, background 0 - gradients likewise;
  * through the projection, z = t.z adds dL/dz W[2,:] to dL_dpositions (radii > 0).
"""
import numpy as np
import pytest
import torch

from util import max_err_over_max, np_, oracle_backward, oracle_forward

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4     # the project's bar: error relative to each tensor's scale


def _scene(pkg, n, w, h, deg, seed, mu_s=-4.6, view=0):
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=deg, seed=seed, mu_s=mu_s)
    cam = pkg.scene.make_camera(w, h, view=view)
    return arrays, cam


def _bits(t):
    a = np_(t) if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _channel_forward(orc, ref, w, h, value):
    """The oracle's blend of a constant-per-Gaussian channel (rgb := value, background 0): its red channel."""
    rgb = np.ascontiguousarray(np.repeat(np.asarray(value, np.float32).reshape(-1, 1), 3, axis=1))
    f = orc.rasterize_forward(w, h, (0.0, 0.0, 0.0), ref["tile_ranges"], ref["values"], ref["means_2d"],
                              ref["cov_2d_inv"], rgb, ref["opacities_act"], threads=orc.host_threads())
    return f["color"][..., 0]


def _channel_backward(orc, ref, w, h, n, value, g):
    """The oracle's backward of that channel for dL/d(channel) = g [H,W] (green and blue get no gradient)."""
    rgb = np.ascontiguousarray(np.repeat(np.asarray(value, np.float32).reshape(-1, 1), 3, axis=1))
    dc = np.zeros((h, w, 3), np.float32)
    dc[..., 0] = g
    return orc.rasterize_backward(w, h, (0.0, 0.0, 0.0), ref["tile_ranges"], ref["values"], ref["means_2d"],
                                  ref["cov_2d_inv"], rgb, ref["opacities_act"], dc, ref["final_T"], ref["n_contrib"], n,
                                  threads=orc.host_threads())


def _map_grads(w, h, seed):
    rng = np.random.default_rng(seed)
    dD = (rng.standard_normal((h, w)) * 0.05).astype(np.float32)
    dA = (rng.standard_normal((h, w)) * 0.3).astype(np.float32)
    return dD, dA


@pytest.mark.parametrize("n,w,h,deg,mu_s,bg", [
    (20000, 640, 360, 3, -4.6, (0.0, 0.0, 0.0)),
    (20000, 333, 211, 3, -3.5, (0.2, 0.4, 0.6)),       # dense: saturated pixels, ragged edge tiles
    (3000, 250, 130, 0, -3.0, (1.0, 1.0, 1.0)),
    (100000, 1920, 1080, 0, -4.6, (0.0, 0.0, 0.0)),    # a 1080p frame
])
def test_depth_map_forward_is_the_red_channel_of_z(pkg, orc, dev, n, w, h, deg, mu_s, bg):
    arrays, cam = _scene(pkg, n, w, h, deg, seed=n + w, mu_s=mu_s)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=list(bg), active_sh_degree=deg)
    plain = pkg.render(model, cam, settings)
    out = pkg.render(model, cam, settings, want_depth_map=True)
    assert plain.depth_map is None and out.depth_map.shape == (h, w) and out.depth_map.dtype == torch.float32
    # the colour outputs do not change, bit for bit
    assert np.array_equal(_bits(out.color), _bits(plain.color))
    assert np.array_equal(_bits(out.final_T), _bits(plain.final_T))
    assert torch.equal(out.n_contrib, plain.n_contrib)
    assert torch.equal(out.alpha, 1.0 - out.final_T)
    ref = oracle_forward(orc, arrays, cam, bg=bg, degree=deg)
    want = _channel_forward(orc, ref, w, h, ref["depths"])
    assert np.array_equal(_bits(out.depth_map), want.view(np.uint32))
    assert float(want.max()) > 0.0
    # the stage function on the unpacked route (oracle arrays) and on the packed, tile-ordered route
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f1 = pkg.rasterize_forward(t(ref["means_2d"]), t(ref["cov_2d_inv"]), t(ref["rgb"]), t(ref["opacities_act"]),
                               t(ref["tile_ranges"]), t(ref["values"]), w, h, bg, packed=None, depths=t(ref["depths"]))
    order = pkg.rasterizer.tile_order_of(out.tile_ranges, w, h)
    f2 = pkg.rasterize_forward(out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                               out.gaussian_indices, w, h, bg, packed=out.packed, tile_order=order, depths=out.depths)
    for f in (f1, f2):
        assert np.array_equal(_bits(f.depth_map), want.view(np.uint32))
        assert np.array_equal(_bits(f.color), ref["color"].view(np.uint32))
        assert np.array_equal(np_(f.n_contrib), ref["n_contrib"])


def test_depth_map_of_an_empty_model_is_zero(pkg, dev):
    model = pkg.GaussianModel(torch.zeros((0, 3), device=dev), torch.zeros((0, 3, 1), device=dev),
                              torch.zeros((0, 1), device=dev), torch.zeros((0, 4), device=dev),
                              torch.zeros((0, 3), device=dev))
    cam = pkg.scene.make_camera(40, 24)
    out = pkg.render(model, cam, pkg.RenderSettings(background=[0.5, 0.5, 0.5]), want_depth_map=True)
    assert out.depth_map.shape == (24, 40) and not out.depth_map.any() and not out.alpha.any()


@pytest.mark.parametrize("n,w,h,deg,mu_s,bg,packed_route", [
    (20000, 333, 211, 3, -3.5, (0.2, 0.4, 0.6), False),
    (6000, 320, 240, 0, -3.8, (0.0, 0.0, 0.0), True),
])
def test_depth_and_alpha_blend_backward_against_the_oracle(pkg, orc, dev, n, w, h, deg, mu_s, bg, packed_route):
    arrays, cam = _scene(pkg, n, w, h, deg, seed=n + 5, mu_s=mu_s)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=list(bg), active_sh_degree=deg)
    out = pkg.render(model, cam, settings, want_depth_map=True)
    ref = oracle_forward(orc, arrays, cam, bg=bg, degree=deg)
    dC = pkg.scene.make_dl_dcolor(w, h)
    dD, dA = _map_grads(w, h, n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    z = ref["depths"]
    A = _channel_backward(orc, ref, w, h, n, z, dD)
    B = _channel_backward(orc, ref, w, h, n, np.ones(n, np.float32), dA)
    Cc = orc.rasterize_backward(w, h, bg, ref["tile_ranges"], ref["values"], ref["means_2d"], ref["cov_2d_inv"],
                                ref["rgb"], ref["opacities_act"], dC, ref["final_T"], ref["n_contrib"], n,
                                threads=orc.host_threads())

    def gpu(dc, dd, da):
        if packed_route:
            return pkg.rasterize_backward(t(dc), out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act,
                                          out.tile_ranges, out.gaussian_indices, out.final_T, out.n_contrib, w, h, bg, n,
                                          packed=out.packed, tile_order=pkg.rasterizer.tile_order_of(out.tile_ranges, w, h),
                                          depths=out.depths, dL_ddepth_map=None if dd is None else t(dd),
                                          dL_dalpha=None if da is None else t(da))
        return pkg.rasterize_backward(t(dc), t(ref["means_2d"]), t(ref["cov_2d_inv"]), t(ref["rgb"]),
                                      t(ref["opacities_act"]), t(ref["tile_ranges"]), t(ref["values"]), t(ref["final_T"]),
                                      t(ref["n_contrib"]), w, h, bg, n, depths=t(z),
                                      dL_ddepth_map=None if dd is None else t(dd), dL_dalpha=None if da is None else t(da))

    zero = np.zeros((h, w, 3), np.float32)
    geo = ("dL_dopacity_act", "dL_dmeans_2d", "dL_dcov_2d_inv")
    # the depth map alone
    r = gpu(zero, dD, None)
    assert max_err_over_max(np_(r.dL_ddepths), A["dL_drgb"][:, 0]) <= GRAD_TOL
    assert float(np.abs(A["dL_drgb"][:, 0]).max()) > 0.0
    assert not r.dL_drgb.any()
    for k in geo:
        assert max_err_over_max(np_(getattr(r, k)), A[k]) <= GRAD_TOL, ("depth", k)
    # the alpha map alone: no gradient reaches z
    r = gpu(zero, None, dA)
    assert not r.dL_ddepths.any() and not r.dL_drgb.any()
    for k in geo:
        assert max_err_over_max(np_(getattr(r, k)), B[k]) <= GRAD_TOL, ("alpha", k)
    # all three: the sum of the three channels' gradients
    r = gpu(dC, dD, dA)
    assert max_err_over_max(np_(r.dL_drgb), Cc["dL_drgb"]) <= GRAD_TOL
    assert max_err_over_max(np_(r.dL_ddepths), A["dL_drgb"][:, 0]) <= GRAD_TOL
    for k in geo:
        want = Cc[k].astype(np.float64) + A[k] + B[k]
        assert max_err_over_max(np_(getattr(r, k)), want) <= GRAD_TOL, ("all", k)


def test_alpha_gradient_identity_through_the_background(pkg, orc, dev):
    """The identity the kernel relies on: sum_i alpha_i T_i + final_T = 1, so the channel (c = 1, bg = 0) has the
    gradient of (c = 0, bg = -1) - checked on the oracle itself, independently of the kernel."""
    w, h, n = 160, 120, 2000
    arrays, cam = _scene(pkg, n, w, h, 0, seed=3, mu_s=-3.0)
    ref = oracle_forward(orc, arrays, cam, degree=0)
    rng = np.random.default_rng(4)
    g = np.zeros((h, w, 3), np.float32)
    g[..., 0] = rng.standard_normal((h, w)).astype(np.float32)
    args = (ref["tile_ranges"], ref["values"], ref["means_2d"], ref["cov_2d_inv"])
    ones, zeros = np.ones((n, 3), np.float32), np.zeros((n, 3), np.float32)
    a = orc.rasterize_backward(w, h, (0.0, 0.0, 0.0), *args, ones, ref["opacities_act"], g, ref["final_T"],
                               ref["n_contrib"], n)
    b = orc.rasterize_backward(w, h, (-1.0, 0.0, 0.0), *args, zeros, ref["opacities_act"], g, ref["final_T"],
                               ref["n_contrib"], n)
    for k in ("dL_dopacity_act", "dL_dmeans_2d", "dL_dcov_2d_inv"):
        assert max_err_over_max(b[k], a[k]) <= 1e-5, k


def test_projection_backward_adds_dz_times_the_third_row(pkg, dev):
    w, h, n = 320, 240, 6000
    arrays, cam = _scene(pkg, n, w, h, 3, seed=17, mu_s=-3.8, view=4)
    arrays["positions"][:40, 2] = -5.0                  # behind the camera: radius 0, no gradient
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=3)
    out = pkg.render(model, cam, settings)
    R = pkg.rasterizer
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h)).to(dev)
    rb = R.rasterize_backward(g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                              out.gaussian_indices, out.final_T, out.n_contrib, w, h, settings.background, n,
                              packed=out.packed, unpack=False)
    rows0 = rb.grad_accum.clone()
    rows1 = rows0.clone()
    dz = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 0.01
    rows1[:, 9] = dz
    res = []
    for rows in (rows0, rows1):
        dm = torch.empty((n, 2), device=dev)
        pb = R.project_backward(None, None, None, None, model.positions, model.rotations, model.scales, model.opacities,
                                model.sh_coeffs, out.radii, cam, 3, 1.0, grad_accum=rows, colour_gate=out.colour_gate,
                                dL_dmeans_2d_out=dm)
        res.append((pb, dm))
    (p0, m0), (p1, m1) = res
    for k in ("dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs"):
        assert torch.equal(getattr(p0, k), getattr(p1, k)), k
    assert torch.equal(m0, m1)
    W = np.asarray(cam.rotation, np.float64)
    radii = np_(out.radii)
    pos0, pos1 = np_(p0.dL_dpositions).astype(np.float64), np_(p1.dL_dpositions).astype(np.float64)
    want = np_(dz).astype(np.float64)[:, None] * W[2][None, :]
    want[radii <= 0] = 0.0
    assert (radii <= 0).sum() >= 40 and (radii > 0).sum() > 1000
    assert np.array_equal(pos0[radii <= 0], pos1[radii <= 0])
    # |dL/dt| = |dL/dpositions| (W is orthonormal): fp32 rounding of a few operations on that scale
    scale = np.linalg.norm(pos0, axis=1, keepdims=True) + np.abs(np_(dz))[:, None]
    assert np.all(np.abs((pos1 - pos0) - want) <= 1e-6 * scale + 1e-30)


@pytest.mark.parametrize("n,w,h,deg,mu_s,bg,view", [
    (20000, 333, 211, 3, -3.5, (0.2, 0.4, 0.6), 0),
    (6000, 320, 240, 0, -3.8, (0.0, 0.0, 0.0), 4),      # rotated + translated camera
])
def test_render_backward_with_depth_and_alpha_end_to_end(pkg, orc, dev, n, w, h, deg, mu_s, bg, view):
    arrays, cam = _scene(pkg, n, w, h, deg, seed=n + 77, mu_s=mu_s, view=view)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=list(bg), active_sh_degree=deg)
    out = pkg.render(model, cam, settings, want_depth_map=True)
    ref = oracle_forward(orc, arrays, cam, bg=bg, degree=deg)
    dC = pkg.scene.make_dl_dcolor(w, h)
    dD, dA = _map_grads(w, h, n + 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    grads = pkg.render_backward(t(dC), out, model, cam, settings, dL_ddepth_map=t(dD), dL_dalpha=t(dA))
    refC = oracle_backward(orc, dC, ref, arrays, cam, bg=bg)
    A = _channel_backward(orc, ref, w, h, n, ref["depths"], dD)
    B = _channel_backward(orc, ref, w, h, n, np.ones(n, np.float32), dA)
    K = cam.intrinsics
    # z and 1 are not colours: only the 2-D gradients of the two channels go through the projection
    pAB = orc.project_backward(arrays["positions"], arrays["rotations"], arrays["scales"], arrays["opacities"],
                               ref["view"], K.fx, K.fy, K.cx, K.cy, 1.0, ref["radii"],
                               (A["dL_dmeans_2d"] + B["dL_dmeans_2d"]).astype(np.float32),
                               (A["dL_dcov_2d_inv"] + B["dL_dcov_2d_inv"]).astype(np.float32),
                               (A["dL_dopacity_act"] + B["dL_dopacity_act"]).astype(np.float32))
    W = np.asarray(cam.rotation, np.float64)
    zterm = A["dL_drgb"][:, 0].astype(np.float64)[:, None] * W[2][None, :]
    zterm[ref["radii"] <= 0] = 0.0
    want = {
        "dL_dpositions": refC["dL_dpositions"].astype(np.float64) + pAB["dL_dpositions"] + zterm,
        "dL_drotations": refC["dL_drotations"].astype(np.float64) + pAB["dL_drotations"],
        "dL_dscales": refC["dL_dscales"].astype(np.float64) + pAB["dL_dscales"],
        "dL_dopacities": refC["dL_dopacities"].astype(np.float64) + pAB["dL_dopacities"],
        "dL_dsh_coeffs": refC["dL_dsh_coeffs"],
        "dL_dmeans_2d": refC["dL_dmeans_2d"].astype(np.float64) + A["dL_dmeans_2d"] + B["dL_dmeans_2d"],
    }
    assert float(np.abs(zterm).max()) > 0.0
    for k, v in want.items():
        got = np_(getattr(grads, k)).reshape(v.shape)
        assert max_err_over_max(got, v) <= GRAD_TOL, k
    # without these maps the result is the colour-only one; the depth terms are not small against it
    plain = pkg.render_backward(t(dC), pkg.render(model, cam, settings), model, cam, settings)
    assert max_err_over_max(np_(plain.dL_dpositions), want["dL_dpositions"]) > 10 * GRAD_TOL


def test_zero_map_gradients_equal_the_colour_route(pkg, dev):
    w, h, n = 333, 211, 20000
    arrays, cam = _scene(pkg, n, w, h, 3, seed=31, mu_s=-3.5)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=[0.2, 0.4, 0.6], active_sh_degree=3)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h)).to(dev)
    a = pkg.render_backward(g, pkg.render(model, cam, settings), model, cam, settings)
    z = torch.zeros((h, w), device=dev)
    b = pkg.render_backward(g, pkg.render(model, cam, settings, want_depth_map=True), model, cam, settings,
                            dL_ddepth_map=z, dL_dalpha=z)
    for k in ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs", "dL_dmeans_2d"):
        assert max_err_over_max(np_(getattr(b, k)), np_(getattr(a, k))) <= 1e-5, k     # up to the order of the atomics


@pytest.mark.parametrize("mcmc", [False, True])
def test_fused_adam_with_depth_maps_equals_backward_then_adam(pkg, dev, mcmc):
    """The fused optimizer step reads word 9 of the same rows: bit for bit render_backward + apply_gradients + step
    (both consume the SAME accumulator rows; only the blend's atomics could reorder sums)."""
    w, h, n, deg = 200, 150, 3000, 3
    arrays, cam = _scene(pkg, n, w, h, deg, seed=n, mu_s=-3.7)
    settings = pkg.RenderSettings(background=[0.2, 0.1, 0.3], active_sh_degree=deg)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=n + 1) * 3000.0).to(dev)
    dD, dA = _map_grads(w, h, 9)
    dD, dA = torch.from_numpy(dD * 3000.0).to(dev), torch.from_numpy(dA * 3000.0).to(dev)
    ma, mb = pkg.scene.to_model(arrays, dev), pkg.scene.to_model(arrays, dev)
    oa, ob = pkg.FusedAdam(ma), pkg.FusedAdam(mb)
    R = pkg.rasterizer
    names = ("positions", "sh_coeffs", "opacities", "scales", "rotations")
    import ctypes as C
    from cugs_amd._lib import check, lib
    for step in range(3):
        out = pkg.render(ma, cam, settings, want_depth_map=True)
        rb = R.rasterize_backward(g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                  out.gaussian_indices, out.final_T, out.n_contrib, w, h, settings.background, n,
                                  packed=out.packed, unpack=False, depths=out.depths, dL_ddepth_map=dD, dL_dalpha=dA)
        assert rb.grad_accum[:, 9].abs().max() > 0 and not rb.grad_accum[:, 10:].any()
        dm_a = torch.empty((n, 2), device=dev)
        pb = R.project_backward(None, None, None, None, ma.positions, ma.rotations, ma.scales, ma.opacities,
                                ma.sh_coeffs, out.radii, cam, deg, settings.scale_modifier, grad_accum=rb.grad_accum,
                                colour_gate=out.colour_gate, dL_dmeans_2d_out=dm_a)
        oa.apply_gradients(pkg.BackwardOutput(pb.dL_dpositions, pb.dL_drotations, pb.dL_dscales, pb.dL_dopacities,
                                              pb.dL_dsh_coeffs, dm_a))
        oa.step()
        adam = ob.begin_fused_step()
        dm_b = torch.empty((n, 2), device=dev)
        cam_abi = cam.to_abi()
        P = lambda x: C.c_void_p(x.data_ptr())
        check(lib.cugs_project_backward_adam(n, int(mb.sh_coeffs.shape[2]), deg, P(mb.positions), P(mb.rotations),
                                             P(mb.scales), P(mb.opacities), P(mb.sh_coeffs), P(out.radii),
                                             P(out.colour_gate), C.byref(cam_abi), float(settings.scale_modifier),
                                             P(rb.grad_accum), C.byref(adam), P(dm_b),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "cugs_project_backward_adam")
        assert torch.equal(dm_a, dm_b)
        for i, k in enumerate(names):
            assert torch.equal(getattr(ma, k), getattr(mb, k)), (step, k)
            assert torch.equal(oa.m_[i], ob.m_[i]) and torch.equal(oa.v_[i], ob.v_[i]), (step, k)
    # through the host surface, plain fused step or with the MCMC work riding along
    before = mb.positions.clone()
    out = pkg.render(mb, cam, settings, want_depth_map=True)
    kw = {}
    if mcmc:
        kw = dict(mcmc=pkg.MCMCController(pkg.MCMCConfig(), scene_extent=5.0), mcmc_step=3)
    res = pkg.render_backward(g, out, mb, cam, settings, fused_adam=ob, dL_ddepth_map=dD, dL_dalpha=dA, **kw)
    assert res.dL_dpositions is None and res.dL_dmeans_2d.shape == (n, 2)
    assert not torch.equal(before, mb.positions)


def test_depth_map_gradient_without_a_depth_render_is_refused(pkg, dev):
    w, h, n = 64, 48, 200
    arrays, cam = _scene(pkg, n, w, h, 0, seed=2, mu_s=-3.0)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(active_sh_degree=0)
    out = pkg.render(model, cam, settings)
    g = torch.zeros((h, w, 3), device=dev)
    with pytest.raises(RuntimeError, match="want_depth_map"):
        pkg.render_backward(g, out, model, cam, settings, dL_ddepth_map=torch.zeros((h, w), device=dev))
    out = pkg.render(model, cam, settings, want_depth_map=True)
    with pytest.raises(RuntimeError, match=r"\[H, W\]"):
        pkg.render_backward(g, out, model, cam, settings, dL_ddepth_map=torch.zeros((w, h), device=dev))
    with pytest.raises(RuntimeError, match="device"):
        pkg.render_backward(g, out, model, cam, settings, dL_dalpha=torch.zeros((h, w)))
    with pytest.raises(RuntimeError, match="data-parallel"):
        pkg.render_backward(g, out, model, cam, settings, dL_dalpha=torch.zeros((h, w), device=dev),
                            dL_drgb_gated_out=torch.empty((n, 3), device=dev))
    # the alpha map needs no depth render
    r = pkg.render_backward(g, pkg.render(model, cam, settings), model, cam, settings,
                            dL_dalpha=torch.ones((h, w), device=dev))
    assert r.dL_dopacities.abs().max() > 0


def test_fitting_depth_and_alpha_maps_reduces_the_depth_loss(pkg, dev):
    """Perturbed positions pulled back by an L1 loss on the depth and alpha maps of the true scene with FusedAdam.
    A sign error in the z term or in the alpha gradient makes the loss grow instead."""
    w, h, n = 128, 96, 1500
    arrays, cam = _scene(pkg, n, w, h, 0, seed=8, mu_s=-3.0)
    settings = pkg.RenderSettings(active_sh_degree=0)
    true_model = pkg.scene.to_model(arrays, dev)
    target = pkg.render(true_model, cam, settings, want_depth_map=True, for_backward=False)
    tD, tA = target.depth_map.clone(), target.alpha.clone()
    rng = np.random.default_rng(9)
    pert = dict(arrays)
    pert["positions"] = (arrays["positions"] + np.stack([np.zeros(n), np.zeros(n), rng.normal(0.0, 0.4, n)], 1)
                         ).astype(np.float32)
    model = pkg.scene.to_model(pert, dev)
    cfg = pkg.AdamConfig(position_lr_config=pkg.PositionLRConfig(lr_init=1e-2, lr_final=1e-2))
    opt = pkg.FusedAdam(model, cfg)
    hw = float(w * h)
    losses = []
    zero_c = torch.zeros((h, w, 3), device=dev)
    for it in range(100):
        out = pkg.render(model, cam, settings, want_depth_map=True)
        rD, rA = out.depth_map - tD, out.alpha - tA
        losses.append(float(rD.abs().sum() / hw))
        pkg.render_backward(zero_c, out, model, cam, settings, fused_adam=opt,
                            dL_ddepth_map=torch.sign(rD) / hw, dL_dalpha=torch.sign(rA) / hw)
    curve = " ".join(f"{v:.4f}" for v in losses[::10]) + f" ... {losses[-1]:.4f}"
    print("depth L1 loss curve (every 10th):", curve)
    # measured on one MI355X: 0.807 -> 0.054 over the 100 iterations (-93 %); the bar leaves a wide margin
    assert losses[-1] < 0.5 * losses[0], "depth L1 loss curve (every 10th): " + curve
