"""Camera-pose gradient on the GPU: the per-Gaussian rows against the fp64 model tests/pose_ref.py, the
reduction against the fp64 sum of the GPU's own rows, determinism and route equality bit for bit, the end-to-end
identity dL/dtvec = W sum_i dL_dpositions_i, central differences of a rendered loss along se(3), and pose refinement."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pose_ref
from util import np_

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4                           # the project's bar: error relative to each tensor's scale
BLOCK = 256                               # CUGS_BLOCK
RED_BOUND = (math.log2(BLOCK) + 2) * 2.0 ** -24


def _bits(t):
    a = np_(t) if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _camera(pkg, w, h):
    cam = pkg.scene.make_camera(w, h, view=2)
    return pkg.pose.apply_se3(cam, [0.05, -0.03, 0.1, 0.04, -0.06, 0.03])


def _scene(pkg, n, w, h, deg, seed, behind=0, mu_s=-4.0):
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=deg, seed=seed, mu_s=mu_s)
    if behind:
        arrays["positions"][:behind, 2] *= -1.0
    return arrays


def _grads_2d(n, seed, dev):
    rng = np.random.default_rng(seed)
    gm = (rng.standard_normal((n, 2)) * 1e-3).astype(np.float32)
    gc = (rng.standard_normal((n, 3)) * 1e-2).astype(np.float32)
    gr = (rng.standard_normal((n, 3)) * 1e-2).astype(np.float32)
    go = (rng.standard_normal((n, 1)) * 1e-3).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    return gm, gc, t(gm), t(gc), t(gr), t(go)


def _misaligned(t):
    """A contiguous copy of t whose data pointer is 4 bytes past a 16-byte boundary (the kernel's unaligned route)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0
    return out


def _stage(pkg, model, cam, deg, gm, gc, gr, go, proj, gate=True, rows=None, want=True, unaligned=False):
    rot = _misaligned(model.rotations) if unaligned else model.rotations
    return pkg.project_backward(gm, gc, gr, go, model.positions, rot, model.scales, model.opacities, model.sh_coeffs,
                                proj.radii, cam, deg, colour_gate=proj.colour_gate if gate else None,
                                want_camera_grad=want, dL_dview_rows=rows)


@pytest.mark.parametrize("num_coeffs,deg,unaligned,gate", [
    (1, 0, False, True), (4, 1, False, True), (9, 2, True, True), (16, 3, False, True),   # 16 + gate: FACTORS
    (16, 3, False, False),                                                                 # the row tile
    (16, 3, True, True), (4, 1, True, False),
])
def test_rows_match_the_fp64_model(pkg, dev, num_coeffs, deg, unaligned, gate):
    w, h, n = 320, 240, 5 * BLOCK + 37                  # a ragged last workgroup
    arrays = _scene(pkg, n, w, h, 3, seed=num_coeffs + 7, behind=60)
    arrays["sh_coeffs"] = np.ascontiguousarray(arrays["sh_coeffs"][:, :, :num_coeffs])
    cam = _camera(pkg, w, h)
    model = pkg.scene.to_model(arrays, dev)
    proj = pkg.project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam,
                                 deg)
    radii = np_(proj.radii)
    assert (radii == 0).sum() >= 60 and (radii > 0).sum() > n // 2
    gm_np, gc_np, gm, gc, gr, go = _grads_2d(n, num_coeffs, dev)
    rows = torch.full((n, 12), float("nan"), device=dev)
    out = _stage(pkg, model, cam, deg, gm, gc, gr, go, proj, gate=gate, rows=rows, unaligned=unaligned)
    torch.cuda.synchronize()
    want = pose_ref.camera_rows(arrays, cam, gm_np, gc_np, live=radii > 0)
    got = np_(rows).astype(np.float64)
    assert np.isfinite(got).all()
    assert (got[radii == 0] == 0.0).all()
    for cols in (slice(0, 9), slice(9, 12)):             # dL/dW and dL/dtvec, each against its own scale
        scale = np.abs(want[:, cols]).max()
        assert np.abs(got[:, cols] - want[:, cols]).max() <= GRAD_TOL * scale, cols
    # the reduction of these rows
    _check_reduction(np_(out.dL_dviewmat), got)
    # every other output is that of the entry point without the camera gradient, bit for bit
    plain = _stage(pkg, model, cam, deg, gm, gc, gr, go, proj, gate=gate, want=False, unaligned=unaligned)
    assert plain.dL_dviewmat is None
    for k in ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs"):
        assert np.array_equal(_bits(getattr(out, k)), _bits(getattr(plain, k))), k


def _check_reduction(view, rows):
    """dL_dview (4x4) against the fp64 sum of the rows, per element, within (log2(BLOCK) + 2) 2^-24 sum |rows|."""
    assert view.shape == (4, 4)
    assert (view[3] == 0.0).all()
    s = rows.sum(0)
    a = np.abs(rows).sum(0)
    want = np.zeros((3, 4))
    mag = np.zeros((3, 4))
    want[:, :3], want[:, 3] = s[:9].reshape(3, 3), s[9:]
    mag[:, :3], mag[:, 3] = a[:9].reshape(3, 3), a[9:]
    err = np.abs(view[:3].astype(np.float64) - want)
    assert (err <= RED_BOUND * mag).all(), (err / np.maximum(mag, 1e-300)).max()


@pytest.mark.parametrize("n", [1, 255, 1_000_000, 6_000_000])
def test_reduction_is_within_its_bound_and_deterministic(pkg, dev, n):
    w, h = (1920, 1080) if n >= 1_000_000 else (320, 240)
    arrays = _scene(pkg, n, w, h, 0, seed=n % 1000, mu_s=-4.6)
    cam = _camera(pkg, w, h)
    model = pkg.scene.to_model(arrays, dev)
    proj = pkg.project_gaussians(model.positions, model.rotations, model.scales, model.opacities, model.sh_coeffs, cam, 0)
    _, _, gm, gc, gr, go = _grads_2d(n, 3, dev)
    rows = torch.empty((n, 12), device=dev)
    a = _stage(pkg, model, cam, 0, gm, gc, gr, go, proj, rows=rows).dL_dviewmat.clone()
    b = _stage(pkg, model, cam, 0, gm, gc, gr, go, proj).dL_dviewmat.clone()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a), _bits(b))               # two runs (with and without the rows): the same bits
    _check_reduction(np_(a), np_(rows).astype(np.float64))


def test_empty_model_gives_zeros(pkg, dev):
    from cugs_amd import _lib
    from cugs_amd._lib import lib
    cam = _camera(pkg, 64, 48)
    e = lambda *s: torch.empty(s, device=dev)
    out = pkg.project_backward(e(0, 2), e(0, 3), e(0, 3), e(0, 1), e(0, 3), e(0, 4), e(0, 3), e(0, 1), e(0, 3, 16),
                               torch.empty(0, dtype=torch.int32, device=dev), cam, 3, want_camera_grad=True)
    assert torch.equal(out.dL_dviewmat, torch.zeros(4, 4, device=dev))
    # the C entry points themselves write the 16 zeros for n == 0
    view = torch.full((4, 4), 7.0, device=dev)
    pg = _lib.PoseGrad(view.data_ptr(), None, None, 0)
    abi = cam.to_abi()
    adam = _lib.AdamFused()
    mc = _lib.McmcFused()
    P = C.c_void_p
    opts = _lib.ProjectionOpts(pose=C.pointer(pg))
    assert lib.cugs_project_backward_opts(0, 16, 3, *([None] * 7), C.byref(abi), 1.0, *([None] * 12), C.byref(opts),
                                          None) == 0
    torch.cuda.synchronize()
    assert torch.equal(view, torch.zeros(4, 4, device=dev))
    for opts in (_lib.ProjectionOpts(pose=C.pointer(pg)), _lib.ProjectionOpts(mcmc=C.pointer(mc), pose=C.pointer(pg))):
        view.fill_(7.0)
        assert lib.cugs_project_backward_adam_opts(0, 16, 3, *([None] * 7), C.byref(abi), 1.0, None, C.byref(adam), P(0),
                                                   C.byref(opts), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(view, torch.zeros(4, 4, device=dev))


# ---- routes: one accumulator, every entry point -------------------------------------------------------------------
def _training_inputs(pkg, dev, n=40_000, w=640, h=360):
    arrays = _scene(pkg, n, w, h, 3, seed=77, behind=500)
    cam = _camera(pkg, w, h)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=[0.1, 0.2, 0.3], active_sh_degree=3)
    out = pkg.render(model, cam, settings)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h)).to(dev)
    rb = pkg.rasterize_backward(g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                out.gaussian_indices, out.final_T, out.n_contrib, w, h, settings.background, n,
                                packed=out.packed, unpack=False, tile_order=out.tile_order)
    torch.cuda.synchronize()
    return arrays, cam, model, out, rb.grad_accum.clone()


def _fused(pkg, dev, arrays, cam, out, accum, route, pose):
    """One fused step (route 'adam' or 'mcmc') on a fresh copy of the model and zero moments: (model, moments,
    dL_dmeans_2d, dL_dview or None)."""
    from cugs_amd import _lib
    from cugs_amd._lib import lib
    model = pkg.scene.to_model(arrays, dev)
    n = model.num_gaussians()
    names = ("positions", "sh_coeffs", "opacities", "scales", "rotations")
    m = [torch.zeros_like(getattr(model, k)) for k in names]
    v = [torch.zeros_like(getattr(model, k)) for k in names]
    a = _lib.AdamFused()
    for i in range(5):
        a.m[i], a.v[i], a.lr[i] = m[i].data_ptr(), v[i].data_ptr(), 1e-3 * (i + 1)
    a.beta1, a.beta2, a.eps, a.bc1, a.bc2 = 0.9, 0.999, 1e-15, 10.0, 1000.0
    d_means = torch.empty((n, 2), device=dev)
    abi = cam.to_abi()
    P = lambda t: C.c_void_p(t.data_ptr())
    args = (n, 16, 3, P(model.positions), P(model.rotations), P(model.scales), P(model.opacities), P(model.sh_coeffs),
            P(out.radii), P(out.colour_gate), C.byref(abi), 1.0, P(accum), C.byref(a))
    view = torch.full((4, 4), float("nan"), device=dev) if pose else None
    ws = torch.empty(lib.cugs_pose_grad_workspace_bytes(n), dtype=torch.uint8, device=dev)
    pg = _lib.PoseGrad(view.data_ptr(), None, ws.data_ptr(), ws.numel()) if pose else None
    mc = _lib.McmcFused(0.01, 0.01, 5e5, 100.0, 0.005, 3, 1234, None)
    opts = _lib.ProjectionOpts(mcmc=C.pointer(mc) if route == "mcmc" else None, pose=C.pointer(pg) if pose else None)
    assert lib.cugs_project_backward_adam_opts(*args, P(d_means), C.byref(opts), None) == 0
    torch.cuda.synchronize()
    return model, m + v, d_means, view


def test_camera_gradient_is_the_same_on_every_route(pkg, dev):
    arrays, cam, model, out, accum = _training_inputs(pkg, dev)
    stage = lambda gate: pkg.project_backward(None, None, None, None, model.positions, model.rotations, model.scales,
                                              model.opacities, model.sh_coeffs, out.radii, cam, 3, grad_accum=accum,
                                              colour_gate=out.colour_gate if gate else None,
                                              dL_dmeans_2d_out=torch.empty((model.num_gaussians(), 2), device=dev),
                                              want_camera_grad=True)
    ref = stage(True).dL_dviewmat.clone()                  # FACTORS
    again = stage(True).dL_dviewmat.clone()
    row_tile = stage(False).dL_dviewmat.clone()            # the gate recomputed from the coefficients: the row tile
    torch.cuda.synchronize()
    assert np.abs(np_(ref)).max() > 0.0
    assert np.array_equal(_bits(ref), _bits(again))
    assert np.array_equal(_bits(ref), _bits(row_tile))
    for route in ("adam", "mcmc"):
        with_pose = _fused(pkg, dev, arrays, cam, out, accum, route, pose=True)
        without = _fused(pkg, dev, arrays, cam, out, accum, route, pose=False)
        assert np.array_equal(_bits(with_pose[3]), _bits(ref)), route
        for k in ("positions", "rotations", "scales", "opacities", "sh_coeffs"):
            assert np.array_equal(_bits(getattr(with_pose[0], k)), _bits(getattr(without[0], k))), (route, k)
        for i, (x, y) in enumerate(zip(with_pose[1], without[1])):
            assert np.array_equal(_bits(x), _bits(y)), (route, "moment", i)
        assert np.array_equal(_bits(with_pose[2]), _bits(without[2])), (route, "dL_dmeans_2d")


@pytest.mark.parametrize("route", ["plain", "adam", "mcmc"])
def test_render_backward_camera_gradient_end_to_end(pkg, dev, route):
    w, h, n = 640, 360, 30_000
    arrays = _scene(pkg, n, w, h, 3, seed=5, behind=300)
    cam = _camera(pkg, w, h)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=3)
    rng = np.random.default_rng(8)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h)).to(dev)
    dD = torch.from_numpy((rng.standard_normal((h, w)) * 1e-4).astype(np.float32)).to(dev)
    dA = torch.from_numpy((rng.standard_normal((h, w)) * 1e-4).astype(np.float32)).to(dev)
    out = pkg.render(model, cam, settings, want_depth_map=True)
    grads = pkg.render_backward(g, out, model, cam, settings, dL_ddepth_map=dD, dL_dalpha=dA, want_camera_grad=True)
    gv = np_(grads.dL_dviewmat).astype(np.float64)
    assert (gv[3] == 0.0).all() and np.abs(gv).max() > 0.0
    if route == "plain":
        W = cam.world_to_camera()[:3, :3].astype(np.float64)
        dp = np_(grads.dL_dpositions).astype(np.float64)
        dt = dp @ W.T                                        # dt_i = W dL/dp_i
        want = dt.sum(0)
        # the reduction's bound plus the fp32 rounding of dL/dp = W^T dt and of its re-rotation (3 ulp each term)
        bound = (RED_BOUND + 6 * 2.0 ** -24) * (np.abs(dp) @ np.abs(W).T).sum(0)
        assert (np.abs(gv[:3, 3] - want) <= bound).all(), (gv[:3, 3], want, bound)
        return
    # the fused routes: the same camera gradient as the plain route on the same accumulator; compared through the
    # projection stage, since the blend's scatter (float atomics) makes two render_backward calls differ in the last bits
    opt = pkg.FusedAdam(model)
    mcmc = pkg.MCMCController(pkg.MCMCConfig(), 5.0) if route == "mcmc" else None
    out2 = pkg.render(model, cam, settings, want_depth_map=True)
    fused = pkg.render_backward(g, out2, model, cam, settings, fused_adam=opt, mcmc=mcmc, dL_ddepth_map=dD, dL_dalpha=dA,
                                want_camera_grad=True)
    fv = np_(fused.dL_dviewmat).astype(np.float64)
    assert (fv[3] == 0.0).all()
    assert np.abs(fv - gv).max() <= 1e-4 * np.abs(gv).max()


def test_camera_gradient_refused_with_the_data_parallel_exchange(pkg, dev):
    w, h, n = 64, 48, 500
    arrays = _scene(pkg, n, w, h, 3, seed=1)
    cam = _camera(pkg, w, h)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings()
    out = pkg.render(model, cam, settings)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h)).to(dev)
    with pytest.raises(RuntimeError, match="camera gradient"):
        pkg.render_backward(g, out, model, cam, settings, dL_drgb_gated_out=torch.empty((n, 3), device=dev),
                            want_camera_grad=True)
    empty = pkg.scene.to_model(pkg.scene.make_gaussians(0, w, h, sh_degree=3), dev)
    z = pkg.render_backward(g, pkg.render(empty, cam, settings), empty, cam, settings, want_camera_grad=True)
    assert torch.equal(z.dL_dviewmat, torch.zeros(4, 4, device=dev))


# ---- behaviour -----------------------------------------------------------------------------------------------------
def _smooth_scene(pkg, dev, n, w, h, seed):
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=0, seed=seed, mu_s=-2.6)
    arrays["opacities"][:] = np.clip(arrays["opacities"], -3.0, 1.0)
    return arrays, pkg.scene.to_model(arrays, dev)


def test_se3_gradient_matches_central_differences_of_a_rendered_loss(pkg, dev):
    w, h, n = 256, 192, 3000
    arrays, model = _smooth_scene(pkg, dev, n, w, h, seed=12)
    cam = pkg.scene.make_camera(w, h)
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=0)
    rng = np.random.default_rng(4)
    G = torch.from_numpy(rng.standard_normal((h, w, 3)).astype(np.float32) / (w * h)).to(dev)
    G = torch.nn.functional.avg_pool2d(G.permute(2, 0, 1)[None], 9, 1, 4)[0].permute(1, 2, 0).contiguous()  # smooth
    G64 = G.double()

    def loss(c):
        return float((pkg.render(model, c, settings, for_backward=False).color.double() * G64).sum())

    out = pkg.render(model, cam, settings)
    gb = pkg.render_backward(G, out, model, cam, settings, want_camera_grad=True)
    g = np_(pkg.pose.viewmat_grad_to_se3(gb.dL_dviewmat.double(), cam))
    steps = [2e-3] * 3 + [5e-4] * 3
    fd = np.array([(loss(pkg.pose.apply_se3(cam, np.eye(6)[k] * steps[k])) -
                    loss(pkg.pose.apply_se3(cam, -np.eye(6)[k] * steps[k]))) / (2 * steps[k]) for k in range(6)])
    big = np.abs(g) > 0.01 * np.abs(g).max()
    agree = big & (np.abs(fd - g) <= 0.1 * np.abs(g))
    assert big.sum() >= 4, (g, fd)
    assert agree.sum() >= min(5, big.sum()) and agree.sum() >= big.sum() - 1, (g, fd)


def test_pose_refinement_converges(pkg, dev):
    w, h, n = 256, 192, 4000
    arrays, model = _smooth_scene(pkg, dev, n, w, h, seed=21)
    true = pkg.scene.make_camera(w, h)
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=0)
    target = pkg.render(model, true, settings, for_backward=False).color.clone()
    axis = np.array([0.3, -0.8, 0.5]) / np.linalg.norm([0.3, -0.8, 0.5])
    start = pkg.pose.apply_se3(true, np.concatenate([[0.12, -0.08, 0.1], axis * math.radians(2.0)]))

    def errors(c):
        rot = pkg.pose.rotation_angle_deg(c.rotation, true.rotation)
        ctr = np.linalg.norm(c.camera_center().astype(np.float64) - true.camera_center().astype(np.float64))
        return rot, ctr

    rot0, tr0 = errors(start)
    assert rot0 > 1.5 and tr0 > 0.1
    lr = np.array([4e-3] * 3 + [1e-3] * 3)
    b1, b2, eps = 0.9, 0.99, 1e-12
    m = np.zeros(6)
    v = np.zeros(6)
    cam = start
    for it in range(1, 151):
        out = pkg.render(model, cam, settings)
        _, dl = pkg.combined_loss_and_grad(out.color, target)
        gb = pkg.render_backward(dl, out, model, cam, settings, want_camera_grad=True)
        g = np_(pkg.pose.viewmat_grad_to_se3(gb.dL_dviewmat.double(), cam))
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        step = -lr * (m / (1 - b1 ** it)) / (np.sqrt(v / (1 - b2 ** it)) + eps)
        cam = pkg.pose.apply_se3(cam, step)
    rot, tr = errors(cam)
    assert rot < 0.25 * rot0 and tr < 0.25 * tr0, (rot0, tr0, rot, tr)
