"""Sparse Adam on the GPU: FusedAdam.step(visible=) over cugs_fused_adam_groups_rows and
render_backward(..., fused_adam=, sparse_adam=True) over cugs_project_backward_adam_opts with cugs_projection_opts.sparse.

Everything is compared BIT FOR BIT: a visible row takes exactly the dense update of this step, an invisible row keeps
its bits, so  sparse = where(visible row, dense step result, value before)  for the five parameter tensors and the ten
moment tensors.  The blend backward's float atomics may order sums differently from run to run, so the paths compared
always consume the same accumulator rows.

Scenes: pkg.scene.make_gaussians under the identity camera (it looks down +z, every z lies in [2, 10]); rows are made
invisible by negating their z.  The standard pattern (sparse_adam_ref.standard_invisible) is rows 256..511 plus every
third row elsewhere: one workgroup that is invisible as a whole, float4 pieces that straddle a visible and an invisible
row, and mixed workgroups."""
import ctypes as C

import numpy as np
import pytest
import torch

from sparse_adam_ref import standard_invisible

pytestmark = pytest.mark.gpu

NAMES = ("positions", "sh_coeffs", "opacities", "scales", "rotations")      # ParamGroup order
P = lambda t: C.c_void_p(t.data_ptr())


def _pattern_scene(pkg, n, w, h, stored, seed, mu_s=-3.7):
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=stored, seed=seed, mu_s=mu_s)
    inv = standard_invisible(n)
    arrays["positions"][inv, 2] *= -1.0                     # behind the camera
    return arrays, pkg.scene.make_camera(w, h), inv


def _check_radii(radii, inv):
    """The rows made invisible are culled, and the invisible share of the view is a real mix (not all, not none)."""
    r = radii.cpu().numpy()
    assert (r[inv] == 0).all()
    share = float((r <= 0).mean())
    assert 0.25 <= share <= 0.75, share
    return torch.from_numpy(r > 0).to(radii.device)


def _state(model, opt):
    return [getattr(model, k).clone() for k in NAMES] + [t.clone() for t in opt.m_] + [t.clone() for t in opt.v_]


def _twin(pkg, model, opt):
    """A model and optimizer with the same bits, for the dense step the sparse one is compared with."""
    m2 = pkg.GaussianModel(**{k: getattr(model, k).clone() for k in NAMES})
    o2 = pkg.FusedAdam(m2, opt.config_)
    o2.m_, o2.v_ = [t.clone() for t in opt.m_], [t.clone() for t in opt.v_]
    o2.step_count_, o2.learning_rates_ = opt.step_count_, list(opt.learning_rates_)
    return m2, o2


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_where(got, dense, before, vis, what):
    """got == where(visible row, dense, before), bit for bit, for the 15 tensors of a state."""
    for i, (g, d, b) in enumerate(zip(got, dense, before)):
        mask = vis.view(-1, *([1] * (g.dim() - 1)))
        assert _bits_equal(g, torch.where(mask, d, b)), (what, i)


def _random_grads(pkg, model, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda t: (torch.randn(t.shape, generator=gen) * 1e-2).to(t.device)
    # BackwardOutput order: positions, rotations, scales, opacities, sh_coeffs, means_2d
    return pkg.BackwardOutput(mk(model.positions), mk(model.rotations), mk(model.scales), mk(model.opacities),
                              mk(model.sh_coeffs), None)


@pytest.mark.parametrize("stored", [3, 1, 0])
def test_standalone_masked_step(pkg, dev, stored):
    """N = 1301: the position group has 3903 floats (975 pieces and a scalar tail of three); C = 16, 4, 1."""
    n, w, h = 1301, 128, 96
    arrays, cam, inv = _pattern_scene(pkg, n, w, h, stored, seed=n + stored)
    model = pkg.scene.to_model(arrays, dev)
    out = pkg.render(model, cam, pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=stored))
    seen = _check_radii(out.radii, inv)
    ones, none = torch.ones(n, dtype=torch.bool, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)
    for tag, visible, vis in (("pattern", out.radii, seen), ("all", ones, ones), ("none", none, none),
                              ("all-radii", torch.full((n,), 7, dtype=torch.int32, device=dev), ones)):
        m = pkg.scene.to_model(arrays, dev)
        opt = pkg.FusedAdam(m)
        for step in range(3):
            grads = _random_grads(pkg, m, 10 * step + stored)
            before = _state(m, opt)
            md, od = _twin(pkg, m, opt)
            od.apply_gradients(grads)
            od.step()                                         # the dense step of this step, from the same state
            opt.apply_gradients(grads)
            opt.step(visible=visible)
            assert opt.step_count_ == od.step_count_ == step + 1
            got, dense = _state(m, opt), _state(md, od)
            _assert_where(got, dense, before, vis, (tag, step))
            if tag.startswith("all"):
                assert all(_bits_equal(a, b) for a, b in zip(got, dense)), (tag, step)
            if tag == "none":
                assert all(_bits_equal(a, b) for a, b in zip(got, before)), (tag, step)
        if tag != "none":
            assert not torch.equal(m.positions, torch.from_numpy(arrays["positions"]).to(dev))


def test_standalone_masked_step_rejects_a_bad_mask(pkg, dev):
    arrays, cam, inv = _pattern_scene(pkg, 300, 64, 48, 0, seed=3)
    m = pkg.scene.to_model(arrays, dev)
    opt = pkg.FusedAdam(m)
    opt.apply_gradients(_random_grads(pkg, m, 1))
    before = _state(m, opt)
    with pytest.raises(RuntimeError):
        opt.step(visible=torch.ones(299, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        opt.step(visible=torch.ones(300, dtype=torch.int32))                  # on the host
    with pytest.raises(RuntimeError):
        opt.step(visible=torch.ones(300, dtype=torch.float32, device=dev))
    assert opt.step_count_ == 0 and all(_bits_equal(a, b) for a, b in zip(_state(m, opt), before))


def test_masked_step_on_unaligned_pointers(pkg, dev):
    """One group whose four pointers sit 4 bytes off a 16-byte boundary: the scalar route of the kernel, at the ABI."""
    from cugs_amd._lib import AdamGroup, check, lib
    n, width = 1301, 3
    gen = torch.Generator(device="cpu").manual_seed(5)
    mk = lambda s: (torch.randn(n * width + 1, generator=gen) * s).to(dev)
    bufs = [mk(1.0), mk(1e-2), mk(1e-3), mk(1e-6).abs()]                      # param, grad, m, v
    twin = [b.clone() for b in bufs]
    before = [b.clone() for b in bufs]
    radii = torch.from_numpy(np.where(standard_invisible(n), 0, 3).astype(np.int32)).to(dev)

    def group(bs):
        g = (AdamGroup * 1)()
        views = [b[1:] for b in bs]
        assert all(v.data_ptr() % 16 == 4 for v in views)
        g[0].param, g[0].grad, g[0].m, g[0].v = (v.data_ptr() for v in views)
        g[0].n, g[0].lr = n * width, 1e-3
        return g
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(lib.cugs_fused_adam_groups(group(twin), 1, 0.9, 0.999, 1e-15, 10.0, 1000.0, st), "dense")
    check(lib.cugs_fused_adam_groups_rows(group(bufs), 1, (C.c_int32 * 1)(width), P(radii), n, 0.9, 0.999, 1e-15, 10.0,
                                          1000.0, st), "rows")
    vis = (radii > 0).repeat_interleave(width)
    for k in (0, 2, 3):
        assert _bits_equal(bufs[k][1:], torch.where(vis, twin[k][1:], before[k][1:])), k
        assert _bits_equal(bufs[k][:1], before[k][:1])                        # the word in front is not touched
        assert not torch.equal(bufs[k], before[k])


def _misaligned(t):
    """The same values in storage that starts 4 bytes off a 16-byte boundary (contiguous all the same)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# the four shapes of test_fused_adam_backward_equals_backward_then_adam, then 27-float rows (C = 9) on both routes
@pytest.mark.parametrize("n,w,h,deg,stored,aligned", [(3000, 200, 150, 3, 3, True), (777, 96, 64, 1, 1, True),
                                                      (1000, 128, 96, 0, 0, True), (1301, 128, 96, 1, 3, True),
                                                      (600, 96, 64, 2, 2, True), (600, 96, 64, 2, 2, False),
                                                      (600, 96, 64, 3, 3, False)])
def test_fused_sparse_equals_backward_then_masked_step(pkg, dev, n, w, h, deg, stored, aligned):
    """Path A: project_backward -> apply_gradients -> step(visible=radii).  Path B: the fused entry with sparse = 1.
    Same accumulator rows; model, moments and dL_dmeans_2d equal bit for bit over three steps, and path B's
    dL_dmeans_2d is the dense fused route's."""
    from cugs_amd._lib import ProjectionOpts, check, lib
    arrays, cam, inv = _pattern_scene(pkg, n, w, h, stored, seed=n)
    settings = pkg.RenderSettings(background=[0.2, 0.1, 0.3], active_sh_degree=deg)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=n + 1) * 3000.0).to(dev)
    ma, mb = pkg.scene.to_model(arrays, dev), pkg.scene.to_model(arrays, dev)
    if not aligned:
        for m in (ma, mb):
            m.sh_coeffs, m.rotations = _misaligned(m.sh_coeffs), _misaligned(m.rotations)
    oa, ob = pkg.FusedAdam(ma), pkg.FusedAdam(mb)
    R = pkg.rasterizer
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for step in range(3):
        out = pkg.render(ma, cam, settings)
        seen = _check_radii(out.radii, inv)
        assert all(torch.equal(getattr(ma, k), getattr(mb, k)) for k in NAMES)
        rb = R.rasterize_backward(g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                  out.gaussian_indices, out.final_T, out.n_contrib, w, h, settings.background, n,
                                  packed=out.packed, unpack=False)
        before = _state(mb, ob)
        mc, oc = _twin(pkg, mb, ob)                         # the dense fused route, for dL_dmeans_2d and where()
        if not aligned:
            mc.sh_coeffs, mc.rotations = _misaligned(mc.sh_coeffs), _misaligned(mc.rotations)
        dm_a, dm_b, dm_c = (torch.empty((n, 2), device=dev) for _ in range(3))
        pb = R.project_backward(None, None, None, None, ma.positions, ma.rotations, ma.scales, ma.opacities,
                                ma.sh_coeffs, out.radii, cam, deg, settings.scale_modifier, grad_accum=rb.grad_accum,
                                colour_gate=out.colour_gate, dL_dmeans_2d_out=dm_a)
        oa.apply_gradients(pkg.BackwardOutput(pb.dL_dpositions, pb.dL_drotations, pb.dL_dscales, pb.dL_dopacities,
                                              pb.dL_dsh_coeffs, dm_a))
        oa.step(visible=out.radii)
        cam_abi = cam.to_abi()
        for sparse, m, o, dm in ((1, mb, ob, dm_b), (0, mc, oc, dm_c)):
            adam = o.begin_fused_step()
            check(lib.cugs_project_backward_adam_opts(
                n, int(m.sh_coeffs.shape[2]), deg, P(m.positions), P(m.rotations), P(m.scales), P(m.opacities),
                P(m.sh_coeffs), P(out.radii), P(out.colour_gate), C.byref(cam_abi), float(settings.scale_modifier),
                P(rb.grad_accum), C.byref(adam), P(dm), C.byref(ProjectionOpts(sparse=sparse)), st()), "fused")
        assert _bits_equal(dm_a, dm_b) and _bits_equal(dm_b, dm_c)
        got = _state(mb, ob)
        for i, (a, b) in enumerate(zip(_state(ma, oa), got)):
            assert _bits_equal(a, b), (step, i)
        _assert_where(got, _state(mc, oc), before, seen, step)
        assert oa.step_count_ == ob.step_count_ == step + 1
    start = pkg.scene.to_model(arrays, dev)
    for k in NAMES:
        now, was = getattr(mb, k).cpu().numpy(), getattr(start, k).cpu().numpy()
        assert np.array_equal(now[inv].view(np.uint32), was[inv].view(np.uint32)), k      # never seen, never touched
        assert not np.array_equal(now[~inv], was[~inv]), k                                # the model moved


@pytest.fixture
def shared_blend(pkg, monkeypatch):
    """render_backward calls that are handed the same RenderOutput share ONE backward blend: its float atomics may
    order sums differently from run to run, and the comparisons below are bit for bit."""
    real, memo = pkg.rasterizer.rasterize_backward, {}

    def once(dL_dcolor, means_2d, *args, **kwargs):
        key = (id(means_2d), kwargs.get("dL_ddepth_map") is not None)
        if key not in memo:
            memo[key] = (real(dL_dcolor, means_2d, *args, **kwargs), means_2d)
        return memo[key][0]
    monkeypatch.setattr(pkg.rasterizer, "rasterize_backward", once)
    return memo


def test_sparse_with_no_culled_gaussian_is_the_dense_fused_route(pkg, dev, shared_blend):
    n, w, h, deg = 1301, 128, 96, 3
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=deg, seed=77, mu_s=-3.7)
    arrays["positions"][:, :2] *= 0.5                        # everything well inside the image
    cam = pkg.scene.make_camera(w, h)
    settings = pkg.RenderSettings(background=[0.2, 0.1, 0.3], active_sh_degree=deg)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=78) * 3000.0).to(dev)
    ma, mb = pkg.scene.to_model(arrays, dev), pkg.scene.to_model(arrays, dev)
    oa, ob = pkg.FusedAdam(ma), pkg.FusedAdam(mb)
    for step in range(2):
        out = pkg.render(ma, cam, settings)
        assert bool((out.radii > 0).all())
        ra = pkg.render_backward(g, out, ma, cam, settings, fused_adam=oa)
        rs = pkg.render_backward(g, out, mb, cam, settings, fused_adam=ob, sparse_adam=True)
        assert rs.dL_dpositions is None and rs.dL_dsh_coeffs is None
        assert _bits_equal(ra.dL_dmeans_2d, rs.dL_dmeans_2d)
        for i, (a, b) in enumerate(zip(_state(ma, oa), _state(mb, ob))):
            assert _bits_equal(a, b), (step, i)
    assert oa.step_count_ == ob.step_count_ == 2
    assert not torch.equal(mb.positions, torch.from_numpy(arrays["positions"]).to(dev))


@pytest.mark.parametrize("pose,depth", [(True, False), (False, True), (True, True)])
def test_sparse_with_camera_and_depth_map_gradients(pkg, dev, shared_blend, pose, depth):
    """want_camera_grad and dL_ddepth_map on the sparse route: dL_dviewmat and dL_dmeans_2d are the dense fused route's on
    the same accumulator (invisible rows add zeros in both), the model is render_backward + step(visible=radii)."""
    n, w, h, deg = 1301, 128, 96, 3
    arrays, cam, inv = _pattern_scene(pkg, n, w, h, deg, seed=91)
    settings = pkg.RenderSettings(background=[0.2, 0.1, 0.3], active_sh_degree=deg)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=92) * 3000.0).to(dev)
    gd = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=93)[:, :, 0].copy() * 300.0).to(dev) if depth else None
    ma, mb, mc = (pkg.scene.to_model(arrays, dev) for _ in range(3))
    oa, ob, oc = pkg.FusedAdam(ma), pkg.FusedAdam(mb), pkg.FusedAdam(mc)
    out = pkg.render(ma, cam, settings, want_depth_map=depth)
    seen = _check_radii(out.radii, inv)
    before = _state(mb, ob)
    kw = dict(dL_ddepth_map=gd, want_camera_grad=pose)
    plain = pkg.render_backward(g, out, ma, cam, settings, **kw)
    oa.apply_gradients(plain)
    oa.step(visible=out.radii)
    sparse = pkg.render_backward(g, out, mb, cam, settings, fused_adam=ob, sparse_adam=True, **kw)
    dense = pkg.render_backward(g, out, mc, cam, settings, fused_adam=oc, **kw)
    assert len(shared_blend) == 1                            # one blend fed all three
    if pose:
        assert _bits_equal(sparse.dL_dviewmat, dense.dL_dviewmat)
        assert bool((sparse.dL_dviewmat[:3] != 0).any())
    else:
        assert sparse.dL_dviewmat is None
    assert _bits_equal(sparse.dL_dmeans_2d, dense.dL_dmeans_2d) and _bits_equal(sparse.dL_dmeans_2d, plain.dL_dmeans_2d)
    got = _state(mb, ob)
    for i, (a, b) in enumerate(zip(_state(ma, oa), got)):
        assert _bits_equal(a, b), i
    _assert_where(got, _state(mc, oc), before, seen, (pose, depth))
    if depth:                                                # the depth word reached the visible positions
        md = pkg.scene.to_model(arrays, dev)
        od = pkg.FusedAdam(md)
        out2 = pkg.render(md, cam, settings, want_depth_map=True)
        pkg.render_backward(g, out2, md, cam, settings, fused_adam=od, sparse_adam=True)
        assert not torch.equal(md.positions, mb.positions)


def test_sparse_refusals_leave_the_model_alone(pkg, dev):
    n, w, h = 300, 64, 48
    arrays, cam, inv = _pattern_scene(pkg, n, w, h, 0, seed=5)
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=0)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h)).to(dev)
    m = pkg.scene.to_model(arrays, dev)
    opt = pkg.FusedAdam(m)
    ctrl = pkg.MCMCController(pkg.MCMCConfig(), 5.0)
    before = _state(m, opt)
    with pytest.raises(RuntimeError, match="sparse_adam"):
        pkg.render_backward(g, pkg.render(m, cam, settings), m, cam, settings, fused_adam=opt, mcmc=ctrl, sparse_adam=True)
    with pytest.raises(RuntimeError, match="sparse_adam"):
        pkg.render_backward(g, pkg.render(m, cam, settings), m, cam, settings, sparse_adam=True)
    assert opt.step_count_ == 0 and all(_bits_equal(a, b) for a, b in zip(_state(m, opt), before))
