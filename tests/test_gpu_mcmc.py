"""SURVEY §8(f) N5 on the GPU: MCMC densification (csrc/mcmc.hip, the fused route of project_backward.hip, and the
MCMCController mirror) against the numpy restatement of the reference (tests/mcmc_ref.py) on the same counter-based
draws, the reference's own tests (tests/test_mcmc.cpp) restated, and the fused route against the unfused sequence
bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import mcmc_ref as mr
from test_mcmc_oracle import KATS, kat_as_mapping

pytestmark = pytest.mark.gpu
NAMES = ("positions", "sh_coeffs", "opacities", "scales", "rotations")      # ParamGroup order


def _np(t):
    return t.detach().cpu().numpy()


def _ulp(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.max(np.abs(a - b))) if a.size else 0


def _model(pkg, dev, n, opa_val=2.0, scale_val=-2.0, seed=0, coeffs=1):
    """make_mcmc_model of the reference's test (test_mcmc.cpp:26-41)."""
    g = torch.Generator().manual_seed(seed)
    rot = torch.randn((n, 4), generator=g)
    rot = rot / rot.norm(2, 1, True).clamp_min(1e-8)
    return pkg.GaussianModel(positions=(torch.randn((n, 3), generator=g) * 0.5).to(dev),
                             sh_coeffs=(torch.randn((n, 3, coeffs), generator=g) * 0.1).to(dev),
                             opacities=torch.full((n, 1), opa_val).to(dev), rotations=rot.to(dev),
                             scales=torch.full((n, 3), scale_val).to(dev))


def _arrays(model):
    return {k: _np(getattr(model, k)).copy() for k in NAMES}


# ---- generator ----
def test_random_bits_known_answers(pkg, dev):
    for ctr, key, want in KATS:
        seed, stream, step, index = kat_as_mapping(ctr, key)
        got = _np(pkg.mcmc.random_bits(seed, stream, step, index, 1, dev)).view(np.uint32)[0]
        assert [int(x) for x in got] == list(want)


def test_device_normals_and_determinism(pkg, dev):
    n = 4 << 20
    m = pkg.GaussianModel(positions=torch.zeros((n, 3), device=dev), sh_coeffs=torch.zeros((n, 3, 1), device=dev),
                          opacities=torch.full((n, 1), -20.0, device=dev), rotations=torch.zeros((n, 4), device=dev),
                          scales=torch.zeros((n, 3), device=dev))
    # lr 1, scale e^0, gate sigmoid(-100 (sigmoid(-20) - 0.995)) == 1 in float: positions become the normals
    ctrl = pkg.MCMCController(pkg.MCMCConfig(noise_lr_init=1.0, noise_lr_final=1.0, seed=1234), 1.0)
    ctrl.inject_noise(m, 7)
    z = _np(m.positions)
    words = _np(pkg.mcmc.random_bits(1234, mr.STREAM_NOISE, 7, 0, n, dev)).view(np.uint32)
    assert np.array_equal(words[:4096], mr.bits(1234, mr.STREAM_NOISE, 7, np.arange(4096)))
    want = mr.normals_from_words(words)
    assert float(np.max(np.abs(z.astype(np.float64) - want))) <= 4e-6
    zz = z.astype(np.float64).reshape(-1)
    assert abs(zz.mean()) < 2e-3 and abs(zz.var() - 1.0) < 3e-3
    again = _np(pkg.mcmc.random_bits(1234, mr.STREAM_NOISE, 7, 0, n, dev)).view(np.uint32)
    other = _np(pkg.mcmc.random_bits(1234, mr.STREAM_NOISE, 8, 0, n, dev)).view(np.uint32)
    assert np.array_equal(again, words) and (other != words).mean() > 0.99


# ---- regulariser ----
def test_regularization_against_oracle(pkg, orc, dev):
    n = 200_000
    g = torch.Generator().manual_seed(5)
    opa = (torch.randn((n, 1), generator=g) * 4.0).to(dev)
    scl = (torch.randn((n, 3), generator=g) * 1.5 - 3.0).to(dev)
    cfg = pkg.MCMCConfig(lambda_opacity=0.01, lambda_scale=0.02)
    ctrl = pkg.MCMCController(cfg, 1.0)
    m = pkg.GaussianModel(positions=torch.zeros((n, 3), device=dev), sh_coeffs=torch.zeros((n, 3, 1), device=dev),
                          opacities=opa, rotations=torch.zeros((n, 4), device=dev), scales=scl)
    value, g_o, g_s = ctrl.compute_regularization(m)
    assert value.dim() == 0 and value.is_cuda
    ref = mr.MCMCRef(orc, 1.0, lambda_opacity=0.01, lambda_scale=0.02)
    v_ref, o_ref, s_ref = ref.regularization(_np(opa), _np(scl))
    assert _ulp(_np(g_o), o_ref) <= 2 and _ulp(_np(g_s), s_ref) <= 2
    assert abs(float(value) - v_ref) <= 1e-6 * abs(v_ref)
    # add mode: in place into caller-owned gradients
    from cugs_amd._lib import check, lib
    base_o, base_s = torch.randn((n, 1), device=dev) * 1e-6, torch.randn((n, 3), device=dev) * 1e-6
    acc_o, acc_s = base_o.clone(), base_s.clone()
    ws = torch.empty(lib.cugs_mcmc_relocate_workspace_bytes(n), dtype=torch.uint8, device=dev)
    val2 = torch.zeros((), device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    check(lib.cugs_mcmc_regularization(n, P(opa), P(scl), 0.01, 0.02, P(acc_o), P(acc_s), P(acc_o), P(acc_s), P(val2),
                                       P(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "reg")
    assert torch.equal(acc_o, base_o + g_o) and torch.equal(acc_s, base_s + g_s)
    assert torch.equal(val2, value)


# ---- noise ----
def test_noise_explicit_against_oracle(pkg, orc, dev):
    n = 50_000
    g = torch.Generator().manual_seed(9)
    m = pkg.GaussianModel(positions=(torch.randn((n, 3), generator=g) * 2.0).to(dev),
                          sh_coeffs=torch.zeros((n, 3, 1), device=dev),
                          opacities=(torch.randn((n, 1), generator=g) * 6.0).to(dev),
                          rotations=torch.zeros((n, 4), device=dev),
                          scales=(torch.randn((n, 3), generator=g) - 4.0).to(dev))
    noise = torch.randn((n, 3), generator=g).to(dev)
    ctrl = pkg.MCMCController(pkg.MCMCConfig(noise_lr_init=50.0, noise_lr_final=5.0, noise_lr_max_steps=1000), 1.0)
    before = _arrays(m)
    ctrl.inject_noise(m, 300, noise=noise)
    want = mr.MCMCRef(orc, 1.0).inject_noise(before["positions"], before["scales"], before["opacities"],
                                            ctrl.noise_lr(300), _np(noise))
    assert _ulp(_np(m.positions), want) <= 1
    assert np.array_equal(_np(m.scales), before["scales"]) and np.array_equal(_np(m.opacities), before["opacities"])


def test_noise_gate_selectivity(pkg, dev):
    """test_mcmc.cpp:217-256"""
    m = _model(pkg, dev, 100)
    m.opacities[:50] = 10.0
    m.opacities[50:] = -10.0
    before = m.positions.clone()
    ctrl = pkg.MCMCController(pkg.MCMCConfig(noise_lr_init=1.0, noise_lr_final=1.0, noise_gate_k=100.0,
                                             noise_gate_t=0.995), 10.0)
    for _ in range(10):
        ctrl.inject_noise(m, 0)
    disp = (m.positions - before).norm(2, 1)
    assert float(disp[50:].mean()) > 2.0 * float(disp[:50].mean())


def test_noise_injection_modifies_positions(pkg, dev):
    """test_mcmc.cpp:258-277"""
    m = _model(pkg, dev, 10, opa_val=0.0)
    before = m.positions.clone()
    pkg.MCMCController(pkg.MCMCConfig(noise_lr_init=1e4), 10.0).inject_noise(m, 0)
    assert not torch.allclose(before, m.positions) and bool(torch.isfinite(m.positions).all())


# ---- relocation: the reference's tests (test_mcmc.cpp:122-213, 355-380) ----
def test_relocation_fixes_dead_gaussians(pkg, dev):
    m = _model(pkg, dev, 20)
    m.opacities[:10] = 5.0
    m.opacities[10:] = -8.0
    alive_before, dead_before = m.positions[:10].clone(), m.positions[10:].clone()
    ctrl = pkg.MCMCController(pkg.MCMCConfig(dead_opacity_threshold=0.005, relocate_cap=1.0), 10.0)
    st = ctrl.relocate(m, 500)
    assert (st.num_relocated, st.num_dead, st.num_total) == (10, 10, 20)
    assert m.num_gaussians() == 20
    assert not torch.allclose(dead_before, m.positions[10:])
    assert torch.equal(alive_before, m.positions[:10])


def test_relocate_cap_respected(pkg, dev):
    m = _model(pkg, dev, 100)
    m.opacities[:80] = 5.0
    m.opacities[80:] = -8.0
    st = pkg.MCMCController(pkg.MCMCConfig(relocate_cap=0.05), 10.0).relocate(m, 500)
    assert (st.num_relocated, st.num_dead, m.num_gaussians()) == (5, 20, 100)


def test_relocation_with_no_dead_is_noop(pkg, dev):
    m = _model(pkg, dev, 20)
    before = _arrays(m)
    st = pkg.MCMCController(pkg.MCMCConfig(), 10.0).relocate(m, 500)
    assert (st.num_relocated, st.num_dead) == (0, 0)
    assert all(np.array_equal(_np(getattr(m, k)), before[k]) for k in NAMES)
    m.opacities.fill_(-8.0)                                          # all dead: nothing alive to sample from
    st = pkg.MCMCController(pkg.MCMCConfig(), 10.0).relocate(m, 500)
    assert (st.num_relocated, st.num_dead) == (0, 20)


def test_constant_n_across_relocations(pkg, dev):
    m = _model(pkg, dev, 30)
    m.opacities[:20] = 3.0
    m.opacities[20:] = -8.0
    ctrl = pkg.MCMCController(pkg.MCMCConfig(relocate_cap=1.0), 10.0)
    for i in range(5):
        ctrl.relocate(m, 500 + 100 * i)
        assert all(getattr(m, k).shape[0] == 30 for k in NAMES)
        assert all(bool(torch.isfinite(getattr(m, k)).all()) for k in NAMES)


def test_relocation_exact_against_oracle(pkg, orc, dev):
    n, coeffs = 200_000, 16
    rng = np.random.default_rng(11)
    arrays = dict(positions=(rng.standard_normal((n, 3)) * 3.0).astype(np.float32),
                  sh_coeffs=rng.standard_normal((n, 3, coeffs)).astype(np.float32),
                  opacities=np.where(rng.uniform(size=(n, 1)) < 0.3, rng.uniform(-12.0, -5.4, (n, 1)),
                                     rng.normal(0.0, 3.0, (n, 1))).astype(np.float32),
                  rotations=rng.standard_normal((n, 4)).astype(np.float32),
                  scales=(rng.standard_normal((n, 3)) - 4.0).astype(np.float32))
    m = pkg.scene.to_model(arrays, dev)
    cfg = pkg.MCMCConfig(relocate_cap=0.05, seed=0xDEADBEEF12345)
    src_dev = torch.full((n,), -1, dtype=torch.int32, device=dev)
    st = pkg.MCMCController(cfg, 4.0).relocate(m, 1700, sources_out=src_dev)
    ref = mr.MCMCRef(orc, 4.0, relocate_cap=0.05, seed=0xDEADBEEF12345)
    want, (nd, M, dst, src) = ref.relocate(arrays, 1700)
    assert st.num_dead == nd and st.num_relocated == M == int(np.float32(0.05) * np.float32(n)) and M < nd
    assert np.array_equal(_np(src_dev)[:M], src)
    got = _arrays(m)
    for k in ("sh_coeffs", "rotations", "scales", "opacities"):
        assert np.array_equal(got[k], want[k]), k
    # positions: 1 ulp, plus what the device's float Box-Muller may differ from the restatement's (4e-6 per normal,
    # times extent * 0.01) where the source sits so close to 0 that the jitter sets the ulp
    d = np.abs(got["positions"][dst].astype(np.float64) - want["positions"][dst])
    assert (d <= np.spacing(np.abs(want["positions"][dst])) + 4e-6 * 4.0 * 0.01).all()
    assert (d <= np.spacing(np.abs(want["positions"][dst]))).mean() > 0.99
    untouched = np.ones(n, bool)
    untouched[dst] = False
    for k in NAMES:
        assert np.array_equal(got[k][untouched], arrays[k][untouched]), k


def test_relocation_sources_follow_opacity_weights(pkg, orc, dev):
    """chi-square (49 degrees of freedom, p > 1e-3) of 100 000 draws over 50 alive rows of different opacity."""
    alive, dead = 50, 100_000
    n = alive + dead
    opa = torch.full((n, 1), -9.0)
    opa[:alive, 0] = torch.linspace(-4.0, 5.0, alive)
    m = _model(pkg, dev, n)
    m.opacities.copy_(opa.to(dev))
    src = torch.full((n,), -1, dtype=torch.int32, device=dev)
    st = pkg.MCMCController(pkg.MCMCConfig(relocate_cap=1.0, seed=3), 1.0).relocate(m, 500, sources_out=src)
    assert st.num_relocated == dead
    counts = np.bincount(_np(src)[:dead], minlength=alive)
    assert counts.size == alive
    y = mr.MCMCRef(orc, 1.0).sigmoid(opa[:alive, 0].numpy()).astype(np.float64)
    expect = dead * y / y.sum()
    chi2 = float(np.sum((counts - expect) ** 2 / expect))
    assert chi2 < 85.35, chi2                                        # chi2.ppf(0.999, 49)


@pytest.mark.parametrize("with_optimizer", [False, True])
def test_relocation_moments(pkg, dev, with_optimizer):
    m = _model(pkg, dev, 1000, coeffs=4)
    m.opacities[::3] = -8.0
    opt = pkg.FusedAdam(m)
    for i in range(5):
        opt.m_[i].normal_()
        opt.v_[i].uniform_(0.5, 1.0)
    before_m, before_v = [t.clone() for t in opt.m_], [t.clone() for t in opt.v_]
    src = torch.full((1000,), -1, dtype=torch.int32, device=dev)
    st = pkg.MCMCController(pkg.MCMCConfig(relocate_cap=0.1), 1.0).relocate(
        m, 500, optimizer=opt if with_optimizer else None, sources_out=src)
    assert st.num_relocated == 100
    moved = torch.zeros(1000, dtype=torch.bool, device=dev)
    moved[torch.arange(0, 1000, 3, device=dev)[:100]] = True
    for i in range(5):
        for now, old in ((opt.m_[i], before_m[i]), (opt.v_[i], before_v[i])):
            assert torch.equal(now[~moved], old[~moved])
            if with_optimizer:
                assert bool((now[moved] == 0).all())
            else:
                assert torch.equal(now[moved], old[moved])


# ---- the fused route ----
@pytest.mark.parametrize("deg", [1, 3])
@pytest.mark.parametrize("explicit", [False, True])
def test_fused_route_equals_unfused_sequence(pkg, dev, deg, explicit):
    n, w, h = 50_000, 960, 540
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=deg, seed=21, mu_s=-4.0)
    arrays["opacities"][::7] = -7.0                                 # some near-dead rows: gate ~ 1
    cam = pkg.scene.make_camera(w, h)
    settings = pkg.RenderSettings(background=[0.1, 0.2, 0.3], active_sh_degree=deg)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h, seed=22) * 3000.0).to(dev)
    ma, mb = pkg.scene.to_model(arrays, dev), pkg.scene.to_model(arrays, dev)
    oa, ob = pkg.FusedAdam(ma), pkg.FusedAdam(mb)
    ctrl = pkg.MCMCController(pkg.MCMCConfig(noise_lr_init=5.0, noise_lr_final=0.5, noise_lr_max_steps=10,
                                             lambda_opacity=0.05, lambda_scale=0.05, seed=77), 5.0)
    R = pkg.rasterizer
    P = lambda t: C.c_void_p(t.data_ptr())
    from cugs_amd import _lib
    from cugs_amd._lib import check, lib
    for step in range(1, 4):
        out = pkg.render(ma, cam, settings)
        rb = R.rasterize_backward(g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                  out.gaussian_indices, out.final_T, out.n_contrib, w, h, settings.background, n,
                                  packed=out.packed, unpack=False)
        noise = torch.randn((n, 3), device=dev) if explicit else None
        # A: projection backward, + regulariser, step, noise (the reference's trainer.cpp:231-255)
        dm_a = torch.empty((n, 2), device=dev)
        pb = R.project_backward(None, None, None, None, ma.positions, ma.rotations, ma.scales, ma.opacities,
                                ma.sh_coeffs, out.radii, cam, deg, settings.scale_modifier, grad_accum=rb.grad_accum,
                                colour_gate=out.colour_gate, dL_dmeans_2d_out=dm_a)
        _, r_o, r_s = ctrl.compute_regularization(ma)
        oa.apply_gradients(pkg.BackwardOutput(pb.dL_dpositions, pb.dL_drotations, pb.dL_dscales + r_s,
                                              pb.dL_dopacities + r_o, pb.dL_dsh_coeffs, dm_a))
        oa.step()
        ctrl.inject_noise(ma, step, noise=noise)
        # B: one launch on the same accumulator rows
        adam = ob.begin_fused_step()
        mc = ctrl.fused_args(step, noise)
        dm_b = torch.empty((n, 2), device=dev)
        cam_abi = cam.to_abi()
        opts = _lib.ProjectionOpts(mcmc=C.pointer(mc))
        check(lib.cugs_project_backward_adam_opts(n, int(mb.sh_coeffs.shape[2]), deg, P(mb.positions), P(mb.rotations),
                                                  P(mb.scales), P(mb.opacities), P(mb.sh_coeffs), P(out.radii),
                                                  P(out.colour_gate), C.byref(cam_abi), float(settings.scale_modifier),
                                                  P(rb.grad_accum), C.byref(adam), P(dm_b), C.byref(opts),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "fused mcmc")
        assert torch.equal(dm_a, dm_b)
        for i, k in enumerate(NAMES):
            assert torch.equal(getattr(ma, k), getattr(mb, k)), (step, k)
            assert torch.equal(oa.m_[i], ob.m_[i]) and torch.equal(oa.v_[i], ob.v_[i]), (step, k)
    assert not torch.equal(ma.positions, torch.from_numpy(arrays["positions"]).to(dev))
    # and through the host surface
    out = pkg.render(mb, cam, settings)
    res = pkg.render_backward(g, out, mb, cam, settings, fused_adam=ob, mcmc=ctrl, mcmc_step=4)
    assert res.dL_dpositions is None and ob.step_count_ == 4 and bool(torch.isfinite(mb.positions).all())


# ---- end to end ----
def test_training_with_mcmc(pkg, dev):
    n, w, h = 20_000, 256, 256
    cam = pkg.scene.make_camera(w, h)
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=0)
    target_model = pkg.scene.to_model(pkg.scene.make_gaussians(n, w, h, sh_degree=0, seed=31, mu_s=-4.0), dev)
    target = pkg.render(target_model, cam, settings).color.clone()
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=0, seed=32, mu_s=-4.0)
    arrays["opacities"][::4] = -7.0                                  # a quarter starts dead
    model = pkg.scene.to_model(arrays, dev)
    opt = pkg.FusedAdam(model)
    ctrl = pkg.MCMCController(pkg.MCMCConfig(relocate_from=50, relocate_until=300, relocate_every=50,
                                             noise_lr_init=1e-2, noise_lr_final=1e-3, noise_lr_max_steps=300), 5.0)
    losses, relocated = [], 0
    for step in range(1, 301):
        out = pkg.render(model, cam, settings)
        loss, grad = pkg.combined_loss_and_grad(out.color, target)
        losses.append(float(loss))
        pkg.render_backward(grad, out, model, cam, settings, fused_adam=opt, mcmc=ctrl, mcmc_step=step)
        if ctrl.should_relocate(step):
            st = ctrl.relocate(model, step, optimizer=opt)
            relocated += st.num_relocated
            assert st.num_total == n
        assert model.num_gaussians() == n
    assert all(bool(torch.isfinite(getattr(model, k)).all()) for k in NAMES)
    assert np.isfinite(losses).all()
    assert relocated > 0
    assert np.mean(losses[-10:]) < 0.9 * np.mean(losses[:10]), (losses[:10], losses[-10:])
