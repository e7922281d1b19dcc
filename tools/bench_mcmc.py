#!/usr/bin/env python3
"""Times SURVEY §8(f) N5 (MCMC densification) on one MI355X:
  (a) config 4 (6 M Gaussians, SH 3, 1600x1063): the fused projection backward + Adam step with and without MCMC
      (cugs_project_backward_adam_opts without and with cugs_projection_opts.mcmc on the same accumulator rows);
  (b) the stand-alone noise and regulariser kernels against the reference's libtorch op sequence
      (mcmc_densification.cpp:144-186, restated below) on the same GPU;
  (c) one relocation at 1 M and 6 M (cap 5 %) against the reference's op sequence (:56-138)."""
import ctypes as C
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
from cugs_amd._lib import ProjectionOpts, check, lib

dev = torch.device("cuda:0")
cfg = pkg.MCMCConfig(noise_lr_init=1e-3, noise_lr_final=1e-4)


def gpu_ms(fn, reps=20, warm=3, setup=None):
    for _ in range(warm):
        if setup:
            setup()
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if setup:
            setup()                                  # untimed: e.g. the dead rows a relocation revives
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def model_of(n, coeffs, seed=0):
    g = torch.Generator().manual_seed(seed)
    rot = torch.randn((n, 4), generator=g)
    rot = rot / rot.norm(2, 1, True)
    opa = torch.randn((n, 1), generator=g) * 3.0
    opa[torch.rand((n, 1), generator=g) < 0.2] = -8.0          # a fifth dead
    return pkg.GaussianModel(positions=(torch.randn((n, 3), generator=g) * 2).to(dev),
                             sh_coeffs=(torch.randn((n, 3, coeffs), generator=g) * 0.1).to(dev),
                             opacities=opa.to(dev), rotations=rot.to(dev),
                             scales=(torch.randn((n, 3), generator=g) - 4.0).to(dev))


# ---- the reference's libtorch sequences ----
def ref_regularization(m):
    o = m.opacities.clone().detach().requires_grad_(True)
    s = m.scales.clone().detach().requires_grad_(True)
    loss = cfg.lambda_opacity * torch.sigmoid(o).mean() + cfg.lambda_scale * torch.exp(s).mean()
    loss.backward()
    return o.grad.clone(), s.grad.clone(), loss.item()


def ref_noise(m, lr):
    with torch.no_grad():
        gate = torch.sigmoid(-cfg.noise_gate_k * (torch.sigmoid(m.opacities) - cfg.noise_gate_t))
        m.positions += lr * torch.exp(m.scales) * gate * torch.randn_like(m.positions)


def ref_relocate(m, extent, cap):
    with torch.no_grad():
        n = m.positions.shape[0]
        y = torch.sigmoid(m.opacities.squeeze(1))
        dead = y.lt(cfg.dead_opacity_threshold)
        nd = int(dead.sum().item())
        if nd == 0 or nd == n:
            return
        k = min(nd, int(cap * n))
        di = dead.nonzero().squeeze(1)[:k]
        ai = (~dead).nonzero().squeeze(1)
        w = y.index_select(0, ai)
        src = ai.index_select(0, torch.multinomial(w / w.sum(), k, True))
        m.sh_coeffs.index_put_((di,), m.sh_coeffs.index_select(0, src))
        m.rotations.index_put_((di,), m.rotations.index_select(0, src))
        sp = m.positions.index_select(0, src)
        m.positions.index_put_((di,), sp + torch.randn_like(sp) * extent * 0.01)
        m.scales.index_put_((di,), m.scales.index_select(0, src) - math.log(10.0))
        m.opacities.index_put_((di,), torch.full((k, 1), math.log(0.01 / 0.99), device=dev))


def main():
    # (a) fused projection backward + Adam, config 4
    n, w, h = 6_000_000, 1600, 1063
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=3, seed=4, mu_s=-4.6)
    cam = pkg.scene.make_camera(w, h)
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=3)
    m = pkg.scene.to_model(arrays, dev)
    del arrays
    opt = pkg.FusedAdam(m)
    out = pkg.render(m, cam, settings)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h)).to(dev)
    rb = pkg.rasterizer.rasterize_backward(g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act,
                                           out.tile_ranges, out.gaussian_indices, out.final_T, out.n_contrib, w, h,
                                           settings.background, n, packed=out.packed, unpack=False)
    ctrl = pkg.MCMCController(cfg, 5.0)
    P = lambda t: C.c_void_p(t.data_ptr())
    dm = torch.empty((n, 2), device=dev)
    cam_abi = cam.to_abi()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = (n, 16, 3, P(m.positions), P(m.rotations), P(m.scales), P(m.opacities), P(m.sh_coeffs), P(out.radii),
            P(out.colour_gate), C.byref(cam_abi), 1.0, P(rb.grad_accum))
    adam = opt.begin_fused_step()
    mc = ctrl.fused_args(100)
    opts = ProjectionOpts(mcmc=C.pointer(mc))
    plain = lambda: check(lib.cugs_project_backward_adam_opts(*base, C.byref(adam), P(dm), None, st), "adam")
    fused = lambda: check(lib.cugs_project_backward_adam_opts(*base, C.byref(adam), P(dm), C.byref(opts), st), "mcmc")
    t_plain, t_fused = gpu_ms(plain, 30), gpu_ms(fused, 30)
    t_plain2 = gpu_ms(plain, 30)
    print("(a) config 4 projection backward + Adam: %.3f ms | with MCMC %.3f ms (%+.1f %%) | again without %.3f ms"
          % (t_plain, t_fused, 100.0 * (t_fused / t_plain - 1.0), t_plain2))
    del out, rb, opt

    # (b) stand-alone noise and regulariser, 6 M
    t_noise = gpu_ms(lambda: ctrl.inject_noise(m, 100))
    t_noise_x = gpu_ms(lambda: ctrl.inject_noise(m, 100, noise=dm.new_zeros((n, 3))), 10)
    t_reg = gpu_ms(lambda: ctrl.compute_regularization(m))
    t_ref_noise = gpu_ms(lambda: ref_noise(m, 1e-3), 10)
    t_ref_reg = gpu_ms(lambda: ref_regularization(m), 10)
    print("(b) 6 M: inject_noise HIP %.3f ms (%.0f GB/s at 40 B/Gaussian) vs libtorch %.3f ms (%.0fx);"
          " explicit-noise launch incl. a zeros() %.3f ms" % (t_noise, 40 * n / t_noise / 1e6, t_ref_noise,
                                                            t_ref_noise / t_noise, t_noise_x))
    print("    compute_regularization HIP %.3f ms vs libtorch + autograd + item() %.3f ms (%.0fx)"
          % (t_reg, t_ref_reg, t_ref_reg / t_reg))
    del m, dm

    # (c) relocation, cap 5 %
    for nn in (1_000_000, 6_000_000):
        ours = model_of(nn, 16)
        opa0 = ours.opacities.clone()
        fresh = lambda: ours.opacities.copy_(opa0)
        t_ours = gpu_ms(lambda: ctrl.relocate(ours, 500), 10, 2, fresh)
        fresh()
        st_ = ctrl.relocate(ours, 500)
        ref = model_of(nn, 16)
        fresh_ref = lambda: ref.opacities.copy_(opa0)
        t_ref = gpu_ms(lambda: ref_relocate(ref, 5.0, 0.05), 5, 1, fresh_ref)
        print("(c) relocate %d M (dead %d, moved %d): HIP incl. the stats read-back %.3f ms vs libtorch %.3f ms (%.0fx)"
              % (nn // 1_000_000, st_.num_dead, st_.num_relocated, t_ours, t_ref, t_ref / t_ours))
        del ours, ref, opa0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
