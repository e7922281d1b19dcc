#!/usr/bin/env python3
"""Times sparse Adam on one MI355X, on the config-4 model and view (6 M Gaussians, SH 3, 1600x1063):
  fused       cugs_project_backward_adam_opts dense vs cugs_projection_opts.sparse on the same accumulator rows;
  stand-alone cugs_fused_adam_groups (dense) vs cugs_fused_adam_groups_rows on the same five gradient tensors,
for visible fractions 1.0, 0.5 and 0.1, the invisible rows one contiguous block or scattered (a random subset).  Rows
are made invisible by negating their z; x and y are shrunk by 0.9 first so that no other Gaussian is culled and the
fractions are what the table says (the measured share of radii > 0 is printed beside them).

Dense and sparse alternate in one process: every round times a window of back-to-back launches of each, and a figure
is the median over the rounds with [min .. max] beside it; the dense launch is the yardstick (it is the parent's code:
the dense instantiations are unchanged).  Needs a GPU; there is no CPU fallback.

Bytes the algorithm needs (per case, printed beside the time):
  fused       N * 4 (every thread reads its radius) + N_invisible * 8 (the (0, 0) row of dL_dmeans_2d)
              + N_visible * DENSE_FUSED_BYTES
  stand-alone N * 4 + N_visible * 59 floats * 28 B
DENSE_FUSED_BYTES = 1469 at 16 coefficients: read 12 position + 40 gradient-row words 0..9 + 4 radius + 1 gate
+ 12 scales + 16 rotation + 4 opacity + 3 * 192 SH (parameter, m, v) + 2 * 44 geometry moments = 753; written
3 * 192 SH + 3 * 44 geometry + 8 dL_dmeans_2d = 716.  What HBM really moves depends on which 64-byte and 128-byte
lines stay untouched: a scattered invisible row saves whole lines of its 192-byte SH rows, and little of the 4- to
16-byte-per-row streams, whose lines it shares with visible neighbours."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

DENSE_FUSED_BYTES = 753 + 716
ROW_FLOATS = 3 + 48 + 1 + 3 + 4
CASES = ((1.0, "contiguous"), (0.5, "contiguous"), (0.5, "scattered"), (0.1, "contiguous"), (0.1, "scattered"))


def windows(fns, rounds, per_window, warmup):
    """[[ms per launch of fn, one entry per round] for fn in fns], the fns alternating round by round."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_window):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) / per_window)
    return out


def stat(ts):
    s = sorted(ts)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=6_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--per-window", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_adam: needs a GPU (there is no CPU fallback)")
    pkg = ge.load_package()
    from cugs_amd import _lib
    from cugs_amd._lib import AdamGroup, check, lib
    dev = torch.device("cuda:0")
    n, w, h = args.n, 1600, 1063
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=3, seed=4, mu_s=-4.6)
    arrays["positions"][:, :2] *= 0.9
    cam = pkg.scene.make_camera(w, h)
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=3)
    m = pkg.scene.to_model(arrays, dev)
    del arrays
    z0 = m.positions[:, 2].clone()
    opt = pkg.FusedAdam(m)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(w, h)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    names = opt._names
    grads = [torch.randn(getattr(m, k).shape, generator=gen, device=dev) * 1e-4 for k in names]
    perm = torch.randperm(n, generator=gen, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dm = torch.empty((n, 2), device=dev)
    cam_abi = cam.to_abi()
    groups = (AdamGroup * 5)()
    for i, k in enumerate(names):
        p = getattr(m, k)
        groups[i].param, groups[i].grad, groups[i].m, groups[i].v = (t.data_ptr() for t in (p, grads[i], opt.m_[i], opt.v_[i]))
        groups[i].n, groups[i].lr = p.numel(), 1e-6
    row_elems = (C.c_int32 * 5)(3, 48, 1, 3, 4)

    print("bench_sparse_adam: n %d, %dx%d, %d rounds of %d launches; ms = median [min .. max] over the rounds" %
          (n, w, h, args.rounds, args.per_window))
    print("%-18s %8s | %-26s %-26s %7s | %9s %9s" % ("case", "visible", "dense ms", "sparse ms", "ratio", "MB needed",
                                                      "GB/s"))
    for frac, layout in CASES:
        k = n - int(round(frac * n))                             # invisible rows
        m.positions[:, 2] = z0
        if k:
            rows = torch.arange(n - k, n, device=dev) if layout == "contiguous" else perm[:k]
            m.positions[rows, 2] *= -1.0
        out = pkg.render(m, cam, settings)
        torch.cuda.synchronize()
        vis = int((out.radii > 0).sum().item())
        rb = pkg.rasterizer.rasterize_backward(g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act,
                                               out.tile_ranges, out.gaussian_indices, out.final_T, out.n_contrib, w, h,
                                               settings.background, n, packed=out.packed, unpack=False)
        adam = opt.begin_fused_step()
        for i in range(5):
            adam.lr[i] = 1e-6                                    # many launches on one view: keep the model where it is
        base = (n, 16, 3, P(m.positions), P(m.rotations), P(m.scales), P(m.opacities), P(m.sh_coeffs), P(out.radii),
                P(out.colour_gate), C.byref(cam_abi), 1.0, P(rb.grad_accum), C.byref(adam), P(dm))
        opts = _lib.ProjectionOpts(sparse=1)
        dense = lambda: check(lib.cugs_project_backward_adam_opts(*base, None, st), "dense")
        sparse = lambda: check(lib.cugs_project_backward_adam_opts(*base, C.byref(opts), st), "sparse")
        hyper = (0.9, 0.999, 1e-15, adam.bc1, adam.bc2, st)
        dense_s = lambda: check(lib.cugs_fused_adam_groups(groups, 5, *hyper), "dense step")
        sparse_s = lambda: check(lib.cugs_fused_adam_groups_rows(groups, 5, row_elems, P(out.radii), n, *hyper), "rows")
        tag = "%.1f %s" % (frac, layout if k else "(all)")
        for what, fns, need in (("fused", (dense, sparse, dense), n * 4 + (n - vis) * 8 + vis * DENSE_FUSED_BYTES),
                                ("step", (dense_s, sparse_s, dense_s), n * 4 + vis * ROW_FLOATS * 28)):
            td, ts, td2 = (stat(t) for t in windows(fns, args.rounds, args.per_window, args.warmup))
            print("%-18s %7.1f%% | %-26s %-26s %6.3fx | %9.0f %9.0f   (dense again: %.3f)" %
                  (what + " " + tag, 100.0 * vis / n, "%.3f [%.3f .. %.3f]" % td, "%.3f [%.3f .. %.3f]" % ts,
                   ts[0] / td[0], need / 1e6, need / ts[0] / 1e6, td2[0]), flush=True)
        del out, rb


if __name__ == "__main__":
    main()
