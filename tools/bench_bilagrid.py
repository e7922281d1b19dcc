#!/usr/bin/env python3
"""Cost of the bilateral-grid colour correction at 1920x1080 with a (16,16,8) grid, the fused kernels
and the libtorch sequence they replace alternating in one process after a warm-up, timed with device events around
PER_ROUND back-to-back calls (no host sync inside a window):
  (a) combined_loss_and_grad(rendered, target)        the plain loss: csrc/loss.hip is untouched by this feature, so these
                                                      are the parent's kernels - timed beside the rest as the fixed point
  (b) bilagrid_slice(grid, rendered)
  (c) bilagrid_slice_backward(grid, rendered, g)      both gradients
  (d) bilagrid_slice_backward(..., want_grid_grad=False)    the image gradient alone
  (e) bilagrid_tv(grid, dL_dgrid=buffer)
  (f) libtorch forward: grid_sample on the 5-D tensor + einsum, on the same tensors
  (g) libtorch forward + autograd backward (the grid gradient scattered with float atomics)
  (h) libtorch TV value + autograd gradient
Prints one JSON line: median ms per call of each, min/max over the rounds, the ratios fused / libtorch, and each fused
kernel group's algorithmic bytes per second (bytes computed from the shapes below, over the call time - an end-to-end
rate that includes the launch gaps, not a kernel's share of peak).  The results of the two routes are compared before
anything is timed."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import __graft_entry__ as ge
import bilagrid_ref as br

pkg = ge.load_package()
W, H = 1920, 1080
GRID_SHAPE = (16, 16, 8)                      # GX, GY, L
ROUNDS, PER_ROUND, WARMUP = 10, 50, 10


def make_rendered(target, gen, levels):
    """The target plus noise, in [0.02, 0.98], then moved along (1, 1, 1) so that the fractional part of luma (L-1) lies
    in [0.05, 0.95] (tests/bilagrid_ref.py: case): the derivative along z jumps where luma (L-1) is an integer, and two
    fp32 evaluations that round luma differently land on either side of such a kink at a few of 2 M pixels - the
    agreement check below would then measure the jump, not the kernels."""
    r = (target + 0.05 * torch.randn(target.shape, generator=gen)).clamp(0.02, 0.98).double()
    zs = (r @ torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64)) * (levels - 1)
    frac = zs - zs.floor()
    return (r + ((frac.clamp(0.05, 0.95) - frac) / (levels - 1)).unsqueeze(-1)).float()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_bilagrid needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    gx, gy, l = GRID_SHAPE
    t = torch.rand((H, W, 3), generator=gen).to(dev)
    r = make_rendered(t.cpu(), gen, l).to(dev)
    g =(torch.randn((H, W, 3), generator=gen) / (3 * H * W)).to(dev)
    grid = (torch.from_numpy(br.identity_grid(GRID_SHAPE)) + 0.1 * torch.randn((12, l, gy, gx), generator=gen)).contiguous().to(dev)
    buf = torch.zeros_like(grid)

    def lt_forward():
        with torch.no_grad():
            return br.torch_slice(grid, r)

    def lt_backward():
        G, c = grid.detach().requires_grad_(True), r.detach().requires_grad_(True)
        return torch.autograd.grad(br.torch_slice(G, c), (G, c), g)

    def lt_tv():
        G = grid.detach().requires_grad_(True)
        tv = br.torch_tv(G)
        return tv, torch.autograd.grad(tv, G)[0]

    variants = {"a_plain_loss": lambda: pkg.combined_loss_and_grad(r, t),
                "b_slice": lambda: pkg.bilagrid_slice(grid, r),
                "c_backward": lambda: pkg.bilagrid_slice_backward(grid, r, g),
                "d_backward_image_only": lambda: pkg.bilagrid_slice_backward(grid, r, g, want_grid_grad=False),
                "e_tv": lambda: pkg.bilagrid_tv(grid, weight=10.0, dL_dgrid=buf),
                "f_libtorch_forward": lt_forward,
                "g_libtorch_forward_backward": lt_backward,
                "h_libtorch_tv": lt_tv}
    # the same numbers first (libtorch in fp32: its own rounding and its atomics' order are in these bars)
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    back, (lt_dg, lt_dc) = variants["c_backward"](), lt_backward()
    check = {"corrected": rel(variants["b_slice"](), lt_forward()), "dL_drendered": rel(back.dL_drendered, lt_dc),
             "dL_dgrid": rel(back.dL_dgrid, lt_dg), "tv": rel(pkg.bilagrid_tv(grid)[0], lt_tv()[0].detach())}
    assert check["corrected"] <= 1e-5 and check["dL_drendered"] <= 1e-4 and check["dL_dgrid"] <= 1e-3 and check["tv"] <= 1e-5, check
    order = list(variants)
    for _ in range(WARMUP):
        for name in order:
            variants[name]()
    torch.cuda.synchronize()
    times = {name: [] for name in order}
    for rnd in range(ROUNDS):
        k = rnd % len(order)
        for name in (order[k:] + order[:k]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(PER_ROUND):
                variants[name]()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / PER_ROUND)
    med = {name: float(np.median(v)) for name, v in times.items()}
    px, ge_ = H * W, 12 * l * gy * gx
    ws = int(pkg._lib.lib.cugs_bilagrid_workspace_bytes(W, H, pkg._lib.BilagridDims(l=l, gy=gy, gx=gx)))
    # algorithmic bytes: the slice reads and writes one image; the image gradient reads two and writes one; the cell
    # kernel reads two and writes the partials, the combine reads them and writes the grid
    nbytes = {"b_slice": 24 * px, "d_backward_image_only": 36 * px, "c_backward": 36 * px + 24 * px + 2 * ws + 4 * ge_}
    print(json.dumps({"workload": "bilateral grid slice / backward / tv", "width": W, "height": H, "grid_shape": GRID_SHAPE,
                      "per_call_ms": {k: round(v, 5) for k, v in med.items()},
                      "ratio_fused_to_libtorch": {"forward": round(med["b_slice"] / med["f_libtorch_forward"], 4),
                                                  "forward_backward": round((med["b_slice"] + med["c_backward"]) /
                                                                            med["g_libtorch_forward_backward"], 4),
                                                  "tv": round(med["e_tv"] / med["h_libtorch_tv"], 4)},
                      "algorithmic_GBps": {k: round(v / (med[k] * 1e-3) / 1e9, 1) for k, v in nbytes.items()},
                      "workspace_bytes": ws, "agreement_with_libtorch_fp32": {k: float(f"{v:.2e}") for k, v in check.items()},
                      "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
                      "rounds": ROUNDS, "calls_per_round": PER_ROUND}))


if __name__ == "__main__":
    main()
