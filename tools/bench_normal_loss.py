#!/usr/bin/env python3
"""Cost of the fused normal-supervision loss at 1920x1080, the variants alternating in one process
after a warm-up, timed with device events around PER_ROUND back-to-back calls (no host sync inside a window):
  (a) normal_loss(D, A, cam, t)                                    prior only
  (b) normal_loss(D, A, cam, t, weight=w)                          with a weight map
  (c) normal_loss(D, A, cam, t, weight=w, want_normals=True)       and the normal map
  (d) depth_to_normals(D, A, cam)                                  no prior: the normal map alone
  (e) the libtorch sequence (b) replaces: where, div, the back-projection, four slices, cross, norm, the masks, the
      cosine distance, and the autograd backward through all of it to the two maps
  (f) depth_loss(D, A, t_depth, weight=w)                          the yardstick: one flat pass over the same image
Prints one JSON line: median ms per call of each over the rounds, the ratios to (e), min/max.  The results of (b) and
(e) are compared before anything is timed."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda:0")
W, H = 1920, 1080
ROUNDS, PER_ROUND, WARMUP = 10, 10, 20
MIN_ALPHA = 1e-3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_normal_loss needs a GPU: nothing is measured without one")
    g = torch.Generator().manual_seed(5)
    fx = fy = 0.78 * W
    cx, cy = 0.5 * W + 0.7, 0.5 * H - 0.4
    cam = pkg.CameraInfo(width=W, height=H, intrinsics=pkg.CameraIntrinsics(fx=fx, fy=fy, cx=cx, cy=cy))
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    x, y = (u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy
    z = (3.0 + 0.8 * x - 0.5 * y + 0.05 * torch.sin(9.0 * x + 1.0) * torch.cos(7.0 * y)).float()
    A = (0.5 + 0.5 * torch.rand((H, W), generator=g)) * (torch.rand((H, W), generator=g) > 0.05).float()
    D = A * z
    t = 0.4 * torch.randn((3, H, W), generator=g)
    t[2] -= 1.0
    t = t * (torch.rand((1, H, W), generator=g) > 0.1).float()
    w = torch.rand((H, W), generator=g) * (torch.rand((H, W), generator=g) > 0.15).float()
    D, A, t, w, z = (a.to(dev).contiguous() for a in (D, A, t, w, z))
    ax = ((torch.arange(W, device=dev, dtype=torch.float32) + 0.5) - cx) / fx
    ay = ((torch.arange(H, device=dev, dtype=torch.float32) + 0.5) - cy) / fy
    inv_n = 1.0 / float(H * W)

    def libtorch():
        Dg, Ag = D.detach().requires_grad_(), A.detach().requires_grad_()
        ok = Ag.detach() > MIN_ALPHA
        d = torch.where(ok, Dg / torch.where(ok, Ag, torch.ones_like(Ag)), torch.zeros_like(Dg))
        P = torch.stack([ax[None, :] * d, ay[:, None] * d, d], -1)
        Px, Py = P[1:-1, 2:] - P[1:-1, :-2], P[2:, 1:-1] - P[:-2, 1:-1]
        n = torch.cross(Py, Px, dim=-1)
        nn = (n * n).sum(-1)
        ti = t[:, 1:-1, 1:-1].permute(1, 2, 0)
        tt = (ti * ti).sum(-1)
        valid = (ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1] & (nn.detach() > 0)
                 & torch.isfinite(nn.detach()) & (w[1:-1, 1:-1] > 0) & (tt > 0) & torch.isfinite(tt))
        nh = n / torch.where(valid, nn, torch.ones_like(nn)).sqrt()[..., None]
        th = ti / torch.where(valid, tt, torch.ones_like(tt)).sqrt()[..., None]
        ell = torch.where(valid, w[1:-1, 1:-1] * (1.0 - (nh * th).sum(-1)), torch.zeros_like(nn))
        loss = ell.sum() * inv_n
        loss.backward()
        return loss.detach(), Dg.grad, Ag.grad

    t_depth = z * (torch.rand((H, W), device=dev) > 0.1).float()
    variants = {"a_prior": lambda: pkg.normal_loss(D, A, cam, t),
                "b_weight": lambda: pkg.normal_loss(D, A, cam, t, weight=w),
                "c_weight_normals": lambda: pkg.normal_loss(D, A, cam, t, weight=w, want_normals=True),
                "d_normals_only": lambda: pkg.depth_to_normals(D, A, cam),
                "e_libtorch": libtorch,
                "f_depth_loss": lambda: pkg.depth_loss(D, A, t_depth, weight=w)}
    # the same numbers first: float32 autograd against the fused pass, both ~1e-4 of the scale from the exact values at
    # this focal length (differences of neighbouring depths cancel four digits)
    fused, (loss, g_d, g_a) = variants["b_weight"](), libtorch()
    assert float(fused.valid_count) > 0.5 * H * W
    dev_d = float((fused.dL_ddepth_map - g_d).abs().max()) / float(g_d.abs().max())
    dev_a = float((fused.dL_dalpha - g_a).abs().max()) / float(g_a.abs().max())
    print(f"fused vs float32 autograd: loss {float(fused.loss):.8g} vs {float(loss):.8g}, gradients {dev_d:.2e} and "
          f"{dev_a:.2e} of the maximum", file=sys.stderr)
    assert abs(float(fused.loss) - float(loss)) <= 1e-3 * float(loss) and dev_d <= 1e-2 and dev_a <= 1e-2
    order = list(variants)
    for _ in range(WARMUP):
        for name in order:
            variants[name]()
    torch.cuda.synchronize()
    times = {name: [] for name in order}
    for rnd in range(ROUNDS):
        k = rnd % len(order)
        for name in (order[k:] + order[:k]):
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(PER_ROUND):
                variants[name]()
            b_.record()
            b_.synchronize()
            times[name].append(a.elapsed_time(b_) / PER_ROUND)
    med = {name: float(np.median(v)) for name, v in times.items()}
    print(json.dumps({"workload": "normal loss from the rendered depth", "width": W, "height": H,
                      "per_call_ms": {k: round(v, 5) for k, v in med.items()},
                      "ratio_to_e": {k: round(med[k] / med["e_libtorch"], 4) for k in order if k != "e_libtorch"},
                      "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
                      "rounds": ROUNDS, "calls_per_round": PER_ROUND}))


if __name__ == "__main__":
    main()
