#!/usr/bin/env python3
"""Cost of the fused depth-supervision loss at 1920x1080, the variants alternating in one process
after a warm-up, timed with device events around PER_ROUND back-to-back calls (no host sync inside a window):
  (a) depth_loss(D, A, t, weight=w)                     no alignment, depth space
  (b) depth_loss(D, A, t_inv, weight=w, inverse=True)   no alignment, inverse space
  (c) depth_loss(D, A, t, weight=w, align="fit")        the scale/shift fit on the device, four launches
  (d) the libtorch sequence (c) replaces: where, div, the masked five sums and the 2x2 solve (on the device, no
      read-back: the cheapest form of it), abs, sign and both gradients
Prints one JSON line: median ms per call of each over the rounds, the ratios to (d), min/max.  The results of (c) and (d)
are compared before anything is timed."""
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
        raise SystemExit("bench_depth_loss needs a GPU: nothing is measured without one")
    g = torch.Generator().manual_seed(5)
    z = 2.0 + 6.0 * torch.rand((H, W), generator=g)
    A = torch.rand((H, W), generator=g) * (torch.rand((H, W), generator=g) > 0.1).float()
    D = A * z
    t = (0.7 * z + 0.5 + 0.1 * torch.randn((H, W), generator=g)) * (torch.rand((H, W), generator=g) > 0.1).float()
    w = torch.rand((H, W), generator=g) * (torch.rand((H, W), generator=g) > 0.15).float()
    t_inv = torch.where(t > 0, 1.0 / t.clamp_min(1e-6), torch.zeros_like(t))
    D, A, t, t_inv, w = (x.to(dev).contiguous() for x in (D, A, t, t_inv, w))
    inv_n = 1.0 / float(H * W)

    def libtorch():
        valid = (A > MIN_ALPHA) & (w > 0) & (t > 0) & torch.isfinite(t)
        wv = torch.where(valid, w, torch.zeros_like(w))
        x = torch.where(valid, D / A.clamp_min(MIN_ALPHA), torch.zeros_like(D))
        wd, td, xd = wv.double(), t.double(), x.double()
        wt = wd * td
        Sw, St, Sx, Stt, Stx = wd.sum(), wt.sum(), (wd * xd).sum(), (wt * td).sum(), (wt * xd).sum()
        det = Sw * Stt - St * St
        s, b = ((Sw * Stx - St * Sx) / det).float(), ((Stt * Sx - St * Stx) / det).float()
        r = x - (s * t + b)
        loss = (wv * r.abs()).sum() * inv_n
        gx = wv * torch.sign(r) * inv_n
        safe = torch.where(valid, A, torch.ones_like(A))
        return loss, gx / safe, -(gx * x) / safe, s, b

    variants = {"a_depth": lambda: pkg.depth_loss(D, A, t, weight=w),
                "b_inverse": lambda: pkg.depth_loss(D, A, t_inv, weight=w, inverse=True),
                "c_fit": lambda: pkg.depth_loss(D, A, t, weight=w, align="fit"),
                "d_libtorch": libtorch}
    # the same numbers first
    fused, (loss, g_d, g_a, s, b) = variants["c_fit"](), libtorch()
    assert float(fused.fit_ok) == 1.0
    assert abs(float(fused.scale_shift[0]) - float(s)) <= 1e-5 and abs(float(fused.scale_shift[1]) - float(b)) <= 1e-5
    assert abs(float(fused.loss) - float(loss)) <= 1e-4 * float(loss), (float(fused.loss), float(loss))
    # a residual within rounding of 0 may take either sign: compare away from there
    far = (torch.where(A > MIN_ALPHA, D / A.clamp_min(MIN_ALPHA), torch.zeros_like(D)) - (s * t + b)).abs() > 1e-4
    assert float(((fused.dL_ddepth_map - g_d) * far).abs().max()) <= 1e-5 * float(g_d.abs().max())
    assert float(((fused.dL_dalpha - g_a) * far).abs().max()) <= 1e-5 * float(g_a.abs().max())
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
    print(json.dumps({"workload": "depth loss with scale/shift fit", "width": W, "height": H,
                      "per_call_ms": {k: round(v, 5) for k, v in med.items()},
                      "ratio_to_d": {k: round(med[k] / med["d_libtorch"], 4) for k in ("a_depth", "b_inverse", "c_fit")},
                      "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
                      "rounds": ROUNDS, "calls_per_round": PER_ROUND}))


if __name__ == "__main__":
    main()
