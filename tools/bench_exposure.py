#!/usr/bin/env python3
"""Cost of exposure compensation and pixel masks in the fused loss at 1920x1080, four variants
alternating in one process after a warm-up, timed with device events around PER_ROUND back-to-back calls (no host sync
inside a window):
  (a) combined_loss_and_grad(rendered, target)                         the plain route, untouched by this feature
  (b) combined_loss_exposure(rendered, target, exposure=E)             fused: dL_dcolor and dL_dexposure
  (c) combined_loss_exposure(rendered, target, exposure=E, mask=m)     fused, with a mask
  (d) the libtorch sequence (b)/(c) replace: x' = (color @ A.T + b) * m, y' = target * m, combined_loss_and_grad(x', y'),
      dL_dcolor = (g @ A) * m, dL_dE = einsum over the pixels (the b column as the sum of m g)
Prints one JSON line: median ms per call of each, the ratios, min/max over the rounds.  The results of (c) and (d) are
compared before anything is timed."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda:0")
W, H = 1920, 1080
ROUNDS, PER_ROUND, WARMUP = 12, 200, 50


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_exposure needs a GPU: nothing is measured without one")
    g = torch.Generator().manual_seed(3)
    t = torch.rand((H, W, 3), generator=g).to(dev)
    r = (t + 0.05 * torch.randn((H, W, 3), generator=g).to(dev)).clamp(0, 1)
    E = (torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1) + 0.1 * torch.randn((3, 4), generator=g)).contiguous().to(dev)
    m = ((torch.rand((H, W), generator=g) > 0.3).float() * torch.rand((H, W), generator=g).clamp(0.25, 1.0)).to(dev)

    def libtorch():
        A, b, m3 = E[:, :3], E[:, 3], m.unsqueeze(-1)
        x = (r @ A.T + b) * m3
        y = t * m3
        loss, gx = pkg.combined_loss_and_grad(x, y)
        gm = gx * m3
        d_color = gm @ A
        d_E = torch.cat([torch.einsum("hwi,hwj->ij", gm, r), gm.sum(dim=(0, 1)).unsqueeze(1)], dim=1)
        return loss, d_color, d_E

    variants = {"a_plain": lambda: pkg.combined_loss_and_grad(r, t),
                "b_exposure": lambda: pkg.combined_loss_exposure(r, t, exposure=E),
                "c_exposure_mask": lambda: pkg.combined_loss_exposure(r, t, exposure=E, mask=m),
                "d_libtorch": libtorch}
    # the same numbers first
    fused, (loss, d_color, d_E) = variants["c_exposure_mask"](), libtorch()
    assert abs(float(fused.loss) - float(loss)) <= 1e-5, (float(fused.loss), float(loss))
    assert float((fused.dL_dcolor - d_color).abs().max()) <= 1e-4 * float(d_color.abs().max())
    assert float((fused.dL_dexposure - d_E).abs().max()) <= 1e-3 * float(d_E.abs().max())   # torch sums 2M terms in fp32
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
    print(json.dumps({"workload": "combined loss with exposure and mask", "width": W, "height": H,
                      "per_call_ms": {k: round(v, 5) for k, v in med.items()},
                      "ratio_to_d": {k: round(med[k] / med["d_libtorch"], 4) for k in ("b_exposure", "c_exposure_mask")},
                      "ratio_to_a": {k: round(med[k] / med["a_plain"], 4) for k in ("b_exposure", "c_exposure_mask")},
                      "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
                      "rounds": ROUNDS, "calls_per_round": PER_ROUND}))


if __name__ == "__main__":
    main()
