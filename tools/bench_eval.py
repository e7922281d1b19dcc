#!/usr/bin/env python3
"""Cost of the evaluation metrics of one 1920x1080 view, three variants alternating in one process
after a warm-up, timed with device events around PER_ROUND back-to-back calls (no host sync inside a window):
  (a) eval_metrics(rendered, float target)            24 B/pixel read
  (b) eval_metrics(rendered, 8-bit cached target)     15 B/pixel read
  (c) what the package offered before it: image_to_float(cached view) + combined_loss (for the mean SSIM: it also writes
      three derivative maps) + (rendered - target).pow(2).mean() (the reference's MSE, metrics.cpp:27).
Prints one JSON line: median ms per call of each, the ratios to (c), and the bytes/s the two kernels' algorithmic
traffic amounts to at that time (a figure of the whole call, launches included - not a kernel's share of peak).  The
results of (a) and (b) are compared with (c)'s before anything is timed."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda:0")
W, H = 1920, 1080
ROUNDS, PER_ROUND, WARMUP = 10, 300, 50


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval needs a GPU: nothing is measured without one")
    g = torch.Generator().manual_seed(3)
    u8 = (torch.rand((H, W, 3), generator=g) * 255.0).round().to(torch.uint8).to(dev)
    tf = pkg.image_to_float(u8, W, H)
    r = (tf + 0.05 * torch.randn((H, W, 3), generator=g).to(dev)).clamp(0, 1)
    out = torch.empty(4, device=dev)

    def today():
        t = pkg.image_to_float(u8, W, H)
        return pkg.loss._run(r, t, 0.2, 11, False, False)[0], (r - t).pow(2).mean()

    variants = {"a_f32": lambda: pkg.eval_metrics(r, tf, out=out),
                "b_u8": lambda: pkg.eval_metrics(r, u8, out=out),
                "c_today": today}
    # the same numbers first: SSIM bit for bit, the MSE up to torch's float32 summation
    loss_out, mse = today()
    for name in ("a_f32", "b_u8"):
        row = variants[name]().cpu().numpy()
        assert row[1].tobytes() == loss_out[2].cpu().numpy().tobytes(), (name, row, loss_out)
        assert abs(float(row[0]) - float(mse)) <= 1e-5 * float(mse), (name, row, float(mse))
    order = list(variants)
    for _ in range(WARMUP):
        for name in order:
            variants[name]()
    torch.cuda.synchronize()
    times = {name: [] for name in order}
    for rnd in range(ROUNDS):
        for name in (order[rnd % 3:] + order[:rnd % 3]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(PER_ROUND):
                variants[name]()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / PER_ROUND)
    med = {name: float(np.median(v)) for name, v in times.items()}
    px = W * H
    print(json.dumps({"workload": "evaluation metrics of one view", "width": W, "height": H,
                      "per_call_ms": {k: round(v, 5) for k, v in med.items()},
                      "ratio_to_c": {k: round(med[k] / med["c_today"], 4) for k in ("a_f32", "b_u8")},
                      "algorithmic_GBps": {"a_f32": round(24 * px / med["a_f32"] / 1e6, 1),
                                           "b_u8": round(15 * px / med["b_u8"] / 1e6, 1)},
                      "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
                      "rounds": ROUNDS, "calls_per_round": PER_ROUND}))


if __name__ == "__main__":
    main()
