#!/usr/bin/env python3
"""Times transform_gaussians on one MI355X, on the config-3 model (1 M Gaussians) and the config-4 model
(6 M), SH degree 3:
  kernel      cugs_transform_gaussians, one launch: unmasked; half the rows masked out as one block; the same half
              scattered (a random subset)
  libtorch    the sequence it replaces, out of place and unmasked: positions @ M^T + t, the quaternion product by column
              slices, three per-band matmuls on SH slices, scales + log s
  clone       a plain clone of the same five tensors: the bandwidth yardstick of the box
all alternating in one process: every round times a window of back-to-back launches of each, and a figure is the median
over the rounds with [min .. max] beside it.  Successive kernel launches alternate between a similarity and its inverse,
so the model stays where it is.  Needs a GPU; there is no CPU fallback.

Bytes (per case, printed beside the time): the kernel moves 2 * 59 floats per transformed row (positions 3, rotations 4,
scales 3, SH 3 * 16 in and out, less the DC terms where they are not rewritten - counted in full here) plus one mask byte
per row where there is a mask; the clone moves 2 * 60 floats per row.  GB/s = bytes / time, against the clone's and
against the 6.3 TB/s a float4 copy reaches on this part (8 TB/s spec)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

ACHIEVABLE_TBS = 6.3
ROW_BYTES = 2 * 59 * 4
CLONE_ROW_BYTES = 2 * 60 * 4


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


def libtorch_sequence(m, M, t, q, D, log_s):
    """The eager route: a dozen ops and their temporaries, new tensors out."""
    pos = m.positions @ M.T + t
    w, x, y, z = (m.rotations[:, i] for i in range(4))
    rot = torch.stack([q[0] * w - q[1] * x - q[2] * y - q[3] * z, q[0] * x + q[1] * w + q[2] * z - q[3] * y,
                       q[0] * y - q[1] * z + q[2] * w + q[3] * x, q[0] * z + q[1] * y - q[2] * x + q[3] * w], dim=1)
    sh = torch.cat([m.sh_coeffs[:, :, :1], m.sh_coeffs[:, :, 1:4] @ D[0].T, m.sh_coeffs[:, :, 4:9] @ D[1].T,
                    m.sh_coeffs[:, :, 9:16] @ D[2].T], dim=2)
    return pos, rot, sh, m.scales + log_s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 6_000_000])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--per-window", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transform: needs a GPU (there is no CPU fallback)")
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    q = np.array([0.8, 0.2, -0.4, 0.4])
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    sim = pkg.Similarity(1.25, R, [0.5, -0.25, 1.0])
    sims = (sim, sim.inverse())
    xf = sim.to_abi()
    f = lambda a, shape=None: torch.tensor(np.array(a, dtype=np.float32).reshape(shape or -1), device=dev)
    lt = (f(xf.m, (3, 3)), f(xf.t), f(xf.q), [f(xf.d1, (3, 3)), f(xf.d2, (5, 5)), f(xf.d3, (7, 7))], float(xf.log_scale))
    print("bench_transform: %d rounds of %d launches; ms = median [min .. max] over the rounds" %
          (args.rounds, args.per_window))
    for n in args.sizes:
        wl = {1_000_000: (1920, 1080), 6_000_000: (1600, 1063)}.get(n, (1920, 1080))
        m = pkg.scene.to_model(pkg.scene.make_gaussians(n, wl[0], wl[1], sh_degree=3, seed=4, mu_s=-4.6), dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        block = torch.arange(n, device=dev) < n // 2
        scattered = torch.zeros(n, dtype=torch.bool, device=dev)
        scattered[torch.randperm(n, generator=gen, device=dev)[:n // 2]] = True
        calls = {"k": 0}

        def kernel(mask):
            def run():
                pkg.transform_gaussians(m, sims[calls["k"] & 1], mask=mask)
                calls["k"] += 1
            return run
        clone = lambda: [getattr(m, k).clone() for k in ("positions", "sh_coeffs", "opacities", "rotations", "scales")]
        eager = lambda: libtorch_sequence(m, *lt)
        cases = (("kernel unmasked", kernel(None), n * ROW_BYTES),
                 ("kernel half, one block", kernel(block), n + (n // 2) * ROW_BYTES),
                 ("kernel half, scattered", kernel(scattered), n + (n // 2) * ROW_BYTES),
                 ("libtorch sequence", eager, n * ROW_BYTES),
                 ("clone of 5 tensors", clone, n * CLONE_ROW_BYTES))
        # an even number of launches per case: every window ends on the inverse, the model back where it started
        per = args.per_window + (args.per_window & 1)
        warm = args.warmup + (args.warmup & 1)
        times = [stat(t) for t in windows([c[1] for c in cases], args.rounds, per, warm)]
        clone_rate = cases[-1][2] / times[-1][0]
        print("n = %d" % n)
        print("  %-24s %-26s %9s %9s %9s %11s" % ("case", "ms", "MB moved", "GB/s", "of clone", "of %.1f TB/s" % ACHIEVABLE_TBS))
        for (name, _, need), t in zip(cases, times):
            rate = need / t[0]                                       # bytes per ms
            print("  %-24s %-26s %9.0f %9.0f %8.0f%% %10.0f%%" %
                  (name, "%.3f [%.3f .. %.3f]" % t, need / 1e6, rate / 1e6, 100.0 * rate / clone_rate,
                   100.0 * rate / 1e6 / (ACHIEVABLE_TBS * 1e3)), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
