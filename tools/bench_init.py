#!/usr/bin/env python3
"""Times the point-cloud initialisation on one MI355X: cugs_knn_mean_distances on both routes and, as
the thing it replaces on the same GPU, the libtorch op sequence (cdist + topk in row chunks + sqrt / mean / log), on the
uniform and the blobs-plus-outliers cloud of tests/init_ref.py.

  python tools/bench_init.py [--sizes 50000,136000,1000000,6000000] [--exhaustive-max 6000000] [--torch-max 1000000]

An initialisation is called once, so the FIRST call (cold code objects, cold caches, workspace allocation) is reported
next to the steady state (median of `--reps` calls after it).  One JSON line per (cloud, size)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
import init_ref as ir

pkg = ge.load_package()
dev = torch.device("cuda:0")


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def first_and_steady(fn, reps):
    first = wall_ms(fn)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return round(first, 3), round(ts[len(ts) // 2], 3)


def torch_sequence(pos, k):
    """What one writes with libtorch ops: distances of a chunk of rows to every point, the k + 1 smallest (the point
    itself is one of them), mean of the square roots, logarithm."""
    out = torch.empty(pos.shape[0], device=pos.device)
    rows = max(256, min(4096, (1 << 30) // pos.shape[0]))                     # at most 4 GB of distances at a time
    for a in range(0, pos.shape[0], rows):
        d = torch.cdist(pos[a:a + rows], pos)
        best = torch.topk(d, k + 1, dim=1, largest=False).values[:, 1:]
        out[a:a + rows] = best.mean(dim=1)
    return torch.log(out.clamp_min(1e-7))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50000,136000,1000000,6000000")
    ap.add_argument("--clouds", default="uniform,blobs")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--exhaustive-max", type=int, default=6000000)
    ap.add_argument("--torch-max", type=int, default=1000000)
    args = ap.parse_args()
    for kind in args.clouds.split(","):
        for n in (int(s) for s in args.sizes.split(",")):
            pos_np, col_np = ir.make_cloud(kind, n, seed=5)
            pos, col = torch.from_numpy(pos_np).to(dev), torch.from_numpy(col_np).to(dev)
            row = {"cloud": kind, "n": n, "k": args.k}
            row["tree_first_ms"], row["tree_ms"] = first_and_steady(
                lambda: pkg.knn_mean_distances(pos, args.k, route="tree"), args.reps)
            if n <= args.exhaustive_max:
                reps = args.reps if n <= 1000000 else 1
                row["exhaustive_first_ms"], row["exhaustive_ms"] = first_and_steady(
                    lambda: pkg.knn_mean_distances(pos, args.k, route="exhaustive"), reps)
            row["init_first_ms"], row["init_ms"] = first_and_steady(
                lambda: pkg.init_gaussians_from_sparse(pos, col, 3, args.k, route="tree"), args.reps)
            if n <= args.torch_max:
                row["torch_first_ms"], row["torch_ms"] = first_and_steady(lambda: torch_sequence(pos, args.k),
                                                                         2 if n > 200000 else args.reps)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
