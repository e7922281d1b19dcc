#!/usr/bin/env python3
"""Times the vector-quantisation kernels and compress_gaussians on one MI355X:
  assign      cugs_vq_assign (prologue + the MFMA kernel) at n in {1 M, 6 M}, k in {4096, 8192}, d = 45, beside the
              libtorch sequence it replaces: row-chunked x @ c.T, h - ., argmin (chunks of 65536 rows, so that the
              [rows, k] score matrix stays at 2 GB)
  trip count  the assign kernel at d = 9, 24, 45 (5, 12, 23 MFMA steps per tile), n = 1 M, k = 8192: a straight line
              t = a steps + b separates what scales with the MFMA count from what does not (the epilogue's compares,
              the LDS staging, the launch)
  update      cugs_vq_update beside index_add_ + divide, k = 8192
  compress    a whole compress_gaussians of the config-4 model (6 M Gaussians, 8192 codes, 10 iterations), its payload
              against the fp32 PLY's 59 floats per Gaussian, and of the config-3 model with the file written
  PSNR        render(decompressed) against render(original) on three config-3 views.  The synthetic scene's SH
              coefficients are independent normal draws - no two Gaussians share a colour lobe - so this is the worst
              case for a codebook; a trained model's bands cluster.  Information, not a bar.
kernel and libtorch alternate in one process: every round times a window of back-to-back calls of each, a figure is the
median over the rounds with [min .. max] beside it.  Needs a GPU; there is no CPU fallback.

FLOP: the assignment needs 2 n k d (useful); the kernel issues 2 n_pad k_pad 2 steps (d padded to an even length, n to
256 rows, k to 32 codes).  TFLOP/s = useful FLOP / time, beside the 155 TF the f32-input MFMA issues at on this part.
The MFMA floor is the time 4 SIMDs x 256 CUs need to issue the kernel's v_mfma_f32_32x32x2_f32 at 64 cycles each and
2.4 GHz."""
import argparse
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

MFMA_PEAK_TF = 155.0
CLOCK_HZ, SIMDS = 2.4e9, 4 * 256
CHUNK_ROWS = 65536


def windows(fns, rounds, per_window, warmup):
    """[[ms per call of fn, one entry per round] for fn in fns], the fns alternating round by round."""
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


def fmt(t):
    return "%.3f [%.3f .. %.3f]" % t


def steps_of(d):
    s = (d + 1) // 2
    return 5 if s <= 5 else 12 if s <= 12 else 23 if s <= 23 else 24


def mfma_floor_ms(n, k, d):
    tiles = ((n + 255) // 256 * 8) * ((k + 31) // 32)            # 32 x 32 result tiles
    return tiles * steps_of(d) * 64 / (SIMDS * CLOCK_HZ) * 1e3


def libtorch_assign(x, cb):
    h = 0.5 * (cb * cb).sum(1)
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for r0 in range(0, x.shape[0], CHUNK_ROWS):
        out[r0:r0 + CHUNK_ROWS] = torch.argmin(h - x[r0:r0 + CHUNK_ROWS] @ cb.T, dim=1)
    return out


def libtorch_update(x, assign64, k):
    num = torch.zeros((k, x.shape[1]), dtype=torch.float32, device=x.device).index_add_(0, assign64, x)
    den = torch.zeros(k, dtype=torch.float32, device=x.device).index_add_(0, assign64, torch.ones_like(x[:, 0]))
    return num / den.clamp_min(1.0)[:, None]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 6_000_000])
    ap.add_argument("--codes", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-window", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-compress", action="store_true", help="kernels only: no config-4 model, no PSNR")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vq: needs a GPU (there is no CPU fallback)")
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(5)
    print("bench_vq: %d rounds of %d calls; ms = median [min .. max] over the rounds" % (args.rounds, args.per_window))

    print("assign, d = 45 (23 MFMA steps per tile)")
    print("  %-9s %-6s %-26s %-26s %8s %8s %10s %10s %9s" % ("n", "k", "kernel ms", "libtorch ms", "speedup", "TFLOP/s",
                                                         "of %g TF" % MFMA_PEAK_TF, "MFMA floor", "same idx"))
    for n in args.sizes:
        x = 0.5 * torch.randn((n, 45), device=dev, generator=gen)
        for k in args.codes:
            cb = x[(torch.arange(k, device=dev) * n) // k].contiguous()
            tk, tl = (stat(t) for t in windows([lambda: pkg.vq_assign(x, cb), lambda: libtorch_assign(x, cb)],
                                               args.rounds, args.per_window, args.warmup))
            same = float((pkg.vq_assign(x, cb).to(torch.int64) == libtorch_assign(x, cb)).float().mean())
            tf = 2.0 * n * k * 45 / (tk[0] * 1e-3) / 1e12
            print("  %-9d %-6d %-26s %-26s %7.2fx %8.1f %9.0f%% %8.3f ms %8.4f%%" %
                  (n, k, fmt(tk), fmt(tl), tl[0] / tk[0], tf, 100.0 * tf / MFMA_PEAK_TF, mfma_floor_ms(n, k, 45),
                   100.0 * same), flush=True)
        del x
    torch.cuda.empty_cache()

    n, k = min(args.sizes), max(args.codes)
    print("trip count, n = %d, k = %d" % (n, k))
    pts = []
    for d in (9, 24, 45):
        x = 0.5 * torch.randn((n, d), device=dev, generator=gen)
        cb = x[(torch.arange(k, device=dev) * n) // k].contiguous()
        t = stat(windows([lambda: pkg.vq_assign(x, cb)], args.rounds, args.per_window, args.warmup)[0])
        pts.append((steps_of(d), t[0]))
        print("  d = %-3d steps = %-3d %-26s MFMA floor %.3f ms" % (d, steps_of(d), fmt(t), mfma_floor_ms(n, k, d)), flush=True)
    (s0, t0), (s2, t2) = pts[0], pts[2]
    slope = (t2 - t0) / (s2 - s0)
    print("  line through the ends: %.4f ms per step + %.3f ms; the floor's slope is %.4f ms per step; at 23 steps "
          "%.0f%% of the time scales with the MFMA count" %
          (slope, t0 - slope * s0, mfma_floor_ms(n, k, 45) / 23, 100.0 * slope * 23 / t2))

    print("update, k = %d, d = 45" % k)
    print("  %-9s %-26s %-26s %8s" % ("n", "kernel ms", "index_add_ + divide ms", "speedup"))
    for n in args.sizes:
        x = 0.5 * torch.randn((n, 45), device=dev, generator=gen)
        cb = x[(torch.arange(k, device=dev) * n) // k].contiguous()
        assign = pkg.vq_assign(x, cb)
        assign64 = assign.to(torch.int64)
        bits = pkg.vq_frac_bits(n, float(x.abs().max()))
        ws = torch.empty(int(pkg._lib.lib.cugs_vq_workspace_bytes(k, 45)), dtype=torch.uint8, device=dev)
        work = cb.clone()
        tk, tl = (stat(t) for t in windows([lambda: pkg.vq_update(x, assign, work, bits, workspace=ws),
                                            lambda: libtorch_update(x, assign64, k)],
                                           args.rounds, max(args.per_window, 5), args.warmup))
        print("  %-9d %-26s %-26s %7.2fx" % (n, fmt(tk), fmt(tl), tl[0] / tk[0]), flush=True)
        del x
    torch.cuda.empty_cache()
    if args.skip_compress:
        return

    for name in ("config3", "config4"):
        wl = pkg.scene.CONFIGS[name]
        model = pkg.scene.to_model(pkg.scene.make_gaussians(wl.n, wl.width, wl.height, sh_degree=wl.sh_degree, seed=4,
                                                            mu_s=wl.mu_s), dev)
        pkg.compress_gaussians(model, sh_codes=64, iters=1)                      # warm the code paths
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cm = pkg.compress_gaussians(model, sh_codes=8192, iters=10)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        ply = wl.n * 59 * 4
        print("compress_gaussians %s (%s): %.3f s for 8192 codes, 10 iterations; payload %d bytes = %.1f%% of the fp32 "
              "PLY's %d (%.2fx smaller)" % (name, wl.name, sec, pkg.nbytes(cm), 100.0 * pkg.nbytes(cm) / ply, ply,
                                            ply / pkg.nbytes(cm)), flush=True)
        if name == "config3":
            with tempfile.TemporaryDirectory() as tmp:
                size = pkg.write_compressed(os.path.join(tmp, "model.npz"), cm)
            print("  written file: %d bytes" % size)
            back = pkg.decompress_gaussians(cm)
            settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=3)
            for view in range(3):
                cam = pkg.scene.make_camera(wl.width, wl.height, view)
                a, b = pkg.render(model, cam, settings).color, pkg.render(back, cam, settings).color
                print("  view %d: PSNR of render(decompressed) against render(original) %.2f dB (random SH: the worst "
                      "case for a codebook)" % (view, pkg.compute_psnr(b.clamp(0, 1), a.clamp(0, 1))), flush=True)
            del back
        del model, cm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
