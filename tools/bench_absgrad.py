#!/usr/bin/env python3
"""Cost of the absolute 2-D mean gradients (AbsGrad) at BASELINE config 3: one render +
render_backward on the plain route, and the same with render_backward(..., want_abs_grad=True).  The two variants
alternate in one process after a warm-up and are timed with device events; the model stays put (no optimizer step).
Prints one JSON line: median ms per forward+backward of each and their ratio.  `--depth`: both variants also carry the
depth and alpha map gradients (the DEPTH kernel against the DEPTH + ABS kernel)."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda:0")
ROUNDS, PER_ROUND, WARMUP = 10, 10, 20


def main():
    with_depth = "--depth" in sys.argv[1:]
    wl = pkg.scene.CONFIGS["config3"]
    model = pkg.scene.to_model(pkg.scene.make_gaussians(wl.n, wl.width, wl.height, 3), dev)
    cam = pkg.scene.make_camera(wl.width, wl.height)
    settings = pkg.RenderSettings(active_sh_degree=3)
    dC = torch.from_numpy(pkg.scene.make_dl_dcolor(wl.width, wl.height)).to(dev)
    rng = np.random.default_rng(0)
    maps = {}
    if with_depth:
        maps = dict(dL_ddepth_map=torch.from_numpy(rng.standard_normal((wl.height, wl.width)).astype(np.float32)).to(dev),
                    dL_dalpha=torch.from_numpy(rng.standard_normal((wl.height, wl.width)).astype(np.float32)).to(dev))

    def step(absgrad):
        out = pkg.render(model, cam, settings, want_depth_map=with_depth)
        pkg.render_backward(dC, out, model, cam, settings, want_abs_grad=absgrad, **maps)

    for i in range(WARMUP):
        step(i % 2 == 1)
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for r in range(ROUNDS):
        for absgrad in ((False, True) if r % 2 == 0 else (True, False)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(PER_ROUND):
                step(absgrad)
            b.record()
            b.synchronize()
            times[absgrad].append(a.elapsed_time(b) / PER_ROUND)
    plain, absg = float(np.median(times[False])), float(np.median(times[True]))
    print(json.dumps({"workload": "config3 render+render_backward" + (" with depth and alpha maps" if with_depth else ""),
                      "n": wl.n, "width": wl.width, "height": wl.height,
                      "plain_ms": round(plain, 4), "abs_grad_ms": round(absg, 4), "ratio": round(absg / plain, 4),
                      "plain_ms_all": [round(x, 4) for x in times[False]],
                      "abs_grad_ms_all": [round(x, 4) for x in times[True]]}))


if __name__ == "__main__":
    main()
