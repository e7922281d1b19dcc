#!/usr/bin/env python3
"""Cost of the depth and alpha maps at BASELINE config 3: one render + render_backward with the
colour image only, and the same with render(..., want_depth_map=True) and render_backward(..., dL_ddepth_map=,
dL_dalpha=).  The two variants alternate in one process after a warm-up and are timed with device events; the model
stays put (no optimizer step).  Prints one JSON line: median ms per forward+backward of each and their ratio."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda:0")
ROUNDS, PER_ROUND, WARMUP = 10, 10, 20


def main():
    wl = pkg.scene.CONFIGS["config3"]
    model = pkg.scene.to_model(pkg.scene.make_gaussians(wl.n, wl.width, wl.height, 3), dev)
    cam = pkg.scene.make_camera(wl.width, wl.height)
    settings = pkg.RenderSettings(active_sh_degree=3)
    dC = torch.from_numpy(pkg.scene.make_dl_dcolor(wl.width, wl.height)).to(dev)
    rng = np.random.default_rng(0)
    dD = torch.from_numpy(rng.standard_normal((wl.height, wl.width)).astype(np.float32)).to(dev)
    dA = torch.from_numpy(rng.standard_normal((wl.height, wl.width)).astype(np.float32)).to(dev)

    def step(depth):
        if depth:
            out = pkg.render(model, cam, settings, want_depth_map=True)
            pkg.render_backward(dC, out, model, cam, settings, dL_ddepth_map=dD, dL_dalpha=dA)
        else:
            out = pkg.render(model, cam, settings)
            pkg.render_backward(dC, out, model, cam, settings)

    for i in range(WARMUP):
        step(i % 2 == 1)
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for r in range(ROUNDS):
        for depth in ((False, True) if r % 2 == 0 else (True, False)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(PER_ROUND):
                step(depth)
            b.record()
            b.synchronize()
            times[depth].append(a.elapsed_time(b) / PER_ROUND)
    colour, depth = float(np.median(times[False])), float(np.median(times[True]))
    print(json.dumps({"workload": "config3 render+render_backward", "n": wl.n, "width": wl.width, "height": wl.height,
                      "colour_ms": round(colour, 4), "depth_alpha_ms": round(depth, 4),
                      "ratio": round(depth / colour, 4),
                      "colour_ms_all": [round(x, 4) for x in times[False]],
                      "depth_alpha_ms_all": [round(x, 4) for x in times[True]]}))


if __name__ == "__main__":
    main()
