#!/usr/bin/env python3
"""Cost of the camera-pose gradient at BASELINE configs 3 and 4.

Two measurements per config, each alternating the variants in one process after a warm-up, timed with device events,
the model left in place (no optimizer step applied to it between rounds except on the fused route, which updates in
place either way):
  * stage: the projection backward alone on one fixed accumulator - plain route (cugs_project_backward vs _pose) and
    fused-Adam route (cugs_project_backward_adam vs _adam_pose), the POSE side including its two reduction launches;
  * step: render + render_backward vs render + render_backward(want_camera_grad=True) on the plain route.
Prints one JSON line per config: median ms of each and the ratios."""
import argparse, ctypes as C, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
from cugs_amd import _lib                      # noqa: E402  (registered by load_package)
lib = _lib.lib
dev = torch.device("cuda:0")


def timed(fns, rounds, per_round, warmup):
    for i in range(warmup):
        fns[i % len(fns)]()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for r in range(rounds):
        order = list(range(len(fns))) if r % 2 == 0 else list(reversed(range(len(fns))))
        for k in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_round):
                fns[k]()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / per_round)
    return [float(np.median(t)) for t in times]


def run(name, rounds, per_round, warmup):
    wl = pkg.scene.CONFIGS[name]
    model = pkg.scene.to_model(pkg.scene.make_gaussians(wl.n, wl.width, wl.height, 3), dev)
    cam = pkg.scene.make_camera(wl.width, wl.height)
    settings = pkg.RenderSettings(active_sh_degree=3)
    dC = torch.from_numpy(pkg.scene.make_dl_dcolor(wl.width, wl.height)).to(dev)
    n = wl.n
    out = pkg.render(model, cam, settings)
    rb = pkg.rasterize_backward(dC, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                out.gaussian_indices, out.final_T, out.n_contrib, wl.width, wl.height,
                                settings.background, n, packed=out.packed, unpack=False, tile_order=out.tile_order)
    accum = rb.grad_accum
    abi = cam.to_abi()
    P = lambda t: C.c_void_p(t.data_ptr())
    f = dict(dtype=torch.float32, device=dev)
    d = [torch.empty((n, 3), **f), torch.empty((n, 4), **f), torch.empty((n, 3), **f), torch.empty((n, 1), **f),
         torch.empty_like(model.sh_coeffs), torch.empty((n, 2), **f)]
    view = torch.empty((4, 4), **f)
    ws = torch.empty(lib.cugs_pose_grad_workspace_bytes(n), dtype=torch.uint8, device=dev)
    pg = _lib.PoseGrad(view.data_ptr(), None, ws.data_ptr(), ws.numel())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    plain_args = (n, 16, 3, P(model.positions), P(model.rotations), P(model.scales), P(model.opacities),
                  P(model.sh_coeffs), P(out.radii), P(out.colour_gate), C.byref(abi), 1.0, P(accum), None, None, None,
                  None, *[P(t) for t in d], None)
    opt = pkg.FusedAdam(model)
    adam = opt.begin_fused_step()
    adam_args = (n, 16, 3, P(model.positions), P(model.rotations), P(model.scales), P(model.opacities),
                 P(model.sh_coeffs), P(out.radii), P(out.colour_gate), C.byref(abi), 1.0, P(accum), C.byref(adam),
                 P(d[5]))
    opts = _lib.ProjectionOpts(pose=C.pointer(pg))
    stage = timed([lambda: lib.cugs_project_backward_opts(*plain_args, None, st),
                   lambda: lib.cugs_project_backward_opts(*plain_args, C.byref(opts), st),
                   lambda: lib.cugs_project_backward_adam_opts(*adam_args, None, st),
                   lambda: lib.cugs_project_backward_adam_opts(*adam_args, C.byref(opts), st)], rounds, per_round, warmup)

    def step(want):
        o = pkg.render(model, cam, settings)
        pkg.render_backward(dC, o, model, cam, settings, want_camera_grad=want)

    steps = timed([lambda: step(False), lambda: step(True)], rounds, max(1, per_round // 2), warmup)
    return {"workload": name, "n": n, "width": wl.width, "height": wl.height,
            "pb_plain_ms": round(stage[0], 4), "pb_plain_pose_ms": round(stage[1], 4),
            "pb_plain_ratio": round(stage[1] / stage[0], 4),
            "pb_adam_ms": round(stage[2], 4), "pb_adam_pose_ms": round(stage[3], 4),
            "pb_adam_ratio": round(stage[3] / stage[2], 4),
            "step_ms": round(steps[0], 4), "step_pose_ms": round(steps[1], 4),
            "step_ratio": round(steps[1] / steps[0], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="config3,config4")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--per-round", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    for name in a.configs.split(","):
        print(json.dumps(run(name, a.rounds, a.per_round, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
