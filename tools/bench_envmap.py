#!/usr/bin/env python3
"""Cost of the environment-map background at 1920x1080 with R = 256 and R = 1024, the fused kernels and
the libtorch sequence they replace alternating in one process after a warm-up, timed with device events around PER_ROUND
back-to-back calls (no host sync inside a window):
  (a) image.clone()                                         the bytes yardstick: 12 B read + 12 B written per pixel
  (b) composite_environment                                 28 B per pixel + the map's taps
  (c) composite_environment_backward, g = noise             dL_dalpha and dL_denv (clear, accumulate, finish)
  (d) the same with a smooth g, (e) with a constant g       the values do not change the number of atomics; timed as asked
  (f) the same with final_T = 0 on the lower half           covered pixels send nothing: what a real view costs
  (g) composite_environment_backward(want_env_grad=False)   dL_dalpha alone: the pass without its atomics
  (h) libtorch forward: directions, normalisation, octahedral coordinates, grid_sample, multiply-add
  (i) libtorch forward + autograd backward to the map and to final_T
The view looks along the map's +z with the scene camera's field of view, where no sample crosses a fold line, so that
grid_sample (which cannot fold) computes the same function; the two routes are compared before anything is timed.
Prints one JSON line per R: median ms per call, min/max over the rounds, ratios, and bytes per second against the copy."""
import json, os, sys
import numpy as np, torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
W, H = 1920, 1080
ROUNDS, PER_ROUND, WARMUP = 6, 20, 3


def torch_sample(E, cam):
    """B [H,W,3] by libtorch on the device: the function of csrc/envmap.hip away from the fold lines."""
    dev = E.device
    K = cam.intrinsics
    u = (torch.arange(cam.width, device=dev, dtype=torch.float32) + 0.5 - K.cx) / K.fx
    v = (torch.arange(cam.height, device=dev, dtype=torch.float32) + 0.5 - K.cy) / K.fy
    d = torch.stack([u.expand(cam.height, -1), v.unsqueeze(1).expand(-1, cam.width), torch.ones((cam.height, cam.width), device=dev)], dim=-1)
    d = d @ torch.from_numpy(np.asarray(cam.rotation, np.float32)).to(dev)          # d_map = R^T d_c, row-vector form
    n = d / d.abs().sum(dim=-1, keepdim=True)
    sgn = lambda t: torch.where(t >= 0, 1.0, -1.0)
    low = n[..., 2] < 0
    x = torch.where(low, (1 - n[..., 1].abs()) * sgn(n[..., 0]), n[..., 0])
    y = torch.where(low, (1 - n[..., 0].abs()) * sgn(n[..., 1]), n[..., 1])
    grid = torch.stack([x, y], dim=-1).unsqueeze(0)
    return F.grid_sample(E.unsqueeze(0), grid, mode="bilinear", padding_mode="border", align_corners=False)[0].permute(1, 2, 0)


def bench(res, dev, gen):
    cam = pkg.scene.make_camera(W, H)
    env = pkg.EnvironmentMap(resolution=res, device=dev)
    env.texture.copy_(torch.rand((3, res, res), generator=gen).to(dev))
    color = torch.rand((H, W, 3), generator=gen).to(dev)
    T = torch.rand((H, W), generator=gen).to(dev)
    T_half = T.clone()
    T_half[H // 2:] = 0.0
    scale = 1.0 / (3 * H * W)
    bound = 4.0 * scale
    g_noise = (torch.randn((H, W, 3), generator=gen).clamp(-3.5, 3.5) * scale).to(dev)
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 5, W), indexing="ij")
    g_smooth = (torch.stack([torch.sin(xx + yy), torch.cos(xx - yy), torch.sin(2 * yy)], dim=-1) * scale).contiguous().to(dev)
    g_const = torch.full((H, W, 3), 0.7 * scale, device=dev)
    depths = torch.zeros(1, device=dev)
    make_out = lambda t: pkg.RenderOutput(color, t, None, None, depths, None, None, None, None, None, None)
    out, out_half = make_out(T), make_out(T_half)

    def lt_forward():
        with torch.no_grad():
            return torch.addcmul(color, T.unsqueeze(-1), torch_sample(env.texture, cam))

    def lt_backward():
        E, t = env.texture.detach().requires_grad_(True), T.detach().requires_grad_(True)
        image = torch.addcmul(color, t.unsqueeze(-1), torch_sample(E, cam))
        return torch.autograd.grad(image, (E, t), g_noise)

    back = lambda g, o=out, **kw: pkg.composite_environment_backward(g, o, cam, env, grad_bound=bound, **kw)
    variants = {"a_copy": lambda: color.clone(),
                "b_composite": lambda: pkg.composite_environment(out, cam, env),
                "c_backward_noise": lambda: back(g_noise),
                "d_backward_smooth": lambda: back(g_smooth),
                "e_backward_constant": lambda: back(g_const),
                "f_backward_half_covered": lambda: back(g_noise, out_half),
                "g_backward_alpha_only": lambda: back(g_noise, want_env_grad=False),
                "h_libtorch_forward": lt_forward,
                "i_libtorch_forward_backward": lt_backward}
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    mine, (lt_dE, lt_dT) = back(g_noise), lt_backward()
    check = {"image": rel(variants["b_composite"](), lt_forward()), "dL_denv": rel(mine.dL_denv, lt_dE),
             "dL_dalpha": rel(mine.dL_dalpha, -lt_dT), "clamped": int(mine.clamped)}
    # both routes round the texel coordinate x R / 2 + ... in fp32: a few ulp of x (the division, the rotation, the
    # normalisation: 4 * 2^-24) times R / 2 texels, per axis, on a map whose slope is at most 1 per texel - 2.4e-7 R
    # for one route, twice that between two
    bar = 5e-7 * res
    assert check["image"] <= bar and check["dL_denv"] <= 1e-3 and check["dL_dalpha"] <= bar and check["clamped"] == 0, check
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
    px, table = H * W, 8 * 3 * res * res
    # algorithmic bytes: copy 24 B / pixel; composite 12 + 4 read, 12 written; backward 12 + 4 read, 4 written, the int64
    # table written (clear), read (finish) and the map written - the atomics' own traffic stays in the L2 and is not counted
    nbytes = {"a_copy": 24 * px, "b_composite": 28 * px, "c_backward_noise": 20 * px + 2 * table + 12 * res * res,
              "g_backward_alpha_only": 16 * px}
    gbps = {k: v / (med[k] * 1e-3) / 1e9 for k, v in nbytes.items()}
    print(json.dumps({"workload": "environment map composite / backward", "width": W, "height": H, "resolution": res,
                      "per_call_ms": {k: round(v, 5) for k, v in med.items()},
                      "ratio_fused_to_libtorch": {"forward": round(med["b_composite"] / med["h_libtorch_forward"], 4),
                                                  "forward_backward": round((med["b_composite"] + med["c_backward_noise"]) /
                                                                            med["i_libtorch_forward_backward"], 4)},
                      "algorithmic_GBps": {k: round(v, 1) for k, v in gbps.items()},
                      "byte_rate_against_copy": {k: round(v / gbps["a_copy"], 3) for k, v in gbps.items() if k != "a_copy"},
                      "atomics_ms": round(med["c_backward_noise"] - med["g_backward_alpha_only"], 5),
                      "agreement_with_libtorch_fp32": {k: float(f"{v:.2e}") for k, v in check.items()},
                      "min_max_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
                      "rounds": ROUNDS, "calls_per_round": PER_ROUND}), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_envmap needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(7)
    for res in (256, 1024):
        bench(res, dev, gen)


if __name__ == "__main__":
    main()
