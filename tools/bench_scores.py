#!/usr/bin/env python3
"""Cost of the contribution-score launch on the BASELINE config 3 view, next to the two blends it sits
between: the forward blend (rasterize_forward), the score launch (blend_scores into a zeroed table), and the only other
route to the weight sums, the backward blend with dL_dcolor = (1, 0, 0) (rasterize_backward, rows left packed; its
accumulator fill is part of the route).  All three run on the SAME projected and sorted inputs - packed records, tile
order - so only the three kernels differ.  The variants alternate in one process after a warm-up and are timed with
device events.  Prints one JSON line: median microseconds per launch of each, the ratios, and the totals of the two
checks it makes first (pixel counts against n_contrib, weights against 1 - final_T)."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda:0")
ROUNDS, PER_ROUND, WARMUP = 12, 100, 30


def main():
    wl = pkg.scene.CONFIGS["config3"]
    w, h, n = wl.width, wl.height, wl.n
    model = pkg.scene.to_model(pkg.scene.make_gaussians(n, w, h, 3), dev)
    cam = pkg.scene.make_camera(w, h)
    settings = pkg.RenderSettings(active_sh_degree=3)
    out = pkg.render(model, cam, settings)
    order = out.tile_order if out.tile_order is not None else pkg.rasterizer.tile_order_of(out.tile_ranges, w, h)
    red = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    red[..., 0] = 1.0
    bg = settings.background
    scores = pkg.ContributionScores(n, dev)

    def forward():
        return pkg.rasterize_forward(out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                     out.gaussian_indices, w, h, bg, packed=out.packed, tile_order=order)

    def score():
        return pkg.blend_scores(scores, None, None, None, out.tile_ranges, out.gaussian_indices, w, h, packed=out.packed,
                                tile_order=order)

    def backward():
        return pkg.rasterize_backward(red, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                      out.gaussian_indices, out.final_T, out.n_contrib, w, h, bg, n, packed=out.packed,
                                      unpack=False, tile_order=order)

    variants = {"forward_blend": forward, "score_launch": score, "backward_blend_sum_route": backward}
    # what is timed is right at this size: every pixel's contributors are counted once and the weights add up to what
    # the pixels lost
    score()
    torch.cuda.synchronize()
    a = scores.weight_sum.double()
    checks = {"count_total": int(scores.pixel_count.sum()), "n_contrib_total": int(out.n_contrib.sum()),
              "weight_total": float(a.sum()), "one_minus_T_total": float((1.0 - out.final_T.double()).sum()),
              "weight_sum_max": float(a.max())}
    assert checks["count_total"] == checks["n_contrib_total"], checks
    assert abs(checks["weight_total"] - checks["one_minus_T_total"]) <= 1e-5 * checks["one_minus_T_total"], checks
    scores.reset()

    names = list(variants)
    for i in range(WARMUP):
        variants[names[i % 3]]()
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for r in range(ROUNDS):
        for k in names[r % 3:] + names[:r % 3]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(PER_ROUND):
                variants[k]()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1000.0 / PER_ROUND)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"workload": "config3 view, one launch each on the same sorted inputs", "n": n, "width": w,
                      "height": h, "pairs": int(out.total_pairs),
                      **{k + "_us": round(v, 2) for k, v in med.items()},
                      "score_over_forward": round(med["score_launch"] / med["forward_blend"], 4),
                      "score_over_backward_route": round(med["score_launch"] / med["backward_blend_sum_route"], 4),
                      **checks,
                      **{k + "_us_all": [round(x, 2) for x in v] for k, v in times.items()}}))


if __name__ == "__main__":
    main()
