#!/usr/bin/env python3
"""Cost of the pixel-map lift on the BASELINE config 3 view: the lift launch with C = 1, 3 and 4 float
channels and in labels mode (blend_lift into its table), the score launch it is derived from (blend_scores), and the
only route to sum_p w M the project had before - the backward blend with dL_dcolor := M (rasterize_backward, rows left
packed; its accumulator fill is part of the route; three channels at most).  All run on the SAME projected and sorted
inputs - packed records, tile order - so only the kernels differ.  The variants alternate in one process after a warm-up
and are timed with device events.  Before timing, a map of ones is lifted at this size and compared with
sum_p (1 - final_T), the weights every pixel lost.  Prints one JSON line: median microseconds per launch of each, the
ratios, and that check's relative error."""
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
    gen = torch.Generator(device=dev).manual_seed(5)
    maps = {c: torch.randn((h, w, c), dtype=torch.float32, device=dev, generator=gen) for c in (1, 3, 4)}
    labels = torch.randint(0, 4, (h, w), dtype=torch.int32, device=dev, generator=gen)
    bg = settings.background
    tables = {c: pkg.LiftedMaps(n, dev, c) for c in (1, 3, 4)}
    votes = pkg.LiftedMaps(n, dev, 4)
    scores = pkg.ContributionScores(n, dev)

    def lift(table, **m):
        return pkg.blend_lift(table, None, None, None, out.tile_ranges, out.gaussian_indices, w, h, packed=out.packed,
                              tile_order=order, **m)

    def score():
        return pkg.blend_scores(scores, None, None, None, out.tile_ranges, out.gaussian_indices, w, h, packed=out.packed,
                                tile_order=order)

    def backward():
        return pkg.rasterize_backward(maps[3], out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                      out.gaussian_indices, out.final_T, out.n_contrib, w, h, bg, n, packed=out.packed,
                                      unpack=False, tile_order=order)

    variants = {"lift_c1": lambda: lift(tables[1], maps=maps[1]), "lift_c3": lambda: lift(tables[3], maps=maps[3]),
                "lift_c4": lambda: lift(tables[4], maps=maps[4]), "lift_labels4": lambda: lift(votes, labels=labels),
                "score_launch": score, "backward_blend_route_c3": backward}
    # what is timed is right at this size: a map of ones gives every pixel's lost weight, sum_g w = 1 - final_T
    ones = pkg.LiftedMaps(n, dev, 1)
    lift(ones, maps=torch.ones((h, w), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    total, lost = float(ones.sums.double().sum()), float((1.0 - out.final_T.double()).sum())
    checks = {"ones_total": total, "one_minus_T_total": lost, "ones_rel_err": abs(total - lost) / lost}
    print(f"map of ones: sum S = {total:.6f}, sum (1 - final_T) = {lost:.6f}, relative error {checks['ones_rel_err']:.3e}",
          file=sys.stderr)
    assert checks["ones_rel_err"] <= 1e-5, checks

    names = list(variants)
    k_n = len(names)
    for i in range(WARMUP):
        variants[names[i % k_n]]()
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for r in range(ROUNDS):
        for k in names[r % k_n:] + names[:r % k_n]:
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
                      "lift_c3_over_backward_route": round(med["lift_c3"] / med["backward_blend_route_c3"], 4),
                      "lift_c1_over_score": round(med["lift_c1"] / med["score_launch"], 4),
                      "lift_c4_over_lift_c1": round(med["lift_c4"] / med["lift_c1"], 4),
                      **checks,
                      **{k + "_us_all": [round(x, 2) for x in v] for k, v in times.items()}}))


if __name__ == "__main__":
    main()
