#!/usr/bin/env python3
"""Cost of the mesh export on the config-3 scene (1M Gaussians, SH 3) rendered at 1920x1080 from 16
orbiting cameras, into colour volumes of 256^3 and 512^3 voxels.  The variants alternate in one process after a warm-up
and are timed with device events around PER_ROUND back-to-back calls (no host sync inside a window):
  integrate_1 / _8 / _16   cugs_tsdf_integrate with 1, 8 and 16 views in one pass over the volume
  libtorch_1               the libtorch sequence one view of it replaces: the (cached) voxel grid, matmul, divide,
                           floor, index gather, where, weighted update of the five planes
  extract                  cugs_mesh_plan + cugs_mesh_emit on the fused volume (includes the plan's host sync)
Per volume it also counts, on a fresh volume, the voxels and the 16-byte groups of four that each batch touches: the
byte model of DESIGN.md 4.24 is touched x 8 P bytes (P = 5 planes, read and written once).
Prints one JSON line per volume size.  The fused and the libtorch result of one view are compared before timing."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda:0")
ROUNDS, WARMUP = 5, 2
VIEWS = 16
MIN_ALPHA, MIN_DEPTH, MAX_WEIGHT = 0.5, 0.05, 64.0
LO, EXTENT = (-3.0, -3.0, 1.5), 6.0          # the box: the front of the scene, where the expected depth lies


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf needs a GPU: nothing is measured without one")
    wl = pkg.scene.CONFIGS["config3"]
    model = pkg.scene.to_model(pkg.scene.make_gaussians(wl.n, wl.width, wl.height, sh_degree=wl.sh_degree, mu_s=wl.mu_s), dev)
    settings = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=wl.sh_degree)
    cams = [pkg.scene.make_camera(wl.width, wl.height, view=k) for k in range(VIEWS)]
    views = []
    for cam in cams:
        out = pkg.render(model, cam, settings, for_backward=False, want_depth_map=True)
        views.append(pkg.TSDFView((out.depth_map.clone(), out.alpha.clone()), cam, out.color.clone()))
    del model
    torch.cuda.synchronize()
    alpha_cover = float(np.mean([float((v.maps[1] > MIN_ALPHA).float().mean()) for v in views]))
    print(f"rendered {VIEWS} views at {wl.width}x{wl.height}; alpha > {MIN_ALPHA} on {100 * alpha_cover:.1f} % of the pixels",
          file=sys.stderr)

    for n in (256, 512):
        vs = EXTENT / (n - 1)
        trunc = 4.0 * vs
        hi = tuple(l + EXTENT for l in LO)
        new = lambda: pkg.TSDFVolume((LO, hi), vs, dev, color=True, max_weight=MAX_WEIGHT, min_depth=MIN_DEPTH, dims=(n, n, n))
        touched = {}
        for k in (1, 8, 16):                                  # what each batch touches, on a fresh volume
            vol = new()
            vol.integrate_views(views[:k], min_alpha=MIN_ALPHA)
            t = vol.weight > 0
            touched[k] = (int(t.sum()), int(t.view(-1, 4).any(-1).sum()))
            del t
        # vol now holds all 16 views: the volume the timed calls work on and extract reads

        # the libtorch sequence for one view, the voxel grid cached
        ax = [LO[k] + torch.arange(n, device=dev, dtype=torch.float32) * vs for k in range(3)]
        gz, gy, gx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        grid = torch.stack([gx, gy, gz], -1).reshape(-1, 3)
        del gx, gy, gz
        cam = cams[1]
        Rm = torch.from_numpy(np.asarray(cam.rotation, np.float32)).to(dev)
        tv = torch.from_numpy(np.asarray(cam.translation, np.float32)).to(dev)
        K = cam.intrinsics
        D1, A1, C1 = views[1].maps[0].reshape(-1), views[1].maps[1].reshape(-1), views[1].color.reshape(-1, 3)
        Wd, Hd = cam.width, cam.height

        def libtorch(planes):
            pc = grid @ Rm.T + tv
            z = pc[:, 2]
            zs = torch.where(z > MIN_DEPTH, z, torch.ones_like(z))
            u = torch.floor(K.fx * pc[:, 0] / zs + K.cx)
            v = torch.floor(K.fy * pc[:, 1] / zs + K.cy)
            ok = (z > MIN_DEPTH) & (u >= 0) & (u < Wd) & (v >= 0) & (v < Hd)
            pix = torch.where(ok, v * Wd + u, torch.zeros_like(u)).long()
            a = A1[pix]
            ok &= a > MIN_ALPHA
            sdf = D1[pix] / torch.where(ok, a, torch.ones_like(a)) - z
            ok &= sdf >= -trunc
            tn = torch.clamp_max(sdf / trunc, 1.0)
            flat = planes.view(5, -1)
            wo = flat[1]
            wn = wo + 1.0
            flat[0] = torch.where(ok, (wo * flat[0] + tn) / wn, flat[0])
            c = C1[pix]
            for ch in range(3):
                flat[2 + ch] = torch.where(ok, (wo * flat[2 + ch] + c[:, ch]) / wn, flat[2 + ch])
            flat[1] = torch.where(ok, torch.clamp_max(wn, MAX_WEIGHT), wo)

        a_, b_ = new(), new()
        a_.integrate_views(views[1:2], min_alpha=MIN_ALPHA)
        libtorch(b_.planes)
        same = float(((a_.weight > 0) == (b_.weight > 0)).float().mean())
        dev_t = float((a_.tsdf - b_.tsdf).abs().mean())
        print(f"{n}^3: fused vs libtorch, one view: the same touched set on {100 * same:.4f} % of the voxels, mean |tsdf "
              f"difference| {dev_t:.2e}", file=sys.stderr)
        assert same > 0.999 and dev_t < 1e-3
        del a_, b_

        scratch = new()
        variants = {"integrate_1": (lambda: vol.integrate_views(views[:1], min_alpha=MIN_ALPHA), 4),
                    "integrate_8": (lambda: vol.integrate_views(views[:8], min_alpha=MIN_ALPHA), 4),
                    "integrate_16": (lambda: vol.integrate_views(views, min_alpha=MIN_ALPHA), 4),
                    "libtorch_1": (lambda: libtorch(scratch.planes), 2),
                    "extract": (lambda: vol.extract(), 2)}
        order = list(variants)
        for _ in range(WARMUP):
            for name in order:
                variants[name][0]()
        torch.cuda.synchronize()
        times = {name: [] for name in order}
        for rnd in range(ROUNDS):
            k = rnd % len(order)
            for name in (order[k:] + order[:k]):
                fn, per_round = variants[name]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per_round):
                    fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b) / per_round)
        med = {name: float(np.median(v)) for name, v in times.items()}
        mesh = vol.extract()
        model_bytes = {k: 8 * 5 * touched[k][0] for k in touched}
        group_bytes = {k: 8 * 5 * 4 * touched[k][1] for k in touched}
        print(json.dumps({
            "workload": "TSDF fusion and surface nets, config-3 scene", "volume": [n, n, n], "voxel_size": round(vs, 6),
            "width": wl.width, "height": wl.height, "planes": 5,
            "touched_voxels": {str(k): touched[k][0] for k in touched},
            "touched_groups_of_4": {str(k): touched[k][1] for k in touched},
            "per_call_ms": {k: round(v, 4) for k, v in med.items()},
            "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
            "integrate_model_TBps": {str(k): round(model_bytes[k] / (med[f"integrate_{k}"] * 1e-3) / 1e12, 3) for k in touched},
            "integrate_16B_groups_TBps": {str(k): round(group_bytes[k] / (med[f"integrate_{k}"] * 1e-3) / 1e12, 3) for k in touched},
            "ms_per_view": {str(k): round(med[f"integrate_{k}"] / k, 4) for k in touched},
            "libtorch_over_fused_per_view": round(med["libtorch_1"] / med["integrate_1"], 2),
            "mesh": {"vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0])},
            "rounds": ROUNDS}), flush=True)
        del vol, scratch, grid, mesh


if __name__ == "__main__":
    main()
