#!/usr/bin/env python3
"""Do two builds of the library compute the same per-pixel values in the blend kernels?  Compared bit for bit.

A 7x6 image is one tile whose quads 1-3 lie outside the image, so every atomic add of the backward comes from wave 0 in
program order: the sums do not depend on timing (on a full frame two runs of ONE library already differ by the order of
their atomic adds).  900 splats, 15 % opaque: a 900-entry list (four record batches), n_contrib 12 .. 46, outside-image
lanes in both axes; forward outputs and the accumulator rows of {packed, unpacked} x {colour, depth, abs, depth + abs}.

    CUGS_HIP_LIBRARY=<build A> python3 tools/single_wave_bits.py dump a.npz
    CUGS_HIP_LIBRARY=<build B> python3 tools/single_wave_bits.py dump b.npz      (a fresh process per library)
    python3 tools/single_wave_bits.py compare a.npz b.npz
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def dump(out_path):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    w, h, n = 7, 6, 900
    cam = pkg.scene.make_camera(w, h)
    K = cam.intrinsics
    rng = np.random.default_rng(5)
    u, v = rng.uniform(-2.0, w + 2.0, n), rng.uniform(-2.0, h + 2.0, n)
    z = rng.permutation(n) * 0.01 + 2.0
    sig = rng.uniform(0.5, 3.0, n)
    logit = np.where(rng.uniform(size=n) < 0.15, 9.0, rng.uniform(-5.0, 1.0, n))     # some opaque, most faint
    arrays = dict(positions=np.stack([(u - K.cx) * z / K.fx, (v - K.cy) * z / K.fy, z], 1).astype(np.float32),
                  sh_coeffs=rng.uniform(-1, 1, (n, 3, 1)).astype(np.float32), opacities=logit.reshape(n, 1).astype(np.float32),
                  rotations=np.tile([1.0, 0, 0, 0], (n, 1)).astype(np.float32),
                  scales=np.repeat(np.log(sig * z / K.fx)[:, None], 3, 1).astype(np.float32))
    BG = (0.3, 0.1, 0.6)
    model = pkg.scene.to_model(arrays, dev)
    out = pkg.render(model, cam, pkg.RenderSettings(background=list(BG), active_sh_degree=0), want_depth_map=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dC = t((rng.standard_normal((h, w, 3)) / (w * h)).astype(np.float32))
    dD = t((rng.standard_normal((h, w)) * 0.05).astype(np.float32)); dA = t((rng.standard_normal((h, w)) * 0.3).astype(np.float32))
    res = dict(color=out.color, final_T=out.final_T, n_contrib=out.n_contrib, depth_map=out.depth_map)
    for packed in (True, False):
        for route in ("colour", "depth", "abs", "depth_abs"):
            extra = {}
            if "depth" in route: extra.update(depths=out.depths, dL_ddepth_map=dD, dL_dalpha=dA)
            if "abs" in route: extra["want_abs_grad"] = True
            rb = pkg.rasterize_backward(dC, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                        out.gaussian_indices, out.final_T, out.n_contrib, w, h, BG, n,
                                        packed=out.packed if packed else None, **extra)
            res[f"acc_{'packed' if packed else 'unpacked'}_{route}"] = rb.grad_accum
    torch.cuda.synchronize()
    nc = res["n_contrib"].cpu().numpy()
    tr = out.tile_ranges.cpu().numpy().reshape(-1, 2)
    print("lib", pkg.LIB_PATH, "list length", int(tr[0, 1] - tr[0, 0]), "n_contrib min/max", nc.min(), nc.max(),
          "final_T max", float(res["final_T"].max()))
    np.savez(out_path, **{k: v.cpu().numpy() for k, v in res.items()})



def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    ok = True
    for k in a.files:
        eq = a[k].tobytes() == b[k].tobytes()
        ok &= eq
        print(f"{k:28s} shape {a[k].shape} nonzero {int(np.count_nonzero(a[k]))} A == B bit for bit: {eq}")
    print("single wave: ALL BIT-EQUAL" if ok else "single wave: DIFFERENT")

    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
