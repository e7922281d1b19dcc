"""The AbsGrad reference, from the UNCHANGED oracle.

The blend backward is linear in dL_dcolor and a pixel's contributions depend on that pixel's dL_dcolor alone, so the
oracle's backward with dL_dcolor zeroed everywhere but at pixel p (and restricted to p's row) returns exactly p's
summand of dL_dmeans_2d for every Gaussian - with the oracle's own decisions (Q1-Q3, the clamp gate) and exponent.  The
depth and alpha map terms enter as two more channels of the same blend (util.oracle_blend_terms: z with background 0,
and colour 0 with background -1); the channels of a pixel are added BEFORE the absolute value, as the kernel's
dL/dpower holds all of them."""
from __future__ import annotations

import numpy as np


def per_pixel_channels(orc, ref, n, w, h, g=None, bg=(0.0, 0.0, 0.0), dD=None, dA=None, depths=None):
    """{"colour" | "depth" | "alpha": [H*W, n, 2] float64}: every pixel's summand of dL_dmeans_2d, per channel, for the
    channels whose gradient is given (`g` [H,W,3]; `dD`, `dA` [H,W]; `depths` [n] goes with dD)."""
    geo = (ref["tile_ranges"], ref["values"], ref["means_2d"], ref["cov_2d_inv"])
    tail = (ref["final_T"], ref["n_contrib"], n)
    todo = {}
    if g is not None:
        todo["colour"] = (np.ascontiguousarray(ref["rgb"], np.float32), tuple(bg), np.ascontiguousarray(g, np.float32))
    if dD is not None:
        zr = np.zeros((n, 3), np.float32)
        zr[:, 0] = depths
        todo["depth"] = (zr, (0.0, 0.0, 0.0), np.stack([dD, 0 * dD, 0 * dD], axis=2).astype(np.float32))
    if dA is not None:
        todo["alpha"] = (np.zeros((n, 3), np.float32), (-1.0, 0.0, 0.0),
                         np.stack([dA, 0 * dA, 0 * dA], axis=2).astype(np.float32))
    out = {}
    one = np.zeros((h, w, 3), np.float32)                 # dL_dcolor with a single live pixel
    for name, (rgb, bg_, grad) in todo.items():
        res = np.zeros((h * w, n, 2), np.float64)
        for y in range(h):
            for x in range(w):
                if not grad[y, x].any():
                    continue
                one[y, x] = grad[y, x]
                r = orc.rasterize_backward(w, h, bg_, *geo, rgb, ref["opacities_act"], one, *tail, rows=(y, y + 1))
                res[y * w + x] = r["dL_dmeans_2d"]
                one[y, x] = 0.0
        out[name] = res
    return out


def abs_and_signed(*channels):
    """(sum_p |sum_c t|, sum_p sum_c t), [n,2] float64 each, of per-pixel channel tables."""
    pix = channels[0]
    for c in channels[1:]:
        pix = pix + c
    return np.abs(pix).sum(axis=0), pix.sum(axis=0)
