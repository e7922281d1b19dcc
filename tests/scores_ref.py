"""The contribution-score reference, from the UNCHANGED oracle.

The forward blend is linear in rgb.  With background 0 and rgb one-hot on Gaussians g, g+1, g+2 (one per channel),
orc.rasterize_forward returns the blend weight w[p, g] = alpha T of Gaussian g at pixel p EXACTLY in the image: each
channel's accumulator takes fmaf(w, 1, 0) = w once and fmaf(w', 0, C) = C otherwise, and the background adds T * 0.
ceil(n/3) calls give the whole [H*W, n] table with the oracle's own decisions.  From it: the sum in fp64, the maximum
exactly, the count as #(w > 0) - a passing weight is at least 1/255 * 1/255 ~ 1.5e-5 and never underflows."""
from __future__ import annotations

import functools

import numpy as np

from util import oracle_forward

# the scenes of tests/test_gpu_absgrad.py: (n, w, h, mu_s, seed) - frames that are no multiple of 16
SCENES = {
    "40x24": (400, 40, 24, -1.0, 2),
    "33x17": (500, 33, 17, -1.0, 3),
}
_OPAQUE = 3         # splats made opaque, far and centred on a pixel
_BEHIND = 5         # rows behind the camera: in no list


def make_arrays(pkg, key):
    n, w, h, mu_s, seed = SCENES[key]
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=0, seed=seed, mu_s=mu_s)
    K = pkg.scene.make_camera(w, h).intrinsics
    for j in range(_OPAQUE):
        z = 9.9 + 0.01 * j
        px, py = 5 + 11 * j, 3 + 5 * j
        arrays["positions"][j] = ((px + 0.5 - K.cx) * z / K.fx, (py + 0.5 - K.cy) * z / K.fy, z)
        arrays["opacities"][j] = 9.0          # sigmoid = 0.99988
    arrays["positions"][_OPAQUE:_OPAQUE + _BEHIND, 2] = -5.0
    return arrays


def weight_table(orc, ref, n, w, h):
    """[H*W, n] float32: w[p, g] of the oracle's forward blend `ref`, three Gaussians per call."""
    table = np.zeros((h * w, n), np.float32)
    for g0 in range(0, n, 3):
        k = min(3, n - g0)
        rgb = np.zeros((n, 3), np.float32)
        rgb[np.arange(g0, g0 + k), np.arange(k)] = 1.0
        img = orc.rasterize_forward(w, h, (0.0, 0.0, 0.0), ref["tile_ranges"], ref["values"], ref["means_2d"],
                                    ref["cov_2d_inv"], rgb, ref["opacities_act"])["color"]
        table[:, g0:g0 + k] = img.reshape(h * w, 3)[:, :k]
    return table


def scores_of(table):
    """{"sum": fp64 [n], "max": float32 [n], "count": int64 [n]} of a weight table."""
    return dict(sum=table.astype(np.float64).sum(axis=0), max=table.max(axis=0).astype(np.float32),
                count=(table > 0.0).sum(axis=0).astype(np.int64))


@functools.lru_cache(maxsize=None)
def scene(key, view=0):
    """The scene, the oracle's forward of `view` and its reference scores - computed once, shared, never modified."""
    import __graft_entry__ as ge
    pkg, orc = ge.load_package(), ge.load_oracle()
    n, w, h, _, _ = SCENES[key]
    arrays = make_arrays(pkg, key)
    cam = pkg.scene.make_camera(w, h, view=view)
    ref = oracle_forward(orc, arrays, cam, degree=0)
    table = weight_table(orc, ref, n, w, h)
    want = scores_of(table)
    for v in (table, *want.values(), *arrays.values(), *(a for a in ref.values() if isinstance(a, np.ndarray))):
        v.setflags(write=False)
    return dict(arrays=arrays, cam=cam, ref=ref, table=table, want=want, n=n, w=w, h=h)


def combine(*wants):
    """Scores of several views in one table: sums and counts add, the maximum is the maximum."""
    return dict(sum=sum(x["sum"] for x in wants), max=np.maximum.reduce([x["max"] for x in wants]),
                count=sum(x["count"] for x in wants))
