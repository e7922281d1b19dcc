"""The reference of the pixel-map lift, from the weight tables of tests/scores_ref.py.

scores_ref.scene(key, view)["table"] is the unchanged oracle's w[p, g].  The sums the lift kernel must deliver are
S[g, c] = sum_p w[p, g] M[p, c], here table.astype(f64).T @ M, and the tolerance is derived, not measured: for
Gaussian g, channel c and k = its number of pixels with w > 0,

    |got - want| <= k * 2^-23 * sum_p w |m_c|

- twice the first-order bound for k fp32 products summed in any order.  Where that bound is 0 the result must be
exactly 0.  Everything here is computed once per argument set, shared and never modified."""
from __future__ import annotations

import functools

import numpy as np

from scores_ref import SCENES, scene

LABEL_IMAGES = {"stripes": 4, "grid": 6, "checker": 7}          # name -> number of labels


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def wanted(table, maps):
    """{"sum": f64 [n,C], "bound": f64 [n,C], "count": int64 [n]} of a weight table [H*W,n] and a map [H,W,C] or [H,W]
    (non-finite entries of the map count as 0: the NaN test places them itself)."""
    m = np.asarray(maps, np.float64).reshape(table.shape[0], -1)
    m = np.where(np.isfinite(m), m, 0.0)
    t = table.astype(np.float64).T
    count = (table > 0.0).sum(axis=0).astype(np.int64)
    return dict(sum=t @ m, bound=count[:, None] * 2.0 ** -23 * (t @ np.abs(m)), count=count)


def combine(*wants):
    """Several launches into one table: the sums add, and so do the k and the sum of |terms| of the bound."""
    count = sum(x["count"] for x in wants)
    mag = sum(x["bound"] / np.maximum(x["count"], 1)[:, None] for x in wants)      # 2^-23 * sum w|m| of each
    return dict(sum=sum(x["sum"] for x in wants), bound=count[:, None] * mag, count=count)


def check(got, want, label, channels=None):
    """`got` [n,C] float32 against wanted(); prints the worst error / bound ratio; exactly 0 where the bound is 0."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want["sum"].shape, (label, got.dtype, got.shape)
    err = np.abs(got.astype(np.float64) - want["sum"])
    bound = want["bound"]
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"lift {label}: {int((want['count'] > 0).sum())} of {got.shape[0]} contribute, max count "
          f"{int(want['count'].max()) if got.shape[0] else 0}, worst error / bound = {worst:.3f}")
    assert np.all(got[bound == 0.0] == 0.0), label
    assert np.all(err <= bound), (label, worst)
    return worst


@functools.lru_cache(maxsize=None)
def float_map(key, view, channels):
    """[H,W,C] float32, standard normal (signed)."""
    n, w, h, _, seed = SCENES[key]
    m = np.random.default_rng(1000 * seed + 10 * view + channels).standard_normal((h, w, channels)).astype(np.float32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def error_map(key, view):
    """[H,W] float32 in [0,1): a stand-in for a per-pixel error."""
    n, w, h, _, seed = SCENES[key]
    m = np.random.default_rng(7000 * seed + view).random((h, w), dtype=np.float32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def label_image(key, name):
    """[H,W] int32."""
    n, w, h, _, _ = SCENES[key]
    y, x = np.mgrid[0:h, 0:w]
    if name == "stripes":
        lab = (x * 4) // w
    elif name == "grid":
        lab = (x * 3) // w + 3 * ((y * 2) // h)
    else:
        lab = (x // 3 + 2 * (y // 2)) % 7
        lab[(x + 3 * y) % 11 == 0] = -1                         # unlabelled pixels: they vote for nothing
    lab = lab.astype(np.int32)
    assert lab.max() == LABEL_IMAGES[name] - 1
    lab.setflags(write=False)
    return lab


def one_hot(lab, num_labels):
    """[H,W,L] float64 indicators; a label outside 0..L-1 gives a zero row."""
    return (lab[..., None] == np.arange(num_labels)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def lifted(key, view, channels):
    s = scene(key, view)
    return _frozen(wanted(s["table"], float_map(key, view, channels)))


@functools.lru_cache(maxsize=None)
def votes(key, name, views):
    """The wanted votes of label image `name` over the tuple `views`, with "label": the reference argmax (first maximum)
    of every Gaussian that collected a vote and -1 elsewhere, "margin": (top vote - second vote) / (the two bounds'
    sum) of each such Gaussian, and "voters": per Gaussian the number of its pixels that carry a label."""
    num = LABEL_IMAGES[name]
    hot = one_hot(label_image(key, name), num)
    want = combine(*(wanted(scene(key, v)["table"], hot) for v in views))
    labelled = (label_image(key, name) >= 0).reshape(-1)
    want["voters"] = sum((scene(key, v)["table"][labelled] > 0.0).sum(axis=0) for v in views).astype(np.int64)
    top = want["sum"].argmax(axis=1)
    has = want["sum"].max(axis=1) > 0.0
    want["label"] = np.where(has, top, -1).astype(np.int64)
    order = np.argsort(-want["sum"], axis=1, kind="stable")
    rows = np.arange(len(top))
    gap = want["sum"][rows, order[:, 0]] - want["sum"][rows, order[:, 1]]
    slack = want["bound"][rows, order[:, 0]] + want["bound"][rows, order[:, 1]]
    want["margin"] = np.where(has, gap / np.maximum(slack, 1e-300), np.inf)
    return _frozen(want)


@functools.lru_cache(maxsize=None)
def errors(key, views=(0, 1)):
    """Error scores over `views`: "per_view" the wanted() of each, "max" / "max_bound" the maximum over the views of the
    sums and - an upper bound of the maximum's error - of the bounds, and "threshold": the middle of the widest gap
    between neighbouring reference scores in the middle half of their sorted order."""
    per = [wanted(scene(key, v)["table"], error_map(key, v)) for v in views]
    mx = np.maximum.reduce([p["sum"][:, 0] for p in per])
    mb = np.maximum.reduce([p["bound"][:, 0] for p in per])
    srt = np.sort(mx[mx > 0.0])
    lo, hi = len(srt) // 4, 3 * len(srt) // 4
    i = lo + int(np.argmax(np.diff(srt[lo:hi])))
    return _frozen(dict(per_view=per, max=mx, max_bound=mb, threshold=float(np.float32(0.5 * (srt[i] + srt[i + 1])))))
