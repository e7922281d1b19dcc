"""CPU reference for the normal-supervision loss (csrc/normal_loss.hip, cugs_amd.normal_loss): a numpy
float32 mirror of the definition in include/cugs_hip.h, op for op - every float step one correctly rounded numpy
operation, the sums in float64 - and a torch float64 autograd version of the same definition.

  make_case(h, w)      D, A (float32 [h,w]), t (float32 [3,h,w]), w (float32 [h,w]), fx, fy, cx, cy
  reference(...)       dL/dD, dL/dA, normals (float32, the bytes the kernel must give), the masks and the fp64 sums
  autograd64(...)      the same loss in float64 with torch autograd through D and A, masks computed in float64

The kernel's fp64 sums take another order than numpy's; both are within ~2^-53 n relative of the exact sum, far below
half a float32 ulp, so after the final rounding to float32 the loss and the weight sum differ by at most one ulp.

Shared by tests/test_normal_loss_ref.py (CPU) and the GPU tests; callers must not modify a case's arrays."""
import numpy as np

F = np.float32
MIN_ALPHA = 1e-3
TILE_W, TILE_H = 64, 16              # the kernel's tile (normal_loss.hip: TW, TH)

# (h, w): no interior | no interior | one interior pixel, everything valid | a 3x4 alpha hole: nothing valid |
# one tile, ragged | one tile, ragged | 4 x 1 full tiles | one pixel more than a tile each way |
# 2 x 2 tiles, ragged
SHAPES = [(1, 1), (2, 5), (3, 3), (5, 7), (9, 11), (37, 53), (64, 64), (TILE_H + 1, TILE_W + 1), (19, 70)]
# 9 x 33 = 297 tiles: more rows of partials than the finalize kernel has threads (256), so its strided sum and its tree
# both run.  For the GPU tests against the mirror only: the error against float64 grows with fx = W (differences of
# neighbouring depths cancel), here past what that comparison allows, where the shapes above stay below 5e-6.
MANY_TILES = (130, 2070)
EMPTY = [(1, 1), (2, 5), (5, 7)]     # the shapes that must produce exactly nothing
HOLES = {(5, 7): (1, 1, 3, 4)}       # (row, column, rows, columns) of the alpha hole where the rule below is not used


def make_case(h, w):
    """dict(D, A, t, w, fx, fy, cx, cy, h, width).  The surface is a tilted plane plus ripples at depth ~3 seen through
    fx = fy = W with an off-centre principal point; alpha uniform in [0.5, 1]; the prior is random vectors biased to -z
    (of length 0.5 to 2: the kernel normalises); the weight uniform in [0.1, 1].  From 5 x 5 up: an alpha hole (its
    first pixel EQUAL to min_alpha - not valid - the others 0), a block of zero prior vectors, one NaN prior vector,
    and ~15 % zero weights."""
    rng = np.random.default_rng(h * 100003 + w * 17)
    fx = fy = float(w)
    cx, cy = 0.5 * w + 0.7, 0.5 * h - 0.4
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y = (u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy
    z = 3.0 + 0.8 * x - 0.5 * y + 0.05 * np.sin(9.0 * x + 1.0) * np.cos(7.0 * y)
    A = rng.uniform(0.5, 1.0, (h, w)).astype(F)
    t = rng.normal(0.0, 0.4, (3, h, w))
    t[2] -= 1.0
    t = (t * rng.uniform(0.5, 2.0, (1, h, w))).astype(F)
    wt = rng.uniform(0.1, 1.0, (h, w)).astype(F)
    if min(h, w) >= 5:
        r0, c0, nr, nc = HOLES.get((h, w), (h // 4, w // 2, max(1, h // 8), max(1, w // 8)))
        A[r0:r0 + nr, c0:c0 + nc] = 0.0
        A[r0, c0] = F(MIN_ALPHA)
        r0, c0 = h // 2, w // 4
        t[:, r0:r0 + max(1, h // 6), c0:c0 + max(1, w // 6)] = 0.0
        t[:, h - 2, w - 2] = np.nan
        wt[rng.random((h, w)) < 0.15] = 0.0
    D = (A * z.astype(F)).astype(F)
    return dict(D=D, A=A, t=t, w=wt, fx=fx, fy=fy, cx=cx, cy=cy, h=h, width=w)


_cases = {}


def case(h, w):
    """make_case, built once per shape and shared."""
    if (h, w) not in _cases:
        _cases[(h, w)] = make_case(h, w)
    return _cases[(h, w)]


def _pad(a):
    """One ring of +0 (False) around the last two axes: what the kernel reads outside the image."""
    return np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)])


def _cross(a, b):
    return [(a[1] * b[2] - a[2] * b[1]).astype(F), (a[2] * b[0] - a[0] * b[2]).astype(F), (a[0] * b[1] - a[1] * b[0]).astype(F)]


def _dot(a, b):
    return ((a[0] * b[0] + a[1] * b[1]).astype(F) + a[2] * b[2]).astype(F)


def reference(case, weighted=True, prior=True, cos_weight=1.0, l1_weight=0.0, min_alpha=MIN_ALPHA, D=None):
    """dict(gD, gA: float32 [h,w] (None without a prior); normals: float32 [3,h,w]; depth_valid, normal_valid, valid
    (loss-valid): bool [h,w]; n_valid; loss64 and sw64 the unrounded float64 results, loss and sw their float32
    roundings).  D: another depth map than the case's (the descent check)."""
    D = case["D"] if D is None else D
    A = case["A"]
    h, w = D.shape
    cw, lw = F(cos_weight), F(l1_weight)
    with np.errstate(all="ignore"):
        ok = A > F(min_alpha)
        d = np.where(ok, (D / np.where(ok, A, F(1.0))).astype(F), F(0.0)).astype(F)
        ax = (((np.arange(w, dtype=F) + F(0.5)) - F(case["cx"])) / F(case["fx"])).astype(F)[None, :]
        ay = (((np.arange(h, dtype=F) + F(0.5)) - F(case["cy"])) / F(case["fy"])).astype(F)[:, None]
        P = _pad(np.stack([(ax * d).astype(F), (ay * d).astype(F), d]))       # [3, h+2, w+2]
        Px = (P[:, 1:-1, 2:] - P[:, 1:-1, :-2]).astype(F)                     # P(u+1, v) - P(u-1, v), at every pixel
        Py = (P[:, 2:, 1:-1] - P[:, :-2, 1:-1]).astype(F)
        n = _cross(Py, Px)
        nn = ((n[0] * n[0] + n[1] * n[1]).astype(F) + n[2] * n[2]).astype(F)
        interior = np.zeros((h, w), bool)
        interior[1:-1, 1:-1] = True
        okp = _pad(ok)
        ok5 = interior & ok & okp[1:-1, :-2] & okp[1:-1, 2:] & okp[:-2, 1:-1] & okp[2:, 1:-1]
        nvalid = ok5 & (nn > 0) & (nn < np.inf)
        rl = (F(1.0) / np.sqrt(np.where(nvalid, nn, F(1.0)).astype(F))).astype(F)
        nh = [np.where(nvalid, (c * rl).astype(F), F(0.0)).astype(F) for c in n]
        out = dict(normals=np.stack(nh), depth_valid=ok, normal_valid=nvalid, gD=None, gA=None, valid=np.zeros((h, w), bool),
                   n_valid=0, loss64=0.0, sw64=0.0, loss=F(0.0), sw=F(0.0))
        if not prior:
            return out
        t = [np.where(interior, c, F(0.0)).astype(F) for c in case["t"]]
        wt = np.where(interior, case["w"], F(0.0)).astype(F) if weighted else np.ones((h, w), F)
        tt = ((t[0] * t[0] + t[1] * t[1]).astype(F) + t[2] * t[2]).astype(F)
        lvalid = nvalid & (wt > 0) & (tt > 0) & (tt < np.inf)
        rt = (F(1.0) / np.sqrt(np.where(lvalid, tt, F(1.0)).astype(F))).astype(F)
        q = [(c * rt).astype(F) for c in t]
        dot = _dot(nh, q)
        e = [(a - b).astype(F) for a, b in zip(nh, q)]
        l1 = ((np.abs(e[0]) + np.abs(e[1])).astype(F) + np.abs(e[2])).astype(F)
        term = (wt * ((cw * (F(1.0) - dot).astype(F)).astype(F) + (lw * l1).astype(F)).astype(F)).astype(F)
        inv_n = F(1.0) / F(h * w)
        wn = (wt * inv_n).astype(F)
        sgn = [np.where(c > 0, F(1.0), np.where(c < 0, F(-1.0), F(0.0))).astype(F) for c in e]
        b = [(wn * ((lw * s).astype(F) - (cw * c).astype(F)).astype(F)).astype(F) for s, c in zip(sgn, q)]
        s = _dot(nh, b)
        c = [((bk - (hk * s).astype(F)).astype(F) * rl).astype(F) for bk, hk in zip(b, nh)]
        gPx = _pad(np.stack([np.where(lvalid, k, F(0.0)).astype(F) for k in _cross(c, Py)]))
        gPy = _pad(np.stack([np.where(lvalid, k, F(0.0)).astype(F) for k in _cross(Px, c)]))
        lvp = _pad(lvalid)
        anyv = lvp[1:-1, :-2] | lvp[1:-1, 2:] | lvp[:-2, 1:-1] | lvp[2:, 1:-1]
        gP = (((gPx[:, 1:-1, :-2] - gPx[:, 1:-1, 2:]).astype(F) + gPy[:, :-2, 1:-1]).astype(F) - gPy[:, 2:, 1:-1]).astype(F)
        gd = (((gP[0] * ax).astype(F) + (gP[1] * ay).astype(F)).astype(F) + gP[2]).astype(F)
        a = np.where(anyv, A, F(1.0)).astype(F)
        gD = np.where(anyv, (gd / a).astype(F), F(0.0)).astype(F)
        gA = np.where(anyv, (-(((gd * d).astype(F) / a).astype(F))).astype(F), F(0.0)).astype(F)
    loss64 = float(term[lvalid].astype(np.float64).sum() / float(h * w))
    sw64 = float(wt[lvalid].astype(np.float64).sum())
    out.update(gD=gD, gA=gA, valid=lvalid, n_valid=int(lvalid.sum()), loss64=loss64, sw64=sw64, loss=F(loss64), sw=F(sw64))
    return out


def autograd64(case, weighted=True, cos_weight=1.0, l1_weight=0.0, min_alpha=MIN_ALPHA):
    """The definition in float64 with torch autograd: dict(gD, gA, normals, depth_valid, normal_valid, valid, loss).
    Written from the definition (slices, cross, norm), not from the mirror; the masks are computed here, in float64."""
    import torch
    h, w = case["D"].shape
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    D, A = T(case["D"]).requires_grad_(), T(case["A"]).requires_grad_()
    t = T(case["t"])
    wt = T(case["w"]) if weighted else torch.ones((h, w), dtype=torch.float64)
    zero = dict(gD=np.zeros((h, w)), gA=np.zeros((h, w)), normals=np.zeros((3, h, w)), depth_valid=(A.detach() > float(F(min_alpha))).numpy(),
                normal_valid=np.zeros((h, w), bool), valid=np.zeros((h, w), bool), loss=0.0)
    if h < 3 or w < 3:
        return zero
    ok = A.detach() > float(F(min_alpha))
    d = torch.where(ok, D / torch.where(ok, A, torch.ones_like(A)), torch.zeros_like(D))
    u = (torch.arange(w, dtype=torch.float64) + 0.5 - float(F(case["cx"]))) / float(F(case["fx"]))
    v = (torch.arange(h, dtype=torch.float64) + 0.5 - float(F(case["cy"]))) / float(F(case["fy"]))
    P = torch.stack([u[None, :] * d, v[:, None] * d, d], -1)                       # [h, w, 3]
    Px = P[1:-1, 2:] - P[1:-1, :-2]
    Py = P[2:, 1:-1] - P[:-2, 1:-1]
    n = torch.cross(Py, Px, dim=-1)
    nn = (n * n).sum(-1)
    ok5 = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1]
    nvalid = ok5 & (nn.detach() > 0) & torch.isfinite(nn.detach())
    nh = n / torch.where(nvalid, nn, torch.ones_like(nn)).sqrt()[..., None]
    ti = t[:, 1:-1, 1:-1].permute(1, 2, 0)
    tt = (ti * ti).sum(-1)
    lvalid = nvalid & (wt[1:-1, 1:-1] > 0) & (tt > 0) & torch.isfinite(tt)
    th = torch.where(lvalid[..., None], ti, torch.ones_like(ti)) / torch.where(lvalid, tt, torch.ones_like(tt)).sqrt()[..., None]
    ell = float(F(cos_weight)) * (1.0 - (nh * th).sum(-1)) + float(F(l1_weight)) * (nh - th).abs().sum(-1)
    loss = (wt[1:-1, 1:-1] * ell)[lvalid].sum() / (h * w)
    if lvalid.any():
        loss.backward()
        zero.update(gD=D.grad.numpy(), gA=A.grad.numpy())
    full = lambda m: np.pad(m.numpy(), 1)
    normals = np.zeros((3, h, w))
    normals[:, 1:-1, 1:-1] = torch.where(nvalid[..., None], nh.detach(), torch.zeros_like(nh)).permute(2, 0, 1).numpy()
    zero.update(normals=normals, normal_valid=full(nvalid), valid=full(lvalid), loss=float(loss.detach()))
    return zero


def ulp_distance(a, b):
    """Steps between two finite float32 values (through zero too)."""
    def key(v):
        i = int(np.float32(v).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))
