"""The blends' cull (cugs_raster_common.h: may_touch_quad against active_rect) against brute force, through the
DEVELOPMENT build's hook cugsdbg_may_touch_quad (libcugs_hip_dev.so, not part of the public C ABI).  A record the cull
rejects is lost for good in both blends, so the invariant is: if ANY open pixel of the quad lets the Gaussian through
(pixel_alpha_raw + passes_alpha_min, the kernels' own decision), the cull must say "may touch".  The hook builds the
record with write_packed, so tau = ln(255 o) is under test as well.  About a million adversarial cases in one launch:
opacities at and just above 1/255, means a few ulp from the open pixels' edges and on the alpha = 1/255 contour of an
open pixel, condition numbers up to 1e6 with |b| close to sqrt(ac), tiny and huge splats, every active-box size, quad
origins near 0, 1900 and 4000."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = 1 << 20


def _dev_lib(pkg):
    path = os.path.join(os.path.dirname(pkg.LIB_PATH), "libcugs_hip_dev.so")
    if not os.path.exists(path):
        pytest.skip("development library not built (make -C cuda-gaussian-splatting_amd/csrc)")
    return C.CDLL(path)


def _bbox(masks):
    """numpy bounding box of the set lanes (lane = y*8 + x): x0, y0, x1 - x0, y1 - y0."""
    bits = ((masks[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool).reshape(-1, 8, 8)
    cols, rows = bits.any(axis=1), bits.any(axis=2)
    x0, x1 = np.argmax(cols, axis=1), 7 - np.argmax(cols[:, ::-1], axis=1)
    y0, y1 = np.argmax(rows, axis=1), 7 - np.argmax(rows[:, ::-1], axis=1)
    return np.stack([x0, y0, x1 - x0, y1 - y0], axis=1).astype(np.float32)


def _rect_mask(x0, y0, wx, wy):
    m = np.zeros(x0.shape, np.uint64)
    for dy in range(8):
        for dx in range(8):
            inside = (dx >= x0) & (dx <= x0 + wx) & (dy >= y0) & (dy <= y0 + wy)
            m |= np.where(inside, np.uint64(1) << np.uint64(dy * 8 + dx), np.uint64(0))
    return m


def _cases(n, seed=20261016):
    rng = np.random.default_rng(seed)
    # ---- masks: full rectangles of every size 0..7 x 0..7, random subsets of them, single lanes, random density
    i = np.arange(n)
    wx, wy = i % 8, (i // 8) % 8
    x0 = rng.integers(0, 8 - wx)
    y0 = rng.integers(0, 8 - wy)
    rect = _rect_mask(x0, y0, wx, wy)
    fam = rng.integers(0, 4, n)
    rnd = rng.integers(0, 1 << 63, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    sparse = rnd & rng.integers(0, 1 << 63, n, dtype=np.uint64) & rng.integers(0, 1 << 63, n, dtype=np.uint64)
    single = np.uint64(1) << rng.integers(0, 64, n).astype(np.uint64)
    masks = np.select([fam == 0, fam == 1, fam == 2], [rect, rect & (rnd | single), single], sparse | single)
    masks = np.where(masks == 0, single, masks).astype(np.uint64)
    # ---- conics: eigenvalues 3.3 (the 0.3 px^2 low-pass) down to 1e-7, condition numbers up to 1e6
    l1 = 10.0 ** rng.uniform(-5.0, np.log10(3.3), n)
    kappa = 10.0 ** rng.uniform(0.0, 6.0, n)
    kappa = np.where(rng.random(n) < 0.3, 10.0 ** rng.uniform(4.0, 6.0, n), kappa)      # |b| close to sqrt(ac)
    l2 = np.maximum(l1 / kappa, 1e-7)
    th = rng.uniform(0.0, np.pi, n)
    cs, sn = np.cos(th), np.sin(th)
    a = (l1 * cs * cs + l2 * sn * sn).astype(np.float32)
    b = ((l1 - l2) * sn * cs).astype(np.float32)
    c = (l1 * sn * sn + l2 * cs * cs).astype(np.float32)
    # ---- opacities: exactly 1/255, a few ulp above, just above, anywhere, at and past the 0.99 cap
    lo = np.float32(1.0 / 255.0)
    ofam = rng.integers(0, 5, n)
    o = np.select([ofam == 0, ofam == 1, ofam == 2, ofam == 3],
                  [np.full(n, lo), lo + rng.integers(1, 16, n) * np.spacing(lo),
                   lo * (1.0 + 10.0 ** rng.uniform(-6.0, -1.0, n)), rng.uniform(float(lo), 0.99, n)],
                  rng.uniform(0.98, 1.0, n)).astype(np.float32)
    # ---- quads near 0, 1900 and 4000 px
    org = np.array([0, 1900, 4000])
    qx, qy = org[rng.integers(0, 3, n)], org[rng.integers(0, 3, n)]
    # ---- means.  (1) on the alpha = 1/255 contour of a random OPEN pixel (relative offsets +-1e-3 of tau, and 0);
    # (2) within a few ulp of an edge of the open pixels' box; (3) anywhere around the quad
    bits = ((masks[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    pick = np.argmax(rng.random((n, 64)) * bits, axis=1)        # a random open lane of each case
    pcx = (qx + (pick & 7)).astype(np.float64) + 0.5
    pcy = (qy + (pick >> 3)).astype(np.float64) + 0.5
    tau = np.log(255.0 * o.astype(np.float64))
    tau = np.maximum(tau, 0.0)
    u = rng.uniform(0.0, 2.0 * np.pi, n)
    ux, uy = np.cos(u), np.sin(u)
    qf = a.astype(np.float64) * ux * ux + 2.0 * b.astype(np.float64) * ux * uy + c.astype(np.float64) * uy * uy
    delta = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(-1e-3, 1e-3, n))
    t = np.sqrt(np.maximum(2.0 * tau * (1.0 + delta), 0.0) / np.maximum(qf, 1e-30))
    mx1, my1 = pcx - t * ux, pcy - t * uy
    box = _bbox(masks)
    ex = np.where(rng.random(n) < 0.5, box[:, 0], box[:, 0] + box[:, 2]) + qx + 0.5
    ey = np.where(rng.random(n) < 0.5, box[:, 1], box[:, 1] + box[:, 3]) + qy + 0.5
    ulps = rng.integers(-4, 5, n).astype(np.float32)
    mx2 = ex.astype(np.float32) + ulps * np.spacing(ex.astype(np.float32))
    my2 = np.where(rng.random(n) < 0.5, ey + ulps * np.spacing(ey.astype(np.float32)),
                   qy + rng.uniform(-20.0, 28.0, n))
    sig = 1.0 / np.sqrt(np.minimum(l2, 3.3))
    mx3 = qx + 4.0 + rng.normal(0.0, 1.0, n) * np.minimum(sig, 4000.0)
    my3 = qy + 4.0 + rng.normal(0.0, 1.0, n) * np.minimum(sig, 4000.0)
    mfam = rng.integers(0, 5, n)
    mx = np.select([mfam <= 2, mfam == 3], [mx1, mx2], mx3).astype(np.float32)
    my = np.select([mfam <= 2, mfam == 3], [my1, my2], my3).astype(np.float32)
    keep = (a.astype(np.float64) * c.astype(np.float64) - b.astype(np.float64) ** 2) > 0.0   # a real conic
    fields = np.stack([mx, my, a, b, c, o, qx.astype(np.float32), qy.astype(np.float32)], axis=1)[keep]
    return np.ascontiguousarray(fields, np.float32), np.ascontiguousarray(masks[keep]), mfam[keep]


def test_cull_never_rejects_a_gaussian_an_open_pixel_takes(pkg, dev):
    lib = _dev_lib(pkg)
    fields, masks, mfam = _cases(CASES)
    n = fields.shape[0]
    assert n > 0.99 * CASES
    f = torch.from_numpy(fields).to(dev)
    m = torch.from_numpy(masks.view(np.int64)).to(dev)
    hit = torch.empty(n, dtype=torch.int32, device=dev)
    passed = torch.empty(n, dtype=torch.int64, device=dev)
    rect = torch.empty((n, 4), dtype=torch.float32, device=dev)
    P = lambda x: C.c_void_p(x.data_ptr())
    rc = lib.cugsdbg_may_touch_quad(C.c_int(n), P(f), P(m), P(hit), P(passed), P(rect),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    hit, passed, rect = hit.cpu().numpy(), passed.cpu().numpy().view(np.uint64), rect.cpu().numpy()
    # active_rect is the bounding box of the open lanes
    want_rect = _bbox(masks)
    bad = np.flatnonzero((rect != want_rect).any(axis=1))
    assert bad.size == 0, (bad[:5], masks[bad[:5]], rect[bad[:5]], want_rect[bad[:5]])
    # a finished pixel never passes (open = 0 makes alpha 0)
    assert not np.any(passed & ~masks)
    # THE invariant: an open pixel that passes means the cull keeps the record
    lost = np.flatnonzero((passed != 0) & (hit == 0))
    print(f"cull: {n} cases, {int(np.count_nonzero(passed))} with an open pixel passing, "
          f"{int(np.count_nonzero(hit == 0))} culled, {lost.size} culled although a pixel passes; "
          f"contour cases {int(np.count_nonzero(mfam <= 2))}")
    assert lost.size == 0, [dict(zip(("mx", "my", "a", "b", "c", "o", "qx", "qy"), fields[j].tolist()),
                                 hex(int(masks[j])), hex(int(passed[j]))) for j in lost[:5]]
    # not vacuous: the margin is exercised from both sides
    contour = mfam <= 2
    assert np.count_nonzero(contour & (passed != 0)) > 0.2 * np.count_nonzero(contour)
    assert np.count_nonzero(contour & (passed == 0) & (hit == 1)) > 0.05 * np.count_nonzero(contour)
    assert np.count_nonzero(hit == 0) > 0.05 * n
