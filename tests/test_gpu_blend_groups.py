"""The edges only the GROUP form of the blend kernels' hit loop has: both kernels take the hits of a
64-record sub-batch four at a time as straight-line code and vote "all my pixels are closed" once per group; the
backward carries an unfinished group (1-3 record indices) into the next sub-batch of the same 256-record batch and runs
what is left at the end of the batch one step at a time.

Scenes (built in 3-D, SH degree 0, one stack per quad so that every count is known):
  counts        per-quad hit counts 0, 1, 2, 3 | 4, 5, 7, 6 inside one sub-batch, and a 72-entry list whose quad 0 has
                hits at list positions 60 .. 65 (a group that straddles the two sub-batches in the backward, a group plus
                a tail of two in the forward) beside a quad with 60 + 6 hits;
  closing_a/b/c eight opaque tile-wide splats with faint small ones in front of them (quad 0) and behind them (quad 3):
                every pixel closes at the second opaque splat in the forward and at the third from the end in the
                backward, so the waves close on the first, second and third step of a group in both kernels, with at
                least three more hits behind the closing one (the extra steps are taken);
  three_done    374 entries (two batches): quads 1-3 close inside the first batch they walk, in both directions, quad 0
                never does - the second batch is staged by four waves and walked by one.
What the scenes are meant to do is first established on the CPU from the ORACLE's arrays alone (_walk: the cull's exact
minimum of the quadratic form over the rectangle of the open pixels, the per-pixel replay in fp64, checked against the
oracle's n_contrib), then the GPU is compared with the oracle: forward outputs bit for bit, the backward through
oracle/parity.py's all-element term bound and the 1e-4-of-scale bar - {packed, unpacked} x {colour, depth + alpha
maps} x {spatial, longest-list-first order}."""
import math

import numpy as np
import pytest
import torch

from util import check_blend_bounds, load_parity, np_, oracle_blend_terms, oracle_forward

pytestmark = pytest.mark.gpu

BG = (0.3, 0.1, 0.6)
GROUP = 4                     # CUGS_HIT_GROUP
SUB, BATCH = 64, 256          # records per sub-batch / LDS batch
AMIN = 1.0 / 255.0


def _logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p / (1.0 - p))


def _splats(cam, u, v, z, sigma_px, opacity=None, logit=None, seed=0):
    """Isotropic Gaussians whose means project to pixel coordinates (u, v) at depths z, screen sigma sigma_px."""
    K = cam.intrinsics
    u, v, z = (np.atleast_1d(np.asarray(a, np.float64)) for a in (u, v, z))
    n = len(z)
    u, v = np.broadcast_to(u, (n,)), np.broadcast_to(v, (n,))
    pos = np.stack([(u - K.cx) * z / K.fx, (v - K.cy) * z / K.fy, z], axis=1)
    s = np.log(np.broadcast_to(np.asarray(sigma_px, np.float64), (n,)) * z / K.fx)
    op = np.broadcast_to(_logit(opacity) if logit is None else np.asarray(logit, np.float64), (n,))
    rng = np.random.default_rng(seed)
    return dict(positions=pos.astype(np.float32), sh_coeffs=rng.uniform(-1.0, 1.0, (n, 3, 1)).astype(np.float32),
                opacities=op.reshape(n, 1).astype(np.float32),
                rotations=np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)).astype(np.float32),
                scales=np.repeat(s[:, None], 3, axis=1).astype(np.float32))


def _cat(*parts):
    return {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts], axis=0)) for k in parts[0]}


QUAD_C = ((4.0, 4.0), (12.0, 4.0), (4.0, 12.0), (12.0, 12.0))      # quad centres inside a tile (wave = quad)
COUNTS = ((0, 1, 2, 3), (4, 5, 7, 6))
COUNT_TILES, STRADDLE_TILE = (0, 2), 4
CLOSING = {"closing_a": (0, 2), "closing_b": (1, 3), "closing_c": (3, 0)}     # faint splats (in front: quad 0, behind: quad 3)


def _faint(cam, tile, quad, z, seed):
    """Small faint splats at a quad's centre: hits of that quad alone (4.1 px from the nearest centre of any other)."""
    cx, cy = QUAD_C[quad]
    rng = np.random.default_rng(seed)
    k = len(z)
    return _splats(cam, 16 * tile + cx + rng.uniform(-0.4, 0.4, k), cy + rng.uniform(-0.4, 0.4, k), z,
                   rng.uniform(1.0, 1.2, k), opacity=rng.uniform(0.02, 0.05, k), seed=seed)


def _scene(name, pkg):
    if name == "counts":
        cam = pkg.scene.make_camera(80, 16)                # tiles 0, 2, 4 used: a 3-sigma radius reaches no used neighbour
        parts, zs = [], iter(np.linspace(2.0, 9.0, 200))
        for tile, counts in zip(COUNT_TILES, COUNTS):
            for quad, k in enumerate(counts):
                if k:
                    parts.append(_faint(cam, tile, quad, [next(zs) for _ in range(k)], 10 * tile + quad))
        z = 2.0 + 0.05 * np.arange(72)                     # the straddle tile's list in depth order: position p has depth z[p]
        parts.append(_faint(cam, STRADDLE_TILE, 3, z[:60], 31))
        parts.append(_faint(cam, STRADDLE_TILE, 0, z[60:66], 32))
        parts.append(_faint(cam, STRADDLE_TILE, 3, z[66:], 33))
        return _cat(*parts), cam
    cam = pkg.scene.make_camera(16, 16)
    if name in CLOSING:
        near, far = CLOSING[name]
        parts = [_splats(cam, 8.0, 8.0, 4.0 + 0.1 * np.arange(8), 40.0, logit=9.0, seed=1)]
        if near:
            parts.append(_faint(cam, 0, 0, 2.0 + 0.1 * np.arange(near), 2))
        if far:
            parts.append(_faint(cam, 0, 3, 8.0 + 0.1 * np.arange(far), 3))
        return _cat(*parts), cam
    assert name == "three_done"
    parts = [_splats(cam, 8.0, 8.0, np.linspace(1.0, 1.9, 20), 16.0, opacity=0.012, seed=4),
             _splats(cam, 8.0, 8.0, np.linspace(3.0, 10.0, 330), 16.0, opacity=0.012, seed=5)]
    for quad in (1, 2, 3):
        parts.append(_splats(cam, QUAD_C[quad][0], QUAD_C[quad][1], 2.0 + 0.1 * quad + 0.01 * np.arange(8), 5.0,
                             logit=9.0, seed=6 + quad))
    return _cat(*parts), cam


def _qmin(mx, my, a, b, c, x0, y0, x1, y1):
    """min of a dx^2 + 2 b dx dy + c dy^2 over the rectangle of centres [x0, x1] x [y0, y1] (fp64, per entry): 0 with
    the mean inside, else on the boundary, each edge at its clamped 1-D minimiser - what may_touch_quad bounds."""
    lx, hx, ly, hy = x0 - mx, x1 - mx, y0 - my, y1 - my
    best = np.full(mx.shape, np.inf)
    for xe in (lx, hx):
        yv = np.clip(-b * xe / c, ly, hy)
        best = np.minimum(best, a * xe * xe + 2.0 * b * xe * yv + c * yv * yv)
    for ye in (ly, hy):
        xv = np.clip(-b * ye / a, lx, hx)
        best = np.minimum(best, a * xv * xv + 2.0 * b * xv * ye + c * ye * ye)
    return np.where((lx <= 0) & (hx >= 0) & (ly <= 0) & (hy >= 0), 0.0, best)


def _walk(ref, w, tile, quad):
    """One wave's walk of its tile list in both directions, from the oracle's arrays: per 64-record chunk the list
    positions the cull lets through (against the bounding box of the pixels open when the chunk is tested), and the list
    position at which the last pixel closes (None: the wave never closes).  The per-pixel replay is checked against
    the oracle's n_contrib; an entry whose cull margin is inside the kernel's slack would make the count ambiguous and
    fails the test."""
    lo, hi = (int(x) for x in ref["tile_ranges"][tile])
    ids = ref["values"][lo:hi]
    L = len(ids)
    mean = ref["means_2d"][ids].astype(np.float64).reshape(L, 2)
    cov = ref["cov_2d_inv"][ids].astype(np.float64).reshape(L, 3)
    o = ref["opacities_act"].reshape(-1)[ids].astype(np.float64)
    ntx = w // 16
    qx, qy = 16 * (tile % ntx) + 8 * (quad & 1), 16 * (tile // ntx) + 8 * (quad >> 1)
    lane = np.arange(64)
    px, py = qx + (lane & 7) + 0.5, qy + (lane >> 3) + 0.5
    dx, dy = px[None, :] - mean[:, 0:1], py[None, :] - mean[:, 1:2]
    q = cov[:, 0:1] * dx * dx + 2.0 * cov[:, 1:2] * dx * dy + cov[:, 2:3] * dy * dy
    alpha = np.minimum(0.99, o[:, None] * np.exp(-0.5 * q))
    passes = (alpha >= AMIN) & (q >= 0.0)
    tau = np.where(o >= AMIN, np.log(255.0 * np.maximum(o, 1e-30)), -1.0)

    def hits_of(chunk, open_):
        xs, ys = px[open_], py[open_]
        pos = np.arange(chunk * SUB, min(chunk * SUB + SUB, L))
        half = 0.5 * _qmin(mean[pos, 0], mean[pos, 1], cov[pos, 0], cov[pos, 1], cov[pos, 2], xs.min(), ys.min(),
                           xs.max(), ys.max())
        sure = (tau[pos] >= 0.0) & (half <= tau[pos])
        unsure = (tau[pos] >= 0.0) & ~sure & (half <= 1.02 * tau[pos] + 0.2)      # inside the cull's slack (x 2)
        assert not unsure.any(), ("ambiguous cull", tile, quad, pos[unsure])
        return pos[sure]

    nchunks = (L + SUB - 1) // SUB
    # forward: contributes, counts, THEN closes when T < 1/255
    T, open_, ncon = np.ones(64), np.ones(64, bool), np.zeros(64, np.int64)
    fwd, fclose = [], None
    for chunk in range(nchunks):
        if not open_.any():
            break
        fwd.append(hits_of(chunk, open_))
        for p in range(chunk * SUB, min(chunk * SUB + SUB, L)):
            act = passes[p] & open_
            T[act] *= 1.0 - alpha[p][act]
            ncon[act] += 1
            open_ &= ~(act & (T < AMIN))
            if fclose is None and not open_.any():
                fclose = p
    want_n = ref["n_contrib"][qy:qy + 8, qx:qx + 8].reshape(-1)
    assert np.array_equal(ncon, want_n), ("fp64 replay and the oracle disagree on n_contrib", tile, quad)
    # backward (quirk Q1): passers counted from the END, a pixel stops at the one beyond its n_contrib
    rem, open_ = want_n.astype(np.int64).copy(), want_n > 0
    bwd, bclose = [], None
    for chunk in range(nchunks - 1, -1, -1):
        if not open_.any():
            break
        bwd.append(hits_of(chunk, open_))
        for p in range(min(chunk * SUB + SUB, L) - 1, chunk * SUB - 1, -1):
            act = passes[p] & open_
            rem[act] -= 1
            open_ &= ~(act & (rem < 0))
            if bclose is None and not open_.any():
                bclose = p
    return dict(L=L, fwd=fwd, fclose=fclose, bwd=bwd, bclose=bclose)


def _group_step(order, close):
    """order: the hits of one group sequence in walking order (list positions); close: the list position at which the
    wave closes.  Returns (step inside its group 1..4, hits left behind the closing one) - the closing entry is a hit."""
    s = int(np.nonzero(order == close)[0][0])
    return s % GROUP + 1, len(order) - 1 - s


def _expectations(name, ref, w):
    """The CPU half: what each scene is for, established from the oracle alone."""
    ntiles = ref["tile_ranges"].shape[0]
    walks = {(t, qd): _walk(ref, w, t, qd) for t in range(ntiles) for qd in range(4)}
    if name == "counts":
        for t, counts in zip(COUNT_TILES, COUNTS):
            assert walks[(t, 0)]["L"] == sum(counts) < SUB
            for qd, k in enumerate(counts):
                wk = walks[(t, qd)]
                assert [len(c) for c in wk["fwd"]] == [k]                      # one sub-batch, k hits, nobody closes
                assert [len(c) for c in wk["bwd"]] == ([k] if k else [])       # k == 0: every n_contrib is 0, done at once
                assert wk["fclose"] is None and wk["bclose"] is None
        assert sorted(k % GROUP for c in COUNTS for k in c) == [0, 0, 1, 1, 2, 2, 3, 3]   # tails 0-3 with and without a group
        a, b = walks[(STRADDLE_TILE, 0)], walks[(STRADDLE_TILE, 3)]
        assert a["L"] == 72
        assert [c.tolist() for c in a["fwd"]] == [[60, 61, 62, 63], [64, 65]]  # forward: one group, then a tail of two
        assert [c.tolist() for c in a["bwd"]] == [[64, 65], [60, 61, 62, 63]]  # backward: 2 carried + 2 = a straddling group, 2 left
        assert [len(c) for c in b["fwd"]] == [60, 6] and [len(c) for c in b["bwd"]] == [6, 60]
        assert all(walks[(STRADDLE_TILE, qd)]["fwd"][0].size == 0 for qd in (1, 2))
        assert all(c.size == 0 for t in (1, 3) for qd in range(4) for c in walks[(t, qd)]["fwd"])   # listed there, never hit
        return
    if name in CLOSING:
        near, far = CLOSING[name]
        seen_f, seen_b = {}, {}
        for qd in range(4):
            wk = walks[(0, qd)]
            assert wk["L"] == 8 + near + far < SUB and wk["fclose"] is not None and wk["bclose"] is not None
            seen_f[qd] = _group_step(wk["fwd"][0], wk["fclose"])
            seen_b[qd] = _group_step(wk["bwd"][0][::-1], wk["bclose"])
        # every pixel closes at the second opaque splat (forward) / the third from the end (backward, Q1)
        assert seen_f[0][0] == (near + 1) % GROUP + 1 and seen_f[1][0] == 2
        assert seen_b[0][0] == (near + 2) % GROUP + 1 and seen_b[3][0] == (far + 2) % GROUP + 1 and seen_b[1][0] == 3
        # a closing step that is not the group's last is followed by enough hits to complete the group
        for step, left in list(seen_f.values()) + list(seen_b.values()):
            assert left >= GROUP - step
        return seen_f, seen_b
    assert name == "three_done"
    assert walks[(0, 0)]["L"] == 374
    for qd in (1, 2, 3):
        wk = walks[(0, qd)]
        assert wk["fclose"] is not None and wk["fclose"] < BATCH              # done inside the first batch it walks
        assert wk["bclose"] is not None and wk["bclose"] >= BATCH
    assert walks[(0, 0)]["fclose"] is None and walks[(0, 0)]["bclose"] is None
    assert len(walks[(0, 0)]["fwd"]) == 6 and len(walks[(0, 0)]["bwd"]) == 6  # all six sub-batches, both ways


def test_closing_scenes_cover_every_step_of_a_group(pkg, orc):
    """Together the three closing scenes put the closing step on the first, second and third step of a group in the
    forward and in the backward (CPU only: the oracle's arrays)."""
    fsteps, bsteps = set(), set()
    for name in CLOSING:
        arrays, cam = _scene(name, pkg)
        ref = oracle_forward(orc, arrays, cam, bg=BG, degree=0)
        f, b = _expectations(name, ref, cam.width)
        fsteps |= {s for s, _ in f.values()}
        bsteps |= {s for s, _ in b.values()}
    assert {1, 2, 3} <= fsteps and {1, 2, 3} <= bsteps


def _bits(a):
    return np.ascontiguousarray(np_(a) if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def _incoming(w, h, seed):
    rng = np.random.default_rng(seed)
    dC = (rng.standard_normal((h, w, 3)) / (w * h)).astype(np.float32)
    dD = (rng.standard_normal((h, w)) * 0.05 / math.sqrt(w * h)).astype(np.float32)
    dA = (rng.standard_normal((h, w)) * 0.3 / math.sqrt(w * h)).astype(np.float32)
    return dC, dD, dA


@pytest.mark.parametrize("scene", ("counts",) + tuple(CLOSING) + ("three_done",))
def test_blend_groups_against_the_oracle(pkg, orc, dev, scene):
    arrays, cam = _scene(scene, pkg)
    w, h = cam.width, cam.height
    n = arrays["positions"].shape[0]
    ref = oracle_forward(orc, arrays, cam, bg=BG, degree=0)
    _expectations(scene, ref, w)

    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=list(BG), active_sh_degree=0)
    out = pkg.render(model, cam, settings, want_depth_map=True)
    assert np.array_equal(np_(out.gaussian_indices), ref["values"])
    assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"])
    zrgb = np.ascontiguousarray(np.repeat(ref["depths"].astype(np.float32).reshape(-1, 1), 3, axis=1))
    want_depth = orc.rasterize_forward(w, h, (0.0, 0.0, 0.0), ref["tile_ranges"], ref["values"], ref["means_2d"],
                                       ref["cov_2d_inv"], zrgb, ref["opacities_act"])["color"][..., 0]

    def forward_equal(f, route, depth):
        assert np.array_equal(_bits(f.color), _bits(ref["color"])), route
        assert np.array_equal(_bits(f.final_T), _bits(ref["final_T"])), route
        assert np.array_equal(np_(f.n_contrib), ref["n_contrib"]), route
        if depth:
            assert np.array_equal(_bits(f.depth_map), _bits(want_depth)), route

    forward_equal(out, "render", True)
    dC, dD, dA = _incoming(w, h, n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    want_c, mags_c = oracle_blend_terms(orc, ref, dC, BG, n, w, h)
    want_d, mags_d = oracle_blend_terms(orc, ref, dC, BG, n, w, h, dD=dD, dA=dA, depth_route=True)
    entries = np.bincount(ref["values"], minlength=n)
    orders = {"spatial": None, "longest_first": pkg.rasterizer.tile_order_of(out.tile_ranges, w, h)}
    par = load_parity()
    for packed in (True, False):
        src = dict(packed=out.packed) if packed else dict(packed=None)
        for depth in (False, True):
            want, mags = (want_d, mags_d) if depth else (want_c, mags_c)
            for oname, order in orders.items():
                route = f"{scene}: {'packed' if packed else 'unpacked'}/{'depth' if depth else 'colour'}/{oname}"
                dk = dict(depths=out.depths) if depth else {}
                fwd = pkg.rasterize_forward(out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                            out.gaussian_indices, w, h, BG, tile_order=order, **src, **dk)
                forward_equal(fwd, route, depth)
                extra = dict(depths=out.depths, dL_ddepth_map=t(dD), dL_dalpha=t(dA)) if depth else {}
                rb = pkg.rasterize_backward(t(dC), out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act,
                                            out.tile_ranges, out.gaussian_indices, out.final_T, out.n_contrib, w, h, BG,
                                            n, tile_order=order, **src, **extra)
                got = {k: np_(getattr(rb, k)) for k in par.ACCUMULATORS}
                if depth:
                    got["dL_ddepths"] = np_(rb.dL_ddepths)
                check_blend_bounds(got, want, mags, ref["cov_2d_inv"], entries, route)
                for k in par.ACCUMULATORS:
                    assert par.over_scale(got[k], want[k]) <= 1e-4, (route, k)
