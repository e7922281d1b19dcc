"""The blend kernels' per-step decision chain.  The backward keeps ONE state per pixel, the Q1
counter rem = n_contrib - passers seen from the end of the list: the pixel is open while rem >= 0, a step contributes
where k = sat(passf * rem_before), and the open flag is NOT folded into the opacity - a closed pixel that still sees a
passer only takes rem further below zero.  The forward recomputes open = [T >= 1/255] from T alone, with T = 0 for a
pixel outside the image.  The scenes put weight on exactly those arguments:

  saturated   24x20 (outside-image lanes in the last quad column AND the last quad row), 700 opaque splats a few pixels
              wide: every tile list is longer than one 256-record batch and every pixel saturates with n_contrib below
              a third of its list - rem runs far below -1 on closed pixels, across batches, beside open neighbours;
  left_half   the same image with the splats confined to the left half: the right half has n_contrib == 0 and starts
              closed (rem = -1), inside waves whose other pixels are open;
  last        one tile, 8 splats stacked on one pixel that has n_contrib = 3: from the end, three contribute, the
              fourth closes the pixel without contributing (Q1), the fifth and the rest meet a closed pixel.

What each scene is for is first asserted on the ORACLE's output alone; then the GPU is compared with the oracle the way
tests/test_gpu_parity.py and tests/test_gpu_blend_groups.py do: forward outputs bit for bit, backward accumulators through
oracle/parity.py's all-element term bound and the 1e-4-of-scale bar - colour, depth + alpha map and AbsGrad routes, packed
and unpacked."""
import functools
import math

import numpy as np
import pytest
import torch

from absgrad_ref import abs_and_signed, per_pixel_channels
from util import check_blend_bounds, load_parity, max_err_over_max, np_, oracle_blend_terms, oracle_forward

pytestmark = pytest.mark.gpu

BG = (0.3, 0.1, 0.6)
W, H = 24, 20
BATCH = 256                   # records per LDS batch
GRAD_TOL = 1e-4               # the suite's bar: error relative to each tensor's scale
STACK_PX = (5, 6)             # scene "last": the pixel the eight splats sit on
STACK_OPACITY = (0.9, 0.9, 0.9, 0.5, 0.6, 0.3, 0.7, 0.4)      # front to back: T = 0.1, 0.01, 0.001 < 1/255 -> n_contrib 3


def _logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p / (1.0 - p))


def _splats(cam, u, v, z, sigma_px, logit, seed):
    """Isotropic Gaussians whose means project to pixel coordinates (u, v) at depths z, screen sigma sigma_px."""
    K = cam.intrinsics
    u, v, z = (np.atleast_1d(np.asarray(a, np.float64)) for a in (u, v, z))
    n = len(z)
    pos = np.stack([(u - K.cx) * z / K.fx, (v - K.cy) * z / K.fy, z], axis=1)
    s = np.log(np.broadcast_to(np.asarray(sigma_px, np.float64), (n,)) * z / K.fx)
    rng = np.random.default_rng(seed)
    return dict(positions=pos.astype(np.float32), sh_coeffs=rng.uniform(-1.0, 1.0, (n, 3, 1)).astype(np.float32),
                opacities=np.broadcast_to(np.asarray(logit, np.float64), (n,)).reshape(n, 1).astype(np.float32),
                rotations=np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)).astype(np.float32),
                scales=np.repeat(s[:, None], 3, axis=1).astype(np.float32))


def _arrays(name, cam):
    if name == "saturated":
        # 700 opaque splats, sigma 1.5 - 2.5 px, means over the image and a margin around it.  The seed is chosen (on
        # the CPU, test_scenes_do_what_they_are_for) so that every pixel saturates early in a long list.
        # 560 of them uniformly, 140 more around the small corner tile (8 x 4 pixels), whose list would stay short.
        rng = np.random.default_rng(3)
        n, k = 700, 560
        u = np.concatenate([rng.uniform(-2.0, W + 2.0, k), rng.uniform(14.0, W + 2.0, n - k)])
        v = np.concatenate([rng.uniform(-2.0, H + 2.0, k), rng.uniform(14.0, H + 2.0, n - k)])
        return _splats(cam, u, v, rng.permutation(n) * 0.01 + 2.0, rng.uniform(1.5, 2.5, n), 9.0, seed=1)
    if name == "left_half":
        # opaque and small: 3.33 sigma' (alpha >= 1/255) from a mean at x <= 8 stays left of the centre x = 12.5
        rng = np.random.default_rng(4)
        n = 300
        return _splats(cam, rng.uniform(0.0, 8.0, n), rng.uniform(0.0, H, n), rng.permutation(n) * 0.01 + 2.0,
                       rng.uniform(0.8, 1.0, n), 9.0, seed=2)
    assert name == "last"
    k = len(STACK_OPACITY)
    return _splats(cam, STACK_PX[0] + 0.5, STACK_PX[1] + 0.5, 2.0 + 0.25 * np.arange(k), 1.5, _logit(STACK_OPACITY), seed=3)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """The scene, the oracle's forward, the incoming gradients and the oracle's backward sums - computed once, shared,
    never modified."""
    import __graft_entry__ as ge
    pkg, orc = ge.load_package(), ge.load_oracle()
    w, h = (16, 16) if name == "last" else (W, H)
    cam = pkg.scene.make_camera(w, h)
    arrays = _arrays(name, cam)
    n = arrays["positions"].shape[0]
    ref = oracle_forward(orc, arrays, cam, bg=BG, degree=0)
    rng = np.random.default_rng(n)
    dC = (rng.standard_normal((h, w, 3)) / (w * h)).astype(np.float32)
    dD = (rng.standard_normal((h, w)) * 0.05 / math.sqrt(w * h)).astype(np.float32)
    dA = (rng.standard_normal((h, w)) * 0.3 / math.sqrt(w * h)).astype(np.float32)
    zrgb = np.ascontiguousarray(np.repeat(ref["depths"].astype(np.float32).reshape(-1, 1), 3, axis=1))
    want_depth = orc.rasterize_forward(w, h, (0.0, 0.0, 0.0), ref["tile_ranges"], ref["values"], ref["means_2d"],
                                       ref["cov_2d_inv"], zrgb, ref["opacities_act"])["color"][..., 0]
    for v in (dC, dD, dA, want_depth, *(a for a in ref.values() if isinstance(a, np.ndarray))):
        v.setflags(write=False)
    return dict(name=name, arrays=arrays, cam=cam, ref=ref, n=n, w=w, h=h, dC=dC, dD=dD, dA=dA, want_depth=want_depth)


@functools.lru_cache(maxsize=None)
def _terms(name, depth):
    import __graft_entry__ as ge
    s = _scene(name)
    kw = dict(dD=s["dD"], dA=s["dA"], depth_route=True) if depth else {}
    return oracle_blend_terms(ge.load_oracle(), s["ref"], s["dC"], BG, s["n"], s["w"], s["h"], **kw)


@functools.lru_cache(maxsize=None)
def _abs_want(name):
    import __graft_entry__ as ge
    s = _scene(name)
    ch = per_pixel_channels(ge.load_oracle(), s["ref"], s["n"], s["w"], s["h"], g=s["dC"], bg=BG)
    return abs_and_signed(ch["colour"])


def _passers(ref, px, py, w):
    """The tile-list entries (Gaussian ids, list order) that pass alpha >= 1/255 at pixel (px, py) for certain: in fp64,
    with a margin of 1 % above the decision."""
    ntx = (w + 15) // 16
    lo, hi = (int(x) for x in ref["tile_ranges"].reshape(-1, 2)[(py // 16) * ntx + px // 16])
    ids = ref["values"][lo:hi]
    m, ci = ref["means_2d"].astype(np.float64)[ids], ref["cov_2d_inv"].astype(np.float64)[ids]
    o = ref["opacities_act"].reshape(-1).astype(np.float64)[ids]
    dx, dy = px + 0.5 - m[:, 0], py + 0.5 - m[:, 1]
    q = ci[:, 0] * dx * dx + 2.0 * ci[:, 1] * dx * dy + ci[:, 2] * dy * dy
    oe = o * np.exp(-0.5 * q)
    return ids[(q >= 0.0) & (oe >= 1.01 / 255.0)]


def _deepest_rem(ref, qx, qy, w):
    """The backward walk of the wave whose quad starts at pixel (qx, qy), replayed in fp64 from the oracle's arrays: how
    far below zero the counter of a closed pixel sinks before the wave's last pixel closes (passers counted with the
    1 % margin, so at least this far)."""
    rem = ref["n_contrib"][qy:qy + 8, qx:qx + 8].astype(np.int64)
    hh, ww = rem.shape                                     # the quad's pixels inside the image
    ntx = (w + 15) // 16
    lo, hi = (int(x) for x in ref["tile_ranges"].reshape(-1, 2)[(qy // 16) * ntx + qx // 16])
    passes = np.zeros((hi - lo, hh, ww), bool)
    for y in range(hh):
        for x in range(ww):
            passes[np.isin(ref["values"][lo:hi], _passers(ref, qx + x, qy + y, w)), y, x] = True
    for p in range(hi - lo - 1, -1, -1):
        if not (rem >= 0).any():
            break
        rem -= passes[p]
    return int(rem.min())


def _list_lengths(ref, w, h):
    """[H, W]: the length of each pixel's tile list."""
    tr = ref["tile_ranges"].reshape(-1, 2)
    length = (tr[:, 1] - tr[:, 0]).reshape((h + 15) // 16, (w + 15) // 16)
    return np.repeat(np.repeat(length, 16, axis=0), 16, axis=1)[:h, :w]


def test_scenes_do_what_they_are_for():
    """From the oracle's output alone (no GPU work)."""
    # saturated: every list spans more than one batch; every pixel closed in the forward (T < 1/255) with n_contrib
    # below a third of its list; so the backward's closed pixels meet passers in the rest of the list
    s = _scene("saturated")
    ref, length = s["ref"], _list_lengths(s["ref"], W, H)
    assert W % 16 == 8 and H % 16 == 4                      # outside lanes: the last quad column, the last quad row
    assert length.min() > BATCH, length.min()
    assert np.all(ref["final_T"] < 1.0 / 255.0)
    assert np.all(ref["n_contrib"] > 0) and np.all(3 * ref["n_contrib"] < length), (ref["n_contrib"].max(), length.min())
    for qx, qy in ((0, 0), (8, 8), (16, 0), (16, 16)):      # full quads, and the ones cut by the right / bottom edge
        assert _deepest_rem(ref, qx, qy, W) <= -4, (qx, qy)   # closed pixels keep counting beside open neighbours
    # left_half: the right half starts closed, the left half does not, and both kinds share waves (columns 8 .. 15)
    s = _scene("left_half")
    ref = s["ref"]
    assert not ref["n_contrib"][:, 12:].any() and np.all(ref["final_T"][:, 12:] == 1.0)
    assert np.all(ref["n_contrib"][:, 8:12].max(axis=1) > 0) and np.all(ref["n_contrib"][:, :8] > 0)
    # last: n_contrib = 3 on the stack's pixel; all eight pass there
    s = _scene("last")
    ref = s["ref"]
    px, py = STACK_PX
    assert ref["n_contrib"][py, px] == 3
    assert np.array_equal(_passers(ref, px, py, 16), np.arange(8)) and np.array_equal(ref["values"], np.arange(8))
    assert ref["n_contrib"].max() > 4                       # neighbours stay open into the second hit group


def _bits(a):
    return np.ascontiguousarray(np_(a) if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def _t(a, dev):
    return torch.tensor(np.asarray(a)).to(dev)              # a copy: the shared arrays are read-only


def _render(pkg, dev, s):
    model = pkg.scene.to_model({k: np.array(v) for k, v in s["arrays"].items()}, dev)   # copies: the shared ones may be read-only
    out = pkg.render(model, s["cam"], pkg.RenderSettings(background=list(BG), active_sh_degree=0), want_depth_map=True)
    assert np.array_equal(np_(out.gaussian_indices), s["ref"]["values"])
    assert np.array_equal(np_(out.tile_ranges), s["ref"]["tile_ranges"])
    return out


def _forward_equal(s, f, route, depth):
    ref = s["ref"]
    assert np.array_equal(_bits(f.color), _bits(ref["color"])), route
    assert np.array_equal(_bits(f.final_T), _bits(ref["final_T"])), route
    assert np.array_equal(np_(f.n_contrib), ref["n_contrib"]), route
    if depth:
        assert np.array_equal(_bits(f.depth_map), _bits(s["want_depth"])), route


def _backward(pkg, dev, s, out, packed, dC, depth=False, abs_grad=False):
    src = dict(packed=out.packed) if packed else dict(packed=None)
    extra = dict(depths=out.depths, dL_ddepth_map=_t(s["dD"], dev), dL_dalpha=_t(s["dA"], dev)) if depth else {}
    if abs_grad:
        extra["want_abs_grad"] = True
    return pkg.rasterize_backward(_t(dC, dev), out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                  out.gaussian_indices, out.final_T, out.n_contrib, s["w"], s["h"], BG, s["n"], **src,
                                  **extra)


def _check_against_oracle(s, rb, depth, route):
    par = load_parity()
    want, mags = _terms(s["name"], depth)
    got = {k: np_(getattr(rb, k)) for k in par.ACCUMULATORS}
    if depth:
        got["dL_ddepths"] = np_(rb.dL_ddepths)
    entries = np.bincount(s["ref"]["values"], minlength=s["n"])
    check_blend_bounds(got, want, mags, s["ref"]["cov_2d_inv"], entries, route)
    for k in got:
        err = par.over_scale(got[k], want[k])
        print(f"{route}: {k} error / scale = {err:.3e}")
        assert err <= GRAD_TOL, (route, k, err)
    return got


@pytest.mark.parametrize("packed", (True, False), ids=("packed", "unpacked"))
@pytest.mark.parametrize("route", ("colour", "depth", "abs"))
@pytest.mark.parametrize("name", ("saturated", "left_half"))
def test_counter_against_the_oracle(pkg, dev, name, route, packed):
    """Cases 1, 2 and 4: forward + backward of both scenes on every route that shares the step."""
    s = _scene(name)
    out = _render(pkg, dev, s)
    depth, abs_grad = route == "depth", route == "abs"
    label = f"{name}: {'packed' if packed else 'unpacked'}/{route}"
    _forward_equal(s, out, label + " render", True)
    src = dict(packed=out.packed) if packed else dict(packed=None)
    dk = dict(depths=out.depths) if depth else {}
    fwd = pkg.rasterize_forward(out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                out.gaussian_indices, s["w"], s["h"], BG, **src, **dk)
    _forward_equal(s, fwd, label, depth)
    if name == "left_half":
        assert np.all(np_(fwd.final_T)[:, 12:] == 1.0) and not np_(fwd.n_contrib)[:, 12:].any()

    rb = _backward(pkg, dev, s, out, packed, s["dC"], depth=depth, abs_grad=abs_grad)
    _check_against_oracle(s, rb, depth, label)
    if abs_grad:
        want_abs, signed = _abs_want(name)
        got_abs = np_(rb.dL_dmeans_2d_abs)
        err = max_err_over_max(got_abs, want_abs)
        print(f"{label}: dL_dmeans_2d_abs error / scale = {err:.3e}")
        assert np.all(got_abs >= 0.0) and err <= GRAD_TOL, (label, err)
        assert max_err_over_max(np_(rb.dL_dmeans_2d), signed) <= GRAD_TOL

    if name == "left_half":
        # the pixels that start closed carry nothing: with the incoming gradients live ONLY there, every accumulator is
        # exactly zero (their D is not: it starts from the background term)
        dC = np.array(s["dC"])
        dC[:, :12] = 0.0
        assert np.abs(dC).max() > 0
        rz = _backward(pkg, dev, s, out, packed, dC, depth=False, abs_grad=abs_grad)
        for k in load_parity().ACCUMULATORS + (("dL_dmeans_2d_abs",) if abs_grad else ()):
            assert not np_(getattr(rz, k)).any(), (label, k)
        assert not np_(rz.grad_accum).any(), label


@pytest.mark.parametrize("packed", (True, False), ids=("packed", "unpacked"))
def test_last_contributor(pkg, orc, dev, packed):
    """Case 3: from the end of the list the stack's pixel takes three contributions, the fourth passer closes it
    without contributing (Q1), the fifth meets a closed pixel."""
    s = _scene("last")
    ref, n, w, h = s["ref"], s["n"], s["w"], s["h"]
    out = _render(pkg, dev, s)
    label = f"last: {'packed' if packed else 'unpacked'}"
    _forward_equal(s, out, label, True)
    # the whole tile against the oracle
    rb = _backward(pkg, dev, s, out, packed, s["dC"])
    _check_against_oracle(s, rb, False, label)
    # the stack's pixel alone: a gradient that is live only there
    px, py = STACK_PX
    one = np.zeros((h, w, 3), np.float32)
    one[py, px] = (0.7, -0.4, 0.9)
    want = orc.rasterize_backward(w, h, BG, ref["tile_ranges"], ref["values"], ref["means_2d"], ref["cov_2d_inv"],
                                  ref["rgb"], ref["opacities_act"], one, ref["final_T"], ref["n_contrib"], n)
    want_o = np.asarray(want["dL_dopacity_act"], np.float64).reshape(-1)
    got_o = np_(_backward(pkg, dev, s, out, packed, one).dL_dopacity_act).astype(np.float64).reshape(-1)
    print(f"{label}: dL_dopacity_act of the pixel  got {got_o}  want {want_o}")
    assert np.all(want_o[5:] != 0.0) and not want_o[:5].any()          # the oracle: the last three and nobody else
    assert np.max(np.abs(got_o[3:] - want_o[3:])) <= GRAD_TOL * np.abs(want_o).max(), label
    assert got_o[4] == 0.0 and got_o[3] == 0.0, label                  # the closing passer, and the first one after it
    assert not got_o[:3].any(), label
