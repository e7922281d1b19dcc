"""Cameras and models as a real capture has them, shared by the CPU and GPU projection tests.

scene.make_camera / scene.make_gaussians give fx == fy, a principal point at the image centre, a rotation about the y
axis only, unit quaternions.  The cases here give none of that:

cameras (each a rotation R about the scene centre (0, 0, 6), t = c - R c; image sizes no multiple of 16)
  C0  scene.make_camera(w, h, view=2)                                                      the control
  C1  fx 0.93 W, fy 0.61 W, cx 0.37 W, cy 0.64 H, R = Rz(31) Ry(-23) Rx(17)                the general case
  C2  fx, fy as C1, cx -0.2 W, cy 1.3 H, R = Rz(90) Ry(-10) Rx(5)                          principal point outside the
                                                                                           image, a roll of 90 degrees
  C3  C1 moved C3_ADVANCE along its viewing axis into the cloud                            near plane, behind the camera

models (scene.make_gaussians with the quaternions rescaled row by row; log-scale spread 0.5 unless said)
  Q1  |q| log-uniform in [0.05, 20]
  Q2  |q| log-uniform in [1e-3, 1e3]; three rows exactly zero; eight rows with |q| in [5e-8, 2e-7], where the 1e-12
      under the root of the normalisation dominates; one row with three components exactly zero
  A1  Q1 with log-scales mu_s + 1.0 N(0, 1): anisotropic splats, ill-conditioned in fp32 (det Sigma' cancels)

The row metric: row_err(got, want) = max_j |got - want| / max_j |want| per Gaussian, each row judged against its own
largest element (dL/dq scales as 1 / |q|: a tensor-wide scale would see only the small-|q| rows).  A row whose `want`
is all zero is a culled Gaussian: its result must be exactly zero, and it is reported separately.
"""
import math

import numpy as np

N = 5 * 256 + 37                       # a ragged last workgroup
W, H = 300, 220                        # 18.75 x 13.75 tiles
SMALL = (48, 32, 24)                   # w, h, n of the fp64 render model (tests/test_oracle_autograd.py)
MU_S = -3.6
A1_SEED = 1                            # A1's scale draw, chosen likewise
SEED, GRAD_SEED = 2, 0                 # chosen on the CPU: tests/test_projection_ref.py says how and why
CENTRE = np.array([0.0, 0.0, 6.0])
C3_ADVANCE = 5.0                       # world units along the viewing axis; the counts it gives: assert_c3_counts
NEAR = 0.2                             # the projection culls t.z <= 0.2
CAMERAS = ("C0", "C1", "C2", "C3")
MODELS = ("Q1", "Q2")


def _rx(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _ry(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _rz(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _about_centre(pkg, w, h, fx, fy, cx, cy, R, advance=0.0):
    t = CENTRE - R @ CENTRE
    t[2] -= advance                                    # the camera moves forward: every t.z shrinks by `advance`
    return pkg.CameraInfo(width=w, height=h, intrinsics=pkg.CameraIntrinsics(fx, fy, cx, cy),
                          rotation=R.astype(np.float32), translation=t.astype(np.float32))


def camera(pkg, name, w=W, h=H):
    if name == "C0":
        return pkg.scene.make_camera(w, h, view=2)
    if name in ("C1", "C3"):
        return _about_centre(pkg, w, h, 0.93 * w, 0.61 * w, 0.37 * w, 0.64 * h, _rz(31.0) @ _ry(-23.0) @ _rx(17.0),
                             advance=C3_ADVANCE if name == "C3" else 0.0)
    if name == "C2":
        return _about_centre(pkg, w, h, 0.93 * w, 0.61 * w, -0.2 * w, 1.3 * h, _rz(90.0) @ _ry(-10.0) @ _rx(5.0))
    raise KeyError(name)


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), n))


def model(pkg, name, n=N, w=W, h=H, sh_degree=3, seed=SEED, mu_s=MU_S, a1_seed=None):
    """The arrays of scene.make_gaussians (float32, the reference's layouts) with the quaternion rows rescaled."""
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=sh_degree, seed=seed, mu_s=mu_s)
    rng = np.random.Generator(np.random.Philox(key=seed + 1))
    q = arrays["rotations"].astype(np.float64)                       # unit rows
    if name in ("Q1", "A1"):
        q *= _log_uniform(rng, 0.05, 20.0, n)[:, None]
    elif name == "Q2":
        q *= _log_uniform(rng, 1e-3, 1e3, n)[:, None]
        assert n >= 24
        rows = rng.permutation(n)[:12]
        q[rows[:3]] = 0.0                                            # exactly zero: R = I, dL/dq = 1e6 dL/d(unit q)
        unit = q[rows[3:11]] / np.linalg.norm(q[rows[3:11]], axis=1, keepdims=True)
        q[rows[3:11]] = unit * _log_uniform(rng, 5e-8, 2e-7, 8)[:, None]
        q[rows[11], 1:] = 0.0                                        # (w, 0, 0, 0)
    else:
        raise KeyError(name)
    arrays["rotations"] = q.astype(np.float32)
    if name == "A1":
        a1_seed = A1_SEED if a1_seed is None else a1_seed
        wide = np.random.Generator(np.random.Philox(key=a1_seed))
        arrays["scales"] = (mu_s + 1.0 * wide.standard_normal((n, 3))).astype(np.float32)
    if name == "Q2":
        norms = np.linalg.norm(arrays["rotations"].astype(np.float64), axis=1)
        assert (norms == 0.0).sum() == 3 and ((norms >= 4e-8) & (norms <= 2.5e-7)).sum() == 8
        assert ((arrays["rotations"] == 0.0).sum(1) == 3).sum() == 1
    return arrays


def camera_space(cam, positions):
    """t = W p + tvec in fp64 from the camera's float32 entries: [n, 3]."""
    Wm = np.asarray(cam.rotation, np.float32).astype(np.float64)
    tv = np.asarray(cam.translation, np.float32).astype(np.float64)
    return np.asarray(positions, np.float64) @ Wm.T + tv


def assert_c3_counts(cam, arrays):
    """What C3 is there for: between a fifth and a half of the Gaussians at or behind the near plane (negative t.z
    included), survivors just beyond it whose means land far off screen, and every mean below 1e6 px (the C oracle's
    float-to-int conversion stays defined).  Returns the counts."""
    t = camera_space(cam, arrays["positions"])
    n = t.shape[0]
    K = cam.intrinsics
    cut = t[:, 2] <= NEAR
    assert n / 5 <= cut.sum() <= n / 2, cut.sum()
    assert (t[:, 2] < 0.0).sum() >= 8
    close = (t[:, 2] > NEAR) & (t[:, 2] < 0.6)
    assert close.sum() >= 4, close.sum()
    alive = ~cut
    mx = K.fx * t[alive, 0] / t[alive, 2] + K.cx
    my = K.fy * t[alive, 1] / t[alive, 2] + K.cy
    assert max(np.abs(mx).max(), np.abs(my).max()) < 1e6
    cx_, cy_ = K.fx * t[close, 0] / t[close, 2] + K.cx, K.fy * t[close, 1] / t[close, 2] + K.cy
    far = (cx_ < -2.0 * cam.width) | (cx_ > 3.0 * cam.width) | (cy_ < -2.0 * cam.height) | (cy_ > 3.0 * cam.height)
    assert far.sum() >= 2, far.sum()
    return dict(cut=int(cut.sum()), behind=int((t[:, 2] < 0.0).sum()), close=int(close.sum()), far=int(far.sum()))


def row_err(got, want):
    """(err [n] float64, culled [n] bool): per Gaussian max_j |got - want| / max_j |want|; `culled` marks the rows whose
    `want` is all zero - their err is 0 when `got` is exactly zero there and inf otherwise."""
    want = np.asarray(want, np.float64)
    n = want.shape[0]
    want = want.reshape(n, -1)
    got = np.asarray(got, np.float64).reshape(n, -1)
    scale = np.abs(want).max(1)
    culled = scale == 0.0
    diff = np.abs(got - want).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(culled, np.where(diff == 0.0, 0.0, np.inf), diff / np.where(culled, 1.0, scale))
    return err, culled


def worst(err, culled):
    """The largest row error among the rows that are not culled (0 when there is none)."""
    live = ~culled
    return float(err[live].max()) if live.any() else 0.0


def stage_grads(n, seed=GRAD_SEED):
    """Incoming 2-D gradients for the projection backward stage, at the magnitudes a rendered loss gives them:
    dL_dmeans_2d [n,2], dL_dcov_2d_inv [n,3] (stored-b convention), dL_drgb [n,3], dL_dopacity_act [n]."""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((n, 2)) * 1e-3).astype(np.float32), (rng.standard_normal((n, 3)) * 1e-2).astype(np.float32),
            (rng.standard_normal((n, 3)) * 1e-2).astype(np.float32), (rng.standard_normal(n) * 1e-3).astype(np.float32))


def small_scene(pkg, model_name, seed=134):
    """The 48 x 32, n = 24 scene of tests/test_oracle_autograd.py with a model of this module: opacity ~0.17, so that
    no pixel saturates and no alpha reaches the 0.99 clamp.  Returns (arrays, background).  The seed is one whose cloud
    leaves 7 of the 24 Gaussians with a gradient under C2, which looks past most of it (18 under C1)."""
    w, h, n = SMALL
    arrays = model(pkg, model_name, n=n, w=w, h=h, sh_degree=3, seed=seed, mu_s=-2.2)
    arrays["opacities"] = (arrays["opacities"] * 0.5 - 1.6).astype(np.float32)
    return arrays, (0.3, 0.1, 0.2)
