"""Camera-pose gradient without a GPU: the fp64 model tests/pose_ref.py pinned to the oracle and to its
own central differences, pose.viewmat_grad_to_se3 against fp64 autograd through the exponential map, and the C ABI's
argument checks, which fail before anything is queued."""
import ctypes as C

import numpy as np
import torch

import pose_ref

EINVAL, EWORKSPACE = -1, -4
FAKE = C.c_void_p(1 << 20)            # 64-byte aligned, never dereferenced on these paths
NUL = C.c_void_p(0)


def _camera(pkg, w, h):
    """A camera whose W has no zero entry: orbit view 2, turned a little about every axis."""
    cam = pkg.scene.make_camera(w, h, view=2)
    return pkg.pose.apply_se3(cam, [0.05, -0.03, 0.1, 0.04, -0.06, 0.03])


def _grads_2d(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((n, 2)) * 1e-3).astype(np.float32),
            (rng.standard_normal((n, 3)) * 1e-2).astype(np.float32),
            (rng.standard_normal(n) * 1e-3).astype(np.float32))


def test_pose_ref_matches_the_oracle_projection_backward(pkg, orc):
    w, h, n = 320, 240, 3000
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=0, seed=41, mu_s=-4.0)
    arrays["positions"][:100, 2] *= -1.0                       # behind the camera: radius 0
    cam = _camera(pkg, w, h)
    K = cam.intrinsics
    view = cam.world_to_camera()
    fwd = orc.project_forward(arrays["positions"], arrays["rotations"], arrays["scales"], arrays["opacities"], view,
                              K.fx, K.fy, K.cx, K.cy, w, h)
    live = fwd["radii"] > 0
    assert 0.5 * n < live.sum() < n
    gm, gc, go = _grads_2d(n, 5)
    gm[~live] = 0.0
    gc[~live] = 0.0
    ref = orc.project_backward(arrays["positions"], arrays["rotations"], arrays["scales"], arrays["opacities"], view,
                               K.fx, K.fy, K.cx, K.cy, 1.0, fwd["radii"], gm, gc, go)
    # the model's position gradient is the oracle's, element-wise within the project's bar
    dp = pose_ref.position_grads(arrays, cam, gm, gc)
    scale = np.abs(ref["dL_dpositions"]).max()
    assert np.abs(dp - ref["dL_dpositions"]).max() <= 1e-4 * scale
    # and sum_i dL/dtvec_i = W sum_i dL/dp_i (t = W p + tvec, W orthonormal)
    rows = pose_ref.camera_rows(arrays, cam, gm, gc, live=live)
    W = view[:3, :3].astype(np.float64)
    want = W @ ref["dL_dpositions"].astype(np.float64).sum(0)
    bound = 1e-4 * np.abs(rows[:, 9:]).sum(0).max()
    assert np.abs(rows[:, 9:].sum(0) - want).max() <= bound


def test_pose_ref_matches_its_central_differences(pkg):
    w, h, n = 160, 120, 40
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=0, seed=9, mu_s=-3.0)
    cam = _camera(pkg, w, h)
    gm, gc, gz = _grads_2d(n, 6)
    rows = pose_ref.camera_rows(arrays, cam, gm, gc, g_z=gz).sum(0)
    K = cam.intrinsics
    view = torch.as_tensor(cam.world_to_camera().astype(np.float32), dtype=torch.float64)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)

    def loss(v):
        means, conic, z = pose_ref.project(t(arrays["positions"]), t(arrays["rotations"]), t(arrays["scales"]),
                                           v[:3, :3].expand(n, 3, 3), v[:3, 3].expand(n, 3), K.fx, K.fy, K.cx, K.cy)
        return float((means * t(gm)).sum() + (conic * t(gc)).sum() + (z * t(gz)).sum())

    eps = 1e-6
    for k in range(12):
        r, c = (k // 3, k % 3) if k < 9 else (k - 9, 3)
        vp, vm = view.clone(), view.clone()
        vp[r, c] += eps
        vm[r, c] -= eps
        fd = (loss(vp) - loss(vm)) / (2 * eps)
        assert abs(fd - rows[k]) <= 1e-6 * max(np.abs(rows).max(), 1e-12), (k, fd, rows[k])


def test_viewmat_grad_to_se3_matches_autograd_through_the_exponential_map(pkg):
    cam = _camera(pkg, 64, 48)
    rng = np.random.default_rng(2)
    G = torch.as_tensor(rng.standard_normal((4, 4)), dtype=torch.float64)
    G[3] = 0.0
    view = torch.as_tensor(cam.world_to_camera(), dtype=torch.float64)
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    (pkg.pose.se3_exp(xi) @ view * G).sum().backward()
    got = pkg.pose.viewmat_grad_to_se3(G, cam)
    assert got.shape == (6,) and got.dtype == torch.float64
    assert torch.allclose(got, xi.grad, rtol=1e-6, atol=1e-9), (got, xi.grad)
    # away from 0 too: the exponential map against its own central differences
    x0 = torch.as_tensor([0.2, -0.1, 0.3, 0.4, -0.2, 0.1], dtype=torch.float64)
    x = x0.clone().requires_grad_(True)
    (pkg.pose.se3_exp(x) * G).sum().backward()
    for k in range(6):
        e = torch.zeros(6, dtype=torch.float64)
        e[k] = 1e-6
        fd = float(((pkg.pose.se3_exp(x0 + e) - pkg.pose.se3_exp(x0 - e)) * G).sum()) / 2e-6
        assert abs(fd - float(x.grad[k])) <= 1e-6


def test_apply_se3_composes_on_the_left_in_float64(pkg):
    cam = _camera(pkg, 64, 48)
    xi = [0.01, 0.02, -0.03, 0.02, 0.01, -0.04]
    moved = pkg.pose.apply_se3(cam, xi)
    want = pkg.pose.se3_exp(torch.as_tensor(xi, dtype=torch.float64)).numpy() @ cam.world_to_camera().astype(np.float64)
    assert moved.rotation.dtype == np.float32 and moved.translation.dtype == np.float32
    assert np.abs(moved.world_to_camera() - want).max() <= 1e-7                 # float64, rounded once
    R = moved.rotation.astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6
    back = pkg.pose.apply_se3(moved, [-v for v in xi])
    assert np.abs(back.world_to_camera() - cam.world_to_camera()).max() < 1e-6
    assert abs(pkg.pose.rotation_angle_deg(moved.rotation, cam.rotation) - np.degrees(np.linalg.norm(xi[3:]))) < 1e-4


def _opts(pose, mc=None):
    """cugs_projection_opts over a PoseGrad (or None: no block at all) and an McmcFused (or None)."""
    from cugs_amd import _lib
    if pose is None and mc is None:
        return None
    return C.byref(_lib.ProjectionOpts(mcmc=None if mc is None else C.pointer(mc),
                                       pose=None if pose is None else C.pointer(pose)))


def _plain(lib, pose, n=10, camera=True):
    from cugs_amd import _lib
    cam = _lib.Camera()
    return lib.cugs_project_backward_opts(n, 16, 3, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                          C.byref(cam) if camera else None, 1.0, FAKE, NUL, NUL, NUL, NUL,
                                          FAKE, FAKE, FAKE, FAKE, FAKE, NUL, NUL, _opts(pose), NUL)


def _adam(lib, pose, mcmc=False, n=10):
    from cugs_amd import _lib
    cam = _lib.Camera()
    adam = _lib.AdamFused()
    for g in range(5):
        adam.m[g] = adam.v[g] = FAKE.value
    args = (n, 16, 3, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, C.byref(cam), 1.0, FAKE, C.byref(adam))
    return lib.cugs_project_backward_adam_opts(*args, NUL, _opts(pose, _lib.McmcFused() if mcmc else None), NUL)


def test_pose_symbols_bound(pkg):
    from cugs_amd import _lib
    for name in ("cugs_pose_grad_workspace_bytes", "cugs_project_backward_opts", "cugs_project_backward_adam_opts"):
        assert name in _lib.SIGNATURES
        assert getattr(C.CDLL(pkg.LIB_PATH), name)
    for name in ("cugs_project_backward_pose", "cugs_project_backward_adam_pose", "cugs_project_backward_adam_mcmc",
                 "cugs_project_backward_adam_mcmc_pose", "cugs_project_backward_adam_sparse",
                 "cugs_project_backward_adam_sparse_pose"):          # now options of the two entries above
        assert name not in _lib.SIGNATURES
        assert not hasattr(C.CDLL(pkg.LIB_PATH), name)


def test_pose_workspace_bytes(pkg):
    from cugs_amd._lib import lib
    b0, b1, bm = (lib.cugs_pose_grad_workspace_bytes(n) for n in (0, 1, 6_000_000))
    assert 0 < b0 <= b1 < bm
    assert bm >= (6_000_000 // 256) * 12 * 4                       # one 12-float partial per workgroup at least
    assert lib.cugs_pose_grad_workspace_bytes(-1) == b0


def test_pose_entry_points_validate_before_queueing(pkg):
    from cugs_amd import _lib
    from cugs_amd._lib import lib
    n = 1000
    need = lib.cugs_pose_grad_workspace_bytes(n)
    ok = _lib.PoseGrad(FAKE.value, None, FAKE.value, need)
    small = _lib.PoseGrad(FAKE.value, None, FAKE.value, need - 1)
    no_out = _lib.PoseGrad(None, None, FAKE.value, need)
    no_ws = _lib.PoseGrad(FAKE.value, None, None, need)
    for call in (lambda p, **k: _plain(lib, p, **k), lambda p, **k: _adam(lib, p, **k),
                 lambda p, **k: _adam(lib, p, mcmc=True, **k)):
        assert call(no_out, n=n) == EINVAL                      # no dL_dview
        assert call(no_ws, n=n) == EINVAL                       # no workspace
        assert call(small, n=n) == EWORKSPACE                   # one byte short
        assert call(no_out, n=0) == EINVAL                      # checked before the n == 0 early out
        assert call(None, n=0) == 0                             # no pose block: the entry without the camera gradient
        assert call(ok, n=-1) == EINVAL
    assert _plain(lib, ok, camera=False) == EINVAL
