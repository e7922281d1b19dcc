"""Every valid combination of cugs_projection_opts through the two entries that take it (cugs_project_backward_opts,
cugs_project_backward_adam_opts), called directly: an option changes what it says it changes and nothing else, and a
request is served by the kernel it names.  Everything is compared bit for bit (torch.equal); that each mode equals its
unfused sequence stays with test_gpu_pose_grad.py, test_gpu_mcmc.py and test_gpu_sparse_adam.py.

The scene is small: 300 Gaussians (one full 256-thread workgroup and a partial one) in a 100 x 70 image, every seventh
behind the camera (radii == 0).  One rasterize_backward makes the accumulator rows; every call below reads those same
rows, so the blend's atomics do not enter.  Moments start non-zero: a Gaussian that is skipped differs from one that
is stepped with a zero gradient."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_pose_grad import _check_reduction, _misaligned
from util import np_

pytestmark = pytest.mark.gpu

N, W, H = 300, 100, 70
PARAMS = ("positions", "sh_coeffs", "opacities", "scales", "rotations")        # ParamGroup order


@pytest.fixture(scope="module")
def scene(pkg, dev):
    arrays = pkg.scene.make_gaussians(N, W, H, sh_degree=3, seed=31, mu_s=-4.0)
    arrays["positions"][::7, 2] *= -1.0
    cam = pkg.scene.make_camera(W, H)
    settings = pkg.RenderSettings(background=[0.2, 0.1, 0.3], active_sh_degree=3)
    out = pkg.render(pkg.scene.to_model(arrays, dev), cam, settings)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(W, H, seed=32) * 3000.0).to(dev)
    rb = pkg.rasterize_backward(g, out.means_2d, out.cov_2d_inv, out.rgb, out.opacities_act, out.tile_ranges,
                                out.gaussian_indices, out.final_T, out.n_contrib, W, H, settings.background, N,
                                packed=out.packed, unpack=False, tile_order=out.tile_order)
    torch.cuda.synchronize()
    assert bool(rb.grad_accum[:, :9].any())
    gen = torch.Generator(device="cpu").manual_seed(33)
    moments = {k: (torch.randn(arrays[k].shape, generator=gen) * 1e-3, torch.rand(arrays[k].shape, generator=gen) * 1e-6)
               for k in PARAMS}
    return arrays, cam, rb.grad_accum.clone(), moments


class _Case:
    """One storage / degree / alignment: fresh tensors per call, the C calls, and what they leave."""

    def __init__(self, pkg, dev, scene, num_coeffs, deg, aligned):
        arrays, self.cam, self.accum, self.moments = scene
        self.pkg, self.dev, self.c, self.deg, self.aligned = pkg, dev, num_coeffs, deg, aligned
        self.arrays = dict(arrays, sh_coeffs=np.ascontiguousarray(arrays["sh_coeffs"][:, :, :num_coeffs]))
        m = {k: torch.from_numpy(self.arrays[k]).to(dev) for k in PARAMS}
        proj = pkg.project_gaussians(m["positions"], m["rotations"], m["scales"], m["opacities"], m["sh_coeffs"], self.cam,
                                     deg)
        self.radii, self.gate = proj.radii.contiguous(), proj.colour_gate.contiguous()
        self.seen = self.radii > 0
        assert int(self.seen.sum()) > N // 2 and int((~self.seen).sum()) >= N // 7
        self.abi = self.cam.to_abi()
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def start(self):
        """name -> host tensor: the five parameters, and the moments every fused call starts from."""
        s = {k: torch.from_numpy(self.arrays[k]) for k in PARAMS}
        for k in PARAMS:
            cut = (lambda t: t[:, :, :self.c]) if k == "sh_coeffs" else (lambda t: t)
            s["m_" + k], s["v_" + k] = (cut(t) for t in self.moments[k])
        return s

    def _place(self, t, name):
        """On the device; the SH rows and the rotations 4 bytes off a 16-byte boundary on the unaligned route."""
        t = t.to(self.dev).contiguous()
        return t if self.aligned or not name.endswith(("sh_coeffs", "rotations")) else _misaligned(t)

    def model(self):
        return {k: self._place(t, k) for k, t in self.start().items() if k in PARAMS}

    def pose_block(self, rows=None):
        from cugs_amd import _lib
        view = torch.full((4, 4), 7.0, device=self.dev)
        ws = torch.empty(_lib.lib.cugs_pose_grad_workspace_bytes(N), dtype=torch.uint8, device=self.dev)
        pg = _lib.PoseGrad(view.data_ptr(), None if rows is None else rows.data_ptr(), ws.data_ptr(), ws.numel())
        return pg, view, ws

    def plain(self, entry, gate, pose=False, rows=None):
        """entry: 'legacy', 'null' (the _opts entry with NULL) or 'opts' (a block).  -> (outputs, dL_dview or None)."""
        from cugs_amd import _lib
        lib = _lib.lib
        m = self.model()
        shapes = dict(d_pos=(N, 3), d_rot=(N, 4), d_scl=(N, 3), d_opa=(N, 1), d_sh=(N, 3, self.c), d_means=(N, 2),
                      d_gated=(N, 3))
        o = {k: torch.full(s, 7.0, device=self.dev) for k, s in shapes.items()}
        if not self.aligned:
            o["d_rot"], o["d_sh"] = _misaligned(o["d_rot"]), _misaligned(o["d_sh"])
        P = lambda t: C.c_void_p(t.data_ptr())
        args = (N, self.c, self.deg, P(m["positions"]), P(m["rotations"]), P(m["scales"]), P(m["opacities"]),
                P(m["sh_coeffs"]), P(self.radii), P(self.gate) if gate else None, C.byref(self.abi), 1.0, P(self.accum),
                None, None, None, None, P(o["d_pos"]), P(o["d_rot"]), P(o["d_scl"]), P(o["d_opa"]), P(o["d_sh"]),
                P(o["d_means"]), P(o["d_gated"]))
        pg, view, ws = self.pose_block(rows) if pose else (None, None, None)
        if entry == "legacy":
            rc = lib.cugs_project_backward(*args, self.st)
        else:
            opts = _lib.ProjectionOpts(pose=C.pointer(pg) if pose else None)
            rc = lib.cugs_project_backward_opts(*args, None if entry == "null" else C.byref(opts), self.st)
        assert rc == 0
        torch.cuda.synchronize()
        return o, view

    def fused(self, entry, mode="dense", pose=False):
        """mode: 'dense', 'sparse' or 'mcmc'.  -> (parameters + moments + dL_dmeans_2d by name, dL_dview or None)."""
        from cugs_amd import _lib
        lib = _lib.lib
        state = {name: self._place(t, name) for name, t in self.start().items()}
        m = state
        a = _lib.AdamFused()
        for i, k in enumerate(PARAMS):
            a.m[i], a.v[i], a.lr[i] = state["m_" + k].data_ptr(), state["v_" + k].data_ptr(), 1e-3 * (i + 1)
        a.beta1, a.beta2, a.eps, a.bc1, a.bc2 = 0.9, 0.999, 1e-15, 10.0, 1000.0
        state["d_means"] = torch.full((N, 2), 7.0, device=self.dev)
        P = lambda t: C.c_void_p(t.data_ptr())
        args = (N, self.c, self.deg, P(m["positions"]), P(m["rotations"]), P(m["scales"]), P(m["opacities"]),
                P(m["sh_coeffs"]), P(self.radii), P(self.gate), C.byref(self.abi), 1.0, P(self.accum), C.byref(a),
                P(state["d_means"]))
        pg, view, ws = self.pose_block() if pose else (None, None, None)
        mc = _lib.McmcFused(0.05, 0.01, 5e5, 100.0, 0.005, 3, 1234, None)        # lambda_opacity > 0
        if entry == "legacy":
            rc = lib.cugs_project_backward_adam(*args, self.st)
        else:
            opts = _lib.ProjectionOpts(mcmc=C.pointer(mc) if mode == "mcmc" else None, pose=C.pointer(pg) if pose else None,
                                       sparse=1 if mode == "sparse" else 0)
            rc = lib.cugs_project_backward_adam_opts(*args, None if entry == "null" else C.byref(opts), self.st)
        assert rc == 0
        torch.cuda.synchronize()
        return state, view

    def before(self):
        """What fused() starts from, under the names of its result (d_means aside)."""
        return {name: t.to(self.dev) for name, t in self.start().items()}


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


# storage C at its full degree, C = 16 also at degree 1; 16-byte rows and rows 4 bytes off
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("num_coeffs,deg", [(1, 0), (4, 1), (9, 2), (16, 3), (16, 1)])
def test_every_option_combination(pkg, dev, scene, num_coeffs, deg, aligned):
    case = _Case(pkg, dev, scene, num_coeffs, deg, aligned)
    seen = case.seen
    views = {}

    # ---- the entry that writes gradients: with and without the gate bits ----
    rows = torch.full((N, 12), 7.0, device=dev)
    for gate in (True, False):
        legacy, _ = case.plain("legacy", gate)
        null, _ = case.plain("null", gate)
        off, none = case.plain("opts", gate)
        on, views["plain", gate] = case.plain("opts", gate, pose=True, rows=rows if gate else None)
        assert none is None
        _same(legacy, null, ("plain NULL", gate))                  # 1. NULL is the entry without options
        _same(legacy, off, ("plain all-zero block", gate))
        _same(off, on, ("plain pose", gate))                       # 2. pose changes nothing but dL_dview
        assert bool(legacy["d_pos"][seen].any()) and bool(legacy["d_sh"][seen].any())

    # ---- the fused entry: dense, sparse, MCMC ----
    result = {}
    legacy, _ = case.fused("legacy")
    null, _ = case.fused("null")
    _same(legacy, null, "fused NULL")                              # 1.
    for mode in ("dense", "sparse", "mcmc"):
        off, none = case.fused("opts", mode)
        on, views[mode] = case.fused("opts", mode, pose=True)
        assert none is None
        _same(off, on, ("fused pose", mode))                       # 2.
        result[mode] = off
    _same(legacy, result["dense"], "fused all-zero block")

    # 3. one camera gradient on every route, within the reduction's bound of the fp64 sum of the rows
    ref = views["plain", True]
    assert float(ref.abs().max()) > 0.0
    for route, v in views.items():
        assert torch.equal(v, ref), route
    _check_reduction(np_(ref), np_(rows).astype(np.float64))

    # 4. sparse: unseen rows keep their bits, seen rows are the dense step's, and dense does step unseen rows
    before = case.before()
    dense, sparse = result["dense"], result["sparse"]
    stepped_unseen = False
    for k in before:
        assert torch.equal(sparse[k][~seen], before[k][~seen]), ("sparse touched an unseen row", k)
        assert torch.equal(sparse[k][seen], dense[k][seen]), ("sparse differs on a seen row", k)
        stepped_unseen |= not torch.equal(dense[k][~seen], before[k][~seen])
        assert not torch.equal(dense[k][seen], before[k][seen]), ("nothing stepped", k)
    assert stepped_unseen
    assert torch.equal(sparse["d_means"], dense["d_means"])

    # 5. MCMC: the regulariser reaches the opacities
    assert not torch.equal(result["mcmc"]["opacities"], dense["opacities"])
