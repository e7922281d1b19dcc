"""Independent expectations for the data-parallel (multi-view) exchange path, made from the CPU oracle alone.

cugs_sh_backward_views rebuilds the SH gradient of a V-view batch as sum_v gated[v] (x) Y(dir_v), one thread per
Gaussian, starting from +0 and adding the views in order, contraction off: ONE correctly rounded fp32 multiply and ONE
correctly rounded fp32 add per term.  The oracle has that product already: orc.sh_backward with ALL-ZERO coefficients has
raw = 0.5 > 0 on every channel, so its gate is open and it returns exactly the fp32 products g[ch] * Y_k(dir) (0.0 in the
inactive columns), and orc.directions is the kernel's view_direction (the norm clamped at 1e-8).  Adding those in
np.float32, in view order, restates the kernel bit for bit (sh_views_fp32); the same products summed in float64 give the
value the rounding bound of tests/test_multiview_ref.py is taken against (sh_views_fp64).

The gate bits come from the oracle the same way: Y_0 is a non-zero constant, so with an all-ones gradient column 0 of
orc.sh_backward is non-zero exactly where the backward's own gate (raw > 0) is open (colour_gate).
"""
import numpy as np


def _centres(centres):
    c = np.ascontiguousarray(np.asarray(centres, dtype=np.float32).reshape(-1, 3))
    assert c.shape[0] >= 1
    return c


def view_products(orc, degree, positions, centres, gated, num_coeffs):
    """Yields, view by view, the [n, 3, C] float32 products gated[v][:, ch] * Y_k(dir_v) (0.0 for k >= (degree+1)^2)."""
    pos = np.ascontiguousarray(positions, np.float32)
    g = np.asarray(gated, np.float32)
    c = _centres(centres)
    n = pos.shape[0]
    assert g.shape == (c.shape[0], n, 3)
    zeros = np.zeros((n, 3, int(num_coeffs)), np.float32)
    for v in range(c.shape[0]):
        yield orc.sh_backward(int(degree), zeros, orc.directions(pos, c[v]), np.ascontiguousarray(g[v]))


def sh_views_fp32(orc, degree, positions, centres, gated, num_coeffs):
    """The kernel's sum, restated: from +0, acc = fl32(acc + fl32(g * Y)) for v = 0..V-1."""
    acc = np.zeros((np.asarray(positions).shape[0], 3, int(num_coeffs)), np.float32)
    for term in view_products(orc, degree, positions, centres, gated, num_coeffs):
        acc = acc + term
        assert acc.dtype == np.float32
    return acc


def sh_views_fp64(orc, degree, positions, centres, gated, num_coeffs, want_abs=False):
    """sum_v float64(g_v) * float64(Y_v) with the oracle's fp32 basis values (g = 1 returns them exactly); with
    `want_abs` also sum_v |g_v * Y_v|, the magnitude the fp32 rounding bound scales with."""
    pos = np.ascontiguousarray(positions, np.float32)
    g = np.asarray(gated, np.float32).astype(np.float64)
    n = pos.shape[0]
    ones = np.ones((g.shape[0], n, 3), np.float32)
    acc = np.zeros((n, 3, int(num_coeffs)), np.float64)
    mag = np.zeros_like(acc)
    for v, basis in enumerate(view_products(orc, degree, pos, centres, ones, num_coeffs)):
        term = g[v][:, :, None] * basis.astype(np.float64)
        acc += term
        mag += np.abs(term)
    return (acc, mag) if want_abs else acc


def colour_gate(orc, degree, sh_coeffs, positions, centre):
    """[n, 3] bool: the backward's own ReLU gate (raw colour + 0.5 > 0) of every channel for the camera at `centre`.
    `degree` is the ACTIVE degree (already clamped to what the coefficients store)."""
    sh = np.ascontiguousarray(sh_coeffs, np.float32)
    pos = np.ascontiguousarray(positions, np.float32)
    dirs = orc.directions(pos, np.asarray(centre, np.float32))
    return orc.sh_backward(int(degree), sh, dirs, np.ones((pos.shape[0], 3), np.float32))[:, :, 0] != 0


# ---- the reference's SyntheticConvergence (tests/test_training.cpp:159-261), inputs from a seeded numpy generator ----
CONV_SEED = 42
CONV_W, CONV_H, CONV_N, CONV_ITERS = 64, 48, 20, 100
CONV_LRS = (1e-4, 5e-2, 1e-2, 1e-3, 1e-4)            # ParamGroup order: positions, sh, opacities, scales, rotations
CONV_PARAMS = ("positions", "sh_coeffs", "opacities", "scales", "rotations")
CONV_GRADS = ("dL_dpositions", "dL_dsh_coeffs", "dL_dopacities", "dL_dscales", "dL_drotations")


def convergence_scene(seed=CONV_SEED):
    """(arrays, perturbed SH coefficients): 20 Gaussians in front of an identity camera; the target image is rendered
    from `arrays`, the optimisation starts from the same model with `perturbed` coefficients."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    n = CONV_N
    pos = 0.3 * rng.standard_normal((n, 3))
    pos[:, 2] = np.abs(pos[:, 2]) + 3.5
    q = rng.standard_normal((n, 4))
    q /= np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-8)
    scales = -1.5 + 0.2 * rng.standard_normal((n, 3))
    sh = 0.5 * rng.standard_normal((n, 3, 1))
    arrays = dict(positions=pos.astype(np.float32), sh_coeffs=sh.astype(np.float32),
                  opacities=np.full((n, 1), 2.0, np.float32), rotations=q.astype(np.float32),
                  scales=scales.astype(np.float32))
    perturbed = (arrays["sh_coeffs"] + rng.standard_normal((n, 3, 1)).astype(np.float32)).astype(np.float32)
    return arrays, perturbed


def convergence_camera_args():
    return dict(rotation=np.eye(3, dtype=np.float32), translation=np.zeros(3, np.float32), fx=100.0, fy=100.0, cx=32.0,
                cy=24.0)


def oracle_convergence(orc, loss_oracle, seed=CONV_SEED, iters=CONV_ITERS):
    """The whole loop on the CPU oracle.  Returns (initial_loss, final_loss, model): as in the reference, `final` is the
    loss of the LAST iteration's render (before its step), `initial` the loss of the perturbed model."""
    arrays, perturbed = convergence_scene(seed)
    cam = convergence_camera_args()
    K = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    rend = lambda m: orc.render(m, cam["rotation"], cam["translation"], *K, CONV_W, CONV_H, active_degree=0)
    target = rend(arrays)["color"].copy()
    model = {k: np.ascontiguousarray(v).copy() for k, v in arrays.items()}
    model["sh_coeffs"] = perturbed.copy()
    initial = loss_oracle.combined_loss_and_grad(rend(model)["color"], target)[0]
    m = {k: np.zeros_like(model[k]) for k in CONV_PARAMS}
    v = {k: np.zeros_like(model[k]) for k in CONV_PARAMS}
    final = initial
    for it in range(1, iters + 1):
        fwd = rend(model)
        final, g = loss_oracle.combined_loss_and_grad(fwd["color"], target)[:2]
        grads = orc.render_backward(g, fwd, model, *K, CONV_W, CONV_H)
        bc1, bc2 = orc.adam_bias_correction(0.9, 0.999, it)
        for name, gname, lr in zip(CONV_PARAMS, CONV_GRADS, CONV_LRS):
            grad = np.ascontiguousarray(grads[gname], np.float32).reshape(model[name].shape)
            orc.fused_adam(model[name], grad, m[name], v[name], lr, 0.9, 0.999, 1e-15, bc1, bc2)
    return initial, final, model
