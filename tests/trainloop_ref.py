"""One iteration of the adaptive-density training loop, stage by stage, on the CPU oracles - and the small scenario the
loop tests run (tests/test_trainloop_ref.py on the CPU, tests/test_gpu_trainloop.py on the device).

The order of one iteration, restated from the stage oracles the project already has:

  1. position learning rate of the step           orc.position_lr
  2. active SH degree of the step                 active_degree
  3. render the step's view                       orc.render
  4. loss and dL/dcolour                          loss_oracle.combined_loss_and_grad
  5. backward                                     orc.render_backward
  6. Adam                                         orc.fused_adam, orc.adam_bias_correction
  7. densification statistics                     densify_oracle.DensificationController.accumulate_gradients
  8. densify on schedule                          densify_oracle.DensificationController.densify
  9. opacity reset on schedule                    densify_oracle.DensificationController.reset_opacity

Every stage function below takes the state it starts from as arguments, returns new arrays and keeps nothing: the GPU
test hands them the device's own data after each stage.  run() chains them into a free-running loop.

No GPU and no call into the HIP library: `Ctx` carries the oracle modules and the package's scene module (numpy only),
which the tests load the usual way.  A model is a dict of float32 arrays (positions [N,3], sh_coeffs [N,3,16],
opacities [N,1], rotations [N,4], scales [N,3]), the layout orc.render takes.

Two semantics for the optimizer at a densify event:
  carried   the project's densify(optimizer=): survivors keep their moment rows (the oracle's keep mask without the
            split parents, in order), every new row starts at zero, the step count goes on;
  rebuilt   the reference's trainer: after any change a new optimizer - zero moments, step count 0 - whose position
            learning rate is set for the current step.
"""
from collections import namedtuple

import numpy as np
import torch

Ctx = namedtuple("Ctx", "orc loss_oracle densify_oracle scene")

# ---- the scenario ----------------------------------------------------------------------------------------------------
W, H = 100, 72                                  # 7 x 5 tiles: a partial tile column (4 px) and a partial tile row (8 px)
VIEWS = 3                                       # scene.make_camera(W, H, view=0..2), round robin
STEPS = 48                                      # numbered 1..48
N_TRUTH, N_START = 3000, 1500
STORED_DEGREE = 3
SCHEDULE = dict(densify_from=8, densify_every=8, opacity_reset_every=24, densify_until=48)
EVENT_STEPS = tuple(range(8, STEPS + 1, 8))
RESET_STEPS = (24, 48)
SCENE_EXTENT = 8.0
GRAD_THRESHOLD = 2e-5
PERCENT_DENSE = 0.025                           # clone below exp(scale) = 0.2, split from there: about half the start model each
PARAMS = ("positions", "sh_coeffs", "opacities", "scales", "rotations")          # ParamGroup order
GRADS = ("dL_dpositions", "dL_dsh_coeffs", "dL_dopacities", "dL_dscales", "dL_drotations")
MODEL_KEYS = ("positions", "sh_coeffs", "opacities", "rotations", "scales")      # the constructor order of a model
# multiview_ref.CONV_LRS with faster opacities and scales (a reset opacity has 8 steps to fall under the prune
# threshold or to recover), and a position schedule that moves visibly inside 48 steps
LRS = (2e-3, 5e-2, 1e-1, 1e-2, 1e-3)
POS_LR_FINAL, POS_LR_MAX_STEPS = 2e-4, 64
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
TRUTH_SEED, START_SEED, NOISE_SEED = 4801, 4802, 4800
TRUTH_MU_S, START_MU_S = -2.6, -1.8
START_Z_RANGE = (-1.0, 10.0)
# the loss drop (loss_drop) of run() per semantics, measured; tests/test_trainloop_ref.py holds run() to it and records
# the rest of what the scenario reaches
D_REF = {"carried": 0.080918, "rebuilt": 0.098642}


def active_degree(step):
    return min(step // 12, 3)


def view_of(step):
    return (step - 1) % VIEWS


def camera(ctx, view):
    return ctx.scene.make_camera(W, H, view=view)


def camera_args(cam):
    K = cam.intrinsics
    return (cam.rotation, cam.translation, K.fx, K.fy, K.cx, K.cy, cam.width, cam.height)


def truth_model(ctx):
    return ctx.scene.make_gaussians(N_TRUTH, W, H, sh_degree=STORED_DEGREE, seed=TRUTH_SEED, mu_s=TRUTH_MU_S)


def start_model(ctx):
    """Coarser than the truth, and fewer: the loop has to clone the small Gaussians and split the large ones.  The depth
    range starts behind the cameras: about a tenth of the rows are culled in every view, whatever the loop does (they
    get no gradient, so nothing clones, splits or moves them, and a reset opacity stays above the prune threshold)."""
    return ctx.scene.make_gaussians(N_START, W, H, sh_degree=STORED_DEGREE, seed=START_SEED, mu_s=START_MU_S,
                                    z_range=START_Z_RANGE)


_targets = {}


def targets(ctx):
    """The three target images, rendered once by the oracle from the truth model at degree 3 (read only)."""
    if "t" not in _targets:
        truth = truth_model(ctx)
        imgs = []
        for v in range(VIEWS):
            img = ctx.orc.render(truth, *camera_args(camera(ctx, v)), active_degree=STORED_DEGREE)["color"].copy()
            img.setflags(write=False)
            imgs.append(img)
        _targets["t"] = tuple(imgs)
    return _targets["t"]


def split_noise(step, n):
    """The [2, N, 3] standard-normal split noise of the event at `step`: the one rule of every run."""
    rng = np.random.Generator(np.random.Philox(key=NOISE_SEED + step))
    return rng.standard_normal((2, n, 3)).astype(np.float32)


def densify_config(mod):
    """DensificationConfig of `mod` (oracle/densify_oracle.py or the package: the same fields)."""
    return mod.DensificationConfig(grad_threshold=GRAD_THRESHOLD, percent_dense=PERCENT_DENSE, **SCHEDULE)


def copy_model(model):
    return {k: np.ascontiguousarray(model[k], np.float32).copy() for k in MODEL_KEYS}


def zero_moments(model):
    return ({k: np.zeros_like(model[k]) for k in PARAMS}, {k: np.zeros_like(model[k]) for k in PARAMS})


# ---- the stages ------------------------------------------------------------------------------------------------------
def learning_rates(ctx, step):
    """Stage 1: the five learning rates of `step` in ParamGroup order."""
    return (ctx.orc.position_lr(step, LRS[0], POS_LR_FINAL, POS_LR_MAX_STEPS),) + tuple(LRS[1:])


def render_stage(ctx, model, step):
    """Stages 2 and 3."""
    return ctx.orc.render(model, *camera_args(camera(ctx, view_of(step))), active_degree=active_degree(step))


def loss_stage(ctx, color, step):
    """Stage 4: (loss, dL_dcolor) against the target of the step's view.  On one host thread: at 100 x 72 libtorch's
    thread pool costs forty times what the eleven small convolutions do."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        loss, g = ctx.loss_oracle.combined_loss_and_grad(color, np.array(targets(ctx)[view_of(step)]))[:2]
    finally:
        torch.set_num_threads(threads)
    return loss, np.ascontiguousarray(g, np.float32)


def backward_stage(ctx, dL_dcolor, fwd, model, step):
    """Stage 5: `fwd` is render_stage's result on `model`."""
    _, _, fx, fy, cx, cy, w, h = camera_args(camera(ctx, view_of(step)))
    return ctx.orc.render_backward(np.ascontiguousarray(dL_dcolor, np.float32), fwd, model, fx, fy, cx, cy, w, h)


def adam_stage(ctx, model, grads, m, v, lrs, step_count):
    """Stage 6: one dense Adam step with the bias corrections of `step_count` (the optimizer's own count AFTER the
    step).  `grads` maps GRADS names to arrays.  Returns (model, m, v) as new arrays."""
    bc1, bc2 = ctx.orc.adam_bias_correction(BETA1, BETA2, step_count)
    model, m, v = copy_model(model), {k: m[k].copy() for k in PARAMS}, {k: v[k].copy() for k in PARAMS}
    for name, gname, lr in zip(PARAMS, GRADS, lrs):
        g = np.ascontiguousarray(grads[gname], np.float32).reshape(model[name].shape)
        ctx.orc.fused_adam(model[name], g, m[name], v[name], lr, BETA1, BETA2, EPS, bc1, bc2)
    return model, m, v


def _controller(ctx, accum):
    ctrl = ctx.densify_oracle.DensificationController(densify_config(ctx.densify_oracle), SCENE_EXTENT)
    if accum is not None:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32).copy())
        ctrl.grad_accum_, ctrl.grad_count_, ctrl.max_radii_2d_ = (t(a) for a in accum)
    return ctrl


def _accum(ctrl):
    return (ctrl.grad_accum_.numpy().copy(), ctrl.grad_count_.numpy().copy(), ctrl.max_radii_2d_.numpy().copy())


def accumulate_stage(ctx, accum, dL_dmeans_2d, radii):
    """Stage 7: `accum` = (grad_accum, grad_count, max_radii_2d) before, or None.  Returns the three after."""
    ctrl = _controller(ctx, accum)
    ctrl.accumulate_gradients(torch.from_numpy(np.ascontiguousarray(dL_dmeans_2d, np.float32)),
                              torch.from_numpy(np.ascontiguousarray(radii, np.int32)))
    return _accum(ctrl)


def _torch_model(ctx, model):
    return ctx.densify_oracle.Model(*(torch.from_numpy(np.ascontiguousarray(model[k], np.float32).copy())
                                      for k in MODEL_KEYS))


def densify_stage(ctx, model, accum, step, noise=None):
    """Stage 8 on `model` with the accumulators `accum`.  Returns (model, stats, info, accum): info["survivors"] is the
    bool mask over the rows of the OLD model that the new model keeps, in order, as its first rows (clones follow, then
    the split children); info["size_only"] counts the rows only the size rules remove - they pass the opacity test, are
    not split, and fail max_screen_size or the world-size test."""
    ctrl = _controller(ctx, accum)
    tm = _torch_model(ctx, model)
    n0 = tm.num_gaussians()
    split = ctrl.compute_split_mask(tm)
    keep = ctrl.compute_keep_mask(tm, step)
    cfg = ctrl.config_
    opacity_ok = torch.sigmoid(tm.opacities.squeeze(1)).ge(ctx.densify_oracle.f32(cfg.opacity_threshold))
    survivors = (keep & ~split).numpy().copy()
    info = dict(survivors=survivors, size_only=int((opacity_ok & ~keep & ~split).sum()))
    if noise is None:
        noise = split_noise(step, n0)
    stats = ctrl.densify(tm, step, torch.from_numpy(np.ascontiguousarray(noise, np.float32)))
    out = {k: getattr(tm, k).numpy().copy() for k in MODEL_KEYS}
    assert int(survivors.sum()) == stats.num_after - stats.num_cloned - 2 * stats.num_split
    return out, stats, info, _accum(ctrl)


def carry_moments(m, v, survivors, n_after):
    """The carried semantics: survivors' rows first, in order; every other row zero."""
    def carry(t):
        out = np.zeros((n_after,) + t.shape[1:], np.float32)
        kept = t[survivors]
        out[:kept.shape[0]] = kept
        return out
    return {k: carry(m[k]) for k in PARAMS}, {k: carry(v[k]) for k in PARAMS}


def changed(stats):
    return stats.num_cloned > 0 or stats.num_split > 0 or stats.num_pruned > 0


def reset_opacity_stage(ctx, model):
    """Stage 9."""
    tm = _torch_model(ctx, model)
    ctx.densify_oracle.DensificationController(densify_config(ctx.densify_oracle), SCENE_EXTENT).reset_opacity(tm)
    out = copy_model(model)
    out["opacities"] = tm.opacities.numpy().copy()
    return out


def should_densify(step):
    s = SCHEDULE
    return s["densify_from"] <= step <= s["densify_until"] and step % s["densify_every"] == 0


def should_reset_opacity(step):
    s = SCHEDULE
    return s["opacity_reset_every"] > 0 and step >= s["densify_from"] and step % s["opacity_reset_every"] == 0


def culled_rows(ctx, model, view):
    """How many rows of `model` the projection culls (radii <= 0) in `view`."""
    rotation, translation, fx, fy, cx, cy, w, h = camera_args(camera(ctx, view))
    proj = ctx.orc.project_forward(model["positions"], model["rotations"], model["scales"], model["opacities"],
                                   ctx.orc.view_matrix(rotation, translation), fx, fy, cx, cy, w, h)
    return int((proj["radii"] <= 0).sum())


def loss_drop(losses):
    """Mean loss of the first six steps minus that of the last six (two rounds of the three views each)."""
    return float(np.mean(losses[:6]) - np.mean(losses[-6:]))


# ---- the free-running loop -------------------------------------------------------------------------------------------
def run(ctx, semantics):
    """The 48 steps on the oracles.  Returns a record, per step: losses, n (after the step's Adam), pairs, culled (rows
    with radii <= 0, the smallest count over the three views), degrees, lrs; events [(step, stats, size_only)]; model."""
    assert semantics in ("carried", "rebuilt")
    model = copy_model(start_model(ctx))
    m, v = zero_moments(model)
    step_count, accum = 0, None
    rec = dict(losses=[], n=[], pairs=[], culled=[], degrees=[], events=[], lrs=[])
    for step in range(1, STEPS + 1):
        lrs = learning_rates(ctx, step)
        pre = model
        fwd = render_stage(ctx, model, step)
        loss, g = loss_stage(ctx, fwd["color"], step)
        grads = backward_stage(ctx, g, fwd, model, step)
        step_count += 1
        model, m, v = adam_stage(ctx, model, grads, m, v, lrs, step_count)
        if accum is not None and accum[0].shape[0] != model["positions"].shape[0]:
            accum = None
        accum = accumulate_stage(ctx, accum, grads["dL_dmeans_2d"], fwd["radii"])
        rec["losses"].append(loss)
        rec["n"].append(int(model["positions"].shape[0]))
        rec["pairs"].append(int(fwd["total_pairs"]))
        rec["culled"].append(min(culled_rows(ctx, pre, view) for view in range(VIEWS)))
        rec["degrees"].append(int(fwd["degree"]))
        rec["lrs"].append(lrs[0])
        if should_densify(step):
            model, stats, info, accum = densify_stage(ctx, model, accum, step)
            rec["events"].append((step, stats, info["size_only"]))
            if semantics == "carried":
                m, v = carry_moments(m, v, info["survivors"], stats.num_after)
            elif changed(stats):
                m, v = zero_moments(model)
                step_count = 0
            else:
                assert stats.num_after == stats.num_before
        if should_reset_opacity(step):
            model = reset_opacity_stage(ctx, model)
    rec["model"] = model
    return rec
