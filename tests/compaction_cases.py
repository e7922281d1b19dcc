"""Inputs and CPU references for the compaction scans past one scan pass (tests/test_compaction_cases.py checks the
references alone, tests/test_gpu_compaction_scale.py runs them on the device).  Pure numpy / torch on the CPU.

densify, prune_gaussians and MCMCController.relocate order their output with a two-level prefix scan: one sum per
1024-row chunk, then ONE 256-thread workgroup that walks those sums in passes of 256 and carries the totals between
passes (k_scan_counts in csrc/densify.hip, k_reloc_scan in csrc/mcmc.hip).  One pass covers PASS = 256 * 1024 rows; the
carry only exists beyond that.  Test infrastructure (not collected by pytest)."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

f32 = np.float32
CHUNK = 1024                                   # SCAN_CHUNK: rows per count workgroup
PASS = 256 * CHUNK                             # rows per pass of the scan workgroup
SIZES = (PASS, PASS + 1, 2 * PASS + 1027)      # no carry (control) | a second pass of one row | three passes, 3-row tail
NAMES = ("positions", "sh_coeffs", "opacities", "rotations", "scales")


def num_passes(n: int) -> int:
    return -(-(-(-n // CHUNK)) // 256)


def pass_of(rows) -> np.ndarray:
    return np.asarray(rows, np.int64) // PASS


def count_per_pass(mask, n: int) -> np.ndarray:
    """How many set rows of `mask` (bool [n], or row indices) fall into each scan pass."""
    rows = np.nonzero(mask)[0] if np.asarray(mask).dtype == bool else np.asarray(mask, np.int64)
    return np.bincount(pass_of(rows), minlength=num_passes(n))


# ---- 1. flag bytes for cugs_densify_plan: bit 0 clone, bit 1 split, bit 2 keep -------------------------------------
FLAG_PATTERNS = ("random", "keep_all", "split_all", "none", "by_pass", "chunk_ends", "skewed")
# widths, out of 16 consecutive rows, of the keep-only / clone-only / split-only runs of "skewed" in scan pass p % 3;
# row 14 of the 16 is keep + split (counts as a split), row 15 carries no flag
_SKEW = ((2, 4, 8), (4, 8, 2), (8, 2, 4))


def flag_bytes(pattern: str, n: int) -> np.ndarray:
    rows = np.arange(n, dtype=np.int64)
    if pattern == "random":                                     # (a)
        return np.random.default_rng(n).integers(0, 8, n, dtype=np.uint8)
    if pattern == "keep_all":                                   # (b) the identity map
        return np.full(n, 4, np.uint8)
    if pattern == "split_all":                                  # (c) n_out = 2 n, the largest map
        return np.full(n, 2, np.uint8)
    if pattern == "none":                                       # (d) n_out = 0
        return np.zeros(n, np.uint8)
    if pattern == "by_pass":
        # (e) keep only in the first scan pass, clone only in the second, split only in the third; with fewer passes
        # the first pass is cut into equal parts so that the three groups exist and later passes stay pure
        p = num_passes(n)
        cuts = (PASS, 2 * PASS) if p >= 3 else (PASS // 2, PASS) if p == 2 else (n // 3, 2 * n // 3)
        return np.where(rows < cuts[0], 4, np.where(rows < cuts[1], 1, 2)).astype(np.uint8)
    if pattern == "chunk_ends":                                 # (f) only the last row of every chunk, and row n - 1
        f = np.zeros(n, np.uint8)
        ends = np.union1d(np.arange(CHUNK - 1, n, CHUNK), [n - 1])
        f[ends] = np.random.default_rng(n + 1).integers(1, 8, ends.size, dtype=np.uint8)
        return f
    if pattern == "skewed":                                     # (g) per pass three different non-zero totals
        w = np.asarray(_SKEW, np.int64)[pass_of(rows) % 3]
        r = rows % 16
        a, b, c = w[:, 0], w[:, 0] + w[:, 1], w[:, 0] + w[:, 1] + w[:, 2]
        return np.where(r < a, 4, np.where(r < b, 1, np.where(r < c, 2, np.where(r == 14, 6, 0)))).astype(np.uint8)
    raise ValueError(pattern)


def flag_masks(flags: np.ndarray):
    """(survives, clone, split) as the plan decodes a flag byte: an original survives iff kept and not split."""
    f = np.asarray(flags, np.uint8)
    clone, split = (f & 1).astype(bool), ((f >> 1) & 1).astype(bool)
    return ((f >> 2) & 1).astype(bool) & ~split, clone, split


def expected_map(flags: np.ndarray):
    """counts (K, C, M, K + C + 2 M) and the destination -> source row map [kept | clones | children 1 | children 2],
    every group in ascending source row."""
    keep, clone, split = flag_masks(flags)
    k, c, m = (np.nonzero(x)[0] for x in (keep, clone, split))
    return (k.size, c.size, m.size, k.size + c.size + 2 * m.size), np.concatenate([k, c, m, m]).astype(np.int64)


def flag_counts_per_pass(flags: np.ndarray) -> np.ndarray:
    """[passes, 3]: the K, C and M totals of every scan pass."""
    n = flags.shape[0]
    return np.stack([count_per_pass(x, n) for x in flag_masks(flags)], axis=1)


# ---- 2. densification inputs whose every row keeps a margin from every threshold --------------------------------------
EXTENT = 8.0
DENSIFY_STEP = 3100                            # > opacity_reset_every: size pruning is on
DENSIFY_VIEWS = 7
DENSIFY_CFG = dict(densify_from=500, densify_every=100, grad_threshold=0.0002, opacity_threshold=0.05, percent_dense=0.01)
ULP_MARGIN = 64                                # exp / sigmoid of the device may differ from torch's by a few ulp
GRAD_MARGIN = 1e-5                             # relative; ten times the rtol = 1e-6 allowed on grad_accum
LOW_BAND, HIGH_BAND = (2e-5, 1.5e-4), (3e-4, 1e-3)       # |g| of a Gaussian in all of its views: one side of 2e-4
SIZE_THRESHOLD = f32(f32(DENSIFY_CFG["percent_dense"]) * f32(EXTENT))      # densification.cpp:367
WS_THRESHOLD = f32(f32(0.1) * f32(EXTENT))                                  # :436
OPACITY_THRESHOLD = f32(DENSIFY_CFG["opacity_threshold"])
GRAD_THRESHOLD = f32(DENSIFY_CFG["grad_threshold"])
LOG_SPLIT = f32(0.47000366)                    # the kernel's constant for std::log(1.6f)


def ulp_distance(values, threshold) -> np.ndarray:
    """|ordinal(v) - ordinal(threshold)| of positive float32 values."""
    v = np.ascontiguousarray(values, f32).view(np.int32).astype(np.int64)
    return np.abs(v - np.int64(f32(threshold).view(np.int32)))


def _nudge(t: torch.Tensor, activation, thresholds) -> torch.Tensor:
    """Moves by 1e-3 (thousands of ulp of the activation) every element whose activation, as torch computes it, lies
    within twice the margin of a threshold."""
    for _ in range(4):
        act = activation(t).numpy()
        near = np.zeros(act.shape, bool)
        for thr in thresholds:
            near |= ulp_distance(act, thr) < 2 * ULP_MARGIN
        if not near.any():
            return t
        t = t + torch.from_numpy(near).to(torch.float32) * 1e-3
    raise AssertionError("threshold margins not reached")


def densify_inputs(n: int, coeffs: int = 4) -> SimpleNamespace:
    """The model of tests/test_gpu_densify.py::_models with margin-safe scales and opacities, DENSIFY_VIEWS views of
    (dL_dmeans_2d, radii) with every Gaussian's gradient norms in one band, and the split noise.  Read-only."""
    g = torch.Generator().manual_seed(1000 + n + coeffs)
    rot = torch.randn((n, 4), generator=g)
    t = dict(positions=torch.randn((n, 3), generator=g) * 2.0, sh_coeffs=torch.randn((n, 3, coeffs), generator=g) * 0.1,
             opacities=_nudge(torch.randn((n, 1), generator=g) * 3.0, torch.sigmoid, (OPACITY_THRESHOLD,)),
             rotations=rot / rot.norm(2, 1, True).clamp_min(1e-8),
             scales=_nudge(torch.randn((n, 3), generator=g) * 1.5 - 2.5, torch.exp, (SIZE_THRESHOLD, WS_THRESHOLD)))
    high = torch.rand(n, generator=g) < 0.4
    if n % PASS == 1:
        # a last pass of one row can hold one decision only: make the row a split parent (a pruned original too), so
        # that the split channel and the two children rows it places lie behind the carry
        high[n - 1] = True
        t["scales"][n - 1] = torch.tensor([-1.0, -1.5, -2.0])
    lo = torch.where(high, HIGH_BAND[0], LOW_BAND[0])
    hi = torch.where(high, HIGH_BAND[1], LOW_BAND[1])
    views = []
    for _ in range(DENSIFY_VIEWS):
        # 0.02 .. 0.98 of the band: the float32 norm of the pair stays inside it
        mag = lo + (hi - lo) * (0.02 + 0.96 * torch.rand(n, generator=g))
        phi = torch.rand(n, generator=g) * (2.0 * np.pi)
        grads = torch.stack([mag * torch.cos(phi), mag * torch.sin(phi)], 1).contiguous()
        radii = torch.randint(-1, 24, (n,), generator=g, dtype=torch.int32)
        radii[torch.rand(n, generator=g) < 0.3] = 0
        views.append((grads, radii))
    noise = torch.randn((2, n, 3), generator=torch.Generator().manual_seed(9))
    return SimpleNamespace(n=n, coeffs=coeffs, tensors=t, views=views, noise=noise)


_references = {}


def densify_reference(do, n: int, coeffs: int = 4) -> SimpleNamespace:
    """The oracle (oracle/densify_oracle.py, module `do`) run once on densify_inputs(n, coeffs): its accumulators,
    masks, stats and final model.  Shared and read-only; release() drops them."""
    key = (n, coeffs)
    if key in _references:
        return _references[key]
    inp = densify_inputs(n, coeffs)
    ctrl = do.DensificationController(do.DensificationConfig(**DENSIFY_CFG), EXTENT)
    model = do.Model(*(inp.tensors[k].clone() for k in NAMES))
    for grads, radii in inp.views:
        ctrl.accumulate_gradients(grads, radii)
    acc = SimpleNamespace(grad_accum=ctrl.grad_accum_.numpy().copy(), grad_count=ctrl.grad_count_.numpy().copy(),
                          max_radii=ctrl.max_radii_2d_.numpy().copy())
    clone = ctrl.compute_clone_mask(model).numpy().copy()
    split = ctrl.compute_split_mask(model).numpy().copy()
    keep = ctrl.compute_keep_mask(model, DENSIFY_STEP).numpy().copy()
    stats = ctrl.densify(model, DENSIFY_STEP, inp.noise)
    ref = SimpleNamespace(inputs=inp, acc=acc, clone=clone, split=split, survive=keep & ~split, stats=stats, model=model)
    _references[key] = ref
    return ref


def split_children(orc, inp: SimpleNamespace, split: np.ndarray):
    """The children of the rows in `split`, first then second, as the device computes them (k_gather_rows, compiled
    without contraction): float32 `scales - LOG_SPLIT`, the project's own expf of it (orc.expf is cugs_expf on the
    host), one rounded product and one rounded sum.  Returns (positions [2 M, 3], scales [2 M, 3])."""
    parents = np.nonzero(split)[0]
    pos, scl = inp.tensors["positions"].numpy()[parents], inp.tensors["scales"].numpy()[parents]
    child_scl = (scl - LOG_SPLIT).astype(f32)
    actual = orc.expf(child_scl).astype(f32)
    kids = [(pos + (inp.noise.numpy()[w][parents] * actual).astype(f32)).astype(f32) for w in (0, 1)]
    return np.concatenate(kids, 0), np.concatenate([child_scl, child_scl], 0)


# ---- 3. prune masks -------------------------------------------------------------------------------------------------
PRUNE_MASKS = ("random", "second_pass")


def prune_mask(kind: str, n: int) -> np.ndarray:
    if kind == "random":
        return np.random.default_rng(n + 7).uniform(size=n) < 0.4
    if kind == "second_pass":                                   # exactly rows PASS .. 2 PASS - 1
        return pass_of(np.arange(n)) == 1
    raise ValueError(kind)


# ---- 4. MCMC relocation ------------------------------------------------------------------------------------------------
MCMC_EXTENT, MCMC_STEP, MCMC_CAP, MCMC_SEED = 4.0, 1700, 0.05, 0xDEADBEEF12345
# (size, opacity pattern): "dead_tail" needs rows past 2 PASS, "dead_head" and "sparse_dead" a pass after the first
MCMC_CASES = tuple((n, p) for n in SIZES for p in ("mixture", "dead_tail", "dead_head", "one_alive", "sparse_dead")
                   if not (p == "dead_tail" and n <= 2 * PASS) and not (p in ("dead_head", "sparse_dead") and n <= PASS))


def mcmc_opacities(pattern: str, n: int) -> np.ndarray:
    """[n, 1] float32.  A row is dead below logit(0.005) = -5.29; dead draws lie in [-12, -5.4], alive ones in [-4, 4]."""
    rng = np.random.default_rng(n + 13)
    dead, alive = rng.uniform(-12.0, -5.4, (n, 1)), rng.uniform(-4.0, 4.0, (n, 1))
    rows = np.arange(n)[:, None]
    if pattern == "mixture":                                    # (a) the mixture of test_relocation_exact_against_oracle
        o = np.where(rng.uniform(size=(n, 1)) < 0.3, dead, rng.normal(0.0, 3.0, (n, 1)))
    elif pattern == "dead_tail":                                # (b) dead rows only in the third pass, alive everywhere
        o = np.where((rows >= 2 * PASS) & (rng.uniform(size=(n, 1)) < 0.5), dead, alive)
    elif pattern == "dead_head":                                # (c) the first pass all dead, all later rows alive
        o = np.where(rows < PASS, dead, alive)
    elif pattern == "one_alive":                                # (d) every source must be n - 1
        o = dead.copy()
        o[n - 1] = 2.0
    elif pattern == "sparse_dead":
        # 2 % dead in every pass, row n - 1 among them: fewer dead rows than the cap, so EVERY dead row moves, and
        # those of the second and third pass take their slot of the dead list from a non-zero carry of the dead count
        o = np.where(rng.uniform(size=(n, 1)) < 0.02, dead, alive)
        o[n - 1] = dead[n - 1]
    else:
        raise ValueError(pattern)
    return o.astype(f32)


@functools.lru_cache(maxsize=None)
def _mcmc_rows(coeffs: int):
    n = max(SIZES)
    rng = np.random.default_rng(11)
    t = dict(positions=rng.standard_normal((n, 3), dtype=f32) * f32(3.0),
             sh_coeffs=rng.standard_normal((n, 3, coeffs), dtype=f32),
             rotations=rng.standard_normal((n, 4), dtype=f32),
             scales=rng.standard_normal((n, 3), dtype=f32) - f32(4.0))
    for a in t.values():
        a.setflags(write=False)
    return t


def mcmc_arrays(pattern: str, n: int, coeffs: int = 16) -> dict:
    """The model arrays of one relocation case: read-only views of one shared draw, and the pattern's opacities."""
    t = {k: v[:n] for k, v in _mcmc_rows(coeffs).items()}
    t["opacities"] = mcmc_opacities(pattern, n)
    if pattern == "one_alive":
        # every relocated row lands beside this one source.  Keep its coordinates away from 0: the position check
        # expects 99 % of the rows within an ulp of the result, which holds where that ulp (2.4e-7 from |x| = 2) is
        # not smaller than what the device's float Box-Muller may differ by (4e-6 * extent * 0.01 = 1.6e-7)
        t["positions"] = t["positions"].copy()
        t["positions"][n - 1] = (3.0, -2.5, 5.0)
    return t


def release() -> None:
    """Drops the shared references (some hundred MB at the carry sizes); the two test files call it when done."""
    _references.clear()
    _mcmc_rows.cache_clear()
