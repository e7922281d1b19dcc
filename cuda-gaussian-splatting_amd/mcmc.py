"""Host-side mirror of the reference's MCMC densification (optimizer/mcmc_densification.hpp:27-170) over
csrc/mcmc.hip: MCMCConfig, MCMCStats and MCMCController with the reference's method names and
schedule.  N stays constant: nothing is reallocated and the optimizer is never rebuilt.

Per iteration the reference runs, on libtorch ops, the regulariser (an autograd pass and a host sync) before the
optimizer step and the position noise after it.  Here they are one launch each - or none at all: with
render_backward(..., fused_adam=opt, mcmc=controller, mcmc_step=step) both ride inside the projection backward's
fused Adam step (cugs_projection_opts.mcmc), bit for bit the unfused sequence.

Differences from the reference, all at the boundary:
  * random draws (position noise, relocation jitter, relocation sampling) come from a counter-based Philox4x32-10
    keyed by (config.seed, step), not from torch's generator: reproducible, and identical on data-parallel
    replicas without a broadcast.  inject_noise(noise=...) accepts explicit normals (parity tests);
  * sampling weights are opacities quantised to 2^-24 (exact integer weights, an order-independent draw); the
    relative weight error is at most ~1.2e-5 at the default dead threshold 0.005;
  * the noise scale is the reference's, which does NOT multiply by the position learning rate (:156-158): at the
    default noise_lr_init = 5e5 a Gaussian at scale e^-4.6 with gate ~1 moves by ~5 000 units per step.  Kept as
    the reference has it; use a small noise lr where convergence matters;
  * relocate(..., optimizer=FusedAdam) zeroes the relocated rows' Adam moments (the paper's choice); without it
    the moments are left alone, as the reference does (trainer.cpp:265);
  * the VRAM guard (:35-50) is not mirrored, as in densification.py.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ._lib import McmcFused, check, lib
from .rasterizer import _ptr, _skey, _stream, _torch_check
from .types import GaussianModel

_workspaces: Dict[tuple, torch.Tensor] = {}


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """Grow-only scratch per (device, stream): the relocation's scans and the regulariser's partial sums live here from
    one launch to the next of the same call, so two loops on two streams of one device must not share it."""
    key = _skey(device)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


@dataclass
class MCMCConfig:
    """mcmc_densification.hpp:27-51 (the two VRAM fields are not mirrored) plus the generator's seed."""
    relocate_from: int = 500
    relocate_until: int = 15000
    relocate_every: int = 100
    dead_opacity_threshold: float = 0.005
    relocate_cap: float = 0.05
    noise_lr_init: float = 5e5
    noise_lr_final: float = 1e3
    noise_lr_max_steps: int = 30000
    noise_gate_k: float = 100.0
    noise_gate_t: float = 0.995
    lambda_opacity: float = 0.01
    lambda_scale: float = 0.01
    seed: int = 0


@dataclass
class MCMCStats:
    """mcmc_densification.hpp:54-59"""
    num_relocated: int = 0
    num_dead: int = 0
    num_total: int = 0
    skipped_vram: bool = False


def _check_model(model: GaussianModel, what: str) -> None:
    for name in ("positions", "sh_coeffs", "opacities", "scales", "rotations"):
        t = getattr(model, name)
        _torch_check(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(),
                     f"{what}: model.{name} must be a contiguous float32 CUDA tensor (updated in place)")


class MCMCController:
    def __init__(self, config: MCMCConfig, scene_extent: float):
        self.config_ = config
        self.scene_extent_ = float(scene_extent)

    # ---- schedule (mcmc_densification.cpp:30-34) ----
    def should_relocate(self, step: int) -> bool:
        c = self.config_
        return step >= c.relocate_from and step <= c.relocate_until and step % c.relocate_every == 0

    def noise_lr(self, step: int) -> float:
        """Log-linear decay in float32 (:40-50), as fused_adam.position_lr."""
        f32 = np.float32
        c = self.config_
        if step >= c.noise_lr_max_steps:
            return float(f32(c.noise_lr_final))
        if step <= 0:
            return float(f32(c.noise_lr_init))
        t = f32(step) / f32(c.noise_lr_max_steps)
        log_ratio = np.log(f32(c.noise_lr_final) / f32(c.noise_lr_init), dtype=f32)
        return float(f32(c.noise_lr_init) * np.exp(t * log_ratio, dtype=f32))

    def _seed(self) -> int:
        return int(self.config_.seed) & 0xFFFFFFFFFFFFFFFF

    # ---- relocation (:56-138) ----
    def relocate(self, model: GaussianModel, step: int, optimizer=None,
                 sources_out: Optional[torch.Tensor] = None) -> MCMCStats:
        """Moves the first min(num_dead, cap) dead Gaussians onto opacity-weighted samples of the alive ones, in
        place; N is unchanged.  One 8-byte read-back (the statistics).  `optimizer` (a FusedAdam on `model`):
        zero the relocated rows' moments.  `sources_out` (int32 [N] CUDA, optional): the source row of the j-th
        relocated row, j < num_relocated."""
        n = model.num_gaussians()
        stats = MCMCStats(num_total=n)
        if n == 0:
            return stats
        _check_model(model, "relocate")
        dev = model.positions.device
        c = self.config_
        ws = _workspace(dev, lib.cugs_mcmc_relocate_workspace_bytes(n))
        out = torch.zeros(2, dtype=torch.int32, device=dev)
        m = v = None
        if optimizer is not None:
            _torch_check(optimizer.model_ is model, "relocate: the optimizer must have been built on this model")
            for t in optimizer.m_ + optimizer.v_:
                _torch_check(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32,
                             "relocate: the optimizer moments must be contiguous float32 CUDA tensors")
            m = (C.c_void_p * 5)(*[t.data_ptr() for t in optimizer.m_])
            v = (C.c_void_p * 5)(*[t.data_ptr() for t in optimizer.v_])
        if sources_out is not None:
            _torch_check(sources_out.is_cuda and sources_out.dtype == torch.int32 and sources_out.numel() >= n
                         and sources_out.is_contiguous(), "sources_out must be a contiguous int32 CUDA tensor of N")
        check(lib.cugs_mcmc_relocate(n, int(model.sh_coeffs.shape[2]), _ptr(model.positions), _ptr(model.rotations),
                                     _ptr(model.scales), _ptr(model.opacities), _ptr(model.sh_coeffs),
                                     float(c.dead_opacity_threshold), float(c.relocate_cap), self.scene_extent_,
                                     self._seed(), int(step) & 0xFFFFFFFF, m, v, _ptr(ws), ws.numel(), _ptr(out),
                                     _ptr(sources_out), _stream(dev)), "cugs_mcmc_relocate")
        dead, moved = (int(x) for x in out.cpu())
        stats.num_dead, stats.num_relocated = dead, moved
        return stats

    # ---- noise (:144-161) ----
    def inject_noise(self, model: GaussianModel, step: int, noise: Optional[torch.Tensor] = None) -> None:
        """positions += noise_lr(step) * exp(scales) * gate(opacity) * n, in place; n = `noise` ([N, 3] CUDA
        float32) when given, else the generator's draw for (config.seed, step)."""
        n = model.num_gaussians()
        if n == 0:
            return
        _check_model(model, "inject_noise")
        if noise is not None:
            _torch_check(tuple(noise.shape) == (n, 3) and noise.is_cuda, "noise must be [N, 3] on CUDA")
            noise = noise.contiguous().to(torch.float32)
        c = self.config_
        check(lib.cugs_mcmc_inject_noise(n, _ptr(model.positions), _ptr(model.scales), _ptr(model.opacities),
                                         self.noise_lr(step), float(c.noise_gate_k), float(c.noise_gate_t),
                                         _ptr(noise), self._seed(), int(step) & 0xFFFFFFFF,
                                         _stream(model.positions.device)), "cugs_mcmc_inject_noise")

    # ---- regulariser (:167-186) ----
    def compute_regularization(self, model: GaussianModel) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(value, reg_dL_dopacities [N,1], reg_dL_dscales [N,3]); value = lambda_o mean(sigmoid(opa)) +
        lambda_s mean(exp(scales)) as a 0-dim CUDA tensor (no host sync; float(value) reads it back)."""
        n = model.num_gaussians()
        dev = model.positions.device
        f = dict(dtype=torch.float32, device=dev)
        value = torch.zeros((), **f)
        g_o, g_s = torch.empty((n, 1), **f), torch.empty((n, 3), **f)
        if n == 0:
            return value, g_o, g_s
        opa, scl = model.opacities.contiguous().to(torch.float32), model.scales.contiguous().to(torch.float32)
        c = self.config_
        ws = _workspace(dev, lib.cugs_mcmc_relocate_workspace_bytes(0))     # 16 KB of partial sums, whatever N
        check(lib.cugs_mcmc_regularization(n, _ptr(opa), _ptr(scl), float(c.lambda_opacity), float(c.lambda_scale),
                                           None, None, _ptr(g_o), _ptr(g_s), _ptr(value), _ptr(ws), ws.numel(),
                                           _stream(dev)), "cugs_mcmc_regularization")
        return value, g_o, g_s

    # ---- the fused route (render_backward(..., fused_adam=, mcmc=)) ----
    def fused_args(self, step: int, noise: Optional[torch.Tensor] = None) -> McmcFused:
        c = self.config_
        a = McmcFused()
        a.lambda_opacity, a.lambda_scale = float(c.lambda_opacity), float(c.lambda_scale)
        a.noise_lr, a.gate_k, a.gate_t = self.noise_lr(step), float(c.noise_gate_k), float(c.noise_gate_t)
        a.step, a.seed = int(step) & 0xFFFFFFFF, self._seed()
        a.noise = noise.data_ptr() if noise is not None else None
        return a


def random_bits(seed: int, stream_id: int, step: int, first_index: int, count: int,
                device=None) -> torch.Tensor:
    """The generator's raw words: uint32 [count, 4] (as int32) for indices first_index .. first_index + count - 1."""
    dev = torch.device(device) if device is not None else torch.device("cuda")
    out = torch.empty((count, 4), dtype=torch.int32, device=dev)
    if count > 0:
        check(lib.cugs_mcmc_random_bits(int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF,
                                        int(step) & 0xFFFFFFFF, int(first_index) & 0xFFFFFFFFFFFFFFFF, count,
                                        _ptr(out), _stream(dev)), "cugs_mcmc_random_bits")
    return out
