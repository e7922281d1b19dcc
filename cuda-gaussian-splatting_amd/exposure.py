"""Per-view exposure compensation (not in the reference): one learnable 3x4 affine colour transform
[A | b] per training view, applied to the rendered image inside the fused loss (loss.combined_loss_exposure) and
optimised alongside the model with the project's fused Adam kernel."""
from __future__ import annotations

import ctypes as C
import json
from typing import Dict, Sequence

import torch

from ._lib import AdamGroup, check, lib
from .fused_adam import PositionLRConfig, position_lr


class ExposureModel:
    """`params` [V,3,4], every row [I | 0] at the start, with Adam moments of the same shape.

    Sparse by design: step(view, ...) updates the row of the ONE view that was trained in this iteration, with bias
    corrections from that view's own step count (kept on the host: no sync).  A row that is not trained does not
    move and its moments do not decay - a dense Adam over all V rows would feed the other rows zero gradients, decay
    their moments and keep moving them along stale first moments, so they would drift between their turns.
    The learning rate follows the log-linear schedule of position_lr from lr_init to lr_final over max_steps."""

    beta1, beta2, eps = 0.9, 0.999, 1e-15         # AdamConfig's

    def __init__(self, num_views: int, device, lr_init: float = 0.01, lr_final: float = 0.001, max_steps: int = 30000):
        if num_views < 0:
            raise RuntimeError(f"ExposureModel: num_views must be >= 0, got {num_views}")
        self.device = torch.device(device)
        eye = torch.cat([torch.eye(3, dtype=torch.float32), torch.zeros((3, 1), dtype=torch.float32)], dim=1)
        self.params = eye.unsqueeze(0).repeat(num_views, 1, 1).contiguous().to(self.device)
        self.m_ = torch.zeros_like(self.params)
        self.v_ = torch.zeros_like(self.params)
        self.steps_ = [0] * num_views             # per-view Adam step counts
        self.lr_config = PositionLRConfig(lr_init=lr_init, lr_final=lr_final, max_steps=max_steps)

    @property
    def num_views(self) -> int:
        return int(self.params.shape[0])

    def matrix(self, view: int) -> torch.Tensor:
        """The [3,4] matrix of `view`: a zero-copy view of its row, to hand to combined_loss_exposure."""
        return self.params[self._index(view)]

    def lr(self, step: int) -> float:
        return position_lr(step, self.lr_config)

    def step(self, view: int, dL_dexposure: torch.Tensor, step: int) -> None:
        """One Adam update of the row of `view` from its gradient [3,4], at training iteration `step` (for the
        learning rate): cugs_fused_adam_groups with one group of 12 elements.  Stream-ordered, no host sync."""
        view = self._index(view)
        g = dL_dexposure
        if not (g.is_cuda and g.device == self.params.device and g.dtype == torch.float32 and g.numel() == 12):
            raise RuntimeError("ExposureModel.step: dL_dexposure must be 12 float32 values on the model's device")
        g = g.contiguous()
        self.steps_[view] += 1
        bc1, bc2 = C.c_float(), C.c_float()
        lib.cugs_adam_bias_correction(self.beta1, self.beta2, self.steps_[view], C.byref(bc1), C.byref(bc2))
        group = (AdamGroup * 1)()
        group[0].param, group[0].grad = self.params[view].data_ptr(), g.data_ptr()
        group[0].m, group[0].v = self.m_[view].data_ptr(), self.v_[view].data_ptr()
        group[0].n = 12
        group[0].lr = float(self.lr(step))
        stream = C.c_void_p(torch.cuda.current_stream(self.params.device).cuda_stream)
        check(lib.cugs_fused_adam_groups(group, 1, self.beta1, self.beta2, self.eps, bc1.value, bc2.value, stream),
              "cugs_fused_adam_groups")

    def to_json(self, names: Sequence[str]) -> str:
        """{image_name: [[3 x 4]]} for the views in order (one device-to-host copy).  The moments are not stored."""
        if len(names) != self.num_views or len(set(names)) != len(names):
            raise RuntimeError(f"ExposureModel.to_json: need {self.num_views} distinct names, got {len(names)}")
        rows = self.params.cpu().tolist()
        return json.dumps({str(n): rows[v] for v, n in enumerate(names)})

    @classmethod
    def from_json(cls, text: str, names: Sequence[str], device, **kwargs) -> "ExposureModel":
        """The model of to_json's document for the views `names`, in that order; fresh moments and step counts."""
        doc: Dict[str, list] = json.loads(text)
        model = cls(len(names), device, **kwargs)
        rows = []
        for n in names:
            if n not in doc:
                raise RuntimeError(f"ExposureModel.from_json: no exposure for image {n!r}")
            row = torch.tensor(doc[n], dtype=torch.float32)
            if tuple(row.shape) != (3, 4):
                raise RuntimeError(f"ExposureModel.from_json: {n!r} is not a 3x4 matrix")
            rows.append(row)
        if rows:
            model.params.copy_(torch.stack(rows).to(model.device))
        return model

    def _index(self, view: int) -> int:
        view = int(view)
        if not 0 <= view < self.num_views:
            raise RuntimeError(f"ExposureModel: view {view} out of range [0, {self.num_views})")
        return view
