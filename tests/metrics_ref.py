"""CPU reference for the evaluation metrics (csrc/metrics.hip, cugs_amd.metrics), in two parts:

  exact(r, t)          float32 differences, summed in float64 with numpy: what the kernel's fixed-order fp64 sums equal
                       up to ~2^-53 n relative, far below half a float32 ulp - so after the final rounding to float32
                       the MSE and the L1 mean differ from the kernel's by at most one ulp, and the maximum not at all;
                       mean SSIM through oracle/loss_oracle.py's ssim (the reference's libtorch op sequence).
  reference_ops(r, t)  the reference's literal op sequence on CPU (training/metrics.cpp:27-46):
                       (r - t).pow(2).mean().item<float>() -> PSNR in float32; ssim(r, t).mean().item<float>().

Shared by tests/test_metrics_ref.py (CPU) and the GPU tests; image pairs are built as tests/test_gpu_loss.py::_pair."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w): smaller than the window | exactly one tile | ragged edge tiles | several full tiles | 510 tiles: more than one
# workgroup of partials, so the strided fixed-order sum and the tree both run
SHAPES = [(7, 5), (16, 16), (37, 53), (64, 64), (270, 480)]

_lo = None


def loss_oracle():
    """oracle/loss_oracle.py, loaded as tests/test_gpu_loss.py loads it."""
    global _lo
    if _lo is None:
        spec = importlib.util.spec_from_file_location("cugs_loss_oracle", os.path.join(ROOT, "oracle", "loss_oracle.py"))
        _lo = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_lo)
    return _lo


def pair(h, w, seed, noise=0.2):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand((h, w, 3), generator=g)
    r = (t + noise * torch.randn((h, w, 3), generator=g)).clamp(0, 1.5)
    return r, t


def quantise(t):
    """A float image -> the uint8 a view cache would hold."""
    return (t.clamp(0, 1) * 255.0).round().to(torch.uint8)


def psnr_of(mse):
    """metrics.cpp:27-34 in float32."""
    mse = np.float32(mse)
    if mse < np.float32(1e-10):
        return np.float32(100.0)
    return np.float32(10.0) * np.log10(np.float32(1.0) / mse)


def exact(r, t, window_size=11):
    """dict(mse, l1, max_abs as float32; mse64 the unrounded float64 mean; ssim the oracle's mean SSIM (float))."""
    rn, tn = np.asarray(r, np.float32), np.asarray(t, np.float32)
    d = (rn - tn).astype(np.float32)                       # float32 difference, as the kernel forms it
    d64 = d.astype(np.float64)
    n = d.size
    mse64 = float((d64 * d64).sum() / n)
    s = loss_oracle().ssim(torch.from_numpy(rn), torch.from_numpy(tn), window_size)
    return dict(mse=np.float32(mse64), mse64=mse64, l1=np.float32(np.abs(d64).sum() / n), max_abs=np.float32(np.abs(d).max()),
                ssim=float(s.double().mean()), psnr=psnr_of(np.float32(mse64)))


def reference_ops(r, t):
    """The reference's compute_psnr / compute_ssim, op for op, on CPU tensors."""
    r, t = torch.as_tensor(r, dtype=torch.float32), torch.as_tensor(t, dtype=torch.float32)
    mse = np.float32((r - t).pow(2).mean().item())
    return dict(mse=mse, psnr=psnr_of(mse), ssim=np.float32(loss_oracle().ssim(r, t).mean().item()))


_cache = {}


def case(h, w):
    """(r, t, exact, reference_ops) of a shape, computed once and shared; callers must not modify the tensors."""
    key = (h, w)
    if key not in _cache:
        r, t = pair(h, w, h * 1000 + w)
        _cache[key] = (r, t, exact(r, t), reference_ops(r, t))
    return _cache[key]


def ulp_distance(a, b):
    """Steps between two finite float32 values of the same sign."""
    ia, ib = np.float32(a).view(np.int32), np.float32(b).view(np.int32)
    return abs(int(ia) - int(ib))
