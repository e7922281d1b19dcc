"""k-means codebooks through the C++ host (adapter/vq_driver.cpp: cugs_hip::vq_fit and vq_assign) against the Python
host on the same files: indices, codebook and counts bit for bit, with and without weights."""
import numpy as np
import pytest
import torch

from cpp_driver import NO_LEGACY_IPC, read_f32, run_driver, write_f32
from util import np_

pytestmark = pytest.mark.gpu


def test_cpp_vq_driver_matches_python_host(pkg, dev, tmp_path):
    n, d, k, iters = 1000, 24, 257, 4
    rng = np.random.Generator(np.random.Philox(key=2900))
    x = rng.standard_normal((n, d)).astype(np.float32)
    w = rng.uniform(0.0, 3.0, n).astype(np.float32)
    w[::9] = 0.0
    write_f32(tmp_path, x=x, weights=w)
    run_driver("vq_driver", tmp_path, n, d, k, iters, env=NO_LEGACY_IPC)
    xt, wt = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    for prefix, weights in (("fit_", None), ("wfit_", wt)):
        cb, idx, counts = pkg.vq_fit(xt, k, iters=iters, weights=weights)
        assert np.array_equal(read_f32(tmp_path, prefix + "codebook").view(np.uint32), np_(cb).reshape(-1).view(np.uint32))
        assert np.array_equal(read_f32(tmp_path, prefix + "indices"), np_(idx).astype(np.float32))
        assert np.array_equal(read_f32(tmp_path, prefix + "counts"), np_(counts).astype(np.float32))
    cb, idx, _ = pkg.vq_fit(xt, k, iters=iters)
    again, dist = pkg.vq_assign(xt, cb, return_dist=True)
    assert torch.equal(again, idx)
    assert np.array_equal(read_f32(tmp_path, "assign_indices"), np_(again).astype(np.float32))
    assert np.array_equal(read_f32(tmp_path, "assign_dist").view(np.uint32), np_(dist).view(np.uint32))
