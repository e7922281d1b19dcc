"""reduce10r16 (cugs_raster_common.h): reduce9r16 with a tenth value in stage 1's free half, used by the depth-map
backward to deliver dL/dz to word 9 of the accumulator row.  Exercised alone through the DEVELOPMENT build's test hook
(libcugs_hip_dev.so: cugsdbg_reduce10r16, not part of the public C ABI) with exact integer-valued data."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev_lib(pkg):
    path = os.path.join(os.path.dirname(pkg.LIB_PATH), "libcugs_hip_dev.so")
    if not os.path.exists(path):
        pytest.skip("development library not built (make -C cuda-gaussian-splatting_amd/csrc)")
    return C.CDLL(path)


def test_reduce10r16_rows_are_independent(pkg, dev):
    """Every 16-lane row delivers its own ten totals, each slot from exactly one lane; nothing leaks between rows or
    between v7 and v9 (which share one register in stage 1)."""
    lib = _dev_lib(pkg)
    rng = np.random.default_rng(10)
    for trial in range(6):
        vals = rng.integers(-500, 500, size=(10, 64)).astype(np.float32)     # exact in fp32
        if trial == 0:
            vals = np.array([[1000.0 * (k + 1) + l for l in range(64)] for k in range(10)], np.float32)
        if trial == 1:
            vals[:, 16:32] = 0.0                                              # an empty row stays exactly zero
        if trial == 2:                                                        # one hot lane per slot and row
            vals = np.zeros((10, 64), np.float32)
            for k in range(10):
                for row in range(4):
                    vals[k, row * 16 + (5 * k + 3 * row + 1) % 16] = float(100 * row + k + 1)
        if trial == 3:
            vals[7] = 0.0                                                     # v9 alone in the shared register
        if trial == 4:
            vals[9] = 0.0                                                     # v7 alone
        inp = torch.from_numpy(vals).to(dev)
        out = torch.zeros(64, device=dev)
        slots = torch.zeros(64, dtype=torch.int32, device=dev)
        assert lib.cugsdbg_reduce10r16(C.c_void_p(inp.data_ptr()), C.c_void_p(out.data_ptr()),
                                       C.c_void_p(slots.data_ptr()), C.c_void_p(0)) == 0
        torch.cuda.synchronize()
        o, s = out.cpu().numpy(), slots.cpu().numpy()
        for row in range(4):
            sl = s[row * 16:(row + 1) * 16]
            assert sorted(sl[sl >= 0].tolist()) == list(range(10))
            want = vals[:, row * 16:(row + 1) * 16].sum(1)
            for r in range(16):
                if sl[r] >= 0:
                    assert o[row * 16 + r] == want[sl[r]], (trial, row, r, sl[r])
