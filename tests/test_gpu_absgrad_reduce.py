"""reduce12ar16 (cugs_raster_common.h): reduce10r16 with an eleventh and twelfth value folded into the register that
carries v7 | v9, used by the AbsGrad backward to deliver its two sums to words 10 and 11 of the accumulator row.
Exercised alone through the DEVELOPMENT build's test hook (libcugs_hip_dev.so: cugsdbg_reduce12ar16, not part of the
public C ABI): one wave, exact small integers, so that any lane mix-up shows as a wrong integer."""
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


def test_reduce12ar16_rows_are_independent(pkg, dev):
    """Every 16-lane row delivers its own twelve totals, each slot from exactly one lane; nothing leaks between rows or
    between v7, v9, v10 and v11 (which share one register from stage 2 on).  Without the depth slot the same lanes
    deliver all but slot 9."""
    lib = _dev_lib(pkg)
    rng = np.random.default_rng(12)
    for trial in range(8):
        vals = rng.integers(-500, 500, size=(12, 64)).astype(np.float32)     # exact in fp32
        if trial == 0:
            vals = np.array([[1000.0 * (k + 1) + l for l in range(64)] for k in range(12)], np.float32)
        if trial == 1:
            vals[:, 16:32] = 0.0                                              # an empty row stays exactly zero
        if trial == 2:                                                        # one hot lane per slot and row
            vals = np.zeros((12, 64), np.float32)
            for k in range(12):
                for row in range(4):
                    vals[k, row * 16 + (5 * k + 3 * row + 1) % 16] = float(100 * row + k + 1)
        if trial in (3, 4, 5, 6):                                             # each of the four sharers alone
            keep = (7, 9, 10, 11)[trial - 3]
            for k in (7, 9, 10, 11):
                if k != keep:
                    vals[k] = 0.0
        inp = torch.from_numpy(vals).to(dev)
        out = torch.zeros(64, device=dev)
        slots = torch.zeros(64, dtype=torch.int32, device=dev)
        slots_nd = torch.zeros(64, dtype=torch.int32, device=dev)
        assert lib.cugsdbg_reduce12ar16(C.c_void_p(inp.data_ptr()), C.c_void_p(out.data_ptr()),
                                        C.c_void_p(slots.data_ptr()), C.c_void_p(slots_nd.data_ptr()),
                                        C.c_void_p(0)) == 0
        torch.cuda.synchronize()
        o, s, snd = out.cpu().numpy(), slots.cpu().numpy(), slots_nd.cpu().numpy()
        for row in range(4):
            sl, nd = s[row * 16:(row + 1) * 16], snd[row * 16:(row + 1) * 16]
            assert sorted(sl[sl >= 0].tolist()) == list(range(12))
            assert sorted(nd[nd >= 0].tolist()) == [k for k in range(12) if k != 9]
            assert np.array_equal(nd[sl != 9], sl[sl != 9])
            want = vals[:, row * 16:(row + 1) * 16].sum(1)
            for r in range(16):
                if sl[r] >= 0:
                    assert o[row * 16 + r] == want[sl[r]], (trial, row, r, sl[r])
