"""The tests' half of the C++-host test programs (cuda-gaussian-splatting_amd/adapter/*_driver.cpp): running one, and
the raw files they exchange.  The C++ half is adapter/driver_io.hpp; tests/test_driver_io.py holds the two together."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

ADAPTER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-gaussian-splatting_amd", "adapter")
NO_LEGACY_IPC = {"HSA_ENABLE_IPC_MODE_LEGACY": "0"}


def run_driver(name, *args, env=None, timeout=300):
    """Run adapter/<name>.bin on the arguments and return the CompletedProcess of a run that exited 0; `env` holds
    variables set over the caller's environment for this call only.  Skips when the program was not built."""
    exe = os.path.join(ADAPTER, f"{name}.bin")
    if not os.path.exists(exe):
        pytest.skip(f"{name}.bin not built (make -C cuda-gaussian-splatting_amd/adapter)")
    res = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout,
                         env=None if env is None else dict(os.environ, **env))
    assert res.returncode == 0, f"rc={res.returncode} stdout={res.stdout!r} stderr={res.stderr!r}"
    return res


def camera_words(cam):
    """The 25 float32 words read_camera (driver_io.hpp) reads: view[16], fx fy cx cy, width height, cam_center[3]."""
    abi = cam.to_abi() if hasattr(cam, "to_abi") else cam
    return np.array(list(abi.view) + [abi.fx, abi.fy, abi.cx, abi.cy, abi.width, abi.height] + list(abi.cam_center),
                    np.float32)


def write_camera(path, cam):
    camera_words(cam).tofile(path)


def write_f32(directory, **arrays):
    """<directory>/<name>.f32 for every array, as contiguous float32."""
    for name, a in arrays.items():
        np.ascontiguousarray(a, np.float32).tofile(directory / f"{name}.f32")


def read_f32(directory, name):
    return np.fromfile(directory / f"{name}.f32", dtype=np.float32)
