"""The two halves of the C++-host tests' file exchange held to each other, without a GPU: tests/cpp_driver.py writes what
adapter/driver_io.hpp reads and the other way round.  adapter/driver_io_check.cpp is built on its own against libtorch
(host tensors only, not linked to the library) and run on small files."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cpp_driver import ADAPTER, camera_words, write_camera


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    import torch
    t = os.path.dirname(torch.__file__)
    if not os.path.exists(os.path.join(t, "include", "torch", "csrc", "api", "include", "torch", "torch.h")):
        pytest.skip("needs the libtorch headers")
    exe = tmp_path_factory.mktemp("driver_io") / "driver_io_check"
    subprocess.run(["g++", "-std=c++17", "-O0", "-w", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
                    f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}", "-I" + os.path.join(t, "include"),
                    "-I" + os.path.join(t, "include", "torch", "csrc", "api", "include"), "-I/opt/rocm/include",
                    "-o", str(exe), os.path.join(ADAPTER, "driver_io_check.cpp"), "-L" + os.path.join(t, "lib"),
                    "-Wl,-rpath," + os.path.join(t, "lib"), "-ltorch", "-ltorch_cpu", "-lc10"], check=True)
    return lambda *args: subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=60)


class _Abi:
    """Every one of the 25 words distinct, width and height as integers."""
    view = [0.5 + i for i in range(16)]
    fx, fy, cx, cy = 611.25, 609.75, 319.5, 239.5
    width, height = 641, 479
    cam_center = [-1.25, 2.5, 1e-3]


def test_camera_written_by_python_is_the_camera_cpp_reads(check, tmp_path):
    write_camera(tmp_path / "camera.f32", _Abi)
    assert (tmp_path / "camera.f32").stat().st_size == 25 * 4
    res = check("camera", tmp_path / "camera.f32")
    assert res.returncode == 0, res.stderr
    got = res.stdout.split()
    want = np.array(_Abi.view + [_Abi.fx, _Abi.fy, _Abi.cx, _Abi.cy] + _Abi.cam_center, np.float32)
    assert got[20:22] == [str(_Abi.width), str(_Abi.height)]
    assert np.array_equal(np.array(got[:20] + got[22:], np.float64).astype(np.float32), want)   # %.9g round-trips float32
    assert np.array_equal(camera_words(_Abi)[20:22], [_Abi.width, _Abi.height])


@pytest.mark.parametrize("tag,dtype", [("f32", np.float32), ("i32", np.int32), ("u8", np.uint8)])
def test_arrays_come_back_with_the_same_bytes(check, tmp_path, tag, dtype):
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(37) * 1e3).astype(dtype) if dtype != np.uint8 else rng.integers(0, 256, 37).astype(dtype)
    a.tofile(tmp_path / "in.bin")
    res = check("copy", tmp_path / "in.bin", tmp_path / "out.bin", tag, a.size)
    assert res.returncode == 0, res.stderr
    assert (tmp_path / "out.bin").read_bytes() == a.tobytes()


def test_write_as_f32_converts_like_numpy(check, tmp_path):
    a = np.array([0, 1, -1, 7, 16777217, -2147483648, 2147483647, 123456789], np.int32)   # some not exact in float32
    a.tofile(tmp_path / "in.bin")
    res = check("as_f32", tmp_path / "in.bin", tmp_path / "out.bin", a.size)
    assert res.returncode == 0, res.stderr
    assert (tmp_path / "out.bin").read_bytes() == a.astype(np.float32).tobytes()


def test_missing_and_short_files_exit_2(check, tmp_path):
    res = check("copy", tmp_path / "absent.bin", tmp_path / "out.bin", "f32", 4)
    assert res.returncode == 2 and "cannot read" in res.stderr, (res.returncode, res.stderr)
    np.zeros(3, np.float32).tofile(tmp_path / "short.bin")
    res = check("copy", tmp_path / "short.bin", tmp_path / "out.bin", "f32", 4)
    assert res.returncode == 2 and "expected" in res.stderr, (res.returncode, res.stderr)
    np.zeros(24, np.float32).tofile(tmp_path / "short_camera.f32")
    res = check("camera", tmp_path / "short_camera.f32")
    assert res.returncode == 2 and "expected" in res.stderr, (res.returncode, res.stderr)
