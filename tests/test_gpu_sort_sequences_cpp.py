"""The C++ host's own copy of the per-stream sort state (SortState in adapter/cugs_hip_torch.cpp: estimate decaying by
1/32, held capacity, wide-depth counter, keyed workspace) on one scripted run - sparse, dense (a capacity miss), sparse
on the held capacity, wide (the -1 miss), wide again, an in-range view inside the hold - through
adapter/sortseq_driver.cpp.  Every frame's image and index list must be the Python host's, bit for bit, which
tests/test_gpu_sort_sequences.py ties to the oracle (and which is checked against it here once more)."""
import numpy as np
import pytest

from test_gpu_sort_sequences import DEG, _Spy, _Stream, scene
from cpp_driver import NO_LEGACY_IPC, run_driver, write_camera
from util import np_

pytestmark = pytest.mark.gpu
SCRIPT = ("S", "D", "S", "W", "W", "S")


def test_cpp_host_recovers_over_the_same_sequence(pkg, dev, tmp_path, monkeypatch):
    for name in set(SCRIPT):
        sc = scene(name)
        a = sc["arrays"]
        for stem, v in (("positions", a["positions"]), ("sh", a["sh_coeffs"]), ("opacities", a["opacities"]),
                        ("rotations", a["rotations"]), ("scales", a["scales"])):
            np.ascontiguousarray(v, np.float32).tofile(tmp_path / f"{name}.{stem}.f32")
        write_camera(tmp_path / f"{name}.camera.f32", sc["cam"])
    coeffs = (DEG + 1) ** 2
    res = run_driver("sortseq_driver", tmp_path, coeffs, *SCRIPT, env=NO_LEGACY_IPC)
    assert "sortseq_driver ok" in res.stdout

    # the same script through the Python host (checked there against the oracle and the model, frame by frame)
    R = pkg.rasterizer
    spy = _Spy(R.lib, dev)
    monkeypatch.setattr(R, "lib", spy)
    st = _Stream(pkg, dev, spy)
    try:
        for i, name in enumerate(SCRIPT):
            out = st.frame(name, "block" if i % 2 == 0 else "eval")
            sc = scene(name)
            rd = lambda what, dt: np.fromfile(tmp_path / f"frame{i}.{what}", dtype=dt)
            assert f"frame {i} {name} pairs={out.total_pairs}" in res.stdout, (i, name, res.stdout)
            assert np.array_equal(rd("indices.i32", np.int32), np_(out.gaussian_indices)), (i, name)
            assert np.array_equal(rd("ranges.i32", np.int32).reshape(-1, 2), np_(out.tile_ranges)), (i, name)
            assert np.array_equal(rd("color.f32", np.uint32).reshape(sc["h"], sc["w"], 3),
                                  np_(out.color).view(np.uint32)), (i, name)
        assert [f.valid for f in st.model.history] == [True, False, True, False, True, True]
    finally:
        st.restore()
