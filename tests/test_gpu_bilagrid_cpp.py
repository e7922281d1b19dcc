"""The bilateral-grid slice, backward and TV regulariser through the C++ host (cuda-gaussian-splatting_amd/adapter:
cugs_hip::bilagrid_slice / bilagrid_slice_backward / bilagrid_tv) run as a native program (adapter/bilagrid_driver.bin)
on the same raw inputs as the Python host: the same bytes in every output."""
import numpy as np
import pytest
import torch

import bilagrid_ref as br
from cpp_driver import run_driver
from util import np_

pytestmark = pytest.mark.gpu
TV_WEIGHT = 2.5


def test_cpp_bilagrid_matches_python_host(pkg, dev, tmp_path):
    cases = [br.CASES[0], br.CASES[2], br.CASES[5]]           # 7x5 / (4,3,2), 37x53 / (16,16,8), 24x40 / (5,3,4) with the clamp
    manifest = [f"cases {len(cases)}"]
    for i, c in enumerate(cases):
        h, w, (gx, gy, l), _ = c
        for name, a in zip(("grid", "c", "g"), br.case(*c)):
            a.tofile(tmp_path / f"case_{i}_{name}.f32")
        manifest.append(f"{h} {w} {l} {gy} {gx} {TV_WEIGHT}")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")

    res = run_driver("bilagrid_driver", tmp_path)
    assert f"bilagrid_driver ok cases={len(cases)} bad_grid_throws=1" in res.stdout

    for i, c in enumerate(cases):
        grid, img, g = (torch.from_numpy(np.array(a)).to(dev) for a in br.case(*c))
        x = pkg.bilagrid_slice(grid, img)
        back = pkg.bilagrid_slice_backward(grid, img, g)
        tv, with_tv = pkg.bilagrid_tv(grid, weight=TV_WEIGHT, dL_dgrid=back.dL_dgrid.clone())
        want = {"x": x, "dc": back.dL_drendered, "dg": back.dL_dgrid, "tv": tv.reshape(1), "dgtv": with_tv}
        for k, t in want.items():
            got = np.fromfile(tmp_path / f"out_{i}_{k}.f32", np.float32)
            assert got.tobytes() == np_(t).tobytes(), (i, k)
