"""The normal-supervision loss through the C++ host (cuda-gaussian-splatting_amd/adapter: cugs_hip::normal_loss and
depth_to_normals) run as a native program (adapter/normal_loss_driver.bin) on the same raw inputs as the Python host,
with a weight map and both distances: the same bytes in every output."""
import numpy as np
import pytest
import torch

import normal_loss_ref as nr
from cpp_driver import run_driver
from util import np_

pytestmark = pytest.mark.gpu


def test_cpp_normal_loss_matches_python_host(pkg, dev, tmp_path):
    from cugs_amd.types import CameraInfo, CameraIntrinsics
    cases = [(5, 7), (37, 53), (19, 70)]
    manifest = [f"cases {len(cases)}"]
    for i, (h, w) in enumerate(cases):
        c = nr.case(h, w)
        for name, key in (("d", "D"), ("a", "A"), ("t", "t"), ("w", "w")):
            c[key].tofile(tmp_path / f"case_{i}_{name}.f32")
        # the float32 values, written so that they read back exactly
        manifest.append(f"{h} {w} " + " ".join(repr(float(np.float32(c[k]))) for k in ("fx", "fy", "cx", "cy")))
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")

    res = run_driver("normal_loss_driver", tmp_path)
    assert f"normal_loss_driver ok cases={len(cases)} bad_args_throw=1" in res.stdout

    for i, (h, w) in enumerate(cases):
        c = nr.case(h, w)
        cam = CameraInfo(width=w, height=h, intrinsics=CameraIntrinsics(fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"]))
        D, A, t, wt = (torch.from_numpy(c[k]).to(dev) for k in ("D", "A", "t", "w"))
        want = pkg.normal_loss(D, A, cam, t, weight=wt, cos_weight=0.7, l1_weight=0.3, want_normals=True)
        got = {k: np.fromfile(tmp_path / f"out_{i}_{k}.f32", np.float32) for k in ("out", "gd", "ga", "n", "dn")}
        scalars = np.concatenate([np_(want.loss).ravel(), np_(want.valid_weight).ravel(),
                                  np_(want.valid_count).ravel()]).astype(np.float32)
        assert got["out"].tobytes() == scalars.tobytes(), (i, got["out"], scalars)
        assert (scalars[2] > 0) == ((h, w) not in nr.EMPTY)
        assert got["gd"].tobytes() == np_(want.dL_ddepth_map).tobytes(), i
        assert got["ga"].tobytes() == np_(want.dL_dalpha).tobytes(), i
        assert got["n"].tobytes() == np_(want.normals).tobytes(), i
        assert got["dn"].tobytes() == np_(pkg.depth_to_normals(D, A, cam)).tobytes(), i
