"""The depth-supervision loss through the C++ host (cuda-gaussian-splatting_amd/adapter: cugs_hip::depth_loss) run as a
native program (adapter/depth_loss_driver.bin) on the same raw inputs as the Python host, with a weight map and a
fitted alignment, in both spaces: the same bytes in every output."""
import numpy as np
import pytest
import torch

import depth_loss_ref as dr
from cpp_driver import run_driver
from util import np_

pytestmark = pytest.mark.gpu


def test_cpp_depth_loss_matches_python_host(pkg, dev, tmp_path):
    cases = [(h, w, inv) for (h, w) in [(7, 5), (37, 53), (64, 64)] for inv in (False, True)]
    manifest = [f"cases {len(cases)}"]
    for i, (h, w, inv) in enumerate(cases):
        c = dr.case(h, w, inv)
        for name, key in (("d", "D"), ("a", "A"), ("t", "t"), ("w", "w")):
            c[key].tofile(tmp_path / f"case_{i}_{name}.f32")
        manifest.append(f"{h} {w} {int(inv)}")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")

    res = run_driver("depth_loss_driver", tmp_path)
    assert f"depth_loss_driver ok cases={len(cases)} bad_args_throw=1" in res.stdout

    for i, (h, w, inv) in enumerate(cases):
        c = dr.case(h, w, inv)
        D, A, t, wt = (torch.from_numpy(c[k]).to(dev) for k in ("D", "A", "t", "w"))
        want = pkg.depth_loss(D, A, t, weight=wt, inverse=inv, align="fit", want_expected=True)
        got = {k: np.fromfile(tmp_path / f"out_{i}_{k}.f32", np.float32) for k in ("out", "gd", "ga", "x")}
        scalars = np.concatenate([np_(want.loss).ravel(), np_(want.scale_shift), np_(want.valid_weight).ravel(),
                                  np_(want.valid_count).ravel(), np_(want.fit_ok).ravel()]).astype(np.float32)
        assert got["out"].tobytes() == scalars.tobytes(), (i, got["out"], scalars)
        assert scalars[5] == 1.0
        assert got["gd"].tobytes() == np_(want.dL_ddepth_map).tobytes(), i
        assert got["ga"].tobytes() == np_(want.dL_dalpha).tobytes(), i
        assert got["x"].tobytes() == np_(want.expected).tobytes(), i
