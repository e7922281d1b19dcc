"""Host-side mirror of the reference's boundary types and the synthetic scene generator."""
import numpy as np
import torch


def test_gaussian_model_validity_and_degree(pkg):
    n = 5
    m = pkg.GaussianModel(torch.zeros(n, 3), torch.zeros(n, 3, 16), torch.zeros(n, 1), torch.zeros(n, 4),
                          torch.zeros(n, 3))
    assert m.is_valid() and m.num_gaussians() == n and m.max_sh_degree() == 3
    assert pkg.GaussianModel(torch.zeros(n, 3), torch.zeros(n, 3, 9), torch.zeros(n, 1), torch.zeros(n, 4),
                             torch.zeros(n, 3)).max_sh_degree() == 2
    assert not pkg.GaussianModel(torch.zeros(n, 3), torch.zeros(n, 3, 16), torch.zeros(n), torch.zeros(n, 4),
                                 torch.zeros(n, 3)).is_valid()
    assert not pkg.GaussianModel().is_valid()
    assert pkg.sh_coeff_count(3) == 16


def test_camera_to_abi(pkg):
    cam = pkg.scene.make_camera(640, 480, view=2)
    abi = cam.to_abi()
    w2c = cam.world_to_camera()
    assert np.allclose(np.array(list(abi.view), np.float32).reshape(4, 4), w2c)
    R, t = cam.rotation.astype(np.float64), cam.translation.astype(np.float64)
    assert np.allclose(np.array(list(abi.cam_center)), -R.T @ t, atol=1e-6)
    assert (abi.width, abi.height) == (640, 480) and abi.fx == np.float32(0.78 * 640)
    ident = pkg.scene.make_camera(64, 48)
    assert np.array_equal(ident.rotation, np.eye(3, dtype=np.float32)) and not ident.translation.any()


def test_scene_is_reproducible_and_shaped(pkg):
    a = pkg.scene.make_gaussians(1000, 320, 240, sh_degree=3, seed=1234)
    b = pkg.scene.make_gaussians(1000, 320, 240, sh_degree=3, seed=1234)
    for k in a:
        assert np.array_equal(a[k], b[k]) and a[k].dtype == np.float32
    assert a["sh_coeffs"].shape == (1000, 3, 16) and a["opacities"].shape == (1000, 1)
    assert np.allclose(np.linalg.norm(a["rotations"], axis=1), 1.0, atol=1e-6)
    c = pkg.scene.make_gaussians(1000, 320, 240, sh_degree=3, seed=1235)
    assert not np.array_equal(a["positions"], c["positions"])
    g = pkg.scene.make_dl_dcolor(320, 240)
    assert g.shape == (240, 320, 3) and abs(float(g.std()) * 320 * 240 - 1.0) < 0.05


def test_render_rejects_cpu_model(pkg):
    import pytest
    n = 3
    m = pkg.GaussianModel(torch.zeros(n, 3), torch.zeros(n, 3, 1), torch.zeros(n, 1), torch.zeros(n, 4),
                          torch.zeros(n, 3))
    with pytest.raises(RuntimeError, match="CUDA"):          # rasterizer.cpp:28
        pkg.render(m, pkg.scene.make_camera(32, 32), pkg.RenderSettings())
    with pytest.raises(RuntimeError, match="not valid"):     # rasterizer.cpp:27
        pkg.render(pkg.GaussianModel(), pkg.scene.make_camera(32, 32), pkg.RenderSettings())


def test_bench_algorithmic_bytes_match_survey_8d():
    """bench.py's per-stage algorithmic bytes are SURVEY 8d's formulas: the worked number there (C = 16:
    A_fwd + A_bwd = 668 N + 288 P + 40 HW + 8 tiles) and A_adam = 28 (11 + 3C) N."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n, c, p, w, h = 1_000_000, 16, 8_376_524, 1920, 1080
    b = bench.algorithmic_bytes(n, c, p, w, h)
    tiles = 120 * 68
    assert b["frame"] == 668 * n + 288 * p + 40 * w * h + 8 * tiles == 3_163_448_192 + 0 * tiles
    assert b["frame"] == sum(b[k] for k in bench.STAGES)
    assert b["adam"] == 28 * 59 * n
    assert b["raster_backward"] == 714_087_824          # the figure the bench line and DESIGN 4.5 quote


def test_bench_dump_outputs_samples_and_types(tmp_path):
    """bench.py --dump-outputs: per-Gaussian arrays at the same seeded rows in every run, other arrays whole, float32 kept,
    integers written as float64, the byte limit enforced before anything is written."""
    import importlib.util
    import os
    import pytest
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = 3 * bench.DUMP_ROWS
    grad = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    outs = {"total_pairs": torch.tensor([12345], dtype=torch.int64), "color": torch.rand(4, 5, 3),
            "n_contrib": torch.arange(20, dtype=torch.int32).reshape(4, 5), "dL_dpositions": grad}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, n)
    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(got) == set(outs)
    assert got["total_pairs"].dtype == np.float64 and got["total_pairs"].tolist() == [12345.0]
    assert got["n_contrib"].dtype == np.float64 and np.array_equal(got["n_contrib"], outs["n_contrib"].numpy())
    assert got["color"].dtype == np.float32 and np.array_equal(got["color"], outs["color"].numpy())
    rows = got["dL_dpositions"][:, 0] / 3
    assert got["dL_dpositions"].shape == (bench.DUMP_ROWS, 3) and len(np.unique(rows)) == bench.DUMP_ROWS
    assert np.array_equal(got["dL_dpositions"], grad.numpy()[rows.astype(np.int64)])
    assert np.array_equal(got["dL_dpositions"], np.load(tmp_path / "b" / "dL_dpositions.npy"))   # same rows every run
    with pytest.raises(RuntimeError, match="limit"):
        bench.dump_outputs(str(tmp_path / "c"), {"big": torch.zeros(bench.DUMP_LIMIT // 4 + 1)}, n)
    assert not (tmp_path / "c").exists()


def test_bench_rejects_zero_steps():
    import os
    import subprocess
    import sys
    bench = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
    res = subprocess.run([sys.executable, bench, "--gpus", "1", "--steps", "0", "--launcher-dry-run"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and "--steps" in res.stderr
