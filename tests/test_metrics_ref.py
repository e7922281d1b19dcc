"""The CPU reference of the evaluation metrics (tests/metrics_ref.py) checked against itself and the reference's known
answers (tests/test_metrics.cpp:33-120), and the host-only parts of cugs_amd.metrics: PSNR from an MSE, EvalResults'
JSON (test_metrics.cpp:126-169) from the Python host and from the C++ host's hand-written writer.  No GPU."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import metrics_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTER = os.path.join(ROOT, "cuda-gaussian-splatting_amd", "adapter")
KEYS = {"mean_psnr", "mean_ssim", "num_gaussians", "sh_degree", "eval_time_seconds", "num_test_images", "per_image"}


@pytest.mark.parametrize("h,w", mr.SHAPES)
def test_exact_and_reference_ops_agree(h, w):
    _, _, ex, ro = mr.case(h, w)
    print(f"{h}x{w}: psnr exact {ex['psnr']:.6f} reference_ops {ro['psnr']:.6f}  ssim {ex['ssim']:.7f} {ro['ssim']:.7f}")
    assert abs(float(ex["psnr"]) - float(ro["psnr"])) <= 1e-3
    assert abs(ex["ssim"] - float(ro["ssim"])) <= 1e-5


def test_reference_known_answers():
    g = torch.Generator().manual_seed(0)
    img = torch.rand((64, 64, 3), generator=g)
    assert mr.reference_ops(img, img)["psnr"] >= 100.0 and mr.exact(img, img)["psnr"] >= 100.0
    a, b = torch.full((32, 32, 3), 0.5), torch.full((32, 32, 3), 0.7)
    want = 10.0 * np.log10(25.0)
    assert abs(float(mr.reference_ops(a, b)["psnr"]) - want) <= 0.01
    assert abs(float(mr.exact(a, b)["psnr"]) - want) <= 0.01
    x, y = torch.rand((64, 64, 3), generator=g), torch.rand((64, 64, 3), generator=g)
    for f in (mr.reference_ops, mr.exact):
        xy, yx = f(x, y), f(y, x)
        assert abs(float(xy["psnr"]) - float(yx["psnr"])) <= 1e-5
        assert abs(float(xy["ssim"]) - float(yx["ssim"])) <= 1e-5
        assert float(xy["psnr"]) > 0.0 and np.isfinite(float(xy["psnr"]))
    assert abs(float(mr.reference_ops(img, img)["ssim"]) - 1.0) <= 1e-4
    z, o = torch.zeros((64, 64, 3)), torch.ones((64, 64, 3))
    assert float(mr.reference_ops(z, o)["ssim"]) < 0.5 and mr.exact(z, o)["ssim"] < 0.5


def test_host_psnr_from_mse(pkg):
    from cugs_amd import metrics
    assert metrics.psnr_from_mse(0.0) == 100.0 and metrics.psnr_from_mse(9.9e-11) == 100.0     # metrics.cpp:30-32
    assert abs(metrics.psnr_from_mse(0.04) - 10.0 * np.log10(25.0)) <= 1e-5
    for mse in (1e-10, 1e-4, 0.04, 0.25, 3.0):
        assert metrics.psnr_from_mse(mse) == float(mr.psnr_of(mse))
    assert np.isnan(metrics.psnr_from_mse(float("nan")))                                       # NaN propagates


def _sample(pkg):
    res = pkg.EvalResults(mean_psnr=float(np.float32(25.5)), mean_ssim=float(np.float32(0.88)), num_gaussians=100000,
                          sh_degree=3, eval_time_seconds=12.5)
    res.per_image.append(pkg.ImageMetrics("test_001.jpg", float(np.float32(24.3)), float(np.float32(0.86))))
    res.per_image.append(pkg.ImageMetrics("test_002.jpg", float(np.float32(26.7)), float(np.float32(0.90))))
    return res


def _check_sample(j):
    assert set(j) == KEYS
    assert abs(j["mean_psnr"] - 25.5) <= 0.01 and abs(j["mean_ssim"] - 0.88) <= 0.01
    assert j["num_gaussians"] == 100000 and j["sh_degree"] == 3 and j["num_test_images"] == 2
    assert abs(j["eval_time_seconds"] - 12.5) <= 1e-6
    assert len(j["per_image"]) == 2
    assert j["per_image"][0]["image_name"] == "test_001.jpg" and j["per_image"][1]["image_name"] == "test_002.jpg"
    assert abs(j["per_image"][0]["psnr"] - 24.3) <= 0.01 and abs(j["per_image"][1]["ssim"] - 0.90) <= 0.01
    assert set(j["per_image"][0]) == {"image_name", "psnr", "ssim"}


def test_eval_results_json_roundtrip(pkg, tmp_path):
    res = _sample(pkg)
    text = res.to_json()
    for key in KEYS:
        assert f'"{key}"' in text
    assert "test_001.jpg" in text and "test_002.jpg" in text
    assert text.startswith('{\n  "') and '\n    {\n      "image_name"' in text               # dump(2): 2-space indent
    _check_sample(json.loads(text))
    path = tmp_path / "a" / "b" / "eval.json"                                                 # parents are created
    res.save_json(path)
    assert path.read_text() == text + "\n"
    empty = json.loads(pkg.EvalResults().to_json())
    assert set(empty) == KEYS and empty["per_image"] == [] and empty["num_test_images"] == 0
    odd = pkg.EvalResults(mean_psnr=float("inf"), mean_ssim=float("nan"))                     # nlohmann writes null
    assert json.loads(odd.to_json())["mean_psnr"] is None and json.loads(odd.to_json())["mean_ssim"] is None


def test_evaluate_without_views_touches_no_gpu(pkg):
    res = pkg.evaluate(None, [], None, None)                                                  # metrics.cpp:98-102
    assert res == pkg.EvalResults() and res.per_image == [] and res.mean_psnr == 0.0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpp_json_writer_matches_python_host(pkg, tmp_path):
    """adapter/eval_results.hpp (std only) built on its own: the same text as the Python host for the reference's
    sample, valid JSON for names with quotes, control bytes and UTF-8, null for non-finite numbers."""
    exe = tmp_path / "eval_json_check"
    subprocess.run(["g++", "-std=c++17", "-O0", "-o", str(exe), os.path.join(ADAPTER, "eval_json_check.cpp")], check=True)
    saved = tmp_path / "out" / "dir" / "eval.json"
    out = subprocess.run([str(exe), str(saved)], capture_output=True, text=True, check=True, timeout=60).stdout
    sample, empty, odd = out.split("\n===\n")
    assert sample == _sample(pkg).to_json()
    _check_sample(json.loads(sample))
    assert saved.read_text() == sample + "\n"
    assert empty == pkg.EvalResults().to_json()
    j = json.loads(odd)
    assert j["mean_psnr"] is None and j["mean_ssim"] is None and j["num_gaussians"] == -1
    assert j["per_image"][0]["image_name"] == "a\"b\\c\n\t\x01/é" + "x" * 300
    assert j["per_image"][0]["psnr"] == 100.0 and j["per_image"][0]["ssim"] == -1.0
    assert np.float32(j["per_image"][1]["psnr"]) == np.finfo(np.float32).max
    assert np.float32(j["eval_time_seconds"]) == np.float32(1e-7)
