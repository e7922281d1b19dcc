"""Evaluation metrics on the GPU (csrc/metrics.hip through cugs_amd.metrics): the device row {MSE, mean SSIM, L1 mean,
max |x - y|} against cugs_combined_loss (bit for bit where they compute the same thing) and the CPU reference
(tests/metrics_ref.py), the 8-bit target path, compute_psnr / compute_ssim, and evaluate() over a small scene."""
import numpy as np
import pytest
import torch

import metrics_ref as mr
from util import np_

pytestmark = pytest.mark.gpu


def _bits(t):
    return np_(t).astype(np.float32).view(np.uint32)


def _on(dev, h, w):
    r, t, ex, ro = mr.case(h, w)
    return r.to(dev), t.to(dev), ex, ro


@pytest.mark.parametrize("ws", [11, 7])
@pytest.mark.parametrize("h,w", mr.SHAPES)
def test_ssim_and_l1_are_the_loss_kernels_bits(pkg, dev, h, w, ws):
    """Slots [1] and [2] are loss_out[2] and loss_out[1] of cugs_combined_loss: one number in the training log and in the
    evaluation table."""
    from cugs_amd import loss
    r, t, _, _ = _on(dev, h, w)
    want = _bits(loss._run(r, t, 0.2, ws, False, False)[0])
    got = _bits(pkg.eval_metrics(r, t, window_size=ws))
    assert got[1] == want[2], (np_(pkg.eval_metrics(r, t, window_size=ws)), want.view(np.float32))
    assert got[2] == want[1]


@pytest.mark.parametrize("h,w", mr.SHAPES)
def test_row_against_cpu_reference(pkg, dev, h, w):
    r, t, ex, ro = _on(dev, h, w)
    row = pkg.eval_metrics(r, t)
    got = np_(row)
    assert row.shape == (4,) and row.dtype == torch.float32 and row.is_cuda
    psnr, ssim_val = pkg.compute_psnr(r, t), pkg.compute_ssim(r, t)
    print(f"{h}x{w}: row {got}  exact mse {ex['mse']!r} l1 {ex['l1']!r} max {ex['max_abs']!r} ssim {ex['ssim']:.8f}  "
          f"psnr {psnr:.6f} reference_ops {float(ro['psnr']):.6f}")
    # fp64 order effects are ~2^-53 n relative: only the final rounding to float can differ, by one step
    assert mr.ulp_distance(got[0], ex["mse"]) <= 1
    assert mr.ulp_distance(got[2], ex["l1"]) <= 1
    assert got[3] == ex["max_abs"]                                           # order-independent: exact
    assert abs(float(got[1]) - ex["ssim"]) <= 1e-5                           # the bar of ssim_loss (test_gpu_loss.py)
    assert abs(psnr - float(ro["psnr"])) <= 1e-3
    assert psnr == float(mr.psnr_of(got[0])) and ssim_val == float(got[1])   # the scalars are made of the row
    assert abs(ssim_val - float(ro["ssim"])) <= 1e-5
    assert np.array_equal(_bits(pkg.eval_metrics(r, t)), _bits(row))         # two calls, the same bits


@pytest.mark.parametrize("h,w", [(37, 53), (270, 480)])
@pytest.mark.parametrize("ws", [11, 7])
def test_8bit_target_is_the_float_path_on_the_expanded_image(pkg, dev, h, w, ws):
    r, t, _, _ = _on(dev, h, w)
    u8 = mr.quantise(t.cpu()).to(dev)
    as_float = pkg.image_to_float(u8, w, h)
    got = pkg.eval_metrics(r, u8, window_size=ws)
    assert np.array_equal(_bits(got), _bits(pkg.eval_metrics(r, as_float, window_size=ws)))
    assert np.array_equal(_bits(got), _bits(pkg.eval_metrics(r, u8, window_size=ws)))
    assert pkg.compute_psnr(r, u8) == pkg.compute_psnr(r, as_float) and pkg.compute_ssim(r, u8) == pkg.compute_ssim(r, as_float)


def test_out_writes_one_row_of_a_table(pkg, dev):
    r, t, _, _ = _on(dev, 37, 53)
    table = torch.full((4, 4), -7.0, device=dev)
    ret = pkg.eval_metrics(r, t, out=table[2])
    assert ret.data_ptr() == table[2].data_ptr()
    got = np_(table)
    assert np.array_equal(got[[0, 1, 3]], np.full((3, 4), -7.0, np.float32))
    assert np.array_equal(got[2].view(np.uint32), _bits(pkg.eval_metrics(r, t)))
    for bad in (torch.empty(4, device=dev)[:3], torch.empty((4, 2), device=dev)[:, 0], torch.empty(4, dtype=torch.float64, device=dev),
                torch.empty(4)):
        with pytest.raises(RuntimeError):
            pkg.eval_metrics(r, t, out=bad)


def test_reference_known_answers_on_gpu(pkg, dev):
    """tests/test_metrics.cpp:33-120 on the HIP path."""
    g = torch.Generator().manual_seed(0)
    img = torch.rand((64, 64, 3), generator=g).to(dev)
    assert pkg.compute_psnr(img, img) >= 100.0
    assert abs(pkg.compute_ssim(img, img) - 1.0) <= 1e-4
    assert np.array_equal(np_(pkg.eval_metrics(img, img))[[0, 2, 3]], np.zeros(3, np.float32))
    a, b = torch.full((32, 32, 3), 0.5, device=dev), torch.full((32, 32, 3), 0.7, device=dev)
    assert abs(pkg.compute_psnr(a, b) - 10.0 * np.log10(25.0)) <= 0.01
    x, y = torch.rand((64, 64, 3), generator=g).to(dev), torch.rand((64, 64, 3), generator=g).to(dev)
    assert abs(pkg.compute_psnr(x, y) - pkg.compute_psnr(y, x)) <= 1e-5
    assert abs(pkg.compute_ssim(x, y) - pkg.compute_ssim(y, x)) <= 1e-5
    assert pkg.compute_psnr(x, y) > 0.0 and np.isfinite(pkg.compute_psnr(x, y))
    z, o = torch.zeros((64, 64, 3), device=dev), torch.ones((64, 64, 3), device=dev)
    assert pkg.compute_ssim(z, o) < 0.5
    assert np_(pkg.eval_metrics(z, o))[3] == 1.0


def test_validation_and_nan(pkg, dev):
    img = torch.rand((64, 64, 3), generator=torch.Generator().manual_seed(0)).to(dev)
    for f in (pkg.compute_psnr, pkg.compute_ssim, pkg.eval_metrics):
        for bad in (lambda: f(img, img[:32]),                                # shape mismatch
                    lambda: f(img[..., :2], img[..., :2]),                   # wrong channel count
                    lambda: f(img[0], img[0]),                               # not [H, W, 3]
                    lambda: f(img.cpu(), img.cpu()),                         # CPU tensor
                    lambda: f(img, img.cpu()),
                    lambda: f(img.int(), img.int()),                         # wrong dtype
                    lambda: f(img, img.double()),
                    lambda: f(img.to(torch.uint8), img)):                    # only the target may be 8-bit
            with pytest.raises(RuntimeError):
                bad()
    with pytest.raises(RuntimeError, match="PSNR: rendered and target must have same shape"):
        pkg.compute_psnr(img, img[:32])
    with pytest.raises(RuntimeError, match=r"PSNR: expected \[H, W, 3\] tensors"):
        pkg.compute_psnr(img[..., :2], img[..., :2])
    for ws in (10, 1, 17):
        with pytest.raises(RuntimeError):
            pkg.eval_metrics(img, img, window_size=ws)
    # NaN in an input reaches all four sums (the reference's behaviour; documented, not special-cased)
    bad = img.clone()
    bad[40, 21, 1] = float("nan")
    assert np.isnan(np_(pkg.eval_metrics(bad, img))).all() and np.isnan(np_(pkg.eval_metrics(img, bad))).all()
    assert np.isnan(pkg.compute_psnr(bad, img))


# ---- evaluate ---------------------------------------------------------------------------------------------------------
W, H, N = 160, 120, 400


@pytest.fixture(scope="module")
def scene(pkg, dev):
    """3 views of a 400-Gaussian model; the targets are renders of a perturbed copy quantised to 8 bits, view 1 stored at
    twice the camera's size so that the resize route runs."""
    arrays = pkg.scene.make_gaussians(N, W, H, sh_degree=1, seed=12, mu_s=-2.6)
    model = pkg.scene.to_model(arrays, dev)
    rng = np.random.default_rng(5)
    pert = dict(arrays, sh_coeffs=(arrays["sh_coeffs"] + 0.05 * rng.standard_normal(arrays["sh_coeffs"].shape)).astype(np.float32))
    truth = pkg.scene.to_model(pert, dev)
    st = pkg.RenderSettings(background=[0.1, 0.2, 0.3], active_sh_degree=1)
    cams = [pkg.scene.make_camera(W, H, view=v) for v in range(3)]
    images = []
    for v in range(3):
        s = 2 if v == 1 else 1
        color = pkg.render(truth, pkg.scene.make_camera(W * s, H * s, view=v), st, for_backward=False).color
        images.append(mr.quantise(color.cpu()))
    return model, cams, images, st


def _expected(pkg, model, cams, cache, st):
    per = []
    for v, cam in enumerate(cams):
        color = pkg.render(model, cam, st, for_backward=False).color
        tgt = cache.view_u8(v) if cache.size(v) == (cam.width, cam.height) else cache.target(v, cam.width, cam.height)
        per.append((pkg.compute_psnr(color, tgt), pkg.compute_ssim(color, tgt)))
    return per


def test_evaluate(pkg, dev, scene):
    model, cams, images, st = scene
    cache = pkg.ViewCache(dev)
    for img in images:
        cache.add(img)
    assert cache.size(0) == (W, H) and cache.size(1) == (2 * W, 2 * H)
    names = ["view_a.png", "view_b.png", "view_c.png"]
    res = pkg.evaluate(model, cams, cache, st, image_names=names)
    per = _expected(pkg, model, cams, cache, st)
    print("evaluate:", res.mean_psnr, res.mean_ssim, per)
    assert [(im.psnr, im.ssim) for im in res.per_image] == per               # bit for bit: each view on its own
    assert [im.image_name for im in res.per_image] == names
    sp, ss = np.float32(0.0), np.float32(0.0)
    for p, s in per:                                                         # float running sums in view order
        sp, ss = np.float32(sp + np.float32(p)), np.float32(ss + np.float32(s))
    assert res.mean_psnr == float(sp / np.float32(3)) and res.mean_ssim == float(ss / np.float32(3))
    assert res.num_gaussians == N and res.sh_degree == 1 and len(res.per_image) == 3
    assert res.eval_time_seconds > 0.0
    assert all(10.0 < p < 60.0 and 0.5 < s < 1.0 for p, s in per)            # a perturbed copy: close, not identical
    import json
    j = json.loads(res.to_json())
    assert j["num_test_images"] == 3 and [e["psnr"] for e in j["per_image"]] == [p for p, _ in per]

    streamed = pkg.StreamedViewCache(dev)
    for img in images:
        streamed.add(img)
    res2 = pkg.evaluate(model, cams, streamed, st, image_names=names)
    assert res2.per_image == res.per_image and (res2.mean_psnr, res2.mean_ssim) == (res.mean_psnr, res.mean_ssim)
    assert streamed.uploads == 3 and streamed.misses == 0                    # every view travelled ahead of its use

    tensors = [img.to(dev) for img in images]                                # a plain sequence of device tensors
    tensors[2] = pkg.image_to_float(tensors[2], W, H)                        # ... one of them already float
    res3 = pkg.evaluate(model, cams, tensors, st)
    assert [(im.psnr, im.ssim) for im in res3.per_image] == per and [im.image_name for im in res3.per_image] == [""] * 3

    empty = pkg.evaluate(model, [], cache, st)
    assert empty == pkg.EvalResults() and empty.per_image == []
