"""The C++ host side (cuda-gaussian-splatting_amd/adapter: libtorch layer over the C ABI, the code a
maintainer links under the reference's own render()/render_backward()/FusedAdam calls) run as a native
program on the same raw inputs as the Python mirror: same kernels, so identical forward results."""
import numpy as np
import pytest
import torch

from cpp_driver import NO_LEGACY_IPC, run_driver
from util import max_err_over_max, np_

pytestmark = pytest.mark.gpu


def test_cpp_adapter_matches_python_host(pkg, dev, tmp_path):
    w, h, n, deg = 200, 150, 5000, 3
    arrays = pkg.scene.make_gaussians(n, w, h, sh_degree=deg, seed=17, mu_s=-3.8)
    cam = pkg.scene.make_camera(w, h, view=1)
    bg = [0.1, 0.2, 0.3]
    g = pkg.scene.make_dl_dcolor(w, h)
    for k, v in arrays.items():
        np.ascontiguousarray(v, np.float32).tofile(tmp_path / f"{k}.bin")
    g.tofile(tmp_path / "dl_dcolor.bin")
    abi = cam.to_abi()
    camvec = np.array(list(abi.view) + [abi.fx, abi.fy, abi.cx, abi.cy] + list(abi.cam_center) + bg, np.float32)
    assert camvec.size == 26
    camvec.tofile(tmp_path / "camera.bin")
    noise = torch.randn((2, n, 3), generator=torch.Generator().manual_seed(11))
    noise.numpy().tofile(tmp_path / "split_noise.bin")

    res = run_driver("adapter_driver", tmp_path, n, "16", w, h, env=NO_LEGACY_IPC)
    assert "torch_check=1" in res.stdout                     # TORCH_CHECK -> c10::Error on a CPU tensor
    # reference-glue path: a RenderOutput without the packed scratch (the reference's struct has no field for it)
    # gets the records rebuilt and runs the same packed blend kernel: same gradients up to atomic order
    repack = [l for l in res.stdout.splitlines() if l.startswith("glue_repack ")][0].split()
    assert float(repack[1].split("=")[1]) <= 1e-5 and float(repack[2].split("=")[1]) <= 1e-5, repack
    # the fused route of the C++ host: the forward blend cleared the accumulator, render_backward took it out of the
    # RenderOutput, the optimizer step ran inside the projection backward (no gradient tensors), and the updated
    # model equals the one from render_backward + apply_gradients + step up to the atomics' summation order
    fused = dict(kv.split("=") for kv in [l for l in res.stdout.splitlines() if l.startswith("fused_adam ")][0].split()[1:])
    assert fused["cleared"] == "1" and fused["consumed"] == "1", fused
    assert float(fused["dpos"]) <= 1e-7 and float(fused["dsh"]) <= 1e-5 and float(fused["rel_dmeans2d"]) <= 1e-5, fused

    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=bg, active_sh_degree=deg)
    out = pkg.render(model, cam, settings)
    grads = pkg.render_backward(torch.from_numpy(g).to(dev), out, model, cam, settings)
    opt = pkg.FusedAdam(model)
    opt.apply_gradients(grads)
    opt.step()

    rd = lambda name, dt, shape: np.fromfile(tmp_path / name, dtype=dt).reshape(shape)
    assert np.array_equal(rd("out_indices.bin", np.int32, (-1,)), np_(out.gaussian_indices))
    assert np.array_equal(rd("out_n_contrib.bin", np.int32, (h, w)), np_(out.n_contrib))
    assert np.array_equal(rd("out_color.bin", np.uint32, (h, w, 3)), np_(out.color).view(np.uint32))
    # N1 through the C++ host equals the Python host on the same (bit-identical) image
    loss_py, grad_py = pkg.combined_loss_and_grad(out.color, out.color.flip(0).contiguous())
    assert abs(float(rd("out_loss.bin", np.float32, (1,))[0]) - float(loss_py)) <= 1e-6
    assert max_err_over_max(rd("out_loss_grad.bin", np.float32, (h, w, 3)), np_(grad_py)) <= 1e-6
    # gradients: same kernels, atomic order may differ run to run
    assert max_err_over_max(rd("out_dpos.bin", np.float32, (n, 3)), np_(grads.dL_dpositions)) <= 1e-5
    assert max_err_over_max(rd("out_dsh.bin", np.float32, (n, 3, 16)), np_(grads.dL_dsh_coeffs)) <= 1e-5
    # Adam's first step is ~lr * sign(g): elements whose gradient is at rounding-noise level may flip
    a, b = rd("out_positions_after_adam.bin", np.float32, (n, 3)), np_(model.positions)
    assert np.mean(np.abs(a - b) > 1e-6) < 1e-3
    # N2 through the C++ host: same statistics, same noise -> same clone/split/prune as the Python host
    ctrl = pkg.DensificationController(pkg.DensificationConfig(densify_from=0, densify_every=5, opacity_threshold=0.05,
                                                               grad_threshold=2e-7), 6.0)
    ctrl.accumulate_gradients(grads.dL_dmeans_2d, out.radii)
    stats = ctrl.densify(model, 5, noise.to(dev), optimizer=opt)
    # N4 through the C++ host equals the Python host on the same 8-bit view
    u8 = torch.from_numpy(np.fromfile(tmp_path / "out_view_u8.bin", dtype=np.uint8).reshape(h, w, 3)).to(dev)
    half = pkg.image_to_float(u8, w // 2, h // 2)
    assert np.array_equal(rd("out_target_half.bin", np.uint32, (h // 2, w // 2, 3)), np_(half).view(np.uint32))
    # N3 through the C++ host: its checkpoint (with optimizer state) round-trips there, loads here, and the
    # Python writer reproduces the file byte for byte from what it loaded
    assert "ply roundtrip=1 missing_throws=1" in res.stdout
    ck_model, ck_state = pkg.read_gaussian_ply(tmp_path / "out_model.ply", device=dev, return_state=True)
    assert ck_state is not None and ck_state["step"] == 2 and ck_model.is_valid()
    ck_opt = pkg.FusedAdam(ck_model)
    pkg.restore_optimizer(ck_opt, ck_state)
    assert pkg.write_gaussian_ply(tmp_path / "rewritten.ply", ck_model, optimizer=ck_opt)
    assert (tmp_path / "rewritten.ply").read_bytes() == (tmp_path / "out_model.ply").read_bytes()
    line = [l for l in res.stdout.splitlines() if l.startswith("densify ")][0]
    got = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in line.split()[1:]}
    assert stats.num_cloned > 0 and stats.num_split > 0 and stats.num_pruned > stats.num_split
    assert abs(got["after"] - stats.num_after) <= 2 and abs(got["cloned"] - stats.num_cloned) <= 2    # atomics-order noise
    if got["after"] == stats.num_after and got["cloned"] == stats.num_cloned and got["split"] == stats.num_split:
        m2 = stats.num_after
        for name, shape, t in (("out_densify_positions.bin", (m2, 3), model.positions),
                               ("out_densify_sh.bin", (m2, 3, 16), model.sh_coeffs),
                               ("out_densify_scales.bin", (m2, 3), model.scales)):
            a, b = rd(name, np.float32, shape), np_(t)
            assert np.mean(np.abs(a - b) > 1e-5) < 2e-3, name
