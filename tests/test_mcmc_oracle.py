"""N5 (MCMC densification) on the CPU: the numpy restatement (tests/mcmc_ref.py) that the GPU tests compare the
device against - its generator against the Random123 known answers, its regulariser against torch autograd, and the
reference's own known answers (tests/test_mcmc.cpp) restated on it and on the host-side schedule of MCMCController."""
import numpy as np
import pytest
import torch

import mcmc_ref as mr

KATS = [  # philox4x32-10: counter (4 words), key (2 words) -> 4 words (Random123 kat_vectors)
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def kat_as_mapping(ctr, key):
    """(seed, stream_id, step, index) of a known-answer counter/key under the counter layout of cugs_hip.h."""
    return key[0] | (key[1] << 32), ctr[2], ctr[3], ctr[0] | (ctr[1] << 32)


@pytest.mark.parametrize("kat", KATS)
def test_philox_known_answers(kat):
    ctr, key, want = kat
    got = mr.philox4x32_10(*ctr, *key)
    assert [int(x) for x in got] == list(want)
    seed, stream, step, index = kat_as_mapping(ctr, key)
    assert [int(x) for x in mr.bits(seed, stream, step, [index])[0]] == list(want)


def test_uniform_range_and_normals():
    assert mr.uniform(0) == 2.0 ** -24 and mr.uniform(0xFFFFFFFF) == 1.0
    z = mr.normals(7, mr.STREAM_NOISE, 3, np.arange(200000, dtype=np.uint64)).astype(np.float64)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
    assert np.isfinite(z).all()


def test_mulhi64():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 2 ** 63, 1000, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    b = rng.integers(0, 2 ** 40, 1000, dtype=np.uint64)
    want = [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]
    assert [int(v) for v in mr.mulhi64(a, b)] == want


def _ulp_diff(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.max(np.abs(a - b))) if a.size else 0


def test_regularizer_against_torch_autograd(orc):
    g = torch.Generator().manual_seed(3)
    n = 5000
    opa = torch.randn((n, 1), generator=g) * 4.0
    scl = torch.randn((n, 3), generator=g) * 1.5 - 3.0
    ref = mr.MCMCRef(orc, 1.0, lambda_opacity=0.01, lambda_scale=0.02)
    value, g_o, g_s = ref.regularization(opa.numpy(), scl.numpy())
    # torch's own backward kernels (mul, mean, sigmoid_backward, exp_backward) on the oracle's activations: the
    # restatement's operation order, to 2 ulp
    y = torch.from_numpy(ref.sigmoid(opa.numpy())).requires_grad_(True)
    e = torch.from_numpy(orc.expf(scl.numpy())).requires_grad_(True)
    (0.01 * y.mean() + 0.02 * e.mean()).backward()
    assert _ulp_diff(g_o, torch.ops.aten.sigmoid_backward(y.grad, y.detach()).numpy()) <= 2
    assert _ulp_diff(g_s, (e.grad * e.detach()).numpy()) <= 2
    # plain autograd (torch's sigmoid / exp): 1 - y cancels near y = 1, so held to the tensors' scale
    o, s = opa.clone().requires_grad_(True), scl.clone().requires_grad_(True)
    loss = 0.01 * torch.sigmoid(o).mean() + 0.02 * torch.exp(s).mean()        # mcmc_densification.cpp:177-178
    loss.backward()
    for got, want in ((g_o, o.grad.numpy()), (g_s, s.grad.numpy())):
        assert np.max(np.abs(got.astype(np.float64) - want)) <= 1e-6 * np.max(np.abs(want))
    assert abs(value - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))


def test_schedule_boundaries(pkg):
    ctrl = pkg.MCMCController(pkg.MCMCConfig(relocate_from=500, relocate_until=15000, relocate_every=100), 10.0)
    for s in (0, 100, 400, 499, 501, 550, 999, 15100, 20000):
        assert not ctrl.should_relocate(s) and not mr.should_relocate(s)
    for s in (500, 600, 1000, 14900, 15000):
        assert ctrl.should_relocate(s) and mr.should_relocate(s)


def test_noise_lr_endpoints_and_decay(pkg):
    ctrl = pkg.MCMCController(pkg.MCMCConfig(noise_lr_init=5e5, noise_lr_final=1e3, noise_lr_max_steps=30000), 10.0)
    assert ctrl.noise_lr(0) == float(np.float32(5e5))
    assert ctrl.noise_lr(30000) == float(np.float32(1e3)) and ctrl.noise_lr(50000) == float(np.float32(1e3))
    prev = ctrl.noise_lr(0)
    for step in range(1000, 30000, 1000):
        cur = ctrl.noise_lr(step)
        assert cur < prev
        prev = cur


def _model(n, opa_val=2.0, seed=0, coeffs=1):
    rng = np.random.default_rng(seed)
    rot = rng.standard_normal((n, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    return dict(positions=(rng.standard_normal((n, 3)) * 0.5).astype(np.float32),
                sh_coeffs=(rng.standard_normal((n, 3, coeffs)) * 0.1).astype(np.float32),
                opacities=np.full((n, 1), opa_val, np.float32), rotations=rot,
                scales=np.full((n, 3), -2.0, np.float32))


def test_relocation_known_answers(orc):
    ref = mr.MCMCRef(orc, 10.0, relocate_cap=1.0)
    m = _model(20)
    m["opacities"][:10], m["opacities"][10:] = 5.0, -8.0
    out, (nd, M, dst, src) = ref.relocate(m, 500)
    assert (nd, M) == (10, 10) and list(dst) == list(range(10, 20)) and (src < 10).all()
    assert np.array_equal(out["positions"][:10], m["positions"][:10])
    assert not np.allclose(out["positions"][10:], m["positions"][10:])
    assert (ref.sigmoid(out["opacities"][10:]) > 0.005).all()            # relocated rows are alive again

    ref = mr.MCMCRef(orc, 10.0, relocate_cap=0.05)
    m = _model(100)
    m["opacities"][:80], m["opacities"][80:] = 5.0, -8.0
    _, (nd, M, dst, _) = ref.relocate(m, 500)
    assert (nd, M) == (20, 5) and list(dst) == list(range(80, 85))

    m = _model(20)                                                         # no dead: no-op
    out, (nd, M, _, _) = ref.relocate(m, 500)
    assert (nd, M) == (0, 0) and all(np.array_equal(out[k], m[k]) for k in m)

    ref = mr.MCMCRef(orc, 10.0, relocate_cap=1.0)                          # constant N over several relocations
    m = _model(30)
    m["opacities"][:20], m["opacities"][20:] = 3.0, -8.0
    for i in range(5):
        m, _ = ref.relocate(m, 500 + 100 * i)
        assert all(v.shape[0] == 30 for v in m.values()) and all(np.isfinite(v).all() for v in m.values())


def test_noise_gate_selectivity(orc):
    ref = mr.MCMCRef(orc, 10.0)
    m = _model(100)
    m["opacities"][:50], m["opacities"][50:] = 10.0, -10.0
    pos = m["positions"]
    for _ in range(10):
        pos = ref.inject_noise(pos, m["scales"], m["opacities"], 1.0, mr.normals(0, mr.STREAM_NOISE, 0, np.arange(100)))
    disp = np.linalg.norm(pos.astype(np.float64) - m["positions"], axis=1)
    assert disp[50:].mean() > 2.0 * disp[:50].mean()
