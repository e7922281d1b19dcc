"""The densifier's and the MCMC controller's scratch is kept per (device, stream), as the rasterizer's, the
initialiser's and the C++ adapter's is: cugs_densify_plan leaves prefixes that cugs_densify_apply reads back
(densify, prune_gaussians), the relocation keeps its scans there and the regulariser its partial sums, so two loops on
two streams of one device must not share a buffer.  Modelled on test_gpu_init.py::test_deterministic_and_stream_safe:
each call queued alternately on two streams with different models equals the same call run alone - and each stream owns
a buffer of its own, which is the deterministic half (overlap cannot be forced)."""
import numpy as np
import pytest
import torch

from util import np_

pytestmark = pytest.mark.gpu

NAMES = ("positions", "sh_coeffs", "opacities", "rotations", "scales")
SIZES = (5003, 3001)                               # two models of different N: different prefixes, different sums
ROUNDS = 3


def _arrays(pkg, n, seed):
    a = pkg.scene.make_gaussians(n, 200, 150, sh_degree=1, seed=seed, mu_s=-2.5)
    a["opacities"] = (a["opacities"] * np.float32(3.0)).astype(np.float32)       # dead and nearly opaque ones alike
    return a


def _state(model, *more):
    return [getattr(model, k).clone() for k in NAMES] + [t.clone() for t in more]


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, i)


def _densify(pkg, dev, arrays, seed):
    n = arrays["positions"].shape[0]
    g = torch.Generator().manual_seed(seed)
    grads = (torch.randn((n, 2), generator=g) * 0.0004).to(dev)
    radii = torch.randint(0, 40, (n,), generator=g, dtype=torch.int32).to(dev)
    noise = torch.randn((2, n, 3), generator=g).to(dev)
    cfg = pkg.DensificationConfig(densify_from=0, densify_every=5, opacity_reset_every=3, opacity_threshold=0.05)

    def call():
        model = pkg.scene.to_model(arrays, dev)
        opt = pkg.FusedAdam(model)
        for i in range(5):
            opt.m_[i] = torch.full_like(opt.m_[i], 0.25)
        ctrl = pkg.DensificationController(cfg, 8.0)
        ctrl.accumulate_gradients(grads, radii)
        s = ctrl.densify(model, 5, noise, optimizer=opt)
        assert s.num_cloned > 0 and s.num_split > 0 and s.num_pruned > s.num_split
        return _state(model, *opt.m_)
    return call


def _prune(pkg, dev, arrays, seed):
    n = arrays["positions"].shape[0]
    mask = (torch.rand(n, generator=torch.Generator().manual_seed(seed)) < 0.4).to(dev)

    def call():
        model = pkg.scene.to_model(arrays, dev)
        assert pkg.prune_gaussians(model, mask) == int(mask.sum())
        return _state(model)
    return call


def _relocate(pkg, dev, arrays, seed):
    ctrl = pkg.MCMCController(pkg.MCMCConfig(relocate_from=0, relocate_every=1, relocate_cap=0.5, seed=seed), 8.0)

    def call():
        model = pkg.scene.to_model(arrays, dev)
        stats = ctrl.relocate(model, 7)
        assert stats.num_relocated > 0
        return _state(model)
    return call


def _regularization(pkg, dev, arrays, seed):
    ctrl = pkg.MCMCController(pkg.MCMCConfig(seed=seed), 8.0)
    model = pkg.scene.to_model(arrays, dev)

    def call():
        return [t.clone().reshape(-1) for t in ctrl.compute_regularization(model)]
    return call


@pytest.mark.parametrize("what", ["densify", "prune_gaussians", "relocate", "compute_regularization"])
def test_two_streams_own_their_scratch(pkg, dev, what):
    from cugs_amd import densification, mcmc
    make = dict(densify=_densify, prune_gaussians=_prune, relocate=_relocate, compute_regularization=_regularization)[what]
    registry = (mcmc if what in ("relocate", "compute_regularization") else densification)._workspaces
    call_a, call_b = (make(pkg, dev, _arrays(pkg, n, seed=70 + i), seed=80 + i) for i, n in enumerate(SIZES))
    alone_a, alone_b = call_a(), call_b()
    assert alone_a[-1].shape != alone_b[-1].shape                              # two different jobs
    torch.cuda.synchronize(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    outs = []
    for _ in range(ROUNDS):                                                     # two calls in flight, a buffer each
        with torch.cuda.stream(s1):
            ra = call_a()
        with torch.cuda.stream(s2):
            rb = call_b()
        outs.append((ra, rb))
    torch.cuda.synchronize(dev)
    keys = [k for k in registry if k[0] == dev and k[1] in (s1.cuda_stream, s2.cuda_stream)]
    assert len(keys) == 2
    assert registry[keys[0]].data_ptr() != registry[keys[1]].data_ptr()
    for ra, rb in outs:
        _same(ra, alone_a, (what, "stream 1"))
        _same(rb, alone_b, (what, "stream 2"))
