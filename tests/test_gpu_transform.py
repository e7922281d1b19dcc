"""transform_gaussians / merge_gaussians on the device: the kernel against its numpy float32 mirror bit
for bit, untouched rows, the inverse, render invariance against the oracle's own gap, the optimizer rule, merging, and
the path from a voted label to a merged scene."""
import numpy as np
import pytest
import torch

import transform_ref as tr

pytestmark = pytest.mark.gpu
PARAMS = tr.PARAMS


def np_(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np_(a) if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _model(pkg, arrays, dev, offset_views=False):
    if not offset_views:
        return pkg.scene.to_model(arrays, dev)
    tensors = {}
    for k, v in arrays.items():                                       # every tensor starts 4 bytes off a 16-byte boundary
        buf = torch.empty(v.size + 1, dtype=torch.float32, device=dev)
        t = buf[1:].view(v.shape)
        t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        tensors[k] = t
    return pkg.GaussianModel(**tensors)


def _masks(n):
    rng = np.random.Generator(np.random.Philox(key=77 + n))
    last = np.zeros(n, dtype=bool)
    last[-1] = True
    return [("none", None), ("all_clear", np.zeros(n, dtype=bool)), ("all_set", np.ones(n, dtype=bool)),
            ("random_half", rng.uniform(size=n) < 0.5), ("last_row", last)]


def _expected(arrays, full, mask):
    if mask is None:
        return full
    return {k: np.where(mask.reshape((-1,) + (1,) * (arrays[k].ndim - 1)), full[k], arrays[k]) for k in PARAMS}


def _assert_same_bits(model, want, what):
    for k in PARAMS:
        assert np.array_equal(_bits(getattr(model, k)), _bits(want[k])), (what, k)


@pytest.mark.parametrize("coeffs", [1, 4, 9, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 70001])
def test_kernel_equals_the_mirror_bit_for_bit(pkg, dev, n, coeffs):
    arrays = tr.make_arrays(pkg, n, coeffs=coeffs, seed=100 + n)
    for name, sim in tr.similarity_cases(pkg):
        full = tr.mirror32(arrays, sim.to_abi())
        for mname, mask in _masks(n):
            model = _model(pkg, arrays, dev)
            m = None if mask is None else torch.from_numpy(mask).to(dev)
            assert pkg.transform_gaussians(model, sim, mask=m) is None
            want = _expected(arrays, full, mask)
            _assert_same_bits(model, want, (name, mname))
            # rows with a clear mask bit, the whole model under the identity, opacities and the DC term: every bit kept
            assert np.array_equal(_bits(model.opacities), _bits(arrays["opacities"]))
            assert np.array_equal(_bits(model.sh_coeffs[:, :, 0]), _bits(arrays["sh_coeffs"][:, :, 0]))
            if name == "identity" or mname == "all_clear":
                _assert_same_bits(model, arrays, (name, mname, "untouched"))
            elif mask is not None:
                for k in PARAMS:
                    assert np.array_equal(_bits(getattr(model, k))[~mask], _bits(arrays[k])[~mask]), (name, mname, k)


@pytest.mark.parametrize("coeffs", [1, 4, 9, 16])
def test_views_four_bytes_off_a_16_byte_boundary(pkg, dev, coeffs):
    n = 257
    arrays = tr.make_arrays(pkg, n, coeffs=coeffs, seed=9)
    mask = _masks(n)[3][1]
    for name, sim in tr.similarity_cases(pkg)[3:]:
        model = _model(pkg, arrays, dev, offset_views=True)
        pkg.transform_gaussians(model, sim, mask=torch.from_numpy(mask).to(dev))
        _assert_same_bits(model, _expected(arrays, tr.mirror32(arrays, sim.to_abi()), mask), name)


def test_transform_refuses_what_it_cannot_do_in_place(pkg, dev):
    arrays = tr.make_arrays(pkg, 16)
    model = pkg.scene.to_model(arrays, dev)
    sim = tr.similarity_cases(pkg)[4][1]
    with pytest.raises(RuntimeError, match="mask"):
        pkg.transform_gaussians(model, sim, mask=torch.ones(15, dtype=torch.bool, device=dev))
    with pytest.raises(RuntimeError, match="mask"):
        pkg.transform_gaussians(model, sim, mask=torch.ones(16, dtype=torch.uint8, device=dev))
    model.positions = model.positions.t().contiguous().t()
    with pytest.raises(RuntimeError, match="contiguous"):
        pkg.transform_gaussians(model, sim)
    f = dict(dtype=torch.float32, device=dev)
    empty = pkg.GaussianModel(torch.zeros((0, 3), **f), torch.zeros((0, 3, 16), **f), torch.zeros((0, 1), **f),
                              torch.zeros((0, 4), **f), torch.zeros((0, 3), **f))
    pkg.transform_gaussians(empty, sim)
    assert empty.num_gaussians() == 0


@pytest.mark.parametrize("coeffs", [4, 16])
def test_inverse_returns_the_model_within_twice_the_mirror_bound(pkg, dev, coeffs):
    """sim then sim.inverse(): the first pass is within the mirror bound F |A||x| of exact, that error grows by |A^-1|
    through the second pass, which adds its own mirror bound: two mirror-bound terms."""
    n = 2000
    arrays = tr.make_arrays(pkg, n, coeffs=coeffs, seed=5)
    for name, sim in tr.similarity_cases(pkg)[1:]:
        inv = sim.inverse()
        model = pkg.scene.to_model(arrays, dev)
        pkg.transform_gaussians(model, sim)
        mid = {k: np_(getattr(model, k)) for k in PARAMS}
        pkg.transform_gaussians(model, inv)
        _, mag1 = tr.exact64(arrays, sim.scale, sim.rotation, sim.translation)
        _, mag2 = tr.exact64(mid, inv.scale, inv.rotation, inv.translation)
        carried = tr.propagate(mag1, inv.scale, inv.rotation)
        for k in ("positions", "rotations", "scales", "sh_coeffs"):
            err = np.abs(np_(getattr(model, k)).astype(np.float64) - arrays[k])
            bound = tr.MIRROR_FACTOR * (carried[k] + mag2[k])
            print(f"{name} {k}: worst round-trip error / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
            assert np.all(err <= bound), (name, k)
        assert np.array_equal(_bits(model.opacities), _bits(arrays["opacities"]))


# ---- render invariance -----------------------------------------------------------------------------------------------
def _render(pkg, model, cam, degree):
    out = pkg.render(model, cam, pkg.RenderSettings(background=[0.1, 0.2, 0.3], active_sh_degree=degree),
                     for_backward=False, want_depth_map=True)
    return dict(color=np_(out.color).astype(np.float64), alpha=np_(out.alpha).astype(np.float64),
                depth_map=np_(out.depth_map).astype(np.float64), visible=np_(out.radii) > 0)


_CASES = None


def _render_case(pkg, orc, i):
    """The shared cases with the oracle's own gap, computed once."""
    global _CASES
    if _CASES is None:
        _CASES = [dict(case=c, gap=tr.oracle_gap(orc, c[1], c[2], c[3], pkg, c[4])) for c in tr.render_cases(pkg)]
    return _CASES[i]


@pytest.mark.parametrize("i", range(7))
def test_render_of_the_moved_model_from_the_moved_camera(pkg, orc, dev, i):
    entry = _render_case(pkg, orc, i)
    name, arrays, cam, sim, degree = entry["case"]
    gap = entry["gap"]
    assert gap["same_visibility"]
    base = _render(pkg, pkg.scene.to_model(arrays, dev), cam, degree)
    dscale = max(float(np.max(np.abs(gap["ref"]["depth_map"]))), 1e-30)
    moved_cam = pkg.transform_camera(cam, sim)

    whole = pkg.scene.to_model(arrays, dev)
    pkg.transform_gaussians(whole, sim)
    parts = pkg.scene.to_model(arrays, dev)                            # the far rows first, then the complement
    far = parts.positions[:, 2] > 6.0
    near = ~far
    assert 0 < int(far.sum()) < arrays["positions"].shape[0]
    pkg.transform_gaussians(parts, sim, mask=far)
    pkg.transform_gaussians(parts, sim, mask=near)
    for what, model in (("whole", whole), ("two masked calls", parts)):
        got = _render(pkg, model, moved_cam, degree)
        errs = dict(color=float(np.max(np.abs(got["color"] - base["color"]))),
                    alpha=float(np.max(np.abs(got["alpha"] - base["alpha"]))),
                    depth=float(np.max(np.abs(got["depth_map"] / sim.scale - base["depth_map"]))) / dscale)
        for k, e in errs.items():
            print(f"{name} {what} {k}: device {e:.2e}, oracle gap {gap[k]:.2e}")
            assert e <= 4.0 * gap[k] + 1e-6, (name, what, k)
        assert np.array_equal(got["visible"], base["visible"]), (name, what)
    for k in PARAMS:
        assert torch.equal(getattr(parts, k), getattr(whole, k)), k


# ---- the optimizer rule --------------------------------------------------------------------------------------------------
def _trained(pkg, dev, n=1500, steps=3, degree=3):
    arrays = pkg.scene.make_gaussians(n, tr.W, tr.H, sh_degree=degree, seed=61, mu_s=-3.0)
    cam = pkg.scene.make_camera(tr.W, tr.H)
    model = pkg.scene.to_model(arrays, dev)
    settings = pkg.RenderSettings(background=[0.1, 0.2, 0.3], active_sh_degree=degree)
    g = torch.from_numpy(pkg.scene.make_dl_dcolor(tr.W, tr.H)).to(dev)
    opt = pkg.FusedAdam(model)
    for _ in range(steps):
        out = pkg.render(model, cam, settings)
        opt.apply_gradients(pkg.render_backward(g, out, model, cam, settings))
        opt.step()
    assert all(bool(m.any()) for m in opt.m_) and all(bool(v.any()) for v in opt.v_)
    return model, opt, cam, settings, g


def test_optimizer_moments_follow_the_rule(pkg, dev):
    model, opt, cam, settings, g = _trained(pkg, dev)
    n = model.num_gaussians()
    before = [t.clone() for t in (*opt.m_, *opt.v_)]
    pkg.transform_gaussians(model, pkg.Similarity(1.0, np.eye(3), [0.5, -0.25, 1.0]), optimizer=opt)
    for got, old in zip((*opt.m_, *opt.v_), before):
        assert torch.equal(got, old)                                  # a pure translation: every moment kept
    rng = np.random.Generator(np.random.Philox(key=3))
    mask = torch.from_numpy(rng.uniform(size=n) < 0.4).to(dev)
    sim = pkg.Similarity(1.5, tr.random_rotation(21), [0.1, 0.2, 0.3])
    params = {k: getattr(model, k).clone() for k in PARAMS}
    pkg.transform_gaussians(model, sim, mask=mask, optimizer=opt)
    assert opt.step_count_ == 3
    names = opt._names
    for moments, old in ((opt.m_, before[:5]), (opt.v_, before[5:])):
        for gi, name in enumerate(names):
            if name in ("positions", "sh_coeffs", "rotations"):
                assert not moments[gi][mask].any(), name
                assert torch.equal(moments[gi][~mask], old[gi][~mask]), name
                assert bool(old[gi][mask].any())
            else:
                assert torch.equal(moments[gi], old[gi]), name
    want = tr.mirror32({k: np_(v) for k, v in params.items()}, sim.to_abi(), np_(mask))
    _assert_same_bits(model, want, "with an optimizer")
    # training goes on: a fused backward + Adam step on the moved model from the moved camera
    moved_cam = pkg.transform_camera(pkg.transform_camera(cam, pkg.Similarity(1.0, np.eye(3), [0.5, -0.25, 1.0])), sim)
    pkg.transform_gaussians(model, sim, mask=~mask, optimizer=opt)     # the rest follows: one consistent scene again
    assert not opt.m_[0].any() and bool(opt.m_[3].any())
    held = {k: getattr(model, k).clone() for k in PARAMS}
    out = pkg.render(model, moved_cam, settings)
    pkg.render_backward(g, out, model, moved_cam, settings, fused_adam=opt)
    torch.cuda.synchronize()
    assert opt.step_count_ == 4
    for k in PARAMS:
        assert not torch.equal(getattr(model, k), held[k]), k
        assert bool(torch.isfinite(getattr(model, k)).all()), k


# ---- merge_gaussians -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg_a,deg_b", [(3, 3), (3, 1), (1, 3)])
def test_merge_appends_rows_and_moments(pkg, dev, deg_a, deg_b):
    model, opt, cam, settings, g = _trained(pkg, dev, n=700, degree=deg_a)
    other_arrays = pkg.scene.make_gaussians(333, tr.W, tr.H, sh_degree=deg_b, seed=62, mu_s=-3.0)
    other = pkg.scene.to_model(other_arrays, dev)
    a = {k: np_(getattr(model, k)) for k in PARAMS}
    old_m, old_v = [np_(t) for t in opt.m_], [np_(t) for t in opt.v_]
    opt.apply_gradients(pkg.render_backward(g, pkg.render(model, cam, settings), model, cam, settings))
    assert pkg.merge_gaussians(model, other, opt) == 1033 == model.num_gaussians()
    assert all(x is None for x in opt.grads_)                           # pending gradients are cleared
    c = (max(deg_a, deg_b) + 1) ** 2

    def pad(x):
        out = np.zeros(x.shape[:2] + (c,), np.float32)
        out[:, :, :x.shape[2]] = x
        return out
    want = {k: np.concatenate([pad(a[k]) if k == "sh_coeffs" else a[k],
                               pad(other_arrays[k]) if k == "sh_coeffs" else other_arrays[k]]) for k in PARAMS}
    _assert_same_bits(model, want, "merged")
    assert model.is_valid() and all(getattr(model, k).is_contiguous() for k in PARAMS)
    for k in PARAMS:
        assert np.array_equal(_bits(getattr(other, k)), _bits(other_arrays[k]))          # `other` is not modified
    for moments, old in ((opt.m_, old_m), (opt.v_, old_v)):
        for gi, name in enumerate(opt._names):
            keep = pad(old[gi]) if name == "sh_coeffs" else old[gi]
            assert moments[gi].shape == getattr(model, name).shape
            assert np.array_equal(_bits(moments[gi][:700]), _bits(keep)), name
            assert not moments[gi][700:].any(), name
    # a render of the merged model equals a render of the model concatenated on the host
    s3 = pkg.RenderSettings(background=[0.1, 0.2, 0.3], active_sh_degree=3)
    got = pkg.render(model, cam, s3)
    ref = pkg.render(pkg.scene.to_model(want, dev), cam, s3)
    assert torch.equal(got.color, ref.color) and torch.equal(got.radii, ref.radii)
    held = model.positions.clone()
    pkg.render_backward(g, got, model, cam, s3, fused_adam=opt)
    torch.cuda.synchronize()
    assert opt.step_count_ == 4 and not torch.equal(model.positions, held)
    assert bool(torch.isfinite(model.sh_coeffs).all())


def test_merge_without_an_optimizer_and_of_nothing(pkg, dev):
    a = tr.make_arrays(pkg, 50, coeffs=9)
    b = tr.make_arrays(pkg, 0, coeffs=9)
    model = pkg.scene.to_model(a, dev)
    assert pkg.merge_gaussians(model, pkg.scene.to_model(b, dev)) == 50
    _assert_same_bits(model, a, "nothing appended")
    assert pkg.merge_gaussians(model, pkg.scene.to_model(a, dev)) == 100
    _assert_same_bits(model, {k: np.concatenate([a[k], a[k]]) for k in PARAMS}, "doubled")


# ---- from a voted label to a merged scene ----------------------------------------------------------------------------
def test_select_move_and_merge_an_object(pkg, dev):
    w, h = tr.W, tr.H
    arrays = pkg.scene.make_gaussians(1200, w, h, sh_degree=3, seed=71, mu_s=-3.0)
    cams = [pkg.scene.make_camera(w, h, v) for v in (0, 3)]
    settings = pkg.RenderSettings(background=[0.1, 0.2, 0.3], active_sh_degree=3)
    scene_a = pkg.scene.to_model(arrays, dev)
    label_image = torch.zeros((h, w), dtype=torch.int32, device=dev)
    label_image[:, w // 2:] = 1                                       # the object: what the right half of the views shows
    labels, _ = pkg.vote_labels(scene_a, cams, [label_image, label_image], 2, settings)
    picked = labels == 1
    count = int(picked.sum())
    assert 0 < count < 1200
    sim = pkg.Similarity(0.5, tr.random_rotation(31), [0.2, 0.1, 3.0])
    pkg.transform_gaussians(scene_a, sim, mask=picked)
    want = tr.mirror32(arrays, sim.to_abi(), np_(picked))
    _assert_same_bits(scene_a, want, "object moved in its scene")
    assert pkg.select_gaussians(scene_a, picked) == count
    _assert_same_bits(scene_a, {k: want[k][np_(picked)] for k in PARAMS}, "object extracted")

    arrays_b = pkg.scene.make_gaussians(800, w, h, sh_degree=3, seed=72, mu_s=-3.0)
    scene_b = pkg.scene.to_model(arrays_b, dev)
    assert pkg.merge_gaussians(scene_b, scene_a) == 800 + count
    host = {k: np.concatenate([arrays_b[k], want[k][np_(picked)]]) for k in PARAMS}
    _assert_same_bits(scene_b, host, "object placed")
    got = pkg.render(scene_b, cams[0], settings, for_backward=False)
    ref = pkg.render(pkg.scene.to_model(host, dev), cams[0], settings, for_backward=False)
    assert torch.equal(got.color, ref.color)
    alone = pkg.render(pkg.scene.to_model(arrays_b, dev), cams[0], settings, for_backward=False)
    assert not torch.equal(got.color, alone.color)                     # the object is in the picture
