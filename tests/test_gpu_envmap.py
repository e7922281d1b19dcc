"""The environment-map background on the GPU (csrc/envmap.hip through cugs_amd.envmap) against tests/envmap_ref.py: the
composite, the sample and dL_dalpha bit for bit, the fixed-point map gradient bit for bit and from run to run, the clamp
flag, the equivalence with render()'s own constant background, the image-background route, the argument errors, and a
short fit of the map through the fused Adam step."""
import dataclasses

import numpy as np
import pytest
import torch

import envmap_ref as er
from util import GRAD_NAMES, max_err_over_max, np_

pytestmark = pytest.mark.gpu
CASES = er.cases()
COLOUR = (0.25, 0.6, 0.9)


def _info(pkg, cam):
    return pkg.CameraInfo(width=cam["width"], height=cam["height"], rotation=np.array(cam["R"], np.float32),
                          intrinsics=pkg.CameraIntrinsics(cam["fx"], cam["fy"], cam["cx"], cam["cy"]))


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _render_out(pkg, color, final_T):
    """A RenderOutput with what the composites read: colour, final_T and (for the backward's route check) depths."""
    rest = [None] * (len(dataclasses.fields(pkg.RenderOutput)) - 2)
    out = pkg.RenderOutput(color, final_T, *rest[:9])
    out.depths = torch.zeros(1, device=color.device)
    return out


def _env(pkg, dev, E, orient=None):
    env = pkg.EnvironmentMap(resolution=E.shape[1], device=dev, orientation=orient)
    env.texture.copy_(_dev(E, dev))
    return env


@pytest.fixture(scope="module")
def scene(pkg, dev):
    """A small scene that leaves some pixels open and covers others, rendered once on background 0."""
    w, h = 64, 48
    arrays = pkg.scene.make_gaussians(60, w, h, sh_degree=1, seed=11, mu_s=-1.8, cluster=(1.0, 0.2))
    arrays["opacities"] = arrays["opacities"] + np.float32(4.0)
    model = pkg.scene.to_model(arrays, dev)
    cam = pkg.scene.make_camera(w, h)
    zero = pkg.RenderSettings(background=[0.0, 0.0, 0.0], active_sh_degree=1)
    out = pkg.render(model, cam, zero)
    T = np_(out.final_T)
    assert (T == 1.0).sum() > 200 and (T < 0.02).sum() > 100 and ((T > 0.1) & (T < 0.9)).sum() > 200
    return dict(model=model, cam=cam, zero=zero, out=out, w=w, h=h)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_composite_sample_and_gradients_equal_the_mirror_bit_for_bit(pkg, dev, case):
    label, h, w, res, cam, orient = case
    E, C, T, g = er.case_data(h, w, res)
    taps = er.taps32(cam, res, orient)
    B = er.sample32(E, taps, h, w)
    env, info = _env(pkg, dev, E, orient), _info(pkg, cam)
    out = _render_out(pkg, _dev(C, dev), _dev(T, dev))
    assert np_(env.sample(info)).tobytes() == B.tobytes()
    assert np_(pkg.composite_environment(out, info, env)).tobytes() == er.composite32(C, T, B).tobytes()
    back = pkg.composite_environment_backward(_dev(g, dev), out, info, env, grad_bound=1.0)
    assert np_(back.dL_dalpha).tobytes() == er.dalpha32(g, B).tobytes()
    grad, table, clamped = er.denv32(taps, g, T, res, grad_bound=1.0)
    assert clamped == 0 and int(back.clamped) == 0
    assert np_(back.dL_denv).tobytes() == grad.tobytes()
    again = pkg.composite_environment_backward(_dev(g, dev), out, info, env, grad_bound=1.0)
    assert np_(again.dL_denv).tobytes() == np_(back.dL_denv).tobytes()                 # the same bytes on every run
    # without the map gradient: dL_dalpha alone, unchanged
    only = pkg.composite_environment_backward(_dev(g, dev), out, info, env, want_env_grad=False)
    assert only.dL_denv is None and only.clamped is None
    assert np_(only.dL_dalpha).tobytes() == np_(back.dL_dalpha).tobytes()


def test_a_bound_below_the_gradient_clamps_and_raises_the_flag(pkg, dev):
    label, h, w, res, cam, orient = CASES[-1]
    E, C, T, g = er.case_data(h, w, res)
    bound = 2.0 ** -6
    assert np.abs(T[..., None] * g).max() > bound
    taps = er.taps32(cam, res, orient)
    grad, table, clamped = er.denv32(taps, g, T, res, grad_bound=bound)
    assert clamped == 1
    env, info = _env(pkg, dev, E, orient), _info(pkg, cam)
    out = _render_out(pkg, _dev(C, dev), _dev(T, dev))
    back = pkg.composite_environment_backward(_dev(g, dev), out, info, env, grad_bound=bound)
    assert int(back.clamped) == 1
    got = np_(back.dL_denv)
    assert np.isfinite(got).all() and np.abs(got).max() <= 4 * h * w * bound              # nothing overflowed
    assert got.tobytes() == grad.tobytes()
    # a non-finite gradient counts 0 and raises the flag as well
    g2 = g.copy()
    g2[3, 5, 1] = np.nan
    T2 = T.copy()
    T2[3, 5] = 0.5
    out2 = _render_out(pkg, _dev(C, dev), _dev(T2, dev))
    back2 = pkg.composite_environment_backward(_dev(g2, dev), out2, info, env, grad_bound=1.0)
    grad2, _, clamped2 = er.denv32(taps, g2, T2, res, grad_bound=1.0)
    assert clamped2 == 1 and int(back2.clamped) == 1 and np_(back2.dL_denv).tobytes() == grad2.tobytes()


def test_the_ray_of_a_pixel_is_where_the_projection_puts_a_splat(pkg, dev):
    """Step 1's pixel centre (u + 0.5) against the projection: a small opaque splat on the ray of pixel (u, v) must
    cover that pixel most."""
    w, h, u, v = 33, 17, 21, 5
    cam = pkg.CameraInfo(width=w, height=h, intrinsics=pkg.CameraIntrinsics(fx=27.0, fy=31.0, cx=14.3, cy=9.9))
    z = 4.0
    pos = np.array([[((u + 0.5) - 14.3) / 27.0 * z, ((v + 0.5) - 9.9) / 31.0 * z, z]], np.float32)
    arrays = dict(positions=pos, sh_coeffs=np.ones((1, 3, 1), np.float32), opacities=np.full((1, 1), 6.0, np.float32),
                  rotations=np.array([[1, 0, 0, 0]], np.float32), scales=np.full((1, 3), -2.5, np.float32))
    out = pkg.render(pkg.scene.to_model(arrays, dev), cam, pkg.RenderSettings(active_sh_degree=0))
    T = np_(out.final_T)
    assert np.unravel_index(np.argmin(T), T.shape) == (v, u) and T[v, u] < 0.1


def test_a_uniform_map_is_the_constant_background_of_render(pkg, dev, scene):
    model, cam, out = scene["model"], scene["cam"], scene["out"]
    env = pkg.EnvironmentMap(resolution=16, device=dev, init_color=COLOUR)
    image, out0 = pkg.render_with_environment(model, cam, scene["zero"], env)
    on_colour = pkg.RenderSettings(background=list(COLOUR), active_sh_degree=1)
    ref = pkg.render(model, cam, on_colour)
    assert np_(out0.color).tobytes() == np_(out.color).tobytes()
    assert np_(image).tobytes() == np_(ref.color).tobytes()
    assert np_(out0.final_T).tobytes() == np_(ref.final_T).tobytes()

    # the two backward routes: background 0 with the composite's dL_dalpha / background c without it
    g = _dev(pkg.scene.make_dl_dcolor(scene["w"], scene["h"]), dev)
    back = pkg.composite_environment_backward(g, out0, cam, env, grad_bound=1.0)
    via_alpha = pkg.render_backward(g, out0, model, cam, scene["zero"], dL_dalpha=back.dL_dalpha)
    direct = pkg.render_backward(g, ref, model, cam, on_colour)
    for name in GRAD_NAMES:
        a, b = np_(getattr(via_alpha, name)), np_(getattr(direct, name))
        err = max_err_over_max(a, b)
        print(f"{name}: max |diff| / max |ref| = {err:.3e}")
        assert np.abs(b).max() > 0 and err <= 1e-4, name
    # the map's gradient of a uniform map: every share of a pixel sums to T g
    total = np_(back.dL_denv).astype(np.float64).sum(axis=(1, 2))
    shares = np_(out0.final_T).astype(np.float64)[..., None] * np_(g).astype(np.float64)
    # a share carries three float32 roundings (T g, the weight, their product) and 2^-F of quantisation
    assert np.abs(total - shares.sum(axis=(0, 1))).max() <= 1e-6 * np.abs(shares).sum(axis=(0, 1)).max()


def test_the_image_background_route_equals_the_fused_one(pkg, dev, scene):
    cam, out = scene["cam"], scene["out"]
    rng = np.random.default_rng(3)
    env = _env(pkg, dev, rng.random((3, 16, 16), dtype=np.float32), er.orientation_tilted())
    g = _dev((rng.random((scene["h"], scene["w"], 3), dtype=np.float32) - np.float32(0.5)), dev)
    B = env.sample(cam)
    fused = pkg.composite_environment(out, cam, env)
    fused_back = pkg.composite_environment_backward(g, out, cam, env)
    image = pkg.composite_background(out.color, out.final_T, B)
    d_alpha, d_bg = pkg.composite_background_backward(g, out.final_T, B)
    assert np_(image).tobytes() == np_(fused).tobytes()
    assert np_(d_alpha).tobytes() == np_(fused_back.dL_dalpha).tobytes()
    assert np_(d_bg).tobytes() == (np_(out.final_T)[..., None] * np_(g)).tobytes()          # T g, one float32 product
    d_alpha2, none = pkg.composite_background_backward(g, out.final_T, B, want_background_grad=False)
    assert none is None and np_(d_alpha2).tobytes() == np_(d_alpha).tobytes()


def test_errors(pkg, dev, scene):
    model, cam, out = scene["model"], scene["cam"], scene["out"]
    env = pkg.EnvironmentMap(resolution=8, device=dev)
    grey = pkg.RenderSettings(background=[0.0, 0.5, 0.0], active_sh_degree=1)
    g = torch.zeros((scene["h"], scene["w"], 3), device=dev)
    with pytest.raises(RuntimeError, match="background"):
        pkg.render_with_environment(model, cam, grey, env)
    with pytest.raises(RuntimeError, match="background"):
        pkg.composite_environment(out, cam, env, settings=grey)
    with pytest.raises(RuntimeError, match="background"):
        pkg.composite_environment_backward(g, out, cam, env, settings=grey)
    # a RenderOutput without the route that carries dL_dalpha through render_backward
    bare = dataclasses.replace(out, depths=None)
    with pytest.raises(RuntimeError, match="dL_dalpha"):
        pkg.composite_environment_backward(g, bare, cam, env)
    for r in (24, 2, 4096, 0):
        with pytest.raises(RuntimeError, match="power of two"):
            pkg.EnvironmentMap(resolution=r, device=dev)
    env.texture = torch.zeros((3, 24, 24), device=dev)
    with pytest.raises(RuntimeError, match="power of two"):
        pkg.composite_environment(out, cam, env)
    env = pkg.EnvironmentMap(resolution=8, device=dev)
    with pytest.raises(ValueError):
        pkg.composite_environment_backward(g, out, cam, env, grad_bound=0.0)
    with pytest.raises(RuntimeError):
        pkg.composite_environment(out, pkg.scene.make_camera(32, 32), env)                  # another image size
    with pytest.raises(RuntimeError):
        pkg.composite_background(out.color, out.final_T, torch.zeros((4, 4, 3), device=dev))
    with pytest.raises(RuntimeError):
        pkg.EnvironmentMap(resolution=8, device=dev).step(torch.zeros((3, 4, 4), device=dev), 0)


def test_fitting_the_map_lowers_the_loss_and_leaves_unseen_texels_alone(pkg, dev, scene, tmp_path):
    cam, out = scene["cam"], scene["out"]
    h, w, res = scene["h"], scene["w"], 16
    init = (0.2, 0.5, 0.7)
    env = pkg.EnvironmentMap(resolution=res, device=dev, init_color=init, lr_init=0.05, lr_final=0.05, max_steps=50)
    before = np_(env.texture).copy()
    rng = np.random.default_rng(9)
    sky = _env(pkg, dev, rng.random((3, res, res), dtype=np.float32))
    target = pkg.composite_environment(out, cam, sky)                   # a fixed target: the same render under another sky
    losses = []
    for step in range(50):
        image = pkg.composite_environment(out, cam, env)
        diff = image - target
        losses.append(float((diff * diff).sum()))
        back = pkg.composite_environment_backward(2.0 * diff, out, cam, env, grad_bound=2.0)       # |I - target| <= 1
        env.step(back.dL_denv, step)
    assert int(back.clamped) == 0
    print(f"squared error: {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < losses[0]
    after = np_(env.texture)
    K = cam.intrinsics
    taps = er.taps32(dict(R=cam.rotation, fx=K.fx, fy=K.fy, cx=K.cx, cy=K.cy, width=w, height=h), res)
    reached = np.zeros(res * res, bool)
    reached[taps[0].reshape(-1)] = True
    reached = reached.reshape(res, res)
    assert 8 < reached.sum() < res * res - 8
    assert after[:, ~reached].tobytes() == before[:, ~reached].tobytes()                       # the initial bits
    assert (after[:, reached] != before[:, reached]).any()
    # save / load: the texture and the orientation, bit for bit
    env.orientation[:] = er.orientation_tilted()
    path = tmp_path / "sky.npz"
    env.save(path)
    loaded = pkg.EnvironmentMap.load(path, dev)
    assert np_(loaded.texture).tobytes() == after.tobytes() and loaded.orientation.tobytes() == env.orientation.tobytes()
    assert loaded.resolution == res and loaded.steps_ == 0
