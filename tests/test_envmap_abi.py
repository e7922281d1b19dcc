"""cugs_envmap_* (include/cugs_hip.h): the header, the ctypes table and the C++ adapter declare the same surface, and the
argument checks fail - or succeed with nothing to do - before anything touches the device (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, EOVERFLOW, EWORKSPACE = -1, -2, -3, -4
NAMES = ("cugs_envmap_view_init", "cugs_envmap_workspace_bytes", "cugs_envmap_frac_bits", "cugs_envmap_composite",
         "cugs_envmap_composite_backward")
NUL = C.c_void_p(0)
P = lambda k: C.c_void_p((k + 1) << 20)                # aligned, never dereferenced on these paths
OFF2 = C.c_void_p((1 << 20) + 2)                       # not dword aligned
OFF4 = C.c_void_p((1 << 20) + 4)                       # dword aligned, not 8-byte aligned


def _header_block():
    text = open(os.path.join(ROOT, "include", "cugs_hip.h")).read()
    start = text.index("typedef struct cugs_envmap_view")
    return text[start:text.index("/* Device properties", start)]


def test_header_ctypes_and_adapter_declare_the_same_surface(pkg):
    from cugs_amd import _lib
    so = C.CDLL(pkg.LIB_PATH)
    block = re.sub(r"/\*.*?\*/", "", _header_block(), flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and getattr(so, name)
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", block)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name       # the argument counts agree
    # the struct: nine floats, four floats, three int32 - 64 bytes on both sides
    fields = re.search(r"typedef struct cugs_envmap_view \{(.*?)\} cugs_envmap_view;", block, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", fields).strip() == "float m[9]; float fx, fy, cx, cy; int32_t width, height, resolution;"
    assert [f[0] for f in _lib.EnvmapView._fields_] == ["m", "fx", "fy", "cx", "cy", "width", "height", "resolution"]
    assert C.sizeof(_lib.EnvmapView) == 64
    for name in ("EnvironmentMap", "EnvGrad", "composite_environment", "composite_environment_backward",
                 "composite_background", "composite_background_backward", "render_with_environment", "envmap_frac_bits"):
        assert hasattr(pkg, name), name
    adapter = os.path.join(ROOT, "cuda-gaussian-splatting_amd", "adapter")
    hpp = open(os.path.join(adapter, "cugs_hip_torch.hpp")).read()
    for name in ("class EnvironmentMap", "struct EnvGrad", "composite_environment(", "composite_environment_backward(",
                 "composite_background(", "composite_background_backward(", "render_with_environment("):
        assert name in hpp, name
    cpp = open(os.path.join(adapter, "torch_envmap.cpp")).read()
    for name in NAMES[:1] + NAMES[3:] + ("cugs_envmap_workspace_bytes",):
        assert name in cpp, name
    make = open(os.path.join(adapter, "Makefile")).read()
    assert len(re.findall(r"\benvmap_driver\b", make)) == 1 and "torch_envmap" in make


def _view(pkg, w=33, h=17, res=16, fx=20.0, fy=18.0, cx=16.5, cy=8.5, m=None):
    from cugs_amd._lib import EnvmapView
    v = EnvmapView()
    for i, x in enumerate(np.eye(3).reshape(-1) if m is None else m):
        v.m[i] = float(x)
    v.fx, v.fy, v.cx, v.cy, v.width, v.height, v.resolution = fx, fy, cx, cy, w, h, res
    return v


def test_workspace_and_frac_bits(pkg):
    from cugs_amd._lib import lib
    for r in (0, -4, 2, 3, 24, 100, 4096, 2049):
        assert lib.cugs_envmap_workspace_bytes(r) == 0
    for r in (4, 8, 256, 2048):
        assert lib.cugs_envmap_workspace_bytes(r) == 8 * 3 * r * r
    import envmap_ref as er
    for h, w, bound in ((17, 33, 1.0), (48, 64, 0.3), (1080, 1920, 1.0), (1080, 1920, 4.0 / (3 * 1080 * 1920)),
                        (17, 33, 0.5), (17, 33, 2.0 ** -60), (17, 33, 2.0 ** 24), (1, 1, 3.0)):
        assert lib.cugs_envmap_frac_bits(w, h, bound) == er.frac_bits(h, w, bound)[0] == pkg.envmap_frac_bits(h, w, bound)
    assert lib.cugs_envmap_frac_bits(1920, 1080, 1.0) == 38
    for bound in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** -61, 2.0 ** 24 * 1.5):
        assert lib.cugs_envmap_frac_bits(33, 17, bound) == EINVAL
        with pytest.raises(ValueError):
            pkg.envmap_frac_bits(17, 33, bound)
    assert lib.cugs_envmap_frac_bits(0, 17, 1.0) == EINVAL and lib.cugs_envmap_frac_bits(65536, 65536, 1.0) == EOVERFLOW


def test_view_init_forms_the_matrix_in_fp64(pkg):
    from cugs_amd._lib import Camera, EnvmapView, lib
    import envmap_ref as er
    cam_d = er.cameras(17, 33)["oblique"]
    cam = pkg.CameraInfo(width=33, height=17, rotation=cam_d["R"],
                         intrinsics=pkg.CameraIntrinsics(cam_d["fx"], cam_d["fy"], cam_d["cx"], cam_d["cy"])).to_abi()
    for orient in (None, er.orientation_tilted(), er.UP_MINUS_Y):
        v = EnvmapView()
        o = None if orient is None else np.ascontiguousarray(orient).ctypes.data_as(C.POINTER(C.c_double))
        assert lib.cugs_envmap_view_init(C.byref(v), C.byref(cam), o, 16) == 0
        assert np.array(list(v.m), np.float32).tobytes() == er.view_matrix(cam_d["R"], orient).tobytes()
        assert (v.width, v.height, v.resolution) == (33, 17, 16) and v.fx == np.float32(cam_d["fx"])
    v = EnvmapView()
    assert lib.cugs_envmap_view_init(None, C.byref(cam), None, 16) == EINVAL
    assert lib.cugs_envmap_view_init(C.byref(v), None, None, 16) == EINVAL
    for r in (24, 2, 4096, 0):
        assert lib.cugs_envmap_view_init(C.byref(v), C.byref(cam), None, r) == EINVAL
    bad = (C.c_double * 9)(*([1.0] * 8 + [float("nan")]))
    assert lib.cugs_envmap_view_init(C.byref(v), C.byref(cam), bad, 16) == EINVAL
    empty = Camera()                                                      # fx = 0, no size
    assert lib.cugs_envmap_view_init(C.byref(v), C.byref(empty), None, 16) == EINVAL


def test_composite_rejects_bad_arguments(pkg):
    from cugs_amd._lib import lib
    fwd = lib.cugs_envmap_composite
    ok = _view(pkg)
    E, bg, c, t, img, smp = (P(k) for k in range(6))
    assert fwd(None, E, NUL, c, t, img, NUL, NUL) == EINVAL
    assert fwd(C.byref(ok), NUL, NUL, c, t, img, NUL, NUL) == EINVAL              # neither a map nor an image
    assert fwd(C.byref(ok), E, bg, c, t, img, NUL, NUL) == EINVAL                 # both
    assert fwd(C.byref(ok), E, NUL, c, t, NUL, NUL, NUL) == EINVAL                # nothing to write
    assert fwd(C.byref(ok), E, NUL, NUL, t, img, NUL, NUL) == EINVAL
    assert fwd(C.byref(ok), E, NUL, c, NUL, img, NUL, NUL) == EINVAL
    assert fwd(C.byref(ok), NUL, bg, c, t, img, smp, NUL) == EINVAL               # the image route has no sample
    for kw in (dict(res=24), dict(res=2), dict(res=4096), dict(w=0), dict(h=-1), dict(fx=0.0), dict(fy=float("inf")),
               dict(cx=float("nan")), dict(cy=float("inf")), dict(m=[1, 0, 0, 0, 1, 0, 0, 0, float("nan")])):
        assert fwd(C.byref(_view(pkg, **kw)), E, NUL, c, t, img, NUL, NUL) == EINVAL, kw
    # the image route reads the size only
    assert fwd(C.byref(_view(pkg, res=0, fx=0.0, w=0)), NUL, bg, c, t, img, NUL, NUL) == EINVAL
    assert fwd(C.byref(_view(pkg, w=65536, h=65536)), E, NUL, c, t, img, NUL, NUL) == EOVERFLOW
    assert fwd(C.byref(_view(pkg, w=65536, h=65536, res=0, fx=0.0)), NUL, bg, c, t, img, NUL, NUL) == EOVERFLOW
    for k in range(5):
        args = [E, NUL, c, t, img, smp]
        args[k if k < 1 else k + 1] = OFF2
        assert fwd(C.byref(ok), *args, NUL) == EALIGN, k


def test_composite_backward_rejects_bad_arguments(pkg):
    from cugs_amd._lib import lib
    bwd = lib.cugs_envmap_composite_backward
    ok = _view(pkg)
    E, bg, g, t, ws, da, de, db, fl = (P(k) for k in range(9))
    need = lib.cugs_envmap_workspace_bytes(16)
    call = lambda view=ok, env=E, back=NUL, grad=g, T=t, bound=1.0, w=ws, size=need, a=da, e=de, b=NUL, f=fl: \
        bwd(C.byref(view), env, back, grad, T, bound, w, size, a, e, b, f, NUL)
    assert call(env=NUL) == EINVAL and call(back=bg) == EINVAL
    assert call(grad=NUL) == EINVAL and call(T=NUL) == EINVAL and call(w=NUL) == EINVAL and call(f=NUL) == EINVAL
    assert call(b=db) == EINVAL                                                   # the map route has no image gradient
    assert call(env=NUL, back=bg, e=de, b=db) == EINVAL                           # and the other way round
    for bound in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** -61, 2.0 ** 25):
        assert call(bound=bound) == EINVAL
    assert call(view=_view(pkg, res=24)) == EINVAL
    # the order: arguments, then the size, then the workspace, then the alignment
    assert call(view=_view(pkg, w=65536, h=65536), size=0) == EOVERFLOW
    assert call(size=need - 1) == EWORKSPACE and call(size=need - 1, grad=NUL) == EINVAL
    assert call(size=need - 1, a=OFF2) == EWORKSPACE
    for key in ("env", "grad", "T", "a", "e", "f"):
        assert call(**{key: OFF2}) == EALIGN, key
    assert call(w=OFF4) == EALIGN
    # without the map gradient neither the workspace, the flag nor the bound is looked at
    assert call(e=NUL, a=NUL, w=NUL, size=0, f=NUL, bound=float("nan"), T=NUL) == 0          # nothing to do
    # the image route
    img = lambda **kw: call(**dict(dict(env=NUL, back=bg, e=NUL, w=NUL, size=0, f=NUL), **kw))
    assert img(a=NUL, b=NUL) == 0
    assert img(b=db, T=NUL) == EINVAL and img(b=OFF2) == EALIGN and img(back=OFF2, b=db) == EALIGN
    assert img(view=_view(pkg, res=0, fx=0.0), a=NUL, b=NUL) == 0
