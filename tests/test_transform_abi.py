"""cugs_similarity_init / cugs_transform_gaussians (include/cugs_hip.h): the symbols, and the argument checks that fail -
or succeed with nothing to do - before anything touches the device (no GPU needed)."""
import ctypes as C
import math

import numpy as np

EINVAL, EALIGN = -1, -2
FAKE = C.c_void_p(1 << 20)            # 64-byte aligned, never dereferenced on these paths
OFF4 = C.c_void_p((1 << 20) + 4)      # dword aligned
OFF2 = C.c_void_p((1 << 20) + 2)      # not dword aligned
NUL = C.c_void_p(0)


def _init(lib, R, t=(0.0, 0.0, 0.0), s=1.0):
    from cugs_amd._lib import Similarity
    out = Similarity()
    Ra = (C.c_double * 9)(*np.asarray(R, dtype=np.float64).reshape(9))
    ta = (C.c_double * 3)(*t)
    return lib.cugs_similarity_init(C.byref(out), Ra, ta, s), out


def _call(lib, n=10, coeffs=16, pos=FAKE, rot=FAKE, scl=FAKE, sh=FAKE, mask=NUL, zero=None, floats=None, num_zero=0,
          xf="identity"):
    if xf == "identity":
        code, xf = _init(lib, np.eye(3))
        assert code == 0
    return lib.cugs_transform_gaussians(n, coeffs, pos, rot, scl, sh, mask, zero, floats, num_zero,
                                        None if xf is None else C.byref(xf), NUL)


def test_transform_symbols_bound_and_exported(pkg):
    from cugs_amd import _lib
    so = C.CDLL(pkg.LIB_PATH)
    for name in ("cugs_similarity_init", "cugs_transform_gaussians"):
        assert name in _lib.SIGNATURES and getattr(so, name)
    assert C.sizeof(_lib.Similarity) == 4 * (9 + 3 + 1 + 4 + 9 + 25 + 49 + 1)
    for name in ("Similarity", "sh_rotation_matrices", "transform_gaussians", "transform_camera", "transform_cameras",
                 "similarity_from_cameras", "merge_gaussians"):
        assert hasattr(pkg, name), name


def test_similarity_init_rejects_what_is_no_similarity(pkg):
    from cugs_amd._lib import lib
    eye = np.eye(3)
    assert _init(lib, eye)[0] == 0
    assert _init(lib, np.diag([1.0, 1.0, -1.0]))[0] == EINVAL                       # a reflection
    assert _init(lib, -eye)[0] == EINVAL
    shear = eye.copy()
    shear[0, 1] = 0.01
    assert _init(lib, shear)[0] == EINVAL
    assert _init(lib, 1.001 * eye)[0] == EINVAL                                     # a scale hidden in the rotation
    for s in (0.0, -1.0, math.nan, math.inf):
        assert _init(lib, eye, s=s)[0] == EINVAL
    bad = eye.copy()
    bad[1, 2] = math.nan
    assert _init(lib, bad)[0] == EINVAL
    assert _init(lib, eye, t=(0.0, math.inf, 0.0))[0] == EINVAL
    assert lib.cugs_similarity_init(None, (C.c_double * 9)(), (C.c_double * 3)(), 1.0) == EINVAL


def test_similarity_init_reorthonormalises_a_nearby_matrix(pkg):
    from cugs_amd._lib import lib
    import transform_ref as tr
    R = tr.random_rotation(3)
    off = R + 1e-6 * np.array([[0.3, -1.0, 0.5], [0.8, 0.1, -0.6], [-0.2, 0.7, 1.0]])
    code, xf = _init(lib, off, s=2.0)
    assert code == 0
    f = tr.abi_matrices(xf)
    u, _, vt = np.linalg.svd(off)
    near = u @ vt                                                                   # the nearest rotation
    assert np.max(np.abs(f["m"].astype(np.float64) / 2.0 - near)) <= 2.0 ** -23
    assert np.max(np.abs(f["m"].astype(np.float64) / 2.0 - off)) > 2e-7             # not the input as given
    for D, want in zip(f["d"], tr.fit_sh_rotation(near)):
        assert np.max(np.abs(D.astype(np.float64) - want)) <= 2.0 ** -23
        assert np.max(np.abs(D.astype(np.float64) @ D.astype(np.float64).T - np.eye(D.shape[0]))) <= 1e-6


def test_transform_rejects_bad_arguments(pkg):
    from cugs_amd._lib import lib
    assert _call(lib, n=-1) == EINVAL
    for c in (0, 2, 3, 5, 8, 15, 17, 25, -1):
        assert _call(lib, coeffs=c) == EINVAL and _call(lib, coeffs=c, n=0) == EINVAL
    assert _call(lib, xf=None) == EINVAL and _call(lib, xf=None, n=0) == EINVAL
    for k in ("pos", "rot", "scl", "sh"):
        assert _call(lib, **{k: NUL}) == EINVAL
    ptrs, floats = (C.c_void_p * 2)(1 << 20, 1 << 21), (C.c_int * 2)(3, 48)
    assert _call(lib, zero=ptrs, floats=floats, num_zero=9) == EINVAL and _call(lib, num_zero=-1) == EINVAL
    assert _call(lib, zero=None, floats=floats, num_zero=2) == EINVAL
    assert _call(lib, zero=ptrs, floats=None, num_zero=2) == EINVAL
    assert _call(lib, zero=ptrs, floats=(C.c_int * 2)(3, 0), num_zero=2) == EINVAL
    assert _call(lib, zero=(C.c_void_p * 2)(1 << 20, 0), floats=floats, num_zero=2) == EINVAL


def test_transform_checks_dword_alignment(pkg):
    from cugs_amd._lib import lib
    for k in ("pos", "rot", "scl", "sh"):
        assert _call(lib, **{k: OFF2}) == EALIGN
        assert _call(lib, n=0, **{k: OFF2}) == EALIGN
    ptrs, floats = (C.c_void_p * 2)(1 << 20, (1 << 21) + 1), (C.c_int * 2)(3, 48)
    assert _call(lib, n=0, zero=ptrs, floats=floats, num_zero=2) == EALIGN
    assert _call(lib, n=-1, pos=OFF2) == EINVAL                                      # the arguments come first


def test_transform_of_nothing_touches_nothing(pkg):
    from cugs_amd._lib import lib
    for c in (1, 4, 9, 16):
        assert _call(lib, n=0, coeffs=c) == 0
    assert _call(lib, n=0, pos=OFF4, rot=OFF4, scl=OFF4, sh=OFF4, mask=FAKE) == 0   # dword-aligned views are fine
    assert _call(lib, n=0, pos=NUL, rot=NUL, scl=NUL, sh=NUL) == 0
    ptrs, floats = (C.c_void_p * 2)(1 << 20, 1 << 21), (C.c_int * 2)(3, 48)
    assert _call(lib, n=0, zero=ptrs, floats=floats, num_zero=2) == 0
