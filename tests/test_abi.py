"""The C-ABI shared library loads without a GPU, exports every function include/cugs_hip.h declares,
and rejects bad arguments with its negative error codes (no compute calls here)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "cugs_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cugs_[a-z_0-9]+)\s*\(", text)))


def test_header_functions_all_exported_and_bound(pkg):
    names = _declared()
    assert len(names) >= 16
    lib = C.CDLL(pkg.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/cugs_hip.h but not exported"
    from cugs_amd import _lib
    assert sorted(_lib.SIGNATURES) == names            # the ctypes table covers exactly the header


def test_version_and_error_strings(pkg):
    from cugs_amd._lib import lib
    assert "gfx950" in pkg.version()
    assert lib.cugs_error_string(0) == b"success"
    for code in (-1, -2, -3, -4):
        assert lib.cugs_error_string(code).startswith(b"cugs:")


def test_argument_validation_without_gpu(pkg):
    from cugs_amd._lib import lib, Camera
    cam = Camera()
    null = C.c_void_p(0)
    # degree out of range / too few coefficients / unsupported coefficient count -> CUGS_EINVAL
    args = lambda n, c, d: (n, c, d, null, null, null, null, null, C.byref(cam), 1.0, null, null, null, null, null,
                            null, null, null, null, null)
    assert lib.cugs_project_forward(*args(10, 16, 4)) == -1
    assert lib.cugs_project_forward(*args(10, 4, 2)) == -1
    assert lib.cugs_project_forward(*args(10, 5, 1)) == -1
    assert lib.cugs_project_forward(*args(10, 16, 3)) == -1          # null pointers with n > 0
    assert lib.cugs_project_forward(*args(0, 16, 3)) == 0            # n == 0: nothing to do
    # the keyed variant: a sort workspace is mandatory, and the same argument checks apply before it is touched
    assert lib.cugs_project_forward_keyed(*args(0, 16, 3)[:-1], null, 0, null) == -1
    assert lib.cugs_project_forward_keyed(*args(10, 16, 4)[:-1], C.c_void_p(0x1000), 1 << 20, null) == -1
    assert lib.cugs_project_forward_keyed(*args(0, 16, 3)[:-1], C.c_void_p(0x1000), 1 << 20, null) == 0
    assert lib.cugs_sort_pairs_predicted_keyed(-1, 0, null, null, null, null, 16, 16, null, 0, null, 0, null, null, null,
                                               None, null) == -1
    assert lib.cugs_sort_pairs_predicted_wide(-1, 0, null, null, null, null, 16, 16, null, 0, null, 0, null, null, null,
                                              None, null) == -1
    total = C.c_int64(7)
    assert lib.cugs_sort_count_pairs_wide(0, null, null, null, null, 16, 16, null, 0, C.byref(total), null) == 0
    assert total.value == 0                                          # n == 0: nothing queued, count 0
    assert lib.cugs_sort_count_pairs_wide(5, null, null, null, null, 16, 16, null, 0, C.byref(total), null) == -1
    assert lib.cugs_evaluate_sh(5, 1, 16, null, null, null, null) == -1
    assert lib.cugs_evaluate_sh(2, 1, 4, null, null, null, null) == -1
    assert lib.cugs_evaluate_sh(1, 0, 4, null, null, null, null) == 0
    assert lib.cugs_fused_adam(null, null, null, null, 0, 0.1, 0.9, 0.999, 1e-15, 1.0, 1.0, null) == 0
    assert lib.cugs_fused_adam(null, null, null, null, 8, 0.1, 0.9, 0.999, 1e-15, 1.0, 1.0, null) == -1
    assert lib.cugs_sort_workspace_bytes(-1) == 0 and lib.cugs_sort_pair_workspace_bytes(-1) == 0
    assert 0 < lib.cugs_sort_workspace_bytes(1000) < lib.cugs_sort_workspace_bytes(100000)
    assert 0 < lib.cugs_sort_pair_workspace_bytes(10) < lib.cugs_sort_pair_workspace_bytes(5000)
    # misaligned accumulator -> CUGS_EALIGN
    bg = (C.c_float * 3)(0, 0, 0)
    assert lib.cugs_rasterize_backward(16, 16, bg, null, null, null, null, null, null, null, null, null, null, 4,
                                       C.c_void_p(0x1004), null, null, null, null, null) == -2
    # the same through the entry with options: none (NULL), then a misaligned tile_order in them
    assert lib.cugs_rasterize_backward_opts(16, 16, bg, null, null, null, null, null, null, null, null, null, null, 4,
                                            C.c_void_p(0x1004), null, null, null, null, None, null) == -2
    from cugs_amd._lib import BlendBackwardOpts
    opts = BlendBackwardOpts(prezeroed=1, tile_order=0x2004)
    assert lib.cugs_rasterize_backward_opts(16, 16, bg, null, null, null, null, null, null, null, null, null, null, 4,
                                            C.c_void_p(0x1000), null, null, null, null, C.byref(opts), null) == -2   # CUGS_EALIGN
    # the gated colour gradient on its own (data-parallel early gather)
    assert lib.cugs_gated_colour_grad(-1, null, null, null, null) == -1
    assert lib.cugs_gated_colour_grad(0, null, null, null, null) == 0
    assert lib.cugs_gated_colour_grad(4, null, null, null, null) == -1
    assert lib.cugs_gated_colour_grad(4, C.c_void_p(0x1004), C.c_void_p(0x2000), C.c_void_p(0x3000), null) == -2


def test_bias_correction_matches_oracle(pkg, orc):
    from cugs_amd._lib import lib
    for step in (1, 2, 10, 1000, 30000):
        a, b = C.c_float(), C.c_float()
        lib.cugs_adam_bias_correction(0.9, 0.999, step, C.byref(a), C.byref(b))
        assert (a.value, b.value) == orc.adam_bias_correction(0.9, 0.999, step)


def test_missing_library_fails_loudly(pkg, tmp_path, monkeypatch):
    """No fallback: with the .so absent the product package refuses to import."""
    import importlib.util
    import sys
    from cugs_amd import _lib
    src = os.path.dirname(_lib.__file__)
    dst = tmp_path / "pkgcopy"
    dst.mkdir()
    for f in ("_lib.py",):
        (dst / f).write_text(open(os.path.join(src, f)).read())
    spec = importlib.util.spec_from_file_location("cugs_lib_copy", str(dst / "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    with pytest.raises(ImportError, match="no fallback"):
        spec.loader.exec_module(mod)
    sys.modules.pop("cugs_lib_copy", None)


def test_release_library_has_no_debug_surface(pkg):
    """the shipped library exports exactly the declared C ABI (no cugsdbg_* hooks), never reads
    the environment (no getenv import), and so cannot be switched into a timing/ablation mode by a stray variable."""
    import subprocess
    if os.environ.get("CUGS_HIP_LIBRARY"):
        pytest.skip("a non-default library is loaded")
    exported = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    funcs = sorted(l.split()[-1] for l in exported.splitlines() if " T " in l)
    assert funcs == _declared(), set(funcs) ^ set(_declared())
    undefined = subprocess.run(["nm", "-D", "--undefined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in undefined
