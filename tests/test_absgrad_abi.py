"""cugs_rasterize_backward_opts with abs_grad / cugs_densify_accumulate_strided: argument validation that fails before
anything touches the device (no GPU needed)."""
import ctypes as C

EINVAL, EALIGN = -1, -2
FAKE = C.c_void_p(1 << 20)            # 64-byte aligned, never dereferenced on these paths
NUL = C.c_void_p(0)
BG = (C.c_float * 3)(0.0, 0.0, 0.0)


def _bwd(lib, soa, d_abs, d_depths=NUL, depths=NUL, dD=NUL, dA=NUL, n=10):
    a = FAKE if soa >= 1 else NUL
    b = FAKE if soa >= 2 else NUL
    c = FAKE if soa >= 3 else NUL
    d = FAKE if soa >= 4 else NUL
    from cugs_amd._lib import BlendBackwardOpts
    # prezeroed = 1: no fill is queued before the checks
    opts = BlendBackwardOpts(prezeroed=1, abs_grad=1, depths=depths, dL_ddepth_map=dD, dL_dalpha=dA, dL_ddepths=d_depths,
                             dL_dmeans_2d_abs=d_abs)
    return lib.cugs_rasterize_backward_opts(32, 32, BG, FAKE, FAKE, NUL, NUL, NUL, NUL, FAKE, FAKE, FAKE, FAKE, n, FAKE,
                                            a, b, c, d, C.byref(opts), NUL)


def test_absgrad_symbols_bound(pkg):
    from cugs_amd import _lib
    for name in ("cugs_rasterize_backward_opts", "cugs_densify_accumulate_strided"):
        assert name in _lib.SIGNATURES
        assert getattr(C.CDLL(pkg.LIB_PATH), name)


def test_backward_abs_outputs_come_with_the_four_or_not_at_all(pkg):
    from cugs_amd._lib import lib
    assert _bwd(lib, 4, NUL) == EINVAL                                   # the four without dL_dmeans_2d_abs
    assert _bwd(lib, 0, FAKE) == EINVAL                                  # dL_dmeans_2d_abs without the four
    assert _bwd(lib, 2, FAKE) == EINVAL                                  # partial SoA outputs
    assert _bwd(lib, 4, FAKE, d_depths=FAKE) == EINVAL                   # dL_ddepths on the colour-only route
    # the depth route keeps the depth entry's rules
    assert _bwd(lib, 4, FAKE, d_depths=NUL, depths=FAKE, dD=FAKE) == EINVAL     # the four without dL_ddepths
    assert _bwd(lib, 4, NUL, d_depths=FAKE, depths=FAKE, dD=FAKE) == EINVAL     # ... without dL_dmeans_2d_abs
    assert _bwd(lib, 0, NUL, depths=NUL, dA=FAKE) == EINVAL              # a map gradient but no depths
    assert _bwd(lib, 0, NUL, n=0) == 0 and _bwd(lib, 4, NUL, n=0) == 0   # n == 0 is a no-op
    assert _bwd(lib, 0, NUL, n=-1) == EINVAL


def test_strided_accumulate_checks_its_stride(pkg):
    from cugs_amd._lib import lib
    acc = lambda n, stride, base=FAKE: lib.cugs_densify_accumulate_strided(n, base, stride, FAKE, FAKE, FAKE, FAKE, NUL)
    assert acc(10, 1) == EINVAL and acc(10, 0) == EINVAL and acc(10, -16) == EINVAL
    assert acc(0, 1) == EINVAL                                           # also for an empty model
    assert acc(0, 2) == 0 and acc(0, 16) == 0
    assert acc(-1, 2) == EINVAL
    assert acc(10, 16, NUL) == EINVAL
    assert acc(10, 3) == EALIGN                                          # each pair is read as one 8-byte word
    assert acc(10, 16, C.c_void_p((1 << 20) + 4)) == EALIGN
