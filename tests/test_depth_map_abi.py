"""The depth options of cugs_rasterize_forward_opts / cugs_rasterize_backward_opts: argument validation that fails
before anything touches the device (no GPU needed): CUGS_EINVAL (-1) for a missing depth input or output and for
partial reference-layout outputs, 0 for the empty no-op."""
import ctypes as C

EINVAL = -1
FAKE = C.c_void_p(1 << 20)            # 64-byte aligned, never dereferenced on these paths
NUL = C.c_void_p(0)
BG = (C.c_float * 3)(0.0, 0.0, 0.0)


def _fwd(lib, depths, out_depth, w=32, h=32, indices=FAKE):
    from cugs_amd._lib import BlendForwardOpts
    opts = BlendForwardOpts(depths=depths, out_depth=out_depth)
    return lib.cugs_rasterize_forward_opts(w, h, BG, FAKE, indices, NUL, NUL, NUL, NUL, FAKE, FAKE, FAKE, FAKE,
                                           C.byref(opts), NUL)


def _bwd(lib, soa, d_depths, depths=FAKE, n=10):
    a = FAKE if soa >= 1 else NUL
    b = FAKE if soa >= 2 else NUL
    c = FAKE if soa >= 3 else NUL
    d = FAKE if soa >= 4 else NUL
    from cugs_amd._lib import BlendBackwardOpts
    # prezeroed = 1: no fill is queued before the checks
    opts = BlendBackwardOpts(prezeroed=1, depths=depths, dL_ddepth_map=FAKE, dL_dalpha=FAKE, dL_ddepths=d_depths)
    return lib.cugs_rasterize_backward_opts(32, 32, BG, FAKE, FAKE, NUL, NUL, NUL, NUL, FAKE, FAKE, FAKE, FAKE, n, FAKE,
                                            a, b, c, d, C.byref(opts), NUL)


def test_depth_map_symbols_bound(pkg):
    from cugs_amd import _lib
    for name in ("cugs_rasterize_forward_opts", "cugs_rasterize_backward_opts"):
        assert name in _lib.SIGNATURES
        assert getattr(C.CDLL(pkg.LIB_PATH), name)


def test_forward_depth_needs_its_inputs_and_output(pkg):
    from cugs_amd._lib import lib
    assert _fwd(lib, NUL, FAKE) == EINVAL                # pairs to blend but no depths
    assert _fwd(lib, FAKE, NUL) == EINVAL                # no depth map to write
    assert _fwd(lib, FAKE, NUL, w=0, h=0) == 0           # empty image: nothing to draw, nothing required


def test_backward_depth_reference_outputs_come_all_or_none(pkg):
    from cugs_amd._lib import lib
    assert _bwd(lib, 2, FAKE) == EINVAL                  # partial SoA outputs
    assert _bwd(lib, 4, NUL) == EINVAL                   # the four without dL_ddepths
    assert _bwd(lib, 0, FAKE) == EINVAL                  # dL_ddepths without the four
    assert _bwd(lib, 0, NUL, depths=NUL) == EINVAL       # pairs to replay but no depths
    assert _bwd(lib, 0, NUL, n=0) == 0                   # n == 0 is a no-op
