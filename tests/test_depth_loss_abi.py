"""cugs_depth_loss_workspace_bytes / cugs_depth_loss (include/cugs_hip.h): the workspace size and the argument checks,
through ctypes with null or never-dereferenced pointers - every call here returns before anything is queued.  No GPU."""
import ctypes as C

EINVAL, EOVERFLOW, EWORKSPACE = -1, -3, -4


def test_depth_loss_workspace_bytes(pkg):
    from cugs_amd._lib import lib
    size = lib.cugs_depth_loss_workspace_bytes
    assert size(-1, 4) == 0 and size(4, -1) == 0 and size(-1, -1) == 0
    for w, h in ((5, 7), (16, 16), (53, 37), (500, 540), (1920, 1080)):
        rows = -(-w * h // 1024)
        assert size(w, h) % 256 == 0
        assert size(w, h) >= (6 + 3) * 8 * rows                            # six fit sums and three loss sums, fp64
    # grows with the number of partials, not with the shape: the image is a flat run of pixels
    assert size(1024, 1) == size(32, 32) == size(1, 1024)
    assert size(16, 16) <= size(64, 64) < size(500, 540) < size(1920, 1080)     # 1, 4, 264, 2025 rows, each part
    assert size(1920, 1080) - size(500, 540) >= (6 + 3) * 8 * (2025 - 264) - 512   # rounded up to 256 bytes
    assert size(1920, 1080) < 1 << 18                                       # and stays small: no per-pixel scratch


def test_depth_loss_argument_validation(pkg):
    from cugs_amd._lib import DepthLossOpts, lib
    null = C.c_void_p(0)
    p = lambda a: C.c_void_p(a)                                             # never dereferenced: the checks come first
    d, a, t, ws, out, gd, ga = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000), p(0x6000), p(0x7000)
    big = 1 << 20
    call = lib.cugs_depth_loss

    def opts(**kw):
        kw.setdefault("min_alpha", 1e-3)
        return C.byref(DepthLossOpts(**kw))

    variants = [opts(), opts(weight=0x8000, inverse=1, expected=0x9000), opts(fit=1), opts(scale_shift=0xA000)]
    for o in variants:
        for w, h in ((0, 16), (16, 0), (-1, 16), (16, -1)):                 # non-positive size
            assert call(w, h, d, a, t, o, ws, big, out, gd, ga, null) == EINVAL
        assert call(16, 16, null, a, t, o, ws, big, out, gd, ga, null) == EINVAL      # null maps
        assert call(16, 16, d, null, t, o, ws, big, out, gd, ga, null) == EINVAL
        assert call(16, 16, d, a, null, o, ws, big, out, gd, ga, null) == EINVAL
        assert call(16, 16, d, a, t, o, null, big, out, gd, ga, null) == EINVAL       # null workspace
        assert call(16, 16, d, a, t, o, ws, big, null, gd, ga, null) == EINVAL        # null loss_out
        assert call(16, 16, d, a, t, o, ws, 0, out, gd, ga, null) == EWORKSPACE       # short workspace
        need = lib.cugs_depth_loss_workspace_bytes(16, 16)
        assert call(16, 16, d, a, t, o, ws, need - 1, out, gd, ga, null) == EWORKSPACE
    assert call(16, 16, d, a, t, None, ws, big, out, gd, ga, null) == EINVAL          # null opts
    for bad in (0.0, -1e-3, float("inf"), float("nan"), -float("inf")):               # min_alpha > 0 and finite
        assert call(16, 16, d, a, t, opts(min_alpha=bad), ws, big, out, gd, ga, null) == EINVAL
    # a fit and a given (s, b) exclude each other
    assert call(16, 16, d, a, t, opts(fit=1, scale_shift=0xA000), ws, big, out, gd, ga, null) == EINVAL
    # the order of the checks: a bad argument is reported before a short workspace, a short workspace before the size
    assert call(16, 16, d, a, t, opts(min_alpha=0.0), ws, 0, out, gd, ga, null) == EINVAL
    assert call(16, 16, d, a, t, opts(fit=1, scale_shift=0xA000), ws, 0, out, gd, ga, null) == EINVAL
    assert call(65536, 65536, d, a, t, opts(), ws, 0, out, gd, ga, null) == EWORKSPACE
    assert call(65536, 65536, d, a, t, opts(), ws, 1 << 40, out, gd, ga, null) == EOVERFLOW    # H W > 2^31 - 1
