"""cugs_loss_opts_workspace_bytes / cugs_combined_loss_opts (include/cugs_hip.h): the workspace size and the argument
checks, through ctypes with null or never-dereferenced pointers - every call here returns before anything is queued.
No GPU."""
import ctypes as C

EINVAL, EWORKSPACE = -1, -4


def test_loss_opts_workspace_bytes(pkg):
    from cugs_amd._lib import lib
    size, plain = lib.cugs_loss_opts_workspace_bytes, lib.cugs_loss_workspace_bytes
    assert size(-1, 4) == 0 and size(4, -1) == 0
    for w, h in ((5, 7), (16, 16), (53, 37), (1920, 1080)):
        tiles = ((w + 15) // 16) * ((h + 15) // 16)
        assert size(w, h) >= plain(w, h) + 12 * 8 * tiles               # twelve fp64 partials per tile on top
        assert size(w, h) % 256 == 0
    # at a fixed pixel count the difference to the plain workspace grows with the tile count
    assert size(16 * 64, 1) - plain(16 * 64, 1) > size(32, 32) - plain(32, 32)
    assert size(160, 16) > size(16, 16)
    assert size(1920, 1080) - plain(1920, 1080) < plain(1920, 1080) // 50   # and stays small beside the three maps


def test_combined_loss_opts_argument_validation(pkg):
    from cugs_amd._lib import LossOpts, lib
    null = C.c_void_p(0)
    p = lambda a: C.c_void_p(a)                                             # never dereferenced: the checks come first
    r, t, ws, out, grad = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000)
    big = 1 << 20
    call = lib.cugs_combined_loss_opts
    full = LossOpts(exposure=0x6000, mask=0x7000, dL_dexposure=0x8000, corrected=0x9000)
    # the exposure gradient needs the exposure and dL_dcolor
    assert call(16, 16, r, t, 0.2, 11, C.byref(LossOpts(dL_dexposure=0x8000)), ws, big, out, null, grad, null) == EINVAL
    assert call(16, 16, r, t, 0.2, 11, C.byref(LossOpts(mask=0x7000, dL_dexposure=0x8000)), ws, big, out, null, grad, null) == EINVAL
    assert call(16, 16, r, t, 0.2, 11, C.byref(full), ws, big, out, null, null, null) == EINVAL
    # the checks of cugs_combined_loss, with options and without (NULL, and a struct of NULLs)
    for opts in (C.byref(full), C.byref(LossOpts(exposure=0x6000)), C.byref(LossOpts(mask=0x7000)), None, C.byref(LossOpts())):
        for window in (10, 1, 2, 0, -3, 17, 16):                            # even or out of 3..15
            assert call(16, 16, r, t, 0.2, window, opts, ws, big, out, null, grad, null) == EINVAL
        assert call(16, 16, null, t, 0.2, 11, opts, ws, big, out, null, grad, null) == EINVAL      # null images
        assert call(16, 16, r, null, 0.2, 11, opts, ws, big, out, null, grad, null) == EINVAL
        assert call(16, 16, r, t, 0.2, 11, opts, null, big, out, null, grad, null) == EINVAL       # null workspace
        assert call(16, 16, r, t, 0.2, 11, opts, ws, big, null, null, grad, null) == EINVAL        # null loss_out
        for w, h in ((0, 16), (16, 0), (-1, 16), (16, -1)):
            assert call(w, h, r, t, 0.2, 11, opts, ws, big, out, null, grad, null) == EINVAL
        assert call(16, 16, r, t, 0.2, 11, opts, ws, 0, out, null, grad, null) == EWORKSPACE       # short workspace
    # with options the larger workspace is required; without, the plain one is enough
    need, plain = lib.cugs_loss_opts_workspace_bytes(16, 16), lib.cugs_loss_workspace_bytes(16, 16)
    assert call(16, 16, r, t, 0.2, 11, C.byref(full), ws, need - 1, out, null, grad, null) == EWORKSPACE
    assert call(16, 16, r, t, 0.2, 11, C.byref(LossOpts(corrected=0x9000)), ws, plain, out, null, grad, null) == EWORKSPACE
    assert call(16, 16, r, t, 0.2, 11, None, ws, plain - 1, out, null, grad, null) == EWORKSPACE
    assert lib.cugs_combined_loss(16, 16, r, t, 0.2, 11, ws, plain - 1, out, null, grad, null) == EWORKSPACE
