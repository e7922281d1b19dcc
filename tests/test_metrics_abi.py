"""cugs_eval_workspace_bytes / cugs_eval_metrics (include/cugs_hip.h): the argument checks, through ctypes with null or
never-dereferenced pointers - every call here returns before anything is queued.  No GPU."""
import ctypes as C

EINVAL = -1


def test_eval_workspace_bytes(pkg):
    from cugs_amd._lib import lib
    assert lib.cugs_eval_workspace_bytes(-1, 4) == 0 and lib.cugs_eval_workspace_bytes(4, -1) == 0
    one = lib.cugs_eval_workspace_bytes(16, 16)
    assert one > 0 and one % 256 == 0
    assert lib.cugs_eval_workspace_bytes(17, 16) >= one                    # a second tile (sizes round up to 256 B)
    assert lib.cugs_eval_workspace_bytes(160, 16) > one                    # ten tiles no longer fit the first 256 B
    assert lib.cugs_eval_workspace_bytes(1920, 1080) >= 32 * 120 * 68      # four fp64 partials per tile
    # no per-pixel scratch: far below the loss's three derivative maps
    assert lib.cugs_eval_workspace_bytes(1920, 1080) < lib.cugs_loss_workspace_bytes(1920, 1080) // 100


def test_eval_metrics_argument_validation(pkg):
    from cugs_amd._lib import lib
    null = C.c_void_p(0)
    p = lambda a: C.c_void_p(a)                                             # never dereferenced: the checks come first
    r, tf, tu, ws, out = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000)
    big = 1 << 20
    call = lib.cugs_eval_metrics
    assert call(16, 16, r, tf, tu, 11, ws, big, out, null) == EINVAL        # both targets
    assert call(16, 16, r, null, null, 11, ws, big, out, null) == EINVAL    # neither
    for window in (10, 1, 2, 0, -3, 17, 16):                                # even or out of 3..15
        assert call(16, 16, r, tf, null, window, ws, big, out, null) == EINVAL
        assert call(16, 16, r, null, tu, window, ws, big, out, null) == EINVAL
    need = lib.cugs_eval_workspace_bytes(16, 16)
    assert call(16, 16, r, tf, null, 11, ws, need - 1, out, null) == EINVAL # short workspace
    assert call(16, 16, r, null, tu, 11, ws, 0, out, null) == EINVAL
    assert call(16, 16, null, tf, null, 11, ws, big, out, null) == EINVAL   # null pointers with pixels to process
    assert call(16, 16, r, tf, null, 11, null, big, out, null) == EINVAL
    assert call(16, 16, r, tf, null, 11, ws, big, null, null) == EINVAL
    assert call(-1, 16, r, tf, null, 11, ws, big, out, null) == EINVAL      # negative size
    assert call(16, -1, r, tf, null, 11, ws, big, out, null) == EINVAL
    for w, h in ((0, 16), (16, 0), (0, 0)):                                 # no pixels: nothing to do
        assert call(w, h, null, null, null, 11, null, 0, null, null) == 0
        assert call(w, h, r, tf, null, 7, ws, big, out, null) == 0
    assert call(0, 0, null, null, null, 10, null, 0, null, null) == EINVAL  # the window is checked either way
