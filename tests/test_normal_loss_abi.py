"""cugs_normal_loss_workspace_bytes / cugs_normal_loss (include/cugs_hip.h): the workspace size and the argument checks,
through ctypes with null or never-dereferenced pointers - every call here returns before anything is queued.  No GPU."""
import ctypes as C

EINVAL, EOVERFLOW, EWORKSPACE = -1, -3, -4
TW, TH = 64, 16                                                           # the kernel's tile


def test_normal_loss_workspace_bytes(pkg):
    from cugs_amd._lib import lib
    size = lib.cugs_normal_loss_workspace_bytes
    assert size(-1, 4) == 0 and size(4, -1) == 0 and size(-1, -1) == 0
    tiles = lambda w, h: -(-w // TW) * -(-h // TH)
    for w, h in ((1, 1), (7, 5), (53, 37), (64, 64), (65, 17), (70, 19), (2070, 130), (1920, 1080)):
        assert size(w, h) % 256 == 0
        assert 3 * 8 * tiles(w, h) <= size(w, h) < 3 * 8 * tiles(w, h) + 256      # three fp64 sums per tile, no more
    # grows with the number of tiles, whatever the shape
    assert size(64, 16) == size(1, 1) == size(63, 15) and size(128, 160) == size(64 * 20, 16)
    assert size(64, 160) < size(2070, 130) < size(1920, 1080)                     # 10, 297, 2040 tiles
    assert size(1920, 1080) < 1 << 18                                             # stays small: no per-pixel scratch


def test_normal_loss_argument_validation(pkg):
    from cugs_amd._lib import NormalLossOpts, lib
    null = C.c_void_p(0)
    p = lambda a: C.c_void_p(a)                                             # never dereferenced: the checks come first
    d, a, t, ws, out, gd, ga = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000), p(0x6000), p(0x7000)
    big = 1 << 20
    inf, nan = float("inf"), float("nan")

    def opts(**kw):
        kw.setdefault("min_alpha", 1e-3)
        kw.setdefault("cos_weight", 1.0)
        return C.byref(NormalLossOpts(**kw))

    def call(w, h, D, A, T, o, W, wb, O, gD, gA, fx=50.0, fy=50.0, cx=8.0, cy=8.0):
        return lib.cugs_normal_loss(w, h, fx, fy, cx, cy, D, A, T, o, W, wb, O, gD, gA, null)

    variants = [opts(), opts(weight=0x8000, normals_out=0x9000, l1_weight=0.5), opts(cos_weight=0.0, l1_weight=1.0)]
    need = lib.cugs_normal_loss_workspace_bytes(16, 16)
    for o in variants:
        for w, h in ((0, 16), (16, 0), (-1, 16), (16, -1)):                 # non-positive size
            assert call(w, h, d, a, t, o, ws, big, out, gd, ga) == EINVAL
        assert call(16, 16, null, a, t, o, ws, big, out, gd, ga) == EINVAL            # null maps
        assert call(16, 16, d, null, t, o, ws, big, out, gd, ga) == EINVAL
        assert call(16, 16, d, a, t, o, null, big, out, gd, ga) == EINVAL             # null workspace
        assert call(16, 16, d, a, t, o, ws, big, null, gd, ga) == EINVAL              # null loss_out
        assert call(16, 16, d, a, t, o, ws, 0, out, gd, ga) == EWORKSPACE             # short workspace
        assert call(16, 16, d, a, t, o, ws, need - 1, out, gd, ga) == EWORKSPACE
        assert call(16, 16, d, a, t, o, ws, need - 1, out, null, null) == EWORKSPACE  # the gradients are optional
    assert call(16, 16, d, a, t, None, ws, big, out, gd, ga) == EINVAL                # null opts
    for bad in (0.0, -1e-3, inf, nan, -inf):                                          # min_alpha > 0 and finite
        assert call(16, 16, d, a, t, opts(min_alpha=bad), ws, big, out, gd, ga) == EINVAL
    for bad in (0.0, -50.0, inf, nan, -inf):                                          # fx, fy > 0 and finite
        assert call(16, 16, d, a, t, opts(), ws, big, out, gd, ga, fx=bad) == EINVAL
        assert call(16, 16, d, a, t, opts(), ws, big, out, gd, ga, fy=bad) == EINVAL
    for bad in (inf, nan, -inf):                                                      # cx, cy finite
        assert call(16, 16, d, a, t, opts(), ws, big, out, gd, ga, cx=bad) == EINVAL
        assert call(16, 16, d, a, t, opts(), ws, big, out, gd, ga, cy=bad) == EINVAL
    for bad in (-1.0, inf, nan, -inf):                                                # loss weights >= 0 and finite
        assert call(16, 16, d, a, t, opts(cos_weight=bad), ws, big, out, gd, ga) == EINVAL
        assert call(16, 16, d, a, t, opts(l1_weight=bad), ws, big, out, gd, ga) == EINVAL
        assert call(16, 16, d, a, null, opts(l1_weight=bad, normals_out=0x9000), ws, big, out, null, null) == EINVAL
    assert call(16, 16, d, a, t, opts(cos_weight=0.0, l1_weight=0.0), ws, big, out, gd, ga) == EINVAL   # both 0, a prior
    # no prior: the normal map is the only output
    nrm = dict(normals_out=0x9000)
    assert call(16, 16, d, a, null, opts(), ws, big, out, null, null) == EINVAL                   # nothing to write
    assert call(16, 16, d, a, null, opts(weight=0x8000, **nrm), ws, big, out, null, null) == EINVAL
    assert call(16, 16, d, a, null, opts(**nrm), ws, big, out, gd, null) == EINVAL
    assert call(16, 16, d, a, null, opts(**nrm), ws, big, out, null, ga) == EINVAL
    assert call(16, 16, d, a, null, opts(**nrm), ws, 0, out, null, null) == EWORKSPACE            # otherwise accepted
    assert call(16, 16, d, a, null, opts(cos_weight=0.0, **nrm), ws, 0, out, null, null) == EWORKSPACE  # weights unused
    # the order of the checks: a bad argument is reported before a short workspace, a short workspace before the size
    assert call(16, 16, d, a, t, opts(min_alpha=0.0), ws, 0, out, gd, ga) == EINVAL
    assert call(16, 16, d, a, t, opts(), ws, 0, out, gd, ga, fx=0.0) == EINVAL
    assert call(16, 16, d, a, t, opts(cos_weight=0.0), ws, 0, out, gd, ga) == EINVAL
    assert call(65536, 65536, d, a, t, opts(), ws, 0, out, gd, ga) == EWORKSPACE
    assert call(65536, 65536, d, a, t, opts(), ws, 1 << 40, out, gd, ga) == EOVERFLOW          # H W > 2^31 - 1
