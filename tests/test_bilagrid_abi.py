"""cugs_bilagrid_workspace_bytes / cugs_bilagrid_slice / _slice_backward / _tv (include/cugs_hip.h): the workspace size
and the argument checks, through ctypes with null or never-dereferenced pointers - every call here returns before
anything is queued.  No GPU."""
import ctypes as C

EINVAL, EOVERFLOW, EWORKSPACE = -1, -3, -4
CHUNK = 1024                                  # pixels of an xy-cell per row of partials


def _dims(l, gy, gx):
    from cugs_amd._lib import BilagridDims
    return C.byref(BilagridDims(l=l, gy=gy, gx=gx))


def test_bilagrid_workspace_bytes(pkg):
    from cugs_amd._lib import lib
    size = lib.cugs_bilagrid_workspace_bytes
    d = _dims(8, 16, 16)
    assert size(-1, 4, d) == 0 and size(4, 0, d) == 0 and size(4, 4, None) == 0
    assert size(4, 4, _dims(1, 16, 16)) == 0 and size(4, 4, _dims(8, 65, 16)) == 0
    for w, h, (l, gy, gx) in ((5, 7, (2, 3, 4)), (9, 1, (3, 2, 2)), (53, 37, (8, 16, 16)), (480, 270, (2, 4, 4)),
                              (1920, 1080, (8, 16, 16))):
        cells = (gx - 1) * (gy - 1)
        biggest = -(-w // (gx - 1)) * -(-h // (gy - 1))          # a cell is at least the even share of the image
        q = max(1, -(-biggest // CHUNK))
        got = size(w, h, _dims(l, gy, gx))
        assert got % 256 == 0
        assert got >= 4 * 48 * l * cells * q, (w, h, got)
        assert got <= 4 * 48 * l * cells * (q + 1) + 256, (w, h, got)
    # monotone in the number of partials: more levels, more cells, more chunks per cell
    assert size(64, 64, _dims(2, 4, 4)) < size(64, 64, _dims(4, 4, 4)) < size(64, 64, _dims(4, 8, 4)) < size(64, 64, _dims(4, 8, 8))
    assert size(64, 64, _dims(2, 2, 2)) < size(128, 64, _dims(2, 2, 2)) < size(128, 128, _dims(2, 2, 2))
    # a function of the partials alone: 9 cells of one chunk each, whatever the image below a chunk per cell
    assert size(30, 30, _dims(2, 4, 4)) == size(60, 40, _dims(2, 4, 4)) == round_up(4 * 48 * 2 * 9)
    # and small at 1080p: an eighth of one [H,W,3] image, no per-pixel scratch
    assert size(1920, 1080, d) < 1 << 22


def round_up(b):
    return -(-b // 256) * 256


def test_bilagrid_argument_validation(pkg):
    from cugs_amd._lib import lib
    null = C.c_void_p(0)
    p = lambda a: C.c_void_p(a)                                             # never dereferenced: the checks come first
    G, c, g, ws, out, dc, dg = p(0x1000), p(0x2000), p(0x3000), p(0x4000), p(0x5000), p(0x6000), p(0x7000)
    big = 1 << 30
    d = _dims(8, 16, 16)
    fwd, bwd, tv = lib.cugs_bilagrid_slice, lib.cugs_bilagrid_slice_backward, lib.cugs_bilagrid_tv
    bad_dims = [None] + [_dims(*t) for t in ((1, 16, 16), (8, 1, 16), (8, 16, 1), (65, 16, 16), (8, 65, 16), (8, 16, 65),
                                             (0, 16, 16), (8, -3, 16))]

    for w, h in ((0, 16), (16, 0), (-1, 16), (16, -1)):                     # non-positive size
        assert fwd(w, h, d, G, c, out, null) == EINVAL
        assert bwd(w, h, d, G, c, g, ws, big, dc, dg, null) == EINVAL
    for bad in bad_dims:                                                    # null dims, extents below 2 or above 64
        assert fwd(16, 16, bad, G, c, out, null) == EINVAL
        assert bwd(16, 16, bad, G, c, g, ws, big, dc, dg, null) == EINVAL
        assert tv(bad, G, 1.0, out, dg, 0, null) == EINVAL
    assert fwd(16, 16, d, null, c, out, null) == EINVAL                     # null required pointers
    assert fwd(16, 16, d, G, null, out, null) == EINVAL
    assert fwd(16, 16, d, G, c, null, null) == EINVAL
    assert bwd(16, 16, d, null, c, g, ws, big, dc, dg, null) == EINVAL
    assert bwd(16, 16, d, G, null, g, ws, big, dc, dg, null) == EINVAL
    assert bwd(16, 16, d, G, c, null, ws, big, dc, dg, null) == EINVAL
    assert bwd(16, 16, d, G, c, g, null, big, dc, dg, null) == EINVAL       # a grid gradient needs the workspace
    assert tv(d, null, 1.0, out, dg, 0, null) == EINVAL
    assert tv(d, G, 1.0, null, null, 0, null) == EINVAL                     # nothing to write

    need = lib.cugs_bilagrid_workspace_bytes(16, 16, d)
    assert need > 0
    assert bwd(16, 16, d, G, c, g, ws, 0, dc, dg, null) == EWORKSPACE       # short workspace
    assert bwd(16, 16, d, G, c, g, ws, need - 1, dc, dg, null) == EWORKSPACE
    assert bwd(16, 16, d, G, c, g, ws, need - 1, null, dg, null) == EWORKSPACE

    # the order of the checks: a bad argument before a short workspace, a short workspace before the size
    assert bwd(16, 16, _dims(8, 16, 99), G, c, g, ws, 0, dc, dg, null) == EINVAL
    assert bwd(16, 16, d, G, c, null, ws, 0, dc, dg, null) == EINVAL
    assert bwd(65536, 65536, d, G, c, g, ws, 0, dc, dg, null) == EWORKSPACE
    assert bwd(65536, 65536, d, G, c, g, ws, 1 << 50, dc, dg, null) == EOVERFLOW     # H W > 2^31 - 1
    assert bwd(65536, 65536, d, G, c, g, null, 0, dc, null, null) == EOVERFLOW       # no grid gradient: no workspace check
    assert fwd(65536, 65536, d, G, c, out, null) == EOVERFLOW
    assert fwd(65536, 65536, d, G, null, out, null) == EINVAL
    # neither gradient asked for: nothing to do, nothing queued
    assert bwd(16, 16, d, G, c, g, null, 0, null, null, null) == 0
