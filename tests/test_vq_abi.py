"""cugs_vq_workspace_bytes / cugs_vq_assign / cugs_vq_update (include/cugs_hip.h): the symbols, and the argument checks
that fail - or succeed with nothing to do - before anything touches the device (no GPU needed)."""
import ctypes as C

EINVAL, EALIGN, EWORKSPACE = -1, -2, -4
FAKE = C.c_void_p(1 << 20)            # 64-byte aligned, never dereferenced on these paths
OFF4 = C.c_void_p((1 << 20) + 4)      # dword aligned only
OFF2 = C.c_void_p((1 << 20) + 2)      # not dword aligned
NUL = C.c_void_p(0)


def _assign(lib, n=10, d=45, k=64, x=FAKE, ldx=None, cb=FAKE, out=FAKE, dist=NUL, ws=FAKE, short=0):
    size = max(int(lib.cugs_vq_workspace_bytes(k, d)), 256) - short
    return lib.cugs_vq_assign(n, d, k, x, d if ldx is None else ldx, cb, out, dist, ws, size, NUL)


def _update(lib, n=10, d=45, k=64, x=FAKE, ldx=None, w=NUL, a=FAKE, bits=40, cb=FAKE, counts=NUL, ws=FAKE, short=0):
    size = max(int(lib.cugs_vq_workspace_bytes(k, d)), 256) - short
    return lib.cugs_vq_update(n, d, k, x, d if ldx is None else ldx, w, a, bits, cb, counts, ws, size, NUL)


def test_vq_symbols_bound_and_exported(pkg):
    from cugs_amd import _lib
    so = C.CDLL(pkg.LIB_PATH)
    for name in ("cugs_vq_workspace_bytes", "cugs_vq_assign", "cugs_vq_update"):
        assert name in _lib.SIGNATURES and getattr(so, name)
    for name in ("vq_assign", "vq_fit", "vq_update", "vq_frac_bits", "compress_gaussians", "decompress_gaussians",
                 "CompressedGaussians", "write_compressed", "read_compressed", "nbytes"):
        assert hasattr(pkg, name), name


def test_vq_workspace_bytes_is_zero_for_bad_sizes_and_monotone(pkg):
    from cugs_amd._lib import lib
    for k, d in ((0, 45), (-1, 45), (65537, 45), (8, 0), (8, -3), (8, 49)):
        assert lib.cugs_vq_workspace_bytes(k, d) == 0
    ks, ds = (1, 2, 127, 128, 129, 1000, 8192, 65536), (1, 2, 9, 24, 45, 48)
    for d in ds:
        sizes = [lib.cugs_vq_workspace_bytes(k, d) for k in ks]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    for k in ks:
        sizes = [lib.cugs_vq_workspace_bytes(k, d) for d in ds]
        assert sizes == sorted(sizes)
    assert lib.cugs_vq_workspace_bytes(8192, 45) % 256 == 0


def test_vq_rejects_bad_arguments(pkg):
    from cugs_amd._lib import lib
    for call in (_assign, _update):                                # every call here fails a check: nothing is queued
        assert call(lib, n=-1) == EINVAL and call(lib, n=1 << 31) == EINVAL
        for d in (0, -1, 49):
            assert call(lib, d=d, ldx=64) == EINVAL and call(lib, d=d, ldx=64, n=0) == EINVAL
        for k in (0, -5, 65537):
            assert call(lib, k=k) == EINVAL and call(lib, k=k, n=0) == EINVAL
        assert call(lib, ldx=44) == EINVAL and call(lib, d=9, ldx=8, n=0) == EINVAL
        assert call(lib, x=NUL) == EINVAL and call(lib, cb=NUL) == EINVAL and call(lib, ws=NUL) == EINVAL
    assert _assign(lib, out=NUL) == EINVAL and _update(lib, a=NUL) == EINVAL
    for bits in (-1, 63, 1000):
        assert _update(lib, bits=bits) == EINVAL and _update(lib, bits=bits, n=0) == EINVAL


def test_vq_checks_workspace_then_alignment(pkg):
    from cugs_amd._lib import lib
    for call in (_assign, _update):
        assert call(lib, short=1) == EWORKSPACE and call(lib, short=1, n=0) == EWORKSPACE
        assert call(lib, n=-1, short=1) == EINVAL                  # the arguments come first
        assert call(lib, short=1, x=OFF2) == EWORKSPACE            # then the workspace size
        for key in ("x", "cb"):
            assert call(lib, **{key: OFF2}) == EALIGN and call(lib, n=0, **{key: OFF2}) == EALIGN
        assert call(lib, ws=OFF4, n=0) == EALIGN and call(lib, ws=C.c_void_p((1 << 20) + 8), n=0) == 0
    assert _assign(lib, out=OFF2) == EALIGN and _assign(lib, dist=OFF2) == EALIGN
    assert _update(lib, a=OFF2) == EALIGN and _update(lib, w=OFF2) == EALIGN and _update(lib, counts=OFF2) == EALIGN


def test_vq_of_nothing_queues_nothing(pkg):
    from cugs_amd._lib import lib
    for d, k in ((1, 1), (9, 33), (45, 8192), (48, 65536)):
        assert _assign(lib, n=0, d=d, k=k) == 0 and _update(lib, n=0, d=d, k=k) == 0
    assert _assign(lib, n=0, x=NUL, cb=NUL, out=NUL, dist=NUL) == 0
    assert _assign(lib, n=0, x=OFF4, cb=OFF4, out=OFF4, dist=OFF4, ldx=100) == 0     # dword-aligned views are fine
    assert _update(lib, n=0, x=NUL, a=NUL, cb=NUL, w=NUL, counts=NUL) == 0
    for bits in (0, 62):
        assert _update(lib, n=0, bits=bits) == 0


def test_vq_frac_bits_leaves_room_for_the_sums(pkg):
    import vq_ref as vr
    assert pkg.vq_frac_bits(1500, 2.0) == 61 - 11 - 2 == vr.frac_bits_for(1500, 2.0)
    for n, xm, wm in ((1, 1e-3, 1.0), (6_000_000, 7.3, 1.0), (6_000_000, 0.4, 1234.5), (1000, 0.0, 0.0), (77, 3.0, 1e-6)):
        bits = pkg.vq_frac_bits(n, xm, wm)
        assert bits == vr.frac_bits_for(n, xm, wm) and 0 <= bits <= 62
        assert n * max(wm * xm, wm) * 2.0 ** bits < 2.0 ** 62
    import pytest
    with pytest.raises(ValueError):
        pkg.vq_frac_bits(1 << 30, 1e30)
    with pytest.raises(ValueError):
        pkg.vq_frac_bits(10, float("nan"))
