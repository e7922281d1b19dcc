"""cugs_blend_lift: argument validation that fails - or succeeds with nothing to do - before anything touches the
device (no GPU needed)."""
import ctypes as C

EINVAL, EALIGN = -1, -2
FAKE = C.c_void_p(1 << 20)            # 64-byte aligned, never dereferenced on these paths
OFF4 = C.c_void_p((1 << 20) + 4)
NUL = C.c_void_p(0)


def _call(lib, width=32, height=32, tile_ranges=FAKE, gidx=FAKE, means=NUL, cov=NUL, opa=NUL, packed=FAKE,
          tile_order=NUL, n=10, maps=FAKE, labels=NUL, channels=3, label_base=0, table=FAKE):
    return lib.cugs_blend_lift(width, height, tile_ranges, gidx, means, cov, opa, packed, tile_order, n, maps, labels,
                               channels, label_base, table, NUL)


def test_lift_symbol_bound_and_exported(pkg):
    from cugs_amd import _lib
    assert "cugs_blend_lift" in _lib.SIGNATURES
    assert getattr(C.CDLL(pkg.LIB_PATH), "cugs_blend_lift")
    for name in ("LiftedMaps", "blend_lift", "lift_pixel_maps", "lift_maps", "vote_labels", "error_scores",
                 "select_gaussians"):
        assert hasattr(pkg, name), name
    assert hasattr(pkg.DensificationController, "accumulate_error_scores")


def test_lift_rejects_bad_sizes_and_missing_arguments(pkg):
    from cugs_amd._lib import lib
    assert _call(lib, width=-1) == EINVAL and _call(lib, height=-1) == EINVAL and _call(lib, n=-1) == EINVAL
    for ch in (-1, 0, 5):
        assert _call(lib, channels=ch) == EINVAL
        assert _call(lib, channels=ch, n=0) == EINVAL                    # also with nothing to do
    assert _call(lib, maps=FAKE, labels=FAKE) == EINVAL                   # both maps
    assert _call(lib, maps=NUL, labels=NUL) == EINVAL                     # neither
    assert _call(lib, table=NUL) == EINVAL                                # n > 0 without a table
    # indices present: packed, or all three arrays
    assert _call(lib, packed=NUL) == EINVAL
    assert _call(lib, packed=NUL, means=FAKE, cov=FAKE) == EINVAL
    assert _call(lib, packed=NUL, means=FAKE, opa=FAKE) == EINVAL
    assert _call(lib, packed=NUL, cov=FAKE, opa=FAKE) == EINVAL
    assert _call(lib, tile_ranges=NUL) == EINVAL                          # something to launch, no ranges


def test_lift_checks_alignment_after_the_arguments(pkg):
    from cugs_amd._lib import lib
    assert _call(lib, packed=OFF4) == EALIGN
    assert _call(lib, tile_order=OFF4) == EALIGN
    assert _call(lib, table=OFF4) == EALIGN
    assert _call(lib, table=OFF4, n=0) == EALIGN                          # also with nothing to do
    assert _call(lib, packed=OFF4, width=0) == EALIGN
    # the maps need none (asked with nothing to launch: every other path here returns before the device is touched)
    assert _call(lib, maps=OFF4, width=0) == 0 and _call(lib, maps=NUL, labels=OFF4, n=0) == 0
    # a bad size, a bad channel count or a missing argument is reported before the alignment
    assert _call(lib, width=-1, table=OFF4) == EINVAL
    assert _call(lib, channels=5, table=OFF4) == EINVAL
    assert _call(lib, packed=NUL, table=OFF4) == EINVAL
    assert _call(lib, maps=NUL, packed=OFF4) == EINVAL
    assert _call(lib, maps=FAKE, labels=FAKE, tile_order=OFF4) == EINVAL
    assert _call(lib, tile_ranges=NUL, table=OFF4) == EINVAL


def test_lift_empty_cases_launch_nothing(pkg):
    from cugs_amd._lib import lib
    assert _call(lib, n=0) == 0 and _call(lib, n=0, table=NUL) == 0        # no Gaussians: no table needed
    assert _call(lib, n=0, tile_ranges=NUL, gidx=NUL, packed=NUL) == 0
    assert _call(lib, width=0) == 0 and _call(lib, height=0) == 0 and _call(lib, width=0, height=0) == 0
    assert _call(lib, width=0, tile_ranges=NUL, gidx=NUL, packed=NUL) == 0
    # nothing would be launched: the maps are not asked for
    assert _call(lib, n=0, maps=NUL, labels=NUL) == 0 and _call(lib, n=0, maps=FAKE, labels=FAKE) == 0
    assert _call(lib, height=0, maps=NUL, labels=NUL) == 0
