"""cugs_blend_scores: argument validation that fails - or succeeds with nothing to do - before anything touches the
device (no GPU needed)."""
import ctypes as C

EINVAL, EALIGN = -1, -2
FAKE = C.c_void_p(1 << 20)            # 64-byte aligned, never dereferenced on these paths
OFF4 = C.c_void_p((1 << 20) + 4)
NUL = C.c_void_p(0)


def _call(lib, width=32, height=32, tile_ranges=FAKE, gidx=FAKE, means=NUL, cov=NUL, opa=NUL, packed=FAKE,
          tile_order=NUL, n=10, scores=FAKE):
    return lib.cugs_blend_scores(width, height, tile_ranges, gidx, means, cov, opa, packed, tile_order, n, scores, NUL)


def test_scores_symbol_bound_and_exported(pkg):
    from cugs_amd import _lib
    assert "cugs_blend_scores" in _lib.SIGNATURES
    assert getattr(C.CDLL(pkg.LIB_PATH), "cugs_blend_scores")
    for name in ("ContributionScores", "accumulate_contribution_scores", "contribution_scores", "prune_gaussians",
                 "prune_by_scores"):
        assert hasattr(pkg, name), name


def test_scores_rejects_bad_sizes_and_missing_arguments(pkg):
    from cugs_amd._lib import lib
    assert _call(lib, width=-1) == EINVAL and _call(lib, height=-1) == EINVAL and _call(lib, n=-1) == EINVAL
    assert _call(lib, scores=NUL) == EINVAL                               # n > 0 without a table
    # indices present: packed, or all three arrays
    assert _call(lib, packed=NUL) == EINVAL
    assert _call(lib, packed=NUL, means=FAKE, cov=FAKE) == EINVAL
    assert _call(lib, packed=NUL, means=FAKE, opa=FAKE) == EINVAL
    assert _call(lib, packed=NUL, cov=FAKE, opa=FAKE) == EINVAL
    assert _call(lib, tile_ranges=NUL) == EINVAL                          # something to launch, no ranges


def test_scores_checks_alignment(pkg):
    from cugs_amd._lib import lib
    assert _call(lib, packed=OFF4) == EALIGN
    assert _call(lib, tile_order=OFF4) == EALIGN
    assert _call(lib, scores=OFF4) == EALIGN
    assert _call(lib, scores=OFF4, n=0) == EALIGN                         # also with nothing to do
    assert _call(lib, packed=OFF4, width=0) == EALIGN
    # a bad size or a missing argument is reported before the alignment
    assert _call(lib, width=-1, scores=OFF4) == EINVAL
    assert _call(lib, packed=NUL, scores=OFF4) == EINVAL


def test_scores_empty_cases_launch_nothing(pkg):
    from cugs_amd._lib import lib
    assert _call(lib, n=0) == 0 and _call(lib, n=0, scores=NUL) == 0       # no Gaussians: no table needed
    assert _call(lib, n=0, tile_ranges=NUL, gidx=NUL, packed=NUL) == 0
    assert _call(lib, width=0) == 0 and _call(lib, height=0) == 0 and _call(lib, width=0, height=0) == 0
    assert _call(lib, width=0, tile_ranges=NUL, gidx=NUL, packed=NUL) == 0
