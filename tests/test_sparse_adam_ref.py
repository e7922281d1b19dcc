"""The numpy mirror of sparse Adam (tests/sparse_adam_ref.py) against the oracle's dense Adam, without a GPU."""
import numpy as np
import pytest

from sparse_adam_ref import sparse_fused_adam, standard_invisible

B1, B2, EPS, LR = 0.9, 0.999, 1e-15, 2.5e-3
WIDTHS = (3, 48, 27, 1, 4)


def _state(n, width, seed):
    rng = np.random.default_rng(seed)
    mk = lambda s: (s * rng.standard_normal((n, width))).astype(np.float32)
    return mk(1.0), mk(1e-3), mk(1e-3), np.abs(mk(1e-6))


@pytest.mark.parametrize("width", WIDTHS)
def test_all_rows_visible_is_the_dense_step(orc, width):
    n = 301
    p, g, m, v = _state(n, width, width)
    dp, dm, dv = p.copy(), m.copy(), v.copy()
    for step in (1, 2, 3):
        bc1, bc2 = orc.adam_bias_correction(B1, B2, step)
        orc.fused_adam(dp, g, dm, dv, LR, B1, B2, EPS, bc1, bc2)
        sparse_fused_adam(orc, p, g, m, v, np.ones(n, np.int32), LR, B1, B2, EPS, bc1, bc2)
        for a, b in ((p, dp), (m, dm), (v, dv)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (width, step)


@pytest.mark.parametrize("width", WIDTHS)
def test_masked_rows_keep_their_bits_and_the_rest_step_densely(orc, width):
    n = 700
    inv = standard_invisible(n)
    radii = np.where(inv, -(np.arange(n) % 2), 1 + np.arange(n) % 7).astype(np.int32)    # invisible: 0 or -1
    p, g, m, v = _state(n, width, 100 + width)
    p0, m0, v0 = p.copy(), m.copy(), v.copy()
    for step in (1, 2, 3):                                  # bc1 / bc2 advance with the global step
        bc1, bc2 = orc.adam_bias_correction(B1, B2, step)
        before = (p.copy(), m.copy(), v.copy())
        dense = tuple(a.copy() for a in before)
        orc.fused_adam(dense[0], g, dense[1], dense[2], LR, B1, B2, EPS, bc1, bc2)
        sparse_fused_adam(orc, p, g, m, v, radii, LR, B1, B2, EPS, bc1, bc2)
        for got, d, b in zip((p, m, v), dense, before):
            want = np.where(inv[:, None], b, d)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (width, step)
    for a, a0 in ((p, p0), (m, m0), (v, v0)):
        assert np.array_equal(a[inv].view(np.uint32), a0[inv].view(np.uint32))
        assert not np.array_equal(a[~inv], a0[~inv])


def test_no_row_visible_changes_nothing(orc):
    p, g, m, v = _state(50, 3, 9)
    p0, m0, v0 = p.copy(), m.copy(), v.copy()
    sparse_fused_adam(orc, p, g, m, v, np.zeros(50, np.int32), LR, B1, B2, EPS, 10.0, 1000.0)
    assert np.array_equal(p, p0) and np.array_equal(m, m0) and np.array_equal(v, v0)


def test_first_step_of_a_row_seen_late_is_about_3_2_lr(orc):
    """A row with m = v = 0 first stepped at global step t takes lr (1-b1) bc1 / sqrt((1-b2) bc2) -> 3.16 lr for large t
    (DESIGN.md 4.20 documents it; Inria's and gsplat's kernels give the same 3.16 lr, having no bias correction)."""
    p, g = np.zeros((1, 1), np.float32), np.full((1, 1), 0.37, np.float32)
    m, v = np.zeros_like(p), np.zeros_like(p)
    bc1, bc2 = orc.adam_bias_correction(B1, B2, 20000)
    sparse_fused_adam(orc, p, g, m, v, np.ones(1, np.int32), LR, B1, B2, EPS, bc1, bc2)
    assert abs(float(-p[0, 0]) / LR - (1 - B1) / np.sqrt(1 - B2)) < 0.01
