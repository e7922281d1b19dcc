"""Sparse Adam in numpy, over the oracle's Adam: the rows with radii > 0 take exactly the oracle's
dense update (oracle.fused_adam on their slices, with the bias corrections given - the optimizer's global step), every
other row keeps parameter and moments bit for bit.  Shared by test_sparse_adam_ref.py and the GPU tests."""
import numpy as np


def sparse_fused_adam(orc, param, grad, m, v, radii, lr, beta1, beta2, eps, bc1, bc2):
    """In place on param, m, v ([n_rows, ...] contiguous float32); radii: [n_rows] integers, row stepped iff > 0."""
    n_rows = int(radii.shape[0])
    assert all(a.shape[0] == n_rows and a.dtype == np.float32 and a.flags.c_contiguous for a in (param, grad, m, v))
    rows = np.flatnonzero(np.asarray(radii) > 0)
    if rows.size == 0:
        return
    # the update is element-wise, so the visible rows gathered into a contiguous block step as they do in place
    p, g, mm, vv = (np.ascontiguousarray(a[rows]) for a in (param, grad, m, v))
    orc.fused_adam(p, g, mm, vv, lr, beta1, beta2, eps, bc1, bc2)
    param[rows], m[rows], v[rows] = p, mm, vv


def standard_invisible(n):
    """The tests' pattern: rows 256..511 (one whole workgroup) plus every third row elsewhere - float4 pieces that
    straddle a visible and an invisible row, and mixed workgroups."""
    inv = np.zeros(n, bool)
    inv[256:512] = True
    inv[::3] = True
    return inv
