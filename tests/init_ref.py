"""numpy restatement of the point-cloud initialisation contract (the reference's
core/gaussian_init.cpp), for the CPU and GPU tests of cugs_knn_mean_distances / cugs_init_from_points.

Everything is float32 with one numpy operation per rounding, in the contract's order:
    d^2 = (dx*dx + dy*dy) + dz*dz,  dx = p_j.x - p_i.x;   the point itself excluded by INDEX;   k = min(k, n - 1);
    m_i = (sqrt of the k smallest d^2, added smallest first) / float32(k);   n <= 1: m = 1.
The search is a chunked brute force; `queries` restricts it to a list of points so that large clouds can be checked
on a sample.  The logarithm of the scales has no deterministic counterpart on the device: scale_log_yardstick gives the
float64 value the 2-ulp rule is measured against.
"""
import numpy as np

F = np.float32
SH_C0 = F(0.28209479177387814)
OPACITY_LOGIT = F(-2.1972245773362196)
MIN_DIST = F(1e-7)


def make_cloud(kind, n, seed=0):
    """(positions [n,3] float32, colors [n,3] uint8).  uniform: a cube of 10.  blobs: 20 Gaussian blobs, sigma
    log-uniform in [0.01, 1], centres in a box of 10, 1 % of the points replaced by outliers in a box of 200.
    plane: uniform, z constant."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        pos = rng.uniform(0.0, 10.0, (n, 3))
    elif kind == "plane":
        pos = rng.uniform(0.0, 10.0, (n, 3))
        pos[:, 2] = 1.5
    elif kind == "blobs":
        centres = rng.uniform(0.0, 10.0, (20, 3))
        sigma = np.exp(rng.uniform(np.log(0.01), np.log(1.0), 20))
        which = rng.integers(0, 20, n)
        pos = centres[which] + rng.standard_normal((n, 3)) * sigma[which, None]
        out = rng.random(n) < 0.01
        pos[out] = rng.uniform(-95.0, 105.0, (int(out.sum()), 3))
    else:
        raise ValueError(kind)
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    return np.ascontiguousarray(pos, F), col


def knn_sq_distances(positions, k_neighbors=3, queries=None, pairs_per_chunk=1 << 24):
    """The k = min(k_neighbors, n - 1) smallest d^2 of each query, ascending: float32 [len(queries), k]."""
    pos = np.ascontiguousarray(positions, F)
    n = pos.shape[0]
    assert n >= 2
    k = min(int(k_neighbors), n - 1)
    q = np.arange(n) if queries is None else np.asarray(queries, np.int64)
    out = np.empty((len(q), k), F)
    x, y, z = pos[:, 0][None, :], pos[:, 1][None, :], pos[:, 2][None, :]
    step = max(1, pairs_per_chunk // n)
    for a in range(0, len(q), step):
        qi = q[a:a + step]
        dx = x - pos[qi, 0][:, None]
        dy = y - pos[qi, 1][:, None]
        dz = z - pos[qi, 2][:, None]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == F
        d2[np.arange(len(qi)), qi] = np.inf                        # excluded by index, not by distance
        best = np.partition(d2, k - 1, axis=1)[:, :k]
        best.sort(axis=1)
        out[a:a + step] = best
    return out


def mean_of_sorted(best):
    """m from the k best d^2 in the given column order: ((sqrt b0 + sqrt b1) + ...) / float32(k)."""
    best = np.asarray(best, F)
    s = np.sqrt(best[:, 0])
    for j in range(1, best.shape[1]):
        s = s + np.sqrt(best[:, j])
    assert s.dtype == F
    return s / F(best.shape[1])


def knn_mean_distances(positions, k_neighbors=3, queries=None):
    pos = np.ascontiguousarray(positions, F)
    n = pos.shape[0]
    nq = n if queries is None else len(queries)
    if n <= 1:
        return np.ones(nq, F)
    return mean_of_sorted(knn_sq_distances(pos, k_neighbors, queries))


def scale_log_yardstick(mean_dist):
    """fl32(log64(max(m, 1e-7f))): what the device logf is held to within 2 ulp."""
    m = np.maximum(np.asarray(mean_dist, F), MIN_DIST)
    return np.log(m.astype(np.float64)).astype(F)


def scale_ulp_error(scales, mean_dist):
    """|s - yardstick| in units of ulp(s), per element of scales [n, 3]."""
    s = np.asarray(scales, F)
    want = scale_log_yardstick(mean_dist)[:, None]
    diff = np.abs(s.astype(np.float64) - want.astype(np.float64))
    return diff / np.spacing(np.abs(s)).astype(np.float64)


def init_model(positions, colors, sh_degree=3, k_neighbors=3):
    """The five arrays and mean_dist.  `scales` holds the float64-rounded yardstick (see scale_ulp_error)."""
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3)
    col = np.asarray(colors, np.uint8).reshape(-1, 3)
    n, C = pos.shape[0], (int(sh_degree) + 1) ** 2
    m = knn_mean_distances(pos, k_neighbors) if n > 0 else np.zeros(0, F)
    sh = np.zeros((n, 3, C), F)
    sh[:, :, 0] = (col.astype(F) / F(255.0) - F(0.5)) / SH_C0
    rot = np.zeros((n, 4), F)
    rot[:, 0] = 1.0
    return {"positions": pos.copy(), "sh_coeffs": sh, "opacities": np.full((n, 1), OPACITY_LOGIT, F), "rotations": rot,
            "scales": np.repeat(scale_log_yardstick(m)[:, None], 3, axis=1), "mean_dist": m}
