"""csrc/vq.hip through the Python host (compress.py) against the numpy mirror tests/vq_ref.py, bit for bit: assignment
at every seam of the kernel, ties and NaN rows, the fixed-point update, the fit loop, and the compressed container's
round trip.

The assign kernel as built: a workgroup takes 256 rows, a wave 64 of them as two groups of 32; no two waves share a
row.  Codes stream in chunks of 128 = four tiles of 32; in a tile lane half h = (j % 8) // 4 sees code j.  So partial
results meet in a lane (registers, tiles, chunks, in ascending code order) and once between the two lane halves."""
import functools

import numpy as np
import pytest
import torch

import vq_ref as vr
from util import np_

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = [(1, 1, 1), (300, 33, 45), (129, 200, 9), (1000, 257, 24), (64, 64, 48), (4097, 1024, 45)]


def _rng(key):
    return np.random.Generator(np.random.Philox(key=key))


@functools.lru_cache(maxsize=None)
def _case(n, k, d):
    """(x, codebook, mirror assign, mirror dist), computed once per shape; the arrays are read-only."""
    rng = _rng(2800 + n + k + d)
    x = rng.standard_normal((n, d)).astype(F32)
    cb = (x[rng.integers(0, n, k)] + 0.1 * rng.standard_normal((k, d))).astype(F32)
    a, dist = vr.mirror_assign(x, cb, return_dist=True)
    for v in (x, cb, a, dist):
        v.setflags(write=False)
    return x, cb, a, dist


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                  # a copy: the shared cases are read-only


@pytest.mark.parametrize("n,k,d", SHAPES)
def test_assign_and_dist_equal_the_mirror(pkg, dev, n, k, d):
    x, cb, want, want_dist = _case(n, k, d)
    got, dist = pkg.vq_assign(_t(x, dev), _t(cb, dev), return_dist=True)
    assert got.dtype == torch.int32 and dist.dtype == torch.float32
    assert np.array_equal(np_(got), want)
    assert np.array_equal(_bits(np_(dist)), _bits(want_dist))
    assert np.array_equal(np_(pkg.vq_assign(_t(x, dev), _t(cb, dev))), want)


def test_assign_with_a_row_stride(pkg, dev):
    x, cb, want, want_dist = _case(300, 33, 45)
    wide = torch.full((300, 52), float("nan"), device=dev)
    wide[:, :45] = _t(x, dev)
    view = wide[:, :45]
    assert view.stride(0) == 52
    got, dist = pkg.vq_assign(view, _t(cb, dev), return_dist=True)
    assert np.array_equal(np_(got), want) and np.array_equal(_bits(np_(dist)), _bits(want_dist))
    off = torch.empty(300 * 45 + 1, device=dev)[1:].view(300, 45)               # a dword-aligned view
    off.copy_(_t(x, dev))
    assert np.array_equal(np_(pkg.vq_assign(off, _t(cb, dev))), want)


def test_ties_go_to_the_lowest_index(pkg, dev):
    x, cb, _, _ = _case(129, 200, 9)
    x, cb = x.copy(), cb.copy()
    cb[3] = cb[40] = cb[199] = x[17]
    x[100] = x[128] = x[17]
    got = np_(pkg.vq_assign(_t(x, dev), _t(cb, dev)))
    assert got[17] == 3 and got[100] == 3 and got[128] == 3
    assert np.array_equal(got, vr.mirror_assign(x, cb))


def test_ties_across_lane_halves_tiles_chunks_and_workgroups(pkg, dev):
    """Copies at codes 3 (chunk 0, tile 0, half 0), 44 (tile 1, half 1), 131 (chunk 1, half 0) and 260 (chunk 2, half 1);
    the rows that equal them sit in both row groups of a wave (5, 40), in other waves (70, 200) and in the second
    workgroup (256, 299).  Then without the copy at 3, and without those at 3 and 44."""
    rng = _rng(2850)
    x = rng.standard_normal((300, 45)).astype(F32)
    base = rng.standard_normal((300, 45)).astype(F32)
    rows = [5, 40, 70, 200, 256, 299]
    x[rows] = x[5]
    for copies in ([3, 44, 131, 260], [44, 131, 260], [131, 260], [260, 44]):
        cb = base.copy()
        cb[copies] = x[5]
        got = np_(pkg.vq_assign(_t(x, dev), _t(cb, dev)))
        assert got[rows].tolist() == [min(copies)] * len(rows), copies
        assert np.array_equal(got, vr.mirror_assign(x, cb))


def test_a_nan_row_gets_zero_and_leaves_its_neighbours_alone(pkg, dev):
    x, cb, want, _ = _case(300, 33, 45)
    bad = x.copy()
    bad[7, 2] = np.nan
    bad[255] = np.nan
    got = np_(pkg.vq_assign(_t(bad, dev), _t(cb, dev)))
    assert got[7] == 0 and got[255] == 0
    keep = np.ones(300, bool)
    keep[[7, 255]] = False
    assert np.array_equal(got[keep], want[keep])
    assert np.array_equal(got, vr.mirror_assign(bad, cb))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,k,d", [(1000, 257, 24), (300, 33, 45), (1, 1, 1)])
def test_update_equals_the_mirror(pkg, dev, n, k, d, weighted):
    x, cb, assign, _ = _case(n, k, d)
    rng = _rng(2860 + n)
    assign = assign.copy()
    w = None
    if n > 1:
        assign[assign == 5] = 6                                   # code 5 has no member: it keeps its bits
        assign[rng.integers(0, n, n // 10)] = -1                  # rows left out
        if weighted:
            w = rng.uniform(0.0, 4.0, n).astype(F32)
            w[rng.integers(0, n, n // 8)] = 0.0
            w[assign == 9] = 0.0                                  # members without weight: code 9 keeps its bits as well
    elif weighted:
        w = np.array([0.75], F32)
    bits = pkg.vq_frac_bits(n, float(np.abs(x).max()), 1.0 if w is None else float(w.max()))
    want, want_counts = vr.mirror_update(x, assign, cb, bits, w)
    got = _t(cb, dev).clone()
    counts = torch.full((k,), -7, dtype=torch.int32, device=dev)
    pkg.vq_update(_t(x, dev), _t(assign, dev), got, bits, weights=None if w is None else _t(w, dev), counts=counts)
    assert np.array_equal(_bits(np_(got)), _bits(want))
    assert np.array_equal(np_(counts), want_counts)
    if n > 1:
        assert np.array_equal(_bits(np_(got)[5]), _bits(cb[5])) and want_counts[5] == 0
        if weighted:
            assert np.array_equal(_bits(np_(got)[9]), _bits(cb[9]))
    again = _t(cb, dev).clone()
    pkg.vq_update(_t(x, dev), _t(assign, dev), again, bits, weights=None if w is None else _t(w, dev))   # no counts
    assert torch.equal(again, got)


def test_fit_is_deterministic_and_equals_the_mirror(pkg, dev):
    x, _, _, _ = _case(1000, 257, 24)
    w = _rng(2870).uniform(0.0, 2.0, 1000).astype(F32)
    for weights in (None, w):
        wt = None if weights is None else _t(weights, dev)
        a = pkg.vq_fit(_t(x, dev), 257, iters=5, weights=wt)
        b = pkg.vq_fit(_t(x, dev), 257, iters=5, weights=wt)
        for p, q in zip(a, b):
            assert np_(p).tobytes() == np_(q).tobytes()
        want_cb, want_a, want_counts = vr.mirror_fit(x, 257, iters=5, weights=weights)
        assert np.array_equal(_bits(np_(a[0])), _bits(want_cb))
        assert np.array_equal(np_(a[1]), want_a) and np.array_equal(np_(a[2]), want_counts)
        assert a[1].dtype == torch.int32 and a[2].dtype == torch.int32 and int(a[2].sum()) == 1000
    cb, idx, counts = pkg.vq_fit(_t(x[:7], dev), 50, iters=2)     # k' = min(k, n)
    assert tuple(cb.shape) == (7, 24) and np_(idx).tolist() == list(range(7)) and np_(counts).tolist() == [1] * 7


def _prototype_model(pkg, dev, n=1500, protos=50):
    """A degree-3 model whose SH rest rows are draws from `protos` prototype rows on a 2^-10 grid in [-2, 2]: the
    fixed-point mean of identical rows is exact."""
    rng = _rng(2880)
    arrays = pkg.scene.make_gaussians(n, 160, 120, sh_degree=3, seed=91, mu_s=-3.4)
    table = (rng.integers(-2048, 2049, (protos, 45)) / 1024.0).astype(F32)
    pick = rng.integers(0, protos, n)
    pick[:protos] = np.arange(protos)
    arrays["sh_coeffs"] = arrays["sh_coeffs"].copy()
    arrays["sh_coeffs"][:, :, 1:] = table[pick].reshape(n, 3, 15)
    arrays["rotations"] = (arrays["rotations"] * 3.0).astype(F32)              # raw, not unit
    return arrays, pkg.scene.to_model(arrays, dev), table, pick


FIELDS = ("positions", "sh_coeffs", "opacities", "rotations", "scales")


def test_round_trip_of_a_model_made_of_prototypes_is_exact(pkg, dev, tmp_path):
    arrays, model, table, pick = _prototype_model(pkg, dev)
    cm = pkg.compress_gaussians(model, sh_codes=50, iters=3, geometry_dtype=torch.float32, init=_t(table, dev))
    assert cm.sh_index.dtype == torch.uint16 and cm.sh_degree == 3 and tuple(cm.sh_codebook.shape) == (50, 45)
    assert np.array_equal(np_(cm.sh_index), pick.astype(np.uint16))
    assert np.array_equal(_bits(np_(cm.sh_codebook)), _bits(table))
    back = pkg.decompress_gaussians(cm)
    for name in FIELDS:
        assert np.array_equal(_bits(np_(getattr(back, name))), _bits(arrays[name])), name
    path = tmp_path / "model.npz"
    size = pkg.write_compressed(path, cm)
    assert pkg.nbytes(cm) <= size <= pkg.nbytes(cm) + 4096
    loaded = pkg.decompress_gaussians(pkg.read_compressed(path, device=dev))
    cam = pkg.scene.make_camera(160, 120)
    settings = pkg.RenderSettings(background=[0.1, 0.2, 0.3], active_sh_degree=3)
    a, b = pkg.render(model, cam, settings), pkg.render(loaded, cam, settings)
    assert torch.equal(a.color, b.color) and float(a.color.std()) > 0.01


def test_sixteen_bit_geometry_and_the_file(pkg, dev, tmp_path):
    arrays, model, table, _ = _prototype_model(pkg, dev)
    n = 1500
    cm = pkg.compress_gaussians(model, sh_codes=64, iters=2)
    k = int(cm.sh_codebook.shape[0])
    assert k == 64 and pkg.nbytes(cm) <= n * 36 + k * 45 * 4
    rot = model.rotations / model.rotations.norm(dim=1, keepdim=True)
    assert torch.equal(cm.rotations, rot.half()) and bool(torch.isfinite(cm.rotations).all())
    assert torch.equal(cm.sh_dc, model.sh_coeffs[:, :, 0].half())
    assert torch.equal(cm.opacities, model.opacities.half()) and torch.equal(cm.scales, model.scales.half())
    assert torch.equal(cm.positions, model.positions) and cm.positions.dtype == torch.float32
    rest = model.sh_coeffs[:, :, 1:].reshape(n, 45)
    assert torch.equal(cm.sh_index.to(torch.int32), pkg.vq_assign(rest, cm.sh_codebook))
    path = tmp_path / "model16.npz"
    pkg.write_compressed(path, cm)
    back = pkg.read_compressed(path, device=dev)
    for name in ("positions", "sh_dc", "opacities", "scales", "rotations", "sh_index", "sh_codebook"):
        got, want = getattr(back, name), getattr(cm, name)
        assert got.dtype == want.dtype and np_(got).tobytes() == np_(want).tobytes(), name
    with np.load(path) as z:
        assert z["meta"].tolist() == [1, n, 3, k] and sorted(z.files) == sorted(
            ["meta", "positions", "sh_dc", "opacities", "scales", "rotations", "sh_index", "sh_codebook"])
        parts = {name: z[name] for name in z.files}
    wrong = dict(parts, meta=np.array([2, n, 3, k], np.int64))
    np.savez(tmp_path / "v2.npz", **wrong)
    with pytest.raises(ValueError, match="version"):
        pkg.read_compressed(tmp_path / "v2.npz")
    short = dict(parts, sh_index=parts["sh_index"][:-1])
    np.savez(tmp_path / "short.npz", **short)
    with pytest.raises(ValueError):
        pkg.read_compressed(tmp_path / "short.npz")
    np.savez(tmp_path / "k.npz", **dict(parts, meta=np.array([1, n, 3, k + 1], np.int64)))
    with pytest.raises(ValueError):
        pkg.read_compressed(tmp_path / "k.npz")


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_lower_degrees_go_through(pkg, dev, degree):
    n, coeffs = 400, (degree + 1) ** 2
    arrays = pkg.scene.make_gaussians(n, 160, 120, sh_degree=degree, seed=92 + degree, mu_s=-3.4)
    model = pkg.scene.to_model(arrays, dev)
    weights = _t(_rng(2890).uniform(0.0, 1.0, n).astype(F32), dev)
    cm = pkg.compress_gaussians(model, sh_codes=32, iters=3, weights=weights, geometry_dtype=torch.float32)
    back = pkg.decompress_gaussians(cm)
    assert cm.sh_degree == degree and tuple(back.sh_coeffs.shape) == (n, 3, coeffs) and back.is_valid()
    for name in ("positions", "opacities", "rotations", "scales"):
        assert torch.equal(getattr(back, name), getattr(model, name)), name
    assert torch.equal(back.sh_coeffs[:, :, 0], model.sh_coeffs[:, :, 0])
    d = 3 * (coeffs - 1)
    if degree == 0:
        assert cm.sh_index.numel() == 0 and tuple(cm.sh_codebook.shape) == (0, 0)
        return
    assert tuple(cm.sh_codebook.shape) == (32, d) and tuple(cm.sh_index.shape) == (n,)
    rest = model.sh_coeffs[:, :, 1:].reshape(n, d)
    want_cb, want_idx, _ = vr.mirror_fit(np_(rest), 32, iters=3, weights=np_(weights))
    assert np.array_equal(_bits(np_(cm.sh_codebook)), _bits(want_cb))
    assert np.array_equal(np_(cm.sh_index).astype(np.int32), want_idx)
    assert torch.equal(back.sh_coeffs[:, :, 1:].reshape(n, d), cm.sh_codebook[cm.sh_index.to(torch.int64)])
