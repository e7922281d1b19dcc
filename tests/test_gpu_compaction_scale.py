"""The compaction scans of densify, prune_gaussians and MCMCController.relocate past ONE scan pass (262,144 rows), where
k_scan_counts (csrc/densify.hip) and k_reloc_scan (csrc/mcmc.hip) carry their totals from one pass of 256 chunk sums to
the next - the path every production-size model takes.  Inputs and CPU references: tests/compaction_cases.py (checked
on their own by tests/test_compaction_cases.py).  Row maps, copied rows, moments and split children are compared bit
for bit; only the comparisons against the torch oracle keep the tolerances of tests/test_gpu_densify.py.  Also here, at
small n: the non-float4 row routes, the unaligned fallback of cugs_densify_apply, and rows that sit exactly on a
threshold of k_classify."""
import ctypes as C

import numpy as np
import pytest
import torch

import compaction_cases as cc
import mcmc_ref as mr
from test_densify_oracle import load_densify_oracle
from test_gpu_densify import _compare_models
from util import np_

pytestmark = pytest.mark.gpu
PASS, BIG = cc.PASS, cc.SIZES[2]
MCMC_NAMES = ("positions", "sh_coeffs", "opacities", "scales", "rotations")     # ParamGroup order
COPY, STATE = 0, 3                                                                # CUGS_DENSIFY_COPY / _STATE


@pytest.fixture(scope="module")
def do():
    return load_densify_oracle()


@pytest.fixture(scope="module", autouse=True)
def _release_references():
    yield
    cc.release()


def _P(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plan(lib, check, flags):
    """cugs_densify_plan on a uint8 device tensor: (workspace, counts)."""
    n = int(flags.shape[0])
    ws = torch.empty(lib.cugs_densify_workspace_bytes(n), dtype=torch.uint8, device=flags.device)
    counts = (C.c_int64 * 4)()
    check(lib.cugs_densify_plan(n, _P(flags), _P(ws), ws.numel(), counts, _stream()), "cugs_densify_plan")
    return ws, tuple(int(c) for c in counts)


def _apply(lib, check, DensifyArray, n, n_out, ws, arrays):
    """cugs_densify_apply on [(src, dst, row_floats, mode)]."""
    arr = (DensifyArray * len(arrays))()
    for i, (s, d, rf, mode) in enumerate(arrays):
        arr[i].src, arr[i].dst, arr[i].row_floats, arr[i].mode = s.data_ptr(), d.data_ptr(), rf, mode
    check(lib.cugs_densify_apply(n, n_out, _P(ws), ws.numel(), C.c_void_p(0), C.c_void_p(0), arr, len(arrays), _stream()),
          "cugs_densify_apply")


# ---- 1. the row map itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", cc.FLAG_PATTERNS)
@pytest.mark.parametrize("n", cc.SIZES)
def test_row_map_against_numpy(pkg, dev, n, pattern):
    from cugs_amd._lib import DensifyArray, check, lib
    flags = cc.flag_bytes(pattern, n)
    want_counts, want_map = cc.expected_map(flags)
    ws, counts = _plan(lib, check, torch.from_numpy(flags).to(dev))
    assert counts == want_counts
    n_out = counts[3]
    assert n_out == want_map.size and (pattern != "none" or n_out == 0)
    if n_out == 0:
        return
    # one float per row, src[i] = i (exact below 2^24): dst is then the destination -> source map
    src = torch.arange(n, dtype=torch.float32, device=dev)
    dst = torch.full((n_out,), -1.0, dtype=torch.float32, device=dev)
    _apply(lib, check, DensifyArray, n, n_out, ws, [(src, dst, 1, COPY)])
    got = np_(dst)
    assert np.array_equal(got, want_map.astype(np.float32)), \
        f"first wrong destination row {int(np.nonzero(got != want_map)[0][0])} of {n_out}"


# ---- 2. densify end to end, and 5. the row routes -----------------------------------------------------------------
@pytest.mark.parametrize("n,coeffs", [(cc.SIZES[1], 4), (BIG, 4),             # the carry sizes
                                      (3001, 1), (3001, 9), (3001, 16)])      # SH rows of 3 / 27 / 48 floats
def test_densify_parity_with_moments(pkg, do, orc, dev, n, coeffs):
    ref = cc.densify_reference(do, n, coeffs)
    inp = ref.inputs
    ours = pkg.GaussianModel(**{k: inp.tensors[k].to(dev) for k in cc.NAMES})
    ctrl = pkg.DensificationController(pkg.DensificationConfig(**cc.DENSIFY_CFG), cc.EXTENT)
    for grads, radii in inp.views:
        ctrl.accumulate_gradients(grads.to(dev), radii.to(dev))
    assert np.allclose(np_(ctrl.grad_accum_), ref.acc.grad_accum, rtol=1e-6, atol=0)
    assert np.array_equal(np_(ctrl.grad_count_), ref.acc.grad_count)
    assert np.array_equal(np_(ctrl.max_radii_2d_), ref.acc.max_radii)
    opt = pkg.FusedAdam(ours)
    for i in range(5):
        opt.m_[i] = torch.randn_like(opt.m_[i])
        opt.v_[i] = torch.rand_like(opt.v_[i]) + 0.5                             # no zero among the old moments
    m_before, v_before = [t.clone() for t in opt.m_], [t.clone() for t in opt.v_]
    s, s_ref = ctrl.densify(ours, cc.DENSIFY_STEP, inp.noise.to(dev), optimizer=opt), ref.stats
    assert (s.num_before, s.num_cloned, s.num_split, s.num_pruned, s.num_after) == \
        (s_ref.num_before, s_ref.num_cloned, s_ref.num_split, s_ref.num_pruned, s_ref.num_after)
    assert s.num_cloned > 0 and s.num_split > 0 and s.num_pruned > s.num_split
    children = s.num_after - 2 * s.num_split
    _compare_models(ref.model, ours, n_children_start=children)
    assert ctrl.grad_accum_.shape[0] == s.num_after and float(ctrl.grad_accum_.abs().sum()) == 0.0
    # moments: survivors keep theirs bit for bit, in order; every new row starts at zero
    survive = torch.from_numpy(ref.survive).to(dev)
    kept = int(ref.survive.sum())
    assert kept == children - s.num_cloned
    for i, name in enumerate(opt._names):
        assert opt.m_[i].shape == getattr(ours, name).shape == opt.v_[i].shape
        assert torch.equal(opt.m_[i][:kept], m_before[i][survive]), name
        assert torch.equal(opt.v_[i][:kept], v_before[i][survive]), name
        assert not bool(opt.m_[i][kept:].any()) and not bool(opt.v_[i][kept:].any()), name
    # the children, restated in float32 with the project's own expf: the same rounded operations as the kernel
    want_pos, want_scl = cc.split_children(orc, inp, ref.split)
    assert np.array_equal(np_(ours.scales)[children:], want_scl)
    assert np.array_equal(np_(ours.positions)[children:], want_pos)


# ---- 3. prune_gaussians ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cc.PRUNE_MASKS)
@pytest.mark.parametrize("coeffs", [1, 16])             # 3-float SH rows: every array but rotations takes k_gather_rows
def test_prune_at_three_passes(pkg, dev, coeffs, kind):
    n = BIG
    g = torch.Generator(device=dev).manual_seed(coeffs)
    r = lambda *shape: torch.randn(shape, generator=g, device=dev)
    model = pkg.GaussianModel(positions=r(n, 3), sh_coeffs=r(n, 3, coeffs), opacities=r(n, 1), rotations=r(n, 4),
                              scales=r(n, 3))
    opt = pkg.FusedAdam(model)
    for i in range(5):
        opt.m_[i] = torch.randn_like(opt.m_[i])
        opt.v_[i] = torch.rand_like(opt.v_[i]) + 0.5
    before = {k: getattr(model, k).clone() for k in cc.NAMES}
    m_before, v_before = [t.clone() for t in opt.m_], [t.clone() for t in opt.v_]
    mask_host = cc.prune_mask(kind, n)
    mask = torch.from_numpy(mask_host).to(dev)
    assert pkg.prune_gaussians(model, mask, optimizer=opt) == int(mask_host.sum())
    assert model.num_gaussians() == n - int(mask_host.sum()) and model.is_valid()
    for k in cc.NAMES:
        assert torch.equal(getattr(model, k), before[k][~mask]), k
    for i, name in enumerate(opt._names):
        assert torch.equal(opt.m_[i], m_before[i][~mask]) and torch.equal(opt.v_[i], v_before[i][~mask]), name


# ---- 4. MCMC relocation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pattern", cc.MCMC_CASES)
def test_relocation_exact_against_oracle_at_scale(pkg, orc, dev, n, pattern):
    arrays = cc.mcmc_arrays(pattern, n, coeffs=16)
    m = pkg.scene.to_model({k: v.copy() for k, v in arrays.items()}, dev)       # `arrays` is shared and read-only
    opt = pkg.FusedAdam(m)
    for i in range(5):
        opt.m_[i].normal_()
        opt.v_[i].uniform_(0.5, 1.0)
    m_before, v_before = [t.clone() for t in opt.m_], [t.clone() for t in opt.v_]
    cfg = pkg.MCMCConfig(relocate_cap=cc.MCMC_CAP, seed=cc.MCMC_SEED)
    src_dev = torch.full((n,), -1, dtype=torch.int32, device=dev)
    st = pkg.MCMCController(cfg, cc.MCMC_EXTENT).relocate(m, cc.MCMC_STEP, optimizer=opt, sources_out=src_dev)
    ref = mr.MCMCRef(orc, cc.MCMC_EXTENT, relocate_cap=cc.MCMC_CAP, seed=cc.MCMC_SEED)
    want, (nd, M, dst, src) = ref.relocate(arrays, cc.MCMC_STEP)
    cap = int(np.float32(cc.MCMC_CAP) * np.float32(n))
    assert st.num_dead == nd and st.num_relocated == M and M > 0
    if pattern in ("dead_tail", "sparse_dead"):
        assert M == nd < cap                     # fewer dead rows than the cap: all of them move
    else:
        assert M == cap and M < nd
    assert np.array_equal(np_(src_dev)[:M], src)
    if pattern == "one_alive":
        assert (np_(src_dev)[:M] == n - 1).all()
    got = {k: np_(getattr(m, k)) for k in MCMC_NAMES}
    for k in ("sh_coeffs", "rotations", "scales", "opacities"):
        assert np.array_equal(got[k], want[k]), k
    # positions: the bound of test_gpu_mcmc.py::test_relocation_exact_against_oracle
    d = np.abs(got["positions"][dst].astype(np.float64) - want["positions"][dst])
    assert (d <= np.spacing(np.abs(want["positions"][dst])) + 4e-6 * cc.MCMC_EXTENT * 0.01).all()
    assert (d <= np.spacing(np.abs(want["positions"][dst]))).mean() > 0.99
    untouched = np.ones(n, bool)
    untouched[dst] = False
    for k in MCMC_NAMES:
        assert np.array_equal(got[k][untouched], arrays[k][untouched]), k
    # moments: zero on the relocated rows, untouched elsewhere
    moved = torch.from_numpy(~untouched).to(dev)
    for i, name in enumerate(opt._names):
        for now, old in ((opt.m_[i], m_before[i]), (opt.v_[i], v_before[i])):
            assert torch.equal(now[~moved], old[~moved]), name
            assert not bool(now[moved].any()), name


# ---- 5. small related checks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [COPY, STATE])
def test_apply_on_four_byte_aligned_rows(pkg, dev, mode):
    """Rows of 12 floats whose src / dst start one float past a 16-byte boundary: valid input (the header asks for no
    more than a float's alignment), routed to k_gather_rows instead of k_gather_rows4.  Same bytes as the aligned call."""
    from cugs_amd._lib import DensifyArray, check, lib
    n, rf = 3001, 12
    flags = torch.from_numpy(cc.flag_bytes("random", n)).to(dev)
    ws, counts = _plan(lib, check, flags)
    n_out = counts[3]
    assert counts == cc.expected_map(cc.flag_bytes("random", n))[0] and n_out > n
    src_buf = torch.randn(n * rf + 1, device=dev)
    src_off, src_al = src_buf[1:], src_buf[1:].clone()
    dst_buf = torch.full((n_out * rf + 1,), -7.0, device=dev)
    dst_al = torch.full((n_out * rf,), -7.0, device=dev)
    assert src_off.data_ptr() % 16 == 4 and dst_buf[1:].data_ptr() % 16 == 4
    assert src_al.data_ptr() % 16 == 0 and dst_al.data_ptr() % 16 == 0
    _apply(lib, check, DensifyArray, n, n_out, ws, [(src_al, dst_al, rf, mode), (src_off, dst_buf[1:], rf, mode)])
    assert float(dst_buf[0]) == -7.0                                             # nothing written before the rows
    assert torch.equal(dst_buf[1:], dst_al)
    rows = torch.from_numpy(cc.expected_map(cc.flag_bytes("random", n))[1]).to(dev)
    want = src_al.view(n, rf)[rows]
    if mode == STATE:
        want[counts[0]:] = 0.0
    assert torch.equal(dst_al.view(n_out, rf), want)


def test_classify_on_the_thresholds(pkg, orc, dev):
    """k_classify compares with >=, < and <=; every row here sits exactly on a threshold or one ulp beside it."""
    from cugs_amd._lib import check, lib
    f32 = np.float32
    thr = f32(0.0002)
    below = np.nextafter(thr, f32(0))
    s0 = f32(-1.25)
    e = f32(orc.expf(np.array([s0], f32))[0])                                    # cugs_expf(s0), as the device has it
    up, down = np.nextafter(e, f32(np.inf)), np.nextafter(e, f32(0))
    CLONE, SPLIT, KEEP = 1, 2, 4

    def classify(accum, count, radii, scales, opa, grad_thr, size_thr, opa_thr, size_pruning, max_screen, ws_thr):
        n = len(accum)
        rows = [torch.tensor(np.asarray(a, f32).reshape(shape), device=dev)       # named: alive until the read-back
                for a, shape in ((accum, (n,)), (count, (n,)), (radii, (n,)), (scales, (n, 3)), (opa, (n, 1)))]
        flags = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        avg = torch.full((n,), -1.0, device=dev)
        check(lib.cugs_densify_classify(n, *(_P(r) for r in rows), float(grad_thr), float(size_thr),
                                        float(opa_thr), int(size_pruning), float(max_screen), float(ws_thr), _P(flags),
                                        _P(avg), _stream()), "cugs_densify_classify")
        return np_(flags).tolist(), np_(avg)

    small, wide = [-9.0, -9.5, -10.0], [s0 - f32(1), s0, s0 - f32(2)]
    # the average gradient: >= is high; count 0 divides by 1; thresholds far from the scales (small: clone)
    accum = [thr, below, thr, f32(2) * thr, f32(2) * below, f32(0)]
    count = [1, 1, 0, 2, 2, 0]
    flags, avg = classify(accum, count, [0] * 6, [small] * 6, [0.0] * 6, thr, 0.08, 0.05, 1, 20, 0.8)
    assert flags == [KEEP | CLONE, KEEP, KEEP | CLONE, KEEP | CLONE, KEEP, KEEP]
    assert np.array_equal(avg, np.array([thr, below, thr, thr, below, 0], f32))
    # max_scale == size_threshold == ws_threshold: split (>=), not clone (<), kept (<=)
    one = lambda size_thr, ws_thr, pruning=1, radius=0.0, screen=20, opa_thr=0.05: classify(
        [thr], [1], [radius], [wide], [0.0], thr, size_thr, opa_thr, pruning, screen, ws_thr)[0][0]
    assert one(e, e) == KEEP | SPLIT
    assert one(up, e) == KEEP | CLONE                      # threshold one ulp up: max_scale < it, a clone
    assert one(down, e) == KEEP | SPLIT
    assert one(e, down) == SPLIT                           # world-size threshold one ulp down: max_scale > it, pruned
    assert one(e, up) == KEEP | SPLIT
    # the screen-size test: <= keeps; 0 switches it off
    assert one(e, e, radius=20.0) == KEEP | SPLIT
    assert one(e, e, radius=21.0) == SPLIT
    assert one(e, e, radius=1000.0, screen=0) == KEEP | SPLIT
    # without size pruning neither size test applies
    assert one(e, down, pruning=0, radius=1000.0) == KEEP | SPLIT
    # the opacity threshold: cugs_sigmoidf(0) is exactly 0.5, and >= keeps
    assert one(e, e, opa_thr=0.5) == KEEP | SPLIT
    assert one(e, e, opa_thr=np.nextafter(f32(0.5), f32(1))) == SPLIT
