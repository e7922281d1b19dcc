"""The inputs of tests/test_gpu_compaction_scale.py checked on their CPU references alone (no GPU): the flag patterns
put every channel's counts where the scan's carry between passes matters, the densification inputs keep every row away
from every threshold by more than the device's exp / sigmoid may differ from torch's, and the relocation cases draw
sources and relocate rows in the passes they are meant to reach."""
import numpy as np
import pytest
import torch

import compaction_cases as cc
import mcmc_ref as mr
from test_densify_oracle import load_densify_oracle

BIG = cc.SIZES[2]


@pytest.fixture(scope="module")
def do():
    return load_densify_oracle()


@pytest.fixture(scope="module", autouse=True)
def _release_references():
    yield
    cc.release()


def test_sizes_and_passes():
    assert cc.SIZES == (262144, 262145, 525315)
    assert [cc.num_passes(n) for n in cc.SIZES] == [1, 2, 3]
    assert -(-BIG // cc.CHUNK) == 514 and BIG % cc.CHUNK == 3
    assert cc.num_passes(cc.PASS - 1) == 1 and cc.num_passes(2 * cc.PASS + 1) == 3


def test_expected_map_on_a_hand_case():
    #                      keep  clone  split  keep+clone  keep+split  none  all
    flags = np.array([4, 1, 2, 5, 6, 0, 7], np.uint8)
    counts, rows = cc.expected_map(flags)
    assert counts == (2, 3, 3, 11)
    assert rows.tolist() == [0, 3] + [1, 3, 6] + [2, 4, 6] + [2, 4, 6]


@pytest.mark.parametrize("n", cc.SIZES)
def test_flag_patterns_are_what_they_say(n):
    rows = np.arange(n)
    for pattern in cc.FLAG_PATTERNS:
        f = cc.flag_bytes(pattern, n)
        assert f.shape == (n,) and f.dtype == np.uint8 and int(f.max(initial=0)) <= 7
        assert np.array_equal(f, cc.flag_bytes(pattern, n))                       # a function of (pattern, n)
    assert cc.expected_map(cc.flag_bytes("keep_all", n))[0] == (n, 0, 0, n)
    assert np.array_equal(cc.expected_map(cc.flag_bytes("keep_all", n))[1], rows)
    assert cc.expected_map(cc.flag_bytes("split_all", n))[0] == (0, 0, n, 2 * n)
    assert cc.expected_map(cc.flag_bytes("none", n))[0] == (0, 0, 0, 0)
    ends = cc.flag_bytes("chunk_ends", n)
    assert ends[n - 1] != 0 and (ends[cc.CHUNK - 1::cc.CHUNK] != 0).all()
    assert np.count_nonzero(ends) == n // cc.CHUNK + (1 if n % cc.CHUNK else 0)
    # by_pass: three pure runs, every later scan pass pure
    k, c, m = cc.flag_masks(cc.flag_bytes("by_pass", n))
    assert k.any() and c.any() and m.any() and not (k & c).any() and not (c & m).any() and (k | c | m).all()
    assert rows[k].max() < rows[c].min() and rows[c].max() < rows[m].min()
    per_pass = cc.flag_counts_per_pass(cc.flag_bytes("by_pass", n))
    assert (np.count_nonzero(per_pass[1:], axis=1) == 1).all()


def test_flag_counts_meet_the_carry():
    # random and skewed at three passes: every channel counts in at least two passes, so a lost, swapped or truncated
    # carry of any channel moves rows
    for pattern in ("random", "skewed"):
        per_pass = cc.flag_counts_per_pass(cc.flag_bytes(pattern, BIG))
        assert per_pass.shape == (3, 3) and (np.count_nonzero(per_pass, axis=0) >= 2).all(), pattern
    # by_pass is by its definition the opposite: every channel counts in its own pass only, so the carries that
    # enter the second and third pass are (PASS, 0, 0) and (PASS, PASS, 0) - a channel that picks up another's
    # carry lands on a different row
    assert cc.flag_counts_per_pass(cc.flag_bytes("by_pass", BIG)).tolist() == \
        [[cc.PASS, 0, 0], [0, cc.PASS, 0], [0, 0, BIG - 2 * cc.PASS]]
    # skewed: per pass three different non-zero totals, wherever the pass has the rows for it (a second pass of one
    # row, at PASS + 1, cannot: its row is a kept one)
    for n in cc.SIZES:
        per_pass = cc.flag_counts_per_pass(cc.flag_bytes("skewed", n))
        for p, (k, c, m) in enumerate(per_pass.tolist()):
            if n - p * cc.PASS >= 16:
                assert min(k, c, m) > 0 and len({k, c, m}) == 3, (n, p)
            else:
                assert (k, c, m) == (1, 0, 0), (n, p)
    # chunk_ends: the last chunk's only flagged row is n - 1, in the last pass
    assert cc.count_per_pass(cc.flag_bytes("chunk_ends", BIG) != 0, BIG).tolist() == [256, 256, 2]


@pytest.mark.parametrize("n,coeffs", [(cc.SIZES[1], 4), (BIG, 4), (3001, 1), (3001, 9), (3001, 16)])
def test_densify_inputs_keep_their_margins(do, n, coeffs):
    ref = cc.densify_reference(do, n, coeffs)
    t = ref.inputs.tensors
    # by the oracle's own values (torch.exp / torch.sigmoid / its accumulators)
    max_scale = torch.exp(t["scales"]).max(dim=1)[0].numpy()
    assert cc.ulp_distance(max_scale, cc.SIZE_THRESHOLD).min() >= cc.ULP_MARGIN
    assert cc.ulp_distance(max_scale, cc.WS_THRESHOLD).min() >= cc.ULP_MARGIN
    assert cc.ulp_distance(torch.sigmoid(t["opacities"]).numpy(), cc.OPACITY_THRESHOLD).min() >= cc.ULP_MARGIN
    avg = ref.acc.grad_accum.astype(np.float64) / np.maximum(ref.acc.grad_count, 1.0)
    thr = float(cc.GRAD_THRESHOLD)
    assert np.abs(avg - thr).min() >= cc.GRAD_MARGIN * thr
    assert (ref.acc.grad_count > 0).mean() > 0.9 and (avg > thr).any() and (avg < thr).any()
    # every decision on both sides of its threshold
    assert (max_scale < cc.SIZE_THRESHOLD).any() and (max_scale > cc.WS_THRESHOLD).any()
    assert ref.acc.max_radii.max() > 20 and (ref.acc.max_radii <= 20).any()
    s = ref.stats
    assert s.num_cloned == int(ref.clone.sum()) > 0 and s.num_split == int(ref.split.sum()) > 0
    assert s.num_after == int(ref.survive.sum()) + s.num_cloned + 2 * s.num_split
    assert s.num_pruned > s.num_split
    # clones, splits and pruned originals in every scan pass; a last pass of ONE row (PASS + 1) can hold one decision
    # only, and holds a split parent, which is a pruned original too
    full = cc.num_passes(n) - (1 if n % cc.PASS == 1 else 0)
    for mask in (ref.clone, ref.split, ~ref.survive):
        assert (cc.count_per_pass(mask, n)[:full] > 0).all()
    if n % cc.PASS == 1:
        assert ref.split[n - 1] and not ref.clone[n - 1] and not ref.survive[n - 1]


def test_split_children_restatement_is_the_oracles_to_rounding(do, orc):
    ref = cc.densify_reference(do, 3001, 1)
    pos, scl = cc.split_children(orc, ref.inputs, ref.split)
    m = ref.stats.num_split
    assert pos.shape == scl.shape == (2 * m, 3) and pos.dtype == scl.dtype == np.float32
    want_pos, want_scl = ref.model.positions.numpy()[-2 * m:], ref.model.scales.numpy()[-2 * m:]
    assert np.allclose(scl, want_scl, rtol=0, atol=1e-6)
    assert np.max(np.abs(pos - want_pos)) <= 1e-6 * max(1.0, np.abs(want_pos).max())


def test_prune_masks():
    m = cc.prune_mask("second_pass", BIG)
    assert int(m.sum()) == cc.PASS and m[cc.PASS] and m[2 * cc.PASS - 1] and not m[cc.PASS - 1] and not m[2 * cc.PASS]
    r = cc.prune_mask("random", BIG)
    assert (cc.count_per_pass(r, BIG) > 0).all() and (cc.count_per_pass(~r, BIG) > 0).all()


def test_mcmc_cases_listed():
    assert cc.MCMC_CASES == ((cc.SIZES[0], "mixture"), (cc.SIZES[0], "one_alive"),
                             (cc.SIZES[1], "mixture"), (cc.SIZES[1], "dead_head"), (cc.SIZES[1], "one_alive"),
                             (cc.SIZES[1], "sparse_dead"),
                             (BIG, "mixture"), (BIG, "dead_tail"), (BIG, "dead_head"), (BIG, "one_alive"),
                             (BIG, "sparse_dead"))


@pytest.mark.parametrize("n,pattern", cc.MCMC_CASES)
def test_mcmc_reference_reaches_the_passes(orc, n, pattern):
    ref = mr.MCMCRef(orc, cc.MCMC_EXTENT, relocate_cap=cc.MCMC_CAP, seed=cc.MCMC_SEED)
    arrays = cc.mcmc_arrays(pattern, n, coeffs=1)
    dead = ref.sigmoid(arrays["opacities"][:, 0]) < ref.thr
    _, (nd, moved, dst, src) = ref.relocate(arrays, cc.MCMC_STEP)
    cap = int(np.float32(cc.MCMC_CAP) * np.float32(n))
    assert nd == int(dead.sum()) > 0 and moved == min(nd, cap) == dst.size == src.size
    assert dead[dst].all() and not dead[src].any()
    src_passes, dst_passes = cc.count_per_pass(src, n) > 0, cc.count_per_pass(dst, n) > 0
    alive_passes, dead_passes = cc.count_per_pass(~dead, n) > 0, cc.count_per_pass(dead, n) > 0
    if pattern == "mixture":
        # sources in every pass (but a second pass of one row, at PASS + 1, is too narrow to expect a draw in); the
        # relocated rows are the FIRST `cap` dead ones, so they stay in the first pass: sparse_dead is the case whose
        # relocated rows lie behind a non-zero carry of the dead count
        wide = np.bincount(cc.pass_of(np.arange(n))) >= cc.CHUNK
        assert alive_passes[wide].all() and src_passes[wide].all() and moved == cap < nd
        assert dst_passes.tolist() == [True] + [False] * (cc.num_passes(n) - 1)
    elif pattern == "dead_tail":
        # fewer dead rows than the cap: all relocated, all in the third pass.  The dead count carried into that
        # pass is 0 here; what the case pins is a dead list that starts two passes in, beside weight in every pass
        assert moved == nd < cap and dst.min() >= 2 * cc.PASS and np.array_equal(dst_passes, dead_passes)
        assert alive_passes.all() and src_passes[:2].all()
    elif pattern == "dead_head":
        # no weight in the first pass: every source's CDF value includes a carry of the weight
        assert moved == cap < nd and src.min() >= cc.PASS and dst.max() < cc.PASS
        assert np.array_equal(src_passes, alive_passes) and np.array_equal(dst_passes, dead_passes)
    elif pattern == "one_alive":
        assert moved == cap and (src == n - 1).all()
    else:
        # sparse_dead: every dead row moves and every pass has some, the last row included, so the dead rows of the
        # second and third pass take their slot of the dead list from a non-zero carry of the dead count
        assert pattern == "sparse_dead" and moved == nd < cap and np.array_equal(dst, np.nonzero(dead)[0])
        assert dead_passes.all() and np.array_equal(dst_passes, dead_passes) and dead[n - 1]
        carried = np.cumsum(cc.count_per_pass(dead, n))[:-1]
        assert (carried > 0).all() and (cc.count_per_pass(dst, n)[1:] > 0).all()
        wide = np.bincount(cc.pass_of(np.arange(n))) >= cc.CHUNK
        assert alive_passes[wide].all() and src_passes[wide].all()
