"""The contribution-score reference of tests/scores_ref.py pinned against the oracle's own forward, and the two scenes
checked for what they must exercise in the score kernel (CPU only)."""
import numpy as np
import pytest

from scores_ref import SCENES, scene


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("key", list(SCENES))
def test_weight_table_agrees_with_the_oracles_forward(pkg, orc, key, view):
    s = scene(key, view)
    ref, table, h, w = s["ref"], s["table"], s["h"], s["w"]
    assert table.shape == (h * w, s["n"]) and table.dtype == np.float32
    assert np.all(table >= 0.0)
    # a pixel's contributors are exactly the Gaussians with a weight there
    assert np.array_equal((table > 0.0).sum(axis=1).reshape(h, w), ref["n_contrib"])
    # and their weights sum to what the pixel lost: sum_i alpha_i T_i = 1 - T_final (fp32 products against an fp32 T)
    # Per pixel with k contributors the two sides differ by the roundings of k steps, each T <= 1: 1 - alpha and
    # T (1 - alpha) at 2^-25 each, w = alpha T at 2^-25 w - within (k + 1) 2^-24 in all.
    # On view 0 the largest difference is 1.83e-7 on 40x24 and 2.15e-7 on 33x17 (2.13e-7 against 1 - final_T formed
    # in fp32): "2e-7" to the one digit the figure was first reported with, hence the 2.5e-7 below.
    lost = table.astype(np.float64).sum(axis=1).reshape(h, w)
    diff = np.abs(lost - (1.0 - ref["final_T"].astype(np.float64)))
    print(f"{key} view {view}: max |sum w - (1 - T)| = {float(diff.max()):.3e}")
    assert np.all(diff <= (ref["n_contrib"] + 1) * 2.0 ** -24)
    if view == 0:
        assert float(diff.max()) < 2.5e-7
    assert float(table[table > 0.0].min()) >= 1.5e-5                 # no passing weight comes near underflow
    want = s["want"]
    assert want["count"].sum() == int(ref["n_contrib"].sum())
    assert np.array_equal(want["max"] > 0.0, want["count"] > 0) and np.array_equal(want["sum"] > 0.0, want["count"] > 0)


@pytest.mark.parametrize("key", list(SCENES))
def test_scene_exercises_every_path(pkg, orc, key):
    s = scene(key)
    ref, table, n, h, w = s["ref"], s["table"], s["n"], s["h"], s["w"]
    tr = ref["tile_ranges"].reshape(-1, 2)
    length = tr[:, 1] - tr[:, 0]
    assert int(length.max()) > 256                    # a second LDS batch
    assert np.any(length % 4 != 0)                    # a ragged last hit group is possible at all
    # a pixel that closed (T < 1/255) with records of its list still to come
    ntx = (w + 15) // 16
    closed_early = 0
    for py in range(h):
        for px in range(w):
            if not ref["final_T"][py, px] < 1.0 / 255.0:
                continue
            t = (py // 16) * ntx + px // 16
            ids = ref["values"][tr[t, 0]:tr[t, 1]]
            last = np.nonzero(table[py * w + px, ids] > 0.0)[0].max()
            closed_early += int(last < len(ids) - 1)
    assert closed_early > 0
    listed = np.zeros(n, bool)
    listed[ref["values"]] = True
    idle = s["want"]["count"] == 0
    print(f"{key}: longest list {int(length.max())}, {int(idle.sum())} of {n} never contribute, "
          f"{int((idle & listed).sum())} of those are in lists, {closed_early} pixels closed early")
    assert (idle & listed).any()                      # in a list, zero score
    assert (~listed).any() and idle[~listed].all()    # in no list
    assert (~idle).any()
