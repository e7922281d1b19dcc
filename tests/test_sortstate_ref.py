"""The host model of render()'s sort state (tests/sortstate_ref.py) on hand-written sequences: every expected value
below is worked out in the comment next to it, from the rules in DESIGN.md 4.2 (CPU only)."""
import numpy as np
import pytest

import sortstate_ref as M
from sortstate_ref import (COUNT, COUNT_WIDE, KEYED, KEYED_ORDERED, PAIRS, PROJECT, PROJECT_KEYED, TILE_ORDER, WIDE,
                           StreamModel)

N, W, H = 20000, 640, 360           # 40 x 23 tiles; 13 N = 260 000


def test_first_frame_blocks_and_seeds_the_estimate():
    m = StreamModel()
    f = m.frame(100_000, False, N, W, H)
    assert f.calls == (PROJECT_KEYED, COUNT, PAIRS) and f.capacity is None and f.valid and f.resorts == 0
    assert (m.estimate, m.held, m.wide) == (100_000, None, 0)
    # an out-of-range view on the blocking path repeats inside cugs_sort_count_pairs: the counter stays 0
    m2 = StreamModel()
    f = m2.frame(100_000, True, N, W, H)
    assert f.calls == (PROJECT_KEYED, COUNT, PAIRS) and f.valid and m2.wide == 0


def test_estimate_decays_and_capacity_is_held_grown_and_released():
    m = StreamModel()
    m.frame(100_000, False, N, W, H)
    # needed = floor(1.10 * 100 000) + 65 536 = 175 536; nothing held yet: that is the capacity.  < 13 N: unstaged
    f = m.frame(100_000, False, N, W, H)
    assert (f.calls, f.capacity, f.valid, f.resorts, f.route) == ((PROJECT_KEYED, KEYED), 175_536, True, 0, "direct")
    assert m.estimate == 100_000                       # max(100 000, 97 000)
    f = m.frame(90_000, False, N, W, H)
    assert f.capacity == 175_536 and m.estimate == 97_000          # max(90 000, floor(0.97 * 100 000))
    # estimate 97 000: needed = 106 700 + 65 536 = 172 236 <= held 175 536 <= 215 295: held
    f = m.frame(50_000, False, N, W, H)
    assert f.capacity == 175_536 and m.estimate == 94_090          # max(50 000, floor(0.97 * 97 000) = 94 090)
    # a dense view: needed = floor(103 499) + 65 536 = 169 035, held 175 536 stays; 400 000 pairs do not fit
    f = m.frame(400_000, False, N, W, H)
    assert (f.calls, f.capacity, f.valid, f.resorts) == ((PROJECT_KEYED, KEYED, COUNT, PAIRS), 175_536, False, 1)
    assert not f.wide_found and m.estimate == 400_000              # after an overflow: the count itself
    # needed = 440 000 + 65 536 = 505 536 > held: grown with 5 % to spare, floor(530 812.8); >= 13 N: staged
    f = m.frame(400_000, False, N, W, H)
    assert (f.capacity, f.valid, f.route) == (530_812, True, "direct_staged")
    # dense -> sparse: the capacity is held (stale), so the sparse view runs the staged variant
    f = m.frame(100_000, False, N, W, H)
    assert (f.capacity, f.valid, f.route) == (530_812, True, "direct_staged") and m.estimate == 388_000
    # the estimate decays 388 000 -> 376 360 -> 365 069 -> 354 116 -> 343 492 -> 333 187 -> 323 191; the capacity is
    # held while 530 812 <= 1.25 needed, i.e. needed >= 424 650, i.e. estimate >= 326 468: five more held frames ...
    seen = []
    for _ in range(6):
        f = m.frame(100_000, False, N, W, H)
        seen.append((f.capacity, m.estimate))
    assert seen == [(530_812, 376_360), (530_812, 365_069), (530_812, 354_116), (530_812, 343_492), (530_812, 333_187),
                    (530_812, 323_191)]
    # ... and the frame that starts from 323 191 releases it: needed = floor(355 510.1) + 65 536 = 421 046 (staged still)
    f = m.frame(100_000, False, N, W, H)
    assert (f.capacity, f.route, m.held) == (421_046, "direct_staged", 421_046)
    # far down, estimate 100 000 again (needed 175 536): whatever is held by then lies within 1.25 of that, 219 420,
    # which is below 13 N - the unstaged variant is back
    while m.estimate > 100_000:
        m.frame(100_000, False, N, W, H)
    f = m.frame(100_000, False, N, W, H)
    assert 175_536 <= f.capacity <= 219_420 and f.route == "direct" and f.valid


def test_wide_counter_hold_and_probe():
    m = StreamModel()
    m.frame(1000, False, N, W, H)
    # narrow -> wide: keyed, capacity 1100 + 65 536, the count word says -1: one re-sort on the general route
    f = m.frame(1200, True, N, W, H)
    assert (f.calls, f.capacity, f.valid, f.resorts, f.wide_found) == \
        ((PROJECT_KEYED, KEYED, COUNT_WIDE, PAIRS), 66_636, False, 1, True)
    assert (m.wide, m.estimate) == (256, 1200)         # the exact count is the next prediction
    # wide again: the projection does not key the sort, the general route at once, no miss.  1320 + 65 536 = 66 856 is
    # above the held 66 636: grown, floor(1.05 * 66 856) = 70 198
    f = m.frame(1200, True, N, W, H)
    assert (f.calls, f.capacity, f.valid, f.resorts) == ((PROJECT, WIDE), 70_198, True, 0) and m.wide == 255
    # an in-range view inside the hold: the general route still
    f = m.frame(1000, False, N, W, H)
    assert f.calls == (PROJECT, WIDE) and f.valid and m.wide == 254
    for left in range(253, -1, -1):
        f = m.frame(1000, False, N, W, H)
        assert f.calls == (PROJECT, WIDE) and m.wide == left
    # the probe: keyed and narrow again, valid, the counter stays 0
    f = m.frame(1000, False, N, W, H)
    assert (f.calls, f.valid, f.resorts) == ((PROJECT_KEYED, KEYED), True, 0) and m.wide == 0
    # a probe with a view that is still wide: -1 again, the hold starts over
    f = m.frame(1000, True, N, W, H)
    assert f.calls == (PROJECT_KEYED, KEYED, COUNT_WIDE, PAIRS) and not f.valid and m.wide == 256


def test_capacity_miss_inside_and_at_the_end_of_the_hold():
    m = StreamModel(estimate=1000, wide=2)
    # 66 636 < 70 000: a miss on the general route re-sorts on the general route while the counter is positive (1 left) ...
    f = m.frame(70_000, True, N, W, H)
    assert (f.calls, f.valid, f.resorts, f.wide_found) == ((PROJECT, WIDE, COUNT_WIDE, PAIRS), False, 1, False)
    assert (m.wide, m.estimate) == (1, 70_000)
    # ... and on the plain blocking entry (which repeats by itself) when this sort was the last of the hold.
    # needed = 77 000 + 65 536 = 142 536, grown: floor(149 662.8)
    f = m.frame(200_000, True, N, W, H)
    assert (f.calls, f.capacity, f.valid) == ((PROJECT, WIDE, COUNT, PAIRS), 149_662, False) and m.wide == 0


def test_empty_model_and_empty_image_and_tile_order():
    m = StreamModel(estimate=5000, held=71_036, wide=3)
    f = m.frame(0, False, 0, W, H)                      # no Gaussians: not sorted, nothing moves
    assert f.calls == () and f.valid and (m.estimate, m.held, m.wide) == (5000, 71_036, 3)
    f = m.frame(0, False, N, 0, H)                      # no tiles: the blocking entry, count only; a sort, so it counts
    assert f.calls == (PROJECT, COUNT_WIDE) and (m.estimate, m.wide) == (0, 2)
    # zero pairs is an ordinary count: capacity 0 + 65 536 (held 71 036 <= 81 920 stays)
    m = StreamModel(estimate=0, held=71_036)
    f = m.frame(0, False, N, W, H)
    assert (f.calls, f.capacity, f.valid) == ((PROJECT_KEYED, KEYED), 71_036, True) and m.estimate == 0
    # the tile order from 2 M pairs on (the estimate BEFORE the frame decides)
    m = StreamModel(estimate=1_999_999)
    assert m.frame(2_000_000, False, N, W, H).calls == (PROJECT_KEYED, KEYED)
    # (that frame held floor(2 199 998.9) + 65 536 = 2 265 534; this one needs 2 265 536: grown, floor(2 378 812.8))
    f = m.frame(2_000_000, False, N, W, H)
    assert f.calls == (PROJECT_KEYED, KEYED_ORDERED) and f.capacity == 2_378_812
    m.wide = 1
    assert m.frame(2_000_000, False, N, W, H).calls == (PROJECT, WIDE, TILE_ORDER)
    # ... a miss re-sorts with the order too.  the capacity held, 2 378 812, is below 3 000 000
    f = m.frame(3_000_000, False, N, W, H)
    assert f.calls == (PROJECT_KEYED, KEYED_ORDERED, COUNT, PAIRS, TILE_ORDER) and not f.valid
    m = StreamModel()
    assert m.frame(3_000_000, False, N, W, H).calls == (PROJECT_KEYED, COUNT, PAIRS)     # first frame: no estimate


@pytest.mark.parametrize("n,w,h,cap,keyed,want", [
    (20000, 640, 360, 259_999, True, "direct"), (20000, 640, 360, 260_000, True, "direct_staged"),
    (5041, 640, 360, 65_536, True, "direct_staged"),    # 13 * 5041 = 65 533 <= the 64 Ki margin alone
    (5042, 640, 360, 65_536, True, "direct"),           # 13 * 5042 = 65 546
    (20000, 640, 360, 260_000, False, "column"), (20000, 640, 360, 259_999, False, "radix"),   # the general route
    (3000, 2032, 32, 100_000, True, "direct_staged"),   # 127 tile columns: the widest packable rectangle
    (3000, 2064, 32, 39_000, True, "column"), (3000, 2064, 32, 38_999, True, "radix"),        # 129 columns: not packable
    (3000, 4096, 16, 39_000, True, "column"),           # 256 columns: the widest column path
    (3000, 4112, 16, 1_000_000, True, "radix"),         # 257 columns
    (3000, 1920, 1712, 1_000, True, "radix"),           # 120 x 107 = 12 840 tiles > 10 240
    (4096 * 512 + 1, 640, 360, 1_000, True, "radix"),
])
def test_pair_route(n, w, h, cap, keyed, want):
    assert M.pair_route(n, w, h, cap, keyed) == want


def test_out_of_narrow_range():
    f32 = lambda *v: np.array(v, np.float32)
    one = np.array([1], np.int32)
    near = np.float32(0.2)
    # offsets 1 .. 2^27 - 1 from the pattern below 0.2f are in range: 0.2f itself is offset 1, and 0.2f * 65536 (16 binades
    # = 2^27 patterns above it) would be offset 2^27 + 1 - the last depth inside is two patterns below that
    far = np.float32(0.2) * np.float32(65536)
    out = np.nextafter(far, np.float32(0))
    assert not M.out_of_narrow_range(f32(near), one, one)
    assert M.out_of_narrow_range(f32(np.nextafter(near, np.float32(0))), one, one)
    assert not M.out_of_narrow_range(f32(np.nextafter(out, np.float32(0))), one, one)
    assert M.out_of_narrow_range(f32(out), one, one) and M.out_of_narrow_range(f32(far), one, one)
    # a splat that emits no pairs may stand anywhere
    assert not M.out_of_narrow_range(f32(50000.0, 1.0), np.array([0, 4], np.int32), np.array([3, 3], np.int32))
    assert not M.out_of_narrow_range(f32(50000.0, 1.0), np.array([4, 4], np.int32), np.array([0, 3], np.int32))
    assert M.out_of_narrow_range(f32(50000.0, 1.0), np.array([4, 4], np.int32), np.array([3, 3], np.int32))
