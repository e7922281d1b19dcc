"""A host model of render()'s per-stream sort state ("No host round trip"; INTEGRATION.md, sort rows).

Pure Python, written from the documented rules and not from the host mirror's code: tests/test_gpu_sort_sequences.py
drives render() over scripted lists of views and asks this model which C entry points, which pair capacity and how many
blocking re-sorts each frame must take, given only what the oracle knows about the frame.

The rules:
  * first frame on a stream (no estimate yet), or an image without tiles: the exact two-call path,
    cugs_sort_count_pairs + cugs_sort_pairs, which blocks for the pair count; the count becomes the estimate.
  * otherwise the sort runs on a PREDICTED capacity and the host reads the count afterwards:
      estimate   e' = max(p, floor(0.97 e)) after a frame that fitted, e' = p after one that did not;
      capacity   needed = floor(1.10 e) + 64 Ki; the capacity in use is HELD while needed <= held <= 1.25 needed,
                 dropped to `needed` when the estimate has fallen further, and grown to floor(1.05 needed) otherwise.
    A frame whose count exceeds the capacity is a miss: one blocking re-sort on the exact path (and a second blend).
  * depth route: a predicted sort on the narrow route of a view with a pair-emitting splat outside
    [0.2, ~13 107) reports -1: a miss, one blocking re-sort on the general route (cugs_sort_count_pairs_wide), the exact
    count becomes the estimate, and the stream's wide counter is set to WIDE_DEPTH_HOLD.  While the counter is positive
    every sort of the stream takes the general route (cugs_sort_pairs_predicted_wide, cugs_sort_count_pairs_wide) and
    decrements it; at 0 the next sort probes the narrow route again.  The blocking path never sets the counter
    (cugs_sort_count_pairs repeats on the general route by itself).
  * the projection keys the sort (cugs_project_forward_keyed) exactly when the sort that follows is a narrow one:
    a keyed projection must be consumed by a narrow sort (include/cugs_hip.h).
  * the blend kernels' tile order is asked for when the estimate is at least TILE_ORDER_MIN_PAIRS: the keyed sort
    writes it itself (cugs_sort_pairs_predicted_keyed_ordered), every other route adds a cugs_tile_order launch.
  * a model without Gaussians is not sorted at all and touches no state.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

DECAY = 0.97
MARGIN = (1.10, 65536)
HOLD_SLACK = 1.25
GROW_SPARE = 1.05
WIDE_DEPTH_HOLD = 256
TILE_ORDER_MIN_PAIRS = 2_000_000
INT_MAX = 2147483647
TILE = 16

# the narrow depth route covers 2^27 float bit patterns from 0.2f on (three 9-bit passes): [0.2, ~13 107)
DEPTH_KEY_BASE = 0x3E4CCCCC            # bits of 0.2f, minus one
DEPTH_KEY_SPAN = 1 << 27

PROJECT, PROJECT_KEYED = "cugs_project_forward", "cugs_project_forward_keyed"
COUNT, COUNT_WIDE, PAIRS = "cugs_sort_count_pairs", "cugs_sort_count_pairs_wide", "cugs_sort_pairs"
KEYED, KEYED_ORDERED = "cugs_sort_pairs_predicted_keyed", "cugs_sort_pairs_predicted_keyed_ordered"
WIDE, TILE_ORDER = "cugs_sort_pairs_predicted_wide", "cugs_tile_order"


def out_of_narrow_range(depths, tiles_touched, radii) -> bool:
    """Does a splat that emits pairs lie outside the narrow depth route's range?  (The oracle's projection outputs.)"""
    bits = np.ascontiguousarray(depths, np.float32).view(np.uint32).astype(np.int64)
    off = (bits - DEPTH_KEY_BASE) % (1 << 32)
    emits = (np.asarray(tiles_touched) > 0) & (np.asarray(radii) > 0)
    return bool(np.any(emits & ~((off >= 1) & (off < DEPTH_KEY_SPAN))))


def pair_route(n: int, width: int, height: int, capacity: int, keyed: bool) -> str:
    """The pair-level route the library plans for a PREDICTED sort (csrc/sort_workspace.h, make_sort_plan) - chosen from
    the capacity, not from the live count: "direct" / "direct_staged" (keyed, rectangles packable: at most 127 x 127
    tiles, at most 10 240 tiles, at most 2 Mi Gaussians), "column" (at most 256 x 256 tiles and capacity >= 13 n),
    else "radix"."""
    ntx, nty = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    if keyed and ntx <= 127 and nty <= 127 and ntx * nty <= 10240 and n <= 4096 * 512 and capacity < (1 << 30):
        return "direct_staged" if capacity >= 13 * n else "direct"
    if ntx <= 256 and nty <= 256 and capacity >= 13 * n:
        return "column"
    return "radix"


@dataclass
class Frame:
    """What the model says about one render()."""
    calls: Tuple[str, ...]              # projection and sort entry points, in call order, re-sorts included
    capacity: Optional[int]             # capacity handed to the predicted sort; None on the blocking path / no sort
    valid: bool                         # False: a miss (the predicted sort's outputs were not usable)
    resorts: int                        # blocking re-sorts after the predicted sort (0 or 1)
    wide_found: bool = False            # the miss was a depth outside the narrow range
    route: Optional[str] = None         # pair_route() of the predicted sort


@dataclass
class StreamModel:
    estimate: Optional[int] = None
    held: Optional[int] = None
    wide: int = 0
    history: List[Frame] = field(default_factory=list)

    def capacity_for(self, estimate: int) -> int:
        needed = min(int(estimate * MARGIN[0]) + MARGIN[1], INT_MAX)
        if self.held is not None and needed <= self.held <= needed * HOLD_SLACK:
            return self.held
        if self.held is None or needed < self.held:
            self.held = needed
        else:
            self.held = min(int(needed * GROW_SPARE), INT_MAX)
        return self.held

    def frame(self, pairs: int, out_of_range: bool, n: int, width: int, height: int) -> Frame:
        f = self._frame(int(pairs), bool(out_of_range), int(n), int(width), int(height))
        self.history.append(f)
        return f

    def _frame(self, p, out_of_range, n, width, height) -> Frame:
        if n == 0:
            return Frame((), None, True, 0)
        tiles = ((width + TILE - 1) // TILE) * ((height + TILE - 1) // TILE)
        wide = self.wide > 0
        order = (self.estimate or 0) >= TILE_ORDER_MIN_PAIRS
        calls = [PROJECT if wide else PROJECT_KEYED]
        if wide:
            self.wide -= 1
        if self.estimate is None or tiles == 0:
            calls.append(COUNT_WIDE if wide else COUNT)
            if tiles > 0:
                calls.append(PAIRS)
            if order and tiles > 0:
                calls.append(TILE_ORDER)
            self.estimate = p
            return Frame(tuple(calls), None, True, 0)
        prev = self.estimate
        cap = self.capacity_for(prev)
        route = pair_route(n, width, height, cap, keyed=not wide)
        if wide:
            calls.append(WIDE)
            if order:
                calls.append(TILE_ORDER)
        else:
            calls.append(KEYED_ORDERED if order else KEYED)
        if not wide and out_of_range:                   # the count word says -1
            self.wide = WIDE_DEPTH_HOLD
            self.estimate = p
            calls += [COUNT_WIDE, PAIRS] + ([TILE_ORDER] if order else [])
            return Frame(tuple(calls), cap, False, 1, wide_found=True, route=route)
        if p > cap:
            self.estimate = p
            calls += [COUNT_WIDE if self.wide > 0 else COUNT, PAIRS] + ([TILE_ORDER] if order else [])
            return Frame(tuple(calls), cap, False, 1, route=route)
        self.estimate = max(p, int(prev * DECAY))
        return Frame(tuple(calls), cap, True, 0, route=route)
