// sort_bin_cover.h — which tiles of one 8 x 8 tile block a packed rectangle covers, as a 64-bit mask.
// Plain integer C++ with no other header of the project behind it: the binning scatter (sort_bin.h) calls it on the
// device, and tests/test_bin_cover_mask.py compiles it for the host and checks it against a double loop.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CUGS_BIN_HD __host__ __device__ __forceinline__
#else
#define CUGS_BIN_HD static inline
#endif

// prect: a packed rectangle in tiles (pack_rect: x0 | y0 << 7 | w << 14 | h << 21; bit 31 = no rectangle).
// (blk_tx0, blk_ty0): the block's first tile.  Bit ty_local * 8 + tx_local of the result is set when the rectangle covers
// tile (blk_tx0 + tx_local, blk_ty0 + ty_local); 0 when it misses the block or there is no rectangle.
CUGS_BIN_HD uint64_t bin_cover_mask(uint32_t prect, uint32_t blk_tx0, uint32_t blk_ty0) {
    const int x0 = (int)(prect & 127u), y0 = (int)((prect >> 7) & 127u);
    const int w = (int)((prect >> 14) & 127u), h = (int)((prect >> 21) & 127u);
    // the rectangle clipped to the block, in the block's own coordinates: columns [xa, xb), rows [ya, yb), all within 0..8
    int xa = x0 - (int)blk_tx0, xb = xa + w, ya = y0 - (int)blk_ty0, yb = ya + h;
    xa = xa < 0 ? 0 : xa; xb = xb > 8 ? 8 : xb;
    ya = ya < 0 ? 0 : ya; yb = yb > 8 ? 8 : yb;
    if ((prect & 0x80000000u) || xa >= xb || ya >= yb) return 0ull;
    const uint32_t cols = (1u << xb) - (1u << xa);                    // one row's bits
    const uint32_t four = cols * 0x01010101u;                         // four rows
    const uint64_t all = ((uint64_t)four << 32) | four;               // all eight
    return (all >> (8 * (8 - (yb - ya)))) << (8 * ya);                // yb - ya rows (1..8), moved up to row ya (0..7)
}
