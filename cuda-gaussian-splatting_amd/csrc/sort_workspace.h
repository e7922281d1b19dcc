// sort_workspace.h — the sort's two workspaces, their control block, the constants that size them, and the route plan.
#pragma once

#include "cugs_gaussian_math.h"

#include <atomic>
#include <cstddef>

namespace {

constexpr int RADIX = 256;
// The depth sort of views whose depths lie in [near plane, ~13 000) - every view the reference's projection can
// produce in practice: it culls z <= 0.2 - runs THREE passes of 9 bits on the key's offset from the near plane's bit
// pattern instead of four passes of 8 bits on the raw float bits: positive floats order like their bit patterns, and
// [0.2, 13 107) spans 2^27 patterns.  A kernel boundary costs ~5 us on this part and a pass is three kernels.  The key
// kernel checks the range of every Gaussian that emits pairs; a view outside it is reported through the pair count
// (-1: "redo") and takes the four-pass route on the raw bits.
constexpr int RADIX_DEPTH = 512, DEPTH_BITS = CUGS_DEPTH_BITS;      // key range and base: cugs_gaussian_math.h (sort_record_of)
constexpr int IPT = 16;                           // items per thread
constexpr int CHUNK_MIN = CUGS_BLOCK * IPT;       // 4096 items per workgroup: depth sort; sizes the histogram buffers
constexpr int CHUNK_DEPTH = 4096;                 // items per workgroup in the three 9-bit depth passes
static_assert(CHUNK_DEPTH <= CHUNK_MIN && CHUNK_MIN % CHUNK_DEPTH == 0, "the histogram buffers are carved for CHUNK_DEPTH blocks");
constexpr int CHUNK_PAIR = CHUNK_MIN;             // pair-level passes (8192 / 16384: 4 % / 30 % slower, profiles/README.md)
constexpr int FILL_CHUNK = CUGS_BLOCK;            // Gaussians per workgroup in scan/fill (one per thread)
constexpr int COL_WAVES = 16;                     // waves per workgroup of the column-ordered emission: the longer a
constexpr int COL_CHUNK = COL_WAVES * CUGS_WAVE;  // workgroup's run in each tile column, the fewer partial lines it writes
static_assert(COL_CHUNK % FILL_CHUNK == 0, "whole FILL_CHUNK blocks per column workgroup");

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline uint32_t nblocks_for(int64_t count, int chunk) { return (uint32_t)((count + chunk - 1) / chunk); }

// Scatter offsets without a scan kernel (round 3), for passes of up to SCANFREE_MAX_BLOCKS workgroups.  A radix pass
// needs, per workgroup b and digit d, the number of items with digit d in the workgroups before b, and the digit totals.
// Round 2 got them from a third kernel per pass (k_radix_scan_rows over a digit-major table): ~5 us of kernel boundary
// for a few microseconds of work, five times a frame.  Now the histogram kernel writes its counts BLOCK-major (one
// contiguous row per workgroup) and adds them into a per-super-block table (one row per SB workgroups; atomics on a
// table zeroed by an earlier kernel of the stream: SB adds per address), and every scatter workgroup sums, with coalesced
// row loads issued at its very start and shared out over all its threads: the super rows before its own (<= nblk / SB),
// the block rows of its own super-block before it (< SB), and all super rows for the digit totals.
// Same box, config 3: sort 0.2295 -> 0.2099 ms (with the packed rectangles riding along).  What it costs is the row
// sums at the head of every scatter workgroup: (nblk / SB + SB) / GRP loads per thread, GRP = threads per digit.  Beyond
// SCANFREE_MAX_LOADS of them the third kernel stays (6 M Gaussians: 43 per thread in the depth passes, sort +17 us; 40 M
// pairs: +70-100 us, or - with a third table level - thousands of atomics per address at ~15 ns each;
// profiles/r03_m_scanfree_ab.log).
constexpr int SUP_TABLES = 4;                     // passes that may follow one zeroing: 4 depth passes (general route) / 4 pair passes (32-bit tile ids)
constexpr uint32_t SCANFREE_MAX_BLOCKS = 4096u, SCANFREE_MAX_LOADS = 26u;
inline uint32_t sup_block(uint32_t nblk) { return nblk <= 512u ? 16u : 64u; }
// grp: threads per digit of the pass's scatter workgroups (NT >> digit bits)
inline bool scan_free(uint32_t nblk, uint32_t grp) {
    const uint32_t sb = sup_block(nblk);
    return nblk <= SCANFREE_MAX_BLOCKS && ((nblk + sb - 1u) / sb + sb) <= SCANFREE_MAX_LOADS * grp;
}
inline uint32_t sup_rows(uint32_t nblk, uint32_t grp) { return scan_free(nblk, grp) ? (nblk + sup_block(nblk) - 1u) / sup_block(nblk) : 0u; }
// most rows any nblk' <= nblk can need: the workspace is carved for a capacity
inline uint32_t sup_rows_bound(uint32_t nblk) { return (nblk < SCANFREE_MAX_BLOCKS ? nblk : SCANFREE_MAX_BLOCKS) / 16u + 4u; }
// dwords of ONE table for a pass over nblk workgroups with rows of rdx digits: the tables of a sort lie back to back at
// this stride, and that much (x the number of passes) is what the zeroing kernel clears
inline uint32_t sup_used(uint32_t nblk, int rdx, uint32_t grp) { return (uint32_t)rdx * sup_rows(nblk, grp); }

// Direct binning (k_bin_count / k_bin_scan / k_bin_scatter, sort_bin.h): table geometry, needed by the workspace carving
// and by the route plan.
constexpr int BIN_TILES_CAP = 10240;              // tiles of the image (k_bin_count's LDS row)
constexpr uint32_t BIN_GROUP = 4096u, BIN_ROWS_MAX = 512u;
constexpr uint32_t BIN_WINDOWS_MAX = 64u;         // windows (8 tile rows x <= 64 tile columns) whose weights order the scatter's workgroups
// Gaussians per table row (and per workgroup of k_bin_count): measured best of 2048 ... 16384 at 1 M Gaussians.  The route is
// taken for up to BIN_ROWS_MAX rows = 2 M Gaussians: at 6 M (40 M pairs) it ties with the radix passes (0.83 ms both,
// profiles/r03_s_direct_binning.log), which stay in charge there.
inline bool bin_route_n(int64_t n) { return n <= (int64_t)BIN_GROUP * BIN_ROWS_MAX; }
inline uint32_t bin_rows(uint32_t n) { return (n + BIN_GROUP - 1u) / BIN_GROUP; }
inline uint32_t bin_table_rows(int64_t n) { return n > 0 && bin_route_n(n) ? bin_rows((uint32_t)n) : 1u; }
inline bool bin_route(int ntx, int nty) { return cugs_prect_packable(ntx, nty) && ntx * nty <= BIN_TILES_CAP; }

// Two caller-owned scratch buffers.  The N-level one is filled by cugs_sort_count_pairs (depth order,
// scanned block sums, pair total) and read by cugs_sort_pairs; the pair-level one can only be sized
// once the pair count is known.
// The control words at the head of the N-level workspace.  The kernels take pointers to members (and index the
// neighbour: total[1], ctl[1], snap[1]), so the byte offsets are part of their contract.
struct SortCtl {
    unsigned long long live_total;   // what the pair-level kernels read as the live pair count (0: the depth order is invalid)
    unsigned long long host_total;   // what the host is told (-1: a depth key outside the three-pass range, sort again wide)
    uint32_t q12_count, q12_snap;    // quirk Q12's zero pairs: the counter the emission adds to, and the value handed to
                                     // k_tile_ranges when the counter is re-armed (k_radix_hist, k_bin_scan)
    uint32_t range_flag, pad0;       // non-zero: some depth key lay outside the three-pass range (key kernel / projection)
    uint32_t probe_word, pad1;       // development build: violations counted by k_probe_lds_order
    uint32_t snap_q12, snap_range;   // direct route: what k_bin_scan saw in q12_count and range_flag, for k_bin_scatter
};
static_assert(offsetof(SortCtl, live_total) == 0 && offsetof(SortCtl, host_total) == 8, "k_scan_blocksums / k_bin_scatter: total[0], total[1]");
static_assert(offsetof(SortCtl, q12_count) == 16 && offsetof(SortCtl, q12_snap) == 20, "k_radix_hist / k_bin_scan: ctl[0], ctl[1]");
static_assert(offsetof(SortCtl, range_flag) == 24, "range flag");
static_assert(offsetof(SortCtl, probe_word) == 32, "probe word");
static_assert(offsetof(SortCtl, snap_q12) == 40 && offsetof(SortCtl, snap_range) == 44, "k_bin_scatter / k_bin_keys: snap[0], snap[1]");
constexpr size_t SORT_CTL_WORDS = 32;             // 256 bytes carved for the block
static_assert(sizeof(SortCtl) <= SORT_CTL_WORDS * sizeof(unsigned long long), "the control block fits its carve");

struct SortWsN {
    SortCtl* ctl;                // control words
    uint32_t* dkey[2];           // depth bits, ping-pong              [n]
    uint32_t* dval[2];           // Gaussian index, ping-pong          [n]
    int4* rect[2];               // {x0, y0, w | h << 16, tiles_touched} per Gaussian: [0] input order, [1] depth order
    uint32_t* prect[2];          // the same record packed into a dword (pack_rect), riding through the depth passes  [n]
    uint32_t* tot;               // [RADIX_DEPTH]
    uint32_t* blocksum;          // per FILL_CHUNK block pair counts   [nfill + 2]
    uint32_t* hist;              // [nblk_n][RADIX_DEPTH] block-major digit counts of the current depth pass
    uint32_t* sup;               // SUP_TABLES tables [nsb][RADIX_DEPTH]: the same counts summed per super-block, one table per pass
    uint32_t sup_entries;        // dwords in one table
    uint32_t* colhist;           // [RADIX][ncol] pairs per (tile column, COL_CHUNK block), as counted
    uint32_t* colscan;           // ... and scanned along each column's row
    uint32_t* bin_table;         // direct binning: [rows][tiles] pairs per (workgroup of the depth order, tile), then their prefix
    uint32_t* bin_ttot;          // [tiles] pairs per tile
    uint32_t* bin_tpre;          // [tiles] pairs of the earlier tiles of the tile's 64-tile chunk
    uint32_t* bin_csum;          // [chunks] pairs per 64-tile chunk
    uint32_t* bin_win;           // [BIN_WINDOWS_MAX] pairs per window of the scatter's workgroups (k_bin_scan; cleared by k_bin_count)
    uint32_t* bin_tbase;         // [tiles + 1] first real pair of each tile; [tiles] = pair total
    size_t bytes;
};
struct SortWsP {
    void* ptile[2];              // tile id per pair (u16 when the tile count allows, else u32), ping-pong [P]
    uint32_t* pidx[2];           // Gaussian index per pair            [P]
    uint32_t* hist;              // [nblk_p][RADIX] block-major
    uint32_t* sup;               // SUP_TABLES tables [nsb][RADIX], one per pair-level pass
    uint32_t sup_entries;
    size_t bytes;
};

struct Carver {
    char* base; size_t off = 0;
    template <typename T> T* take(size_t count) {
        size_t o = off;
        off = align_up(off + sizeof(T) * count, 256);
        return reinterpret_cast<T*>(base + o);
    }
};

SortWsN carve_n(void* base, int64_t n) {
    Carver c{static_cast<char*>(base)};
    SortWsN w;
    w.ctl = reinterpret_cast<SortCtl*>(c.take<unsigned long long>(SORT_CTL_WORDS));
    for (int i = 0; i < 2; ++i) w.dkey[i] = c.take<uint32_t>((size_t)n);
    for (int i = 0; i < 2; ++i) w.dval[i] = c.take<uint32_t>((size_t)n);
    for (int i = 0; i < 2; ++i) w.rect[i] = c.take<int4>((size_t)n);
    for (int i = 0; i < 2; ++i) w.prect[i] = c.take<uint32_t>((size_t)n);
    w.tot = c.take<uint32_t>(RADIX_DEPTH);
    w.blocksum = c.take<uint32_t>((size_t)nblocks_for(n, FILL_CHUNK) + 2);
    w.hist = c.take<uint32_t>((size_t)RADIX_DEPTH * (nblocks_for(n, CHUNK_DEPTH) + 1));
    w.sup_entries = (uint32_t)RADIX_DEPTH * sup_rows_bound(nblocks_for(n, CHUNK_DEPTH));
    w.sup = c.take<uint32_t>((size_t)SUP_TABLES * w.sup_entries);
    w.colhist = c.take<uint32_t>((size_t)RADIX * (nblocks_for(n, COL_CHUNK) + 1));
    w.colscan = c.take<uint32_t>((size_t)RADIX * (nblocks_for(n, COL_CHUNK) + 1));
    w.bin_table = c.take<uint32_t>((size_t)bin_table_rows(n) * BIN_TILES_CAP);
    w.bin_ttot = c.take<uint32_t>(BIN_TILES_CAP);
    w.bin_tpre = c.take<uint32_t>(BIN_TILES_CAP);
    w.bin_csum = c.take<uint32_t>(BIN_TILES_CAP / 64 + 4);
    w.bin_win = c.take<uint32_t>(BIN_WINDOWS_MAX);
    w.bin_tbase = c.take<uint32_t>(BIN_TILES_CAP + 1);
    w.bytes = c.off;
    return w;
}
SortWsP carve_p(void* base, int64_t pairs) {
    Carver c{static_cast<char*>(base)};
    SortWsP w;
    for (int i = 0; i < 2; ++i) w.ptile[i] = c.take<uint32_t>((size_t)pairs);     // sized for the u32 case
    for (int i = 0; i < 2; ++i) w.pidx[i] = c.take<uint32_t>((size_t)pairs);
    w.hist = c.take<uint32_t>((size_t)RADIX * (nblocks_for(pairs, CHUNK_MIN) + 1));
    w.sup_entries = (uint32_t)RADIX * sup_rows_bound(nblocks_for(pairs, CHUNK_MIN));
    w.sup = c.take<uint32_t>((size_t)SUP_TABLES * w.sup_entries);
    w.bytes = c.off;
    return w;
}

// ------------------------------------------------------------------------------------
// The route plan: every decision about HOW a view is sorted, made once from the call's sizes and handed to each stage.
// The projection (cugs_sort_key_slots) and the sort read the workspace by the same plan.
// ------------------------------------------------------------------------------------
#ifdef CUGS_DEV
// Development build only (libcugs_hip_dev.so): switches for measuring one route against another on one view; set through
// the cugsdbg_* hooks at the end of sort.hip.  The shipped library keeps no such state and reads no environment.
std::atomic<int> g_rank_mode{-1};                 // -1: not probed yet (ballot ranking is used), 0: ballot ranking, 1: atomic ranking
std::atomic<int> g_direct_route{1};               // 0 = the radix route on every view
std::atomic<int> g_col_min_ratio{13};             // pairs per Gaussian from which the column-ordered emission is used
inline int rank_mode() { return g_rank_mode.load(std::memory_order_relaxed); }
inline bool direct_route_enabled() { return g_direct_route.load(std::memory_order_relaxed) != 0; }
inline uint32_t column_min_ratio() { return (uint32_t)g_col_min_ratio.load(std::memory_order_relaxed); }
#else
constexpr int rank_mode() { return 0; }            // ballot ranking: defined by the ISA, no state
constexpr bool direct_route_enabled() { return true; }
constexpr uint32_t column_min_ratio() { return 13u; }
#endif

// Column-ordered pair emission: (row << 8 | column) must fit the 16-bit key.  Measured on MI355X, 1 M Gaussians at
// 1080p, whole sort (tools/sort_routes.py): 8.4 pairs per Gaussian 0.249 ms against 0.218 ms for emission in depth
// order + two radix passes; 14.8: 0.273 / 0.294; 23.5: 0.331 / 0.423; 45.2: 0.513 / 0.706 - it costs more per
// Gaussian and 7 instead of 13 us per million pairs, and pays from ~13 pairs per Gaussian (dense views, close-ups).
inline bool column_path(int ntx, int nty) { return ntx <= 256 && nty <= 256; }
inline bool column_path_pays(uint32_t n, uint32_t pairs) { return (unsigned long long)pairs >= (unsigned long long)column_min_ratio() * n; }
// The direct scatter STAGES a lane's indices in LDS (k_bin_scatter<true>) on dense views, from this many pairs per Gaussian on
constexpr uint32_t BIN_STAGE_RATIO = 13u;

inline int tile_bits(int tiles) {
    int b = 1;
    while (b < 31 && (1 << b) < tiles) ++b;
    return b;
}

enum class DepthRoute { Narrow, Wide };           // three 9-bit passes on the offset from the near plane / four 8-bit passes on the raw bits
enum class KeySource { Built, Prekeyed };         // depth keys and records: k_depth_keys_rect / left by cugs_project_forward_keyed
enum class PairCount { Exact, Predicted };        // `pairs` is the count the host has read / a capacity, the live count is on the device
enum class PairRoute { Direct, Column, Radix };   // k_bin_* / k_col_emit + one pass by tile row / k_fill_pairs + passes over the tile id

struct SortPlan {
    uint32_t n, pairs;           // Gaussians; pairs or, when predicted, the capacity of the pair buffers
    int width, height, ntx, nty, tiles;
    // depth order
    DepthRoute depth;
    KeySource keys;              // Prekeyed only on the narrow route
    int depth_passes;            // 3 / 4
    uint32_t depth_nblk;         // workgroups of a depth pass (CHUNK_DEPTH / CHUNK_MIN items each)
    uint32_t depth_grp;          // threads per digit of its scatter
    uint32_t depth_table;        // dwords of one pass's super table (0: the pass is not scan-free)
    uint32_t depth_clear;        // dwords at SortWsN::sup the key kernel / the projection clears: one table per pass
    bool riding;                 // the packed rectangles ride through the depth passes: the producer fills prect[0], not rect[0]
    // pair level
    PairCount count;
    PairRoute route;
    bool wide_ids;               // tile ids as u32 (more than 2^16 tiles), else u16
    int pair_passes, pair_bits;  // Radix: passes over the tile id and bits of each; Column: the one pass over the tile row
    bool staged;                 // Direct: k_bin_scatter<true>
};

// pairs: 0 where the pair count is not known yet (cugs_sort_count_pairs, cugs_sort_key_slots: the count stage and the
// producer's slots do not depend on it).  The caller has checked n <= INT_MAX and 0 <= pairs <= INT_MAX.
inline SortPlan make_sort_plan(int64_t n, int width, int height, int64_t pairs, KeySource keys, DepthRoute depth, PairCount count) {
    SortPlan p{};
    p.n = (uint32_t)n; p.pairs = (uint32_t)pairs;
    p.width = width; p.height = height;
    p.ntx = (width + CUGS_TILE - 1) / CUGS_TILE; p.nty = (height + CUGS_TILE - 1) / CUGS_TILE;
    p.tiles = p.ntx * p.nty;
    p.depth = depth;
    // a wide sort rebuilds the keys from the arrays: what the projection left is keyed for the narrow route
    p.keys = depth == DepthRoute::Narrow ? keys : KeySource::Built;
    const bool narrow = depth == DepthRoute::Narrow;
    p.depth_passes = narrow ? 3 : 4;
    p.depth_nblk = nblocks_for(n, narrow ? CHUNK_DEPTH : CHUNK_MIN);
    p.depth_grp = 1024u >> (narrow ? DEPTH_BITS : 8);
    p.depth_table = sup_used(p.depth_nblk, narrow ? RADIX_DEPTH : RADIX, p.depth_grp);
    p.depth_clear = (uint32_t)p.depth_passes * p.depth_table;
    // prekeyed on an image of up to 127 x 127 tiles: the projection left PACKED rectangles (prect[0]) and they ride
    // through the passes beside the index, [0] -> [1] -> [0] -> [1]
    // ... when the passes' workgroups are at most one per CU anyway: the second value stream takes the scatter's LDS
    // from 68 to 84 KB, i.e. from two resident workgroups per CU to one - free at 1 M Gaussians (245 workgroups on
    // 256 CUs: sort 0.2285 -> 0.2239 ms, projection -1.5 us, same box), a loss at 6 M (1465 workgroups), where the
    // gather stays (profiles/r03_j_packed_rect_ride_ab.log)
    p.riding = p.keys == KeySource::Prekeyed && cugs_prect_packable(p.ntx, p.nty) && nblocks_for(n, CHUNK_MIN) <= 256u;
    p.count = count;
    p.wide_ids = tile_bits(p.tiles) > 16;         // never when column_path() holds
    // Direct: the projection's own records on an image of up to ~10 000 tiles: every pair is written once, by a counting
    // sort over the tiles (k_bin_*), instead of emitted and carried through two radix passes
    // (capacity below 2^30: the scatter keeps 32-bit byte offsets into the index buffer)
    if (count == PairCount::Predicted && p.keys == KeySource::Prekeyed && bin_route(p.ntx, p.nty) && bin_route_n(n) &&
        pairs < (int64_t(1) << 30) && direct_route_enabled()) {
        p.route = PairRoute::Direct;
        // (the capacity stands for the pair count in the choice of the variant: it follows the previous frames' counts)
        p.staged = (unsigned long long)p.pairs >= (unsigned long long)BIN_STAGE_RATIO * p.n;
    } else if (column_path(p.ntx, p.nty) && column_path_pays(p.n, p.pairs)) {
        p.route = PairRoute::Column;              // pairs emitted in tile-column order, then ONE stable pass by row
        p.pair_passes = 1;
        p.pair_bits = tile_bits(p.nty);
    } else {
        p.route = PairRoute::Radix;
        const int bits = tile_bits(p.tiles);
        p.pair_passes = (bits + 7) / 8;
        p.pair_bits = (bits + p.pair_passes - 1) / p.pair_passes;
    }
    return p;
}

}  // namespace
