// sort.hip — (tile | depth) ordering of (tile, Gaussian) pairs.
//
// Replaces sort_gaussians (rasterizer/sorting.cu:115-227): the int32 cumsum + blocking .item()
// (:145-146), k_fill_sort_pairs (:30-72), cub::DeviceRadixSort::SortPairs over all 64 key bits
// (:191-210) and k_compute_tile_ranges (:82-109).
//
// Required result (bit-exact): pairs ordered by the 64-bit key (tile_id << 32 | float_bits(depth)),
// ties in ascending Gaussian index (CUB's sort is stable and the reference fills in index order).
//
// How it is produced here (not the reference's schedule): a stable LSD sort by the full key is the
// same permutation as (1) a stable sort of the N Gaussians by depth bits, (2) emitting each
// Gaussian's pairs in that order, (3) a stable sort of the P pairs by tile id alone.  (1) moves
// 8 B x N x 3 passes (9-bit digits on the 27-bit offset of the depth bits from the near plane; 4 passes of 8 bits on
// the raw bits for views outside that range), (3) moves 8 B x P x ceil(log2(tiles)/8) passes (2 at 1080p) instead of
// 12 B x P x 8 passes.  Every pass is the same three kernels: per-workgroup digit histogram,
// per-digit row scan, stable scatter with wave64 ballot ranking.  All HBM-bound integer work.
//
// Views with many pairs per Gaussian (>= 13: dense scenes, close-ups), on images of up to 256 x 256 tiles, save
// the first of the pair-level passes: the pairs are EMITTED already ordered by tile column (k_col_emit) - which
// needs a histogram and a ranking per (Gaussian, column) instead of per pair - and one stable pass by tile row
// finishes (3).  Both routes give the same permutation (tests/test_gpu_parity.py runs each against the oracle).
//
// Where things are: sort_workspace.h (the two workspaces, their control block, the route plan: every decision about how a
// view is sorted is made ONCE, by make_sort_plan), sort_radix.h (one radix pass), sort_emit.h (keys, pair counts, pair
// emission, tile ranges), sort_bin.h (direct binning), sort_tile_order.h (the blend kernels' tile order).  This file is
// the host side: the count stage, the pair stage, the entry points.
#include "sort_workspace.h"
#include "sort_radix.h"
#include "sort_emit.h"
#include "sort_tile_order.h"
#include "sort_bin.h"

namespace {

// The count stage, steps (1)-(2a): everything that does not depend on the pair count.  Queued, never blocks.
// Narrow depth route: the depth sort on 27-bit offsets from the near plane (see RADIX_DEPTH); if a depth key turns out to
// lie outside that range the totals say so (k_scan_blocksums / k_bin_scatter) and the caller plans the view again, wide.
int queue_count(const SortPlan& plan, const SortWsN& ws, const float* means_2d, const float* depths, const int32_t* radii,
                const int32_t* tiles_touched, hipStream_t st, unsigned long long* total_mapped) {
    const uint32_t un = plan.n;
    const int ntx = plan.ntx, nty = plan.nty;
    const bool narrow = plan.depth == DepthRoute::Narrow, direct = plan.route == PairRoute::Direct;
    uint32_t* const range_flag = &ws.ctl->range_flag;
    uint32_t* const q12 = &ws.ctl->q12_count;           // [0] Q12 counter, [1] its snapshot
    const uint32_t* const ridden = plan.riding ? ws.prect[1] : nullptr;   // the packed rectangles in depth order, if they rode
    int rc;
    // (1) stable sort of the Gaussians by depth
    // Prekeyed: cugs_project_forward_keyed has left dkey[0], rect[0] / prect[0] and the range flag in this workspace already
    if (plan.keys == KeySource::Built) {
        hipLaunchKernelGGL(k_depth_keys_rect, dim3(nblocks_for(un, CUGS_BLOCK)), dim3(CUGS_BLOCK), 0, st, un, depths,
                           means_2d, radii, tiles_touched, plan.width, plan.height, ntx, nty, ws.dkey[narrow ? 0 : 1], ws.rect[0],
                           narrow ? range_flag : static_cast<uint32_t*>(nullptr), ws.sup, plan.depth_clear);
        CUGS_LAUNCH_CHECK();
    }
    uint32_t* sp[SUP_TABLES];
    for (int t = 0; t < SUP_TABLES; ++t) sp[t] = ws.sup + (size_t)t * plan.depth_table;
    if (narrow) {
        // keys in dkey[0], three passes of 9 bits [0] -> [1] -> [0] -> [1]; the riding rectangles go the same way
        uint32_t* const* pr = ws.prect;
        const bool riding = plan.riding;
        if ((rc = radix_pass<uint32_t, true, 1024, CHUNK_DEPTH, RADIX_DEPTH>(ws.dkey[0], nullptr, un, nullptr, 0, DEPTH_BITS, ws.hist, sp[0], ws.tot, ws.dkey[1], ws.dval[1], nullptr, st, riding ? pr[0] : nullptr, pr[1]))) return rc;
        if ((rc = radix_pass<uint32_t, false, 1024, CHUNK_DEPTH, RADIX_DEPTH>(ws.dkey[1], ws.dval[1], un, nullptr, DEPTH_BITS, DEPTH_BITS, ws.hist, sp[1], ws.tot, ws.dkey[0], ws.dval[0], nullptr, st, riding ? pr[1] : nullptr, pr[0]))) return rc;
        // direct: the last pass's histogram kernel also arms the Q12 counter k_bin_count adds to
        if ((rc = radix_pass<uint32_t, false, 1024, CHUNK_DEPTH, RADIX_DEPTH>(ws.dkey[0], ws.dval[0], un, nullptr, 2 * DEPTH_BITS, DEPTH_BITS, ws.hist, sp[2], ws.tot, ws.dkey[1], ws.dval[1], direct ? q12 : nullptr, st, riding ? pr[0] : nullptr, pr[1]))) return rc;
    } else {
        // the general route: keys in dkey[1], four passes of 8 bits on the raw depth bits (positive floats order as unsigned ints)
        if ((rc = radix_pass<uint32_t, true, 1024, CHUNK_MIN>(ws.dkey[1], nullptr, un, nullptr, 0, 8, ws.hist, sp[0], ws.tot, ws.dkey[0], ws.dval[0], nullptr, st))) return rc;
        if ((rc = radix_pass<uint32_t, false, 1024, CHUNK_MIN>(ws.dkey[0], ws.dval[0], un, nullptr, 8, 8, ws.hist, sp[1], ws.tot, ws.dkey[1], ws.dval[1], nullptr, st))) return rc;
        if ((rc = radix_pass<uint32_t, false, 1024, CHUNK_MIN>(ws.dkey[1], ws.dval[1], un, nullptr, 16, 8, ws.hist, sp[2], ws.tot, ws.dkey[0], ws.dval[0], nullptr, st))) return rc;
        if ((rc = radix_pass<uint32_t, false, 1024, CHUNK_MIN>(ws.dkey[0], ws.dval[0], un, nullptr, 24, 8, ws.hist, sp[3], ws.tot, ws.dkey[1], ws.dval[1], nullptr, st))) return rc;
    }
    if (direct) {
        // (2)-(3a) direct binning: pairs per (workgroup of the depth order, tile), their prefixes, tile starts, the total
        // (the totals are published by the scatter: the pair stage, which the caller launches in any case)
        const uint32_t tiles = (uint32_t)plan.tiles, rows = bin_rows(un);
        hipLaunchKernelGGL(k_bin_count, dim3(rows), dim3(BIN_NT), 0, st, un, BIN_GROUP, ws.dval[1], ws.rect[0], ridden,
                           plan.riding ? static_cast<uint32_t*>(nullptr) : ws.prect[1], (uint32_t)ntx, (uint32_t)nty, ws.bin_table, q12,
                           ws.bin_win);
        CUGS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_bin_scan, dim3((tiles + CUGS_WAVE - 1) / CUGS_WAVE), dim3(BIN_NT), 0, st, rows, tiles, ws.bin_table,
                           ws.bin_ttot, ws.bin_tpre, ws.bin_csum, q12, range_flag, &ws.ctl->snap_q12,
                           bin_windows(ntx, nty) <= BIN_WINDOWS_MAX ? ws.bin_win : nullptr,
                           (uint32_t)ntx, bin_window_cols(ntx), bin_window_groups(ntx));
        CUGS_LAUNCH_CHECK();
        return 0;
    }
    // (2a) pair counts per 256-Gaussian block in depth order, their scan, and the grand total
    const uint32_t nfill = nblocks_for(un, FILL_CHUNK);
    hipLaunchKernelGGL(k_fill_blocksums, dim3(nfill), dim3(CUGS_BLOCK), 0, st, un, ws.dval[1], ws.rect[0], ws.rect[1],
                       ws.blocksum, ridden);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scan_blocksums, dim3(1), dim3(SCAN_NT), 0, st, ws.blocksum, nfill, &ws.ctl->live_total, q12,
                       total_mapped, narrow ? range_flag : static_cast<uint32_t*>(nullptr));
    CUGS_LAUNCH_CHECK();
    return 0;
}

// The pair stage, steps (2b)-(4), for one tile-id width.  dev_count (predicted): the live pair count in the workspace.
template <typename K>
int sort_pairs_typed(const SortPlan& plan, const SortWsN& ws, const SortWsP& wp, const float* depths, uint64_t* keys_sorted,
                     int32_t* values_sorted, int32_t* tile_ranges, hipStream_t st, unsigned long long* total_mapped,
                     uint32_t* tile_order) {
    const uint32_t un = plan.n, up = plan.pairs;
    const int ntx = plan.ntx, nty = plan.nty, tiles = plan.tiles;
    const unsigned long long* dev_count = plan.count == PairCount::Predicted ? &ws.ctl->live_total : nullptr;
    const uint32_t* order = ws.dval[1];                 // left there by the count stage
    if (plan.route == PairRoute::Direct) {
        // (3b) every pair straight to its place (the count stage left the prefixes, the tile starts and the depth-ordered
        // packed rectangles in the N-level workspace); the pair-level workspace is not used
        const uint32_t* zsnap = &ws.ctl->snap_q12;      // [0] Q12 pairs, [1] depth range flag
        // blocks of 8 x 8 tiles, one per wave; workgroups of up to 8 horizontally adjacent blocks, evenly filled
        // (15 block columns: 8 + 7).  Launched for capacity 0 too: the kernel publishes the totals and the ranges.
        const uint32_t nbx = ((uint32_t)ntx + BIN_BLK - 1u) / BIN_BLK, nby = ((uint32_t)nty + BIN_BLK - 1u) / BIN_BLK;
        const uint32_t gxs = bin_window_groups(ntx);
        const uint32_t waves = bin_window_cols(ntx) / BIN_BLK;
        const uint32_t* const win = bin_windows(ntx, nty) <= BIN_WINDOWS_MAX ? ws.bin_win : nullptr;
#define CUGS_LAUNCH_SCATTER(S)                                                                                                        \
        hipLaunchKernelGGL(k_bin_scatter<S>, dim3(bin_rows(un) * nby * gxs), dim3(waves * CUGS_WAVE), 0, st, un, BIN_GROUP, nbx, nby, gxs,   \
                           up, dev_count != nullptr, order, static_cast<const uint32_t*>(ws.prect[1]), (uint32_t)ntx, (uint32_t)nty,      \
                           ws.bin_table, ws.bin_ttot, ws.bin_tpre, ws.bin_csum, zsnap, ws.bin_tbase, &ws.ctl->live_total, total_mapped,  \
                           reinterpret_cast<uint32_t*>(values_sorted), tile_ranges, tile_order, win)
        if (plan.staged) CUGS_LAUNCH_SCATTER(true); else CUGS_LAUNCH_SCATTER(false);
#undef CUGS_LAUNCH_SCATTER
        CUGS_LAUNCH_CHECK();
        if (keys_sorted) {
            hipLaunchKernelGGL(k_bin_keys, dim3(nblocks_for(up, CUGS_BLOCK)), dim3(CUGS_BLOCK), 0, st, up, dev_count, (uint32_t)tiles,
                               ws.bin_tbase, zsnap, values_sorted, depths, keys_sorted);
            CUGS_LAUNCH_CHECK();
        }
        return 0;
    }
    const uint32_t nfill = nblocks_for(un, FILL_CHUNK);
    uint32_t* ctl = &ws.ctl->q12_count;                 // [0] Q12 counter, [1] its snapshot
    K* tk[2] = {static_cast<K*>(wp.ptile[0]), static_cast<K*>(wp.ptile[1])};
    uint32_t* tv[2] = {wp.pidx[0], wp.pidx[1]};
    uint32_t* vals_final = reinterpret_cast<uint32_t*>(values_sorted);
    const uint32_t nblk_p = nblocks_for(up, CHUNK_PAIR);
    if constexpr (sizeof(K) == 2) {
        if (plan.route == PairRoute::Column) {
            // pairs emitted in tile-column order (row << 8 | column keys), then ONE stable pass by row
            const uint32_t ncol = nblocks_for(un, COL_CHUNK);
            hipLaunchKernelGGL(k_col_hist, dim3(ncol), dim3(COL_CHUNK), 0, st, un, ws.rect[1], ws.colhist, ncol);
            CUGS_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_radix_scan_rows, dim3(RADIX), dim3(CUGS_BLOCK), 0, st, ws.colhist, ws.colscan, ncol, ws.tot);
            CUGS_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_col_emit, dim3(ncol), dim3(COL_CHUNK), 0, st, un, up, dev_count, order, ws.rect[1],
                               ws.colscan, ws.tot, ncol, tk[0], tv[0], ctl, tile_ranges, (uint32_t)(2 * tiles), wp.sup,
                               sup_used(nblk_p, RADIX, 512u >> plan.pair_bits));
            CUGS_LAUNCH_CHECK();
            int rc = radix_pass<K, false, 512, CHUNK_PAIR>(tk[0], tv[0], up, dev_count, 8, plan.pair_bits, wp.hist, wp.sup,
                                                           ws.tot, tk[1], vals_final, ctl, st);
            if (rc) return rc;
            hipLaunchKernelGGL((k_tile_ranges<K, true>), dim3(nblocks_for(up, CUGS_BLOCK * 8)), dim3(CUGS_BLOCK), 0, st, up,
                               dev_count, tk[1], (uint32_t)ntx, values_sorted, depths, tile_ranges, keys_sorted, ctl + 1);
            CUGS_LAUNCH_CHECK();
            return 0;
        }
    }
    const int bits = tile_bits(tiles), npass = plan.pair_passes, per = plan.pair_bits;
    if (npass > SUP_TABLES) return CUGS_EINVAL;
    // each pass's super table (if that pass runs scan-free: radix_pass applies the same rule), back to back
    uint32_t sup_off[SUP_TABLES + 1] = {0u};
    for (int p = 0; p < npass; ++p) {
        const int shift = p * per;
        const int b = (bits - shift) < per ? (bits - shift) : per;
        sup_off[p + 1] = sup_off[p] + sup_used(nblk_p, RADIX, 512u >> b);
    }
    hipLaunchKernelGGL((k_fill_pairs<K>), dim3(nfill), dim3(CUGS_BLOCK), 0, st, un, up, dev_count, order, ws.rect[1], ntx,
                       ws.blocksum, tk[0], tv[0], ctl, tile_ranges, (uint32_t)(2 * tiles), wp.sup, sup_off[npass]);
    CUGS_LAUNCH_CHECK();
    int cur = 0, rc;
    for (int p = 0; p < npass; ++p) {
        const int shift = p * per;
        const int b = (bits - shift) < per ? (bits - shift) : per;
        uint32_t* vout = (p == npass - 1) ? vals_final : tv[cur ^ 1];
        rc = radix_pass<K, false, 512, CHUNK_PAIR>(tk[cur], tv[cur], up, dev_count, shift, b, wp.hist, wp.sup + sup_off[p], ws.tot,
                                                   tk[cur ^ 1], vout, p == 0 ? ctl : nullptr, st);   // 512 threads: measured best of 256/512/1024
        if (rc) return rc;
        cur ^= 1;
    }
    hipLaunchKernelGGL((k_tile_ranges<K, false>), dim3(nblocks_for(up, CUGS_BLOCK * 8)), dim3(CUGS_BLOCK), 0, st, up, dev_count, tk[cur],
                       (uint32_t)ntx, values_sorted, depths, tile_ranges, keys_sorted, ctl + 1);
    CUGS_LAUNCH_CHECK();
    return 0;
}

template <typename... A>
int sort_pairs_dispatch(const SortPlan& plan, A... args) {
    if (plan.wide_ids) return sort_pairs_typed<uint32_t>(plan, args...);
    return sort_pairs_typed<uint16_t>(plan, args...);
}

}  // namespace

// Internal (cugs_common.h): where the projection leaves what the count stage of a Prekeyed, Narrow plan picks up.
int cugs_sort_key_slots(void* workspace, size_t bytes, int64_t n, int width, int height, uint32_t** keys, int4** rect,
                        uint32_t** prect, uint32_t** range_flag, uint32_t** zero, uint32_t* nzero) {
    if (!workspace || n < 0 || n > 2147483647ll || width < 0 || height < 0) return CUGS_EINVAL;
    if ((width + CUGS_TILE - 1) / CUGS_TILE > 32767 || (height + CUGS_TILE - 1) / CUGS_TILE > 32767) return CUGS_EOVERFLOW;
    SortWsN ws = carve_n(workspace, n);
    if (bytes < ws.bytes) return CUGS_EWORKSPACE;
    const SortPlan plan = make_sort_plan(n, width, height, 0, KeySource::Prekeyed, DepthRoute::Narrow, PairCount::Predicted);
    *keys = ws.dkey[0];
    *rect = plan.riding ? nullptr : ws.rect[0];
    *prect = plan.riding ? ws.prect[0] : nullptr;
    *range_flag = &ws.ctl->range_flag;
    *zero = ws.sup;                                // the key kernel also clears the depth passes' super tables
    *nzero = plan.depth_clear;
    return 0;
}

extern "C" size_t cugs_sort_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    return carve_n(nullptr, n).bytes;
}

extern "C" size_t cugs_sort_pair_workspace_bytes(int64_t total_pairs) {
    if (total_pairs < 0) return 0;
    return carve_p(nullptr, total_pairs).bytes;
}

// Everything that does not depend on the pair count runs BEFORE the blocking read-back, so the
// device is busy (depth keys, the depth sort, per-block pair sums and their scan) while the
// host waits for the 8-byte total - the reference idles on cumsum[-1].item() instead (sorting.cu:146).
namespace {
int sort_count_pairs_impl(int64_t n, const float* means_2d, const float* depths,
                                     const int32_t* radii, const int32_t* tiles_touched, int width,
                                     int height, void* workspace, size_t workspace_bytes,
                                     int64_t* total_pairs_host, void* stream, DepthRoute depth) {
    if (n < 0 || width < 0 || height < 0 || !total_pairs_host) return CUGS_EINVAL;
    *total_pairs_host = 0;
    if (n == 0) return 0;
    if (n > 2147483647ll) return CUGS_EOVERFLOW;
    if (!means_2d || !depths || !radii || !tiles_touched || !workspace) return CUGS_EINVAL;
    SortWsN ws = carve_n(workspace, n);
    if (workspace_bytes < ws.bytes) return CUGS_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // depth == Wide: the caller knows this view's depths leave the range of the three-pass depth sort (an earlier sort of
    // it said so): the general four-pass route at once instead of a wasted three-pass attempt
    SortPlan plan = make_sort_plan(n, width, height, 0, KeySource::Built, depth, PairCount::Exact);
    if (plan.ntx > 32767 || plan.nty > 32767) return CUGS_EOVERFLOW;          // rectangle extents travel as 16-bit halves
    int rc = queue_count(plan, ws, means_2d, depths, radii, tiles_touched, st, nullptr);
    if (rc) return rc;
#ifdef CUGS_DEV
    // development build: first blocking sort of the process verifies the LDS ordering the atomic ranking relies on
    const bool probing = rank_mode() < 0;
    uint32_t* probe_word = &ws.ctl->probe_word;
    uint32_t violations = 1;
    if (probing) {
        CUGS_RETURN_IF_HIP(hipMemsetAsync(probe_word, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_probe_lds_order, dim3(96), dim3(CUGS_BLOCK), 0, st, probe_word);
        CUGS_LAUNCH_CHECK();
        CUGS_RETURN_IF_HIP(hipMemcpyAsync(&violations, probe_word, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
#endif
    // straight into the caller's variable: if that is pinned host memory the copy is one DMA, no staging
    CUGS_RETURN_IF_HIP(hipMemcpyAsync(total_pairs_host, &ws.ctl->host_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    CUGS_RETURN_IF_HIP(hipStreamSynchronize(st));
    if (*total_pairs_host == -1) {
        // a depth key outside the range of the three-pass depth sort (a view with splats nearer than the near plane
        // or farther than ~13 000 units): the general four-pass route, once more
        plan = make_sort_plan(n, width, height, 0, KeySource::Built, DepthRoute::Wide, PairCount::Exact);
        rc = queue_count(plan, ws, means_2d, depths, radii, tiles_touched, st, nullptr);
        if (rc) return rc;
        CUGS_RETURN_IF_HIP(hipMemcpyAsync(total_pairs_host, &ws.ctl->host_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        CUGS_RETURN_IF_HIP(hipStreamSynchronize(st));
    }
#ifdef CUGS_DEV
    if (probing) g_rank_mode.store(violations == 0 ? 1 : 0, std::memory_order_relaxed);
#endif
    if ((unsigned long long)*total_pairs_host > 2147483647ull) {   // the reference indexes pairs with int
        *total_pairs_host = 0;
        return CUGS_EOVERFLOW;
    }
    return 0;
}
}  // namespace

extern "C" int cugs_sort_count_pairs(int64_t n, const float* means_2d, const float* depths,
                                     const int32_t* radii, const int32_t* tiles_touched, int width,
                                     int height, void* workspace, size_t workspace_bytes,
                                     int64_t* total_pairs_host, void* stream) {
    return sort_count_pairs_impl(n, means_2d, depths, radii, tiles_touched, width, height, workspace, workspace_bytes,
                                 total_pairs_host, stream, DepthRoute::Narrow);
}

extern "C" int cugs_sort_count_pairs_wide(int64_t n, const float* means_2d, const float* depths,
                                          const int32_t* radii, const int32_t* tiles_touched, int width,
                                          int height, void* workspace, size_t workspace_bytes,
                                          int64_t* total_pairs_host, void* stream) {
    return sort_count_pairs_impl(n, means_2d, depths, radii, tiles_touched, width, height, workspace, workspace_bytes,
                                 total_pairs_host, stream, DepthRoute::Wide);
}

extern "C" int cugs_sort_pairs(int64_t n, int64_t total_pairs, const float* means_2d,
                               const float* depths, const int32_t* radii,
                               const int32_t* tiles_touched, int width, int height, void* workspace,
                               size_t workspace_bytes, void* pair_workspace, size_t pair_workspace_bytes,
                               uint64_t* keys_sorted, int32_t* values_sorted, int32_t* tile_ranges,
                               void* stream) {
    if (n < 0 || total_pairs < 0 || width < 0 || height < 0 || !tile_ranges) return CUGS_EINVAL;
    if (n > 2147483647ll || total_pairs > 2147483647ll) return CUGS_EOVERFLOW;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (the depth order is in the workspace already: only the pair level of the plan matters here)
    const SortPlan plan = make_sort_plan(n, width, height, total_pairs, KeySource::Built, DepthRoute::Narrow, PairCount::Exact);
    const int tiles = plan.tiles;
    if (n == 0 || total_pairs == 0 || tiles == 0) {              // sorting.cu:133-139,154-160
        if (tiles > 0)   // every tile stays {0,0} (sorting.cu:216)
            CUGS_RETURN_IF_HIP(hipMemsetAsync(tile_ranges, 0, sizeof(int32_t) * 2 * (size_t)tiles, st));
        return 0;
    }
    if (!means_2d || !depths || !radii || !tiles_touched || !values_sorted || !workspace || !pair_workspace)
        return CUGS_EINVAL;
    SortWsN ws = carve_n(workspace, n);
    SortWsP wp = carve_p(pair_workspace, total_pairs);
    if (workspace_bytes < ws.bytes || pair_workspace_bytes < wp.bytes) return CUGS_EWORKSPACE;

    // (2b) pairs in depth order; (3) stable sort by tile id, last pass landing in values_sorted; (4) ranges
    return sort_pairs_dispatch(plan, ws, wp, depths, keys_sorted, values_sorted, tile_ranges, st,
                               static_cast<unsigned long long*>(nullptr), static_cast<uint32_t*>(nullptr));
}

// The whole sort without a host round trip: the caller PREDICTS the pair count (`capacity`, e.g. the last
// frame's count plus a margin), sizes pair_workspace / keys_sorted / values_sorted for it, and every
// pair-level kernel takes the live count from device memory.  The 8-byte total is copied to
// *total_pairs_host asynchronously (use pinned memory); once the stream (or an event recorded after this
// call) has completed, the results are valid iff 0 <= *total_pairs_host <= capacity - otherwise call
// cugs_sort_pairs with the now known count (the N-level workspace still holds the depth order).  The
// ~45 us the device idles in cugs_sort_count_pairs + cugs_sort_pairs while the host reads the total
// and launches the rest (3 % of a 1 M-Gaussian 1080p frame) disappear.
namespace {
int sort_pairs_predicted_impl(int64_t n, int64_t capacity, const float* means_2d, const float* depths,
                              const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                              void* workspace, size_t workspace_bytes, void* pair_workspace,
                              size_t pair_workspace_bytes, uint64_t* keys_sorted, int32_t* values_sorted,
                              int32_t* tile_ranges, int64_t* total_pairs_host, void* stream, KeySource keys,
                              DepthRoute depth, uint32_t* tile_order) {
    if (n < 0 || capacity < 0 || width < 0 || height < 0 || !tile_ranges || !total_pairs_host) return CUGS_EINVAL;
    if (n > 2147483647ll || capacity > 2147483647ll) return CUGS_EOVERFLOW;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SortPlan plan = make_sort_plan(n, width, height, capacity, keys, depth, PairCount::Predicted);
    const int tiles = plan.tiles;
    if (plan.ntx > 32767 || plan.nty > 32767) return CUGS_EOVERFLOW;
    *total_pairs_host = 0;
    // tile_order (optional): every exit that leaves valid ranges also leaves a valid order of the tiles
    auto order_from_ranges = [&]() -> int {
        if (!tile_order) return 0;
        hipLaunchKernelGGL(k_tile_order, dim3(1), dim3(1024), 0, st, (uint32_t)tiles, tile_ranges, reinterpret_cast<uint4*>(tile_order));
        CUGS_LAUNCH_CHECK();
        return 0;
    };
    if (n == 0 || tiles == 0) {
        if (tiles > 0) {
            CUGS_RETURN_IF_HIP(hipMemsetAsync(tile_ranges, 0, sizeof(int32_t) * 2 * (size_t)tiles, st));
            return order_from_ranges();
        }
        return 0;
    }
    if (!means_2d || !depths || !radii || !tiles_touched || !workspace) return CUGS_EINVAL;
    SortWsN ws = carve_n(workspace, n);
    if (workspace_bytes < ws.bytes) return CUGS_EWORKSPACE;
    // pinned host memory is mapped into the device's address space: the scan kernel then stores the total there
    // itself; anything else (pageable memory) gets the asynchronous copy
    unsigned long long* mapped = nullptr;
    {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, total_pairs_host) == hipSuccess && attr.type == hipMemoryTypeHost &&
            attr.devicePointer)
            mapped = static_cast<unsigned long long*>(attr.devicePointer);
        else
            (void)hipGetLastError();                              // an unregistered pointer is not an error here
    }
    int rc = queue_count(plan, ws, means_2d, depths, radii, tiles_touched, st, mapped);
    if (rc) return rc;
    if (plan.route == PairRoute::Direct) {
        // the scatter publishes the totals (and, with capacity 0, only does that and clears the ranges)
        if (capacity > 0 && !values_sorted) return CUGS_EINVAL;
        SortWsP none{};
        rc = sort_pairs_dispatch(plan, ws, none, depths, capacity > 0 ? keys_sorted : static_cast<uint64_t*>(nullptr),
                                 values_sorted, tile_ranges, st, mapped, tile_order);
        if (rc) return rc;
        if (!mapped)
            CUGS_RETURN_IF_HIP(hipMemcpyAsync(total_pairs_host, &ws.ctl->host_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        return 0;
    }
    if (!mapped)
        CUGS_RETURN_IF_HIP(hipMemcpyAsync(total_pairs_host, &ws.ctl->host_total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (capacity == 0) {                                          // valid iff the total turns out to be 0
        CUGS_RETURN_IF_HIP(hipMemsetAsync(tile_ranges, 0, sizeof(int32_t) * 2 * (size_t)tiles, st));
        return order_from_ranges();
    }
    if (!values_sorted || !pair_workspace) return CUGS_EINVAL;
    SortWsP wp = carve_p(pair_workspace, capacity);
    if (pair_workspace_bytes < wp.bytes) return CUGS_EWORKSPACE;
    rc = sort_pairs_dispatch(plan, ws, wp, depths, keys_sorted, values_sorted, tile_ranges, st, mapped,
                             static_cast<uint32_t*>(nullptr));
    if (rc) return rc;
    return order_from_ranges();      // the radix route's ranges come from the (clamped) sorted pairs: always a valid partition
}
}  // namespace

extern "C" int cugs_sort_pairs_predicted(int64_t n, int64_t capacity, const float* means_2d, const float* depths,
                                         const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                                         void* workspace, size_t workspace_bytes, void* pair_workspace,
                                         size_t pair_workspace_bytes, uint64_t* keys_sorted, int32_t* values_sorted,
                                         int32_t* tile_ranges, int64_t* total_pairs_host, void* stream) {
    return sort_pairs_predicted_impl(n, capacity, means_2d, depths, radii, tiles_touched, width, height, workspace,
                                     workspace_bytes, pair_workspace, pair_workspace_bytes, keys_sorted, values_sorted,
                                     tile_ranges, total_pairs_host, stream, KeySource::Built, DepthRoute::Narrow, nullptr);
}

// cugs_sort_pairs_predicted for a `workspace` that cugs_project_forward_keyed has filled on this stream, for these very
// arrays, since the last sort that used it: the per-Gaussian key / rectangle kernel (one launch, 40 MB per million
// Gaussians) is skipped.  Everything else, the validity rule and the fallback (cugs_sort_count_pairs + cugs_sort_pairs,
// which rebuild the keys from the arrays) are those of cugs_sort_pairs_predicted.
extern "C" int cugs_sort_pairs_predicted_keyed(int64_t n, int64_t capacity, const float* means_2d, const float* depths,
                                               const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                                               void* workspace, size_t workspace_bytes, void* pair_workspace,
                                               size_t pair_workspace_bytes, uint64_t* keys_sorted, int32_t* values_sorted,
                                               int32_t* tile_ranges, int64_t* total_pairs_host, void* stream) {
    return sort_pairs_predicted_impl(n, capacity, means_2d, depths, radii, tiles_touched, width, height, workspace,
                                     workspace_bytes, pair_workspace, pair_workspace_bytes, keys_sorted, values_sorted,
                                     tile_ranges, total_pairs_host, stream, KeySource::Prekeyed, DepthRoute::Narrow, nullptr);
}

// cugs_sort_pairs_predicted_keyed that also leaves, in tile_order[tiles][4], the tiles ordered by the length of their lists,
// longest first ({tile, first pair, one past the last pair, 0} each): what the blends hand their workgroups out by (`tile_order` in their options).
extern "C" int cugs_sort_pairs_predicted_keyed_ordered(int64_t n, int64_t capacity, const float* means_2d, const float* depths,
                                                       const int32_t* radii, const int32_t* tiles_touched, int width,
                                                       int height, void* workspace, size_t workspace_bytes,
                                                       void* pair_workspace, size_t pair_workspace_bytes,
                                                       uint64_t* keys_sorted, int32_t* values_sorted, int32_t* tile_ranges,
                                                       int64_t* total_pairs_host, uint32_t* tile_order, void* stream) {
    if (!tile_order) return CUGS_EINVAL;
    if (reinterpret_cast<uintptr_t>(tile_order) & 15u) return CUGS_EALIGN;
    return sort_pairs_predicted_impl(n, capacity, means_2d, depths, radii, tiles_touched, width, height, workspace,
                                     workspace_bytes, pair_workspace, pair_workspace_bytes, keys_sorted, values_sorted,
                                     tile_ranges, total_pairs_host, stream, KeySource::Prekeyed, DepthRoute::Narrow, tile_order);
}

// The same order from any valid tile_ranges (e.g. after cugs_sort_pairs): one small launch.
extern "C" int cugs_tile_order(int width, int height, const int32_t* tile_ranges, uint32_t* tile_order, void* stream) {
    if (width < 0 || height < 0) return CUGS_EINVAL;
    const int64_t tiles = (int64_t)((width + CUGS_TILE - 1) / CUGS_TILE) * ((height + CUGS_TILE - 1) / CUGS_TILE);
    if (tiles == 0) return 0;
    if (!tile_ranges || !tile_order || tiles > 2147483647ll) return CUGS_EINVAL;
    if (reinterpret_cast<uintptr_t>(tile_order) & 15u) return CUGS_EALIGN;
    hipLaunchKernelGGL(k_tile_order, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), (uint32_t)tiles, tile_ranges,
                       reinterpret_cast<uint4*>(tile_order));
    CUGS_LAUNCH_CHECK();
    return 0;
}

// cugs_sort_pairs_predicted on the GENERAL depth route (four 8-bit passes over the raw depth bits): for views whose
// depths leave the range of the three-pass sort - an earlier sort of the view reported -1.  Never reports -1 itself.
extern "C" int cugs_sort_pairs_predicted_wide(int64_t n, int64_t capacity, const float* means_2d, const float* depths,
                                              const int32_t* radii, const int32_t* tiles_touched, int width, int height,
                                              void* workspace, size_t workspace_bytes, void* pair_workspace,
                                              size_t pair_workspace_bytes, uint64_t* keys_sorted, int32_t* values_sorted,
                                              int32_t* tile_ranges, int64_t* total_pairs_host, void* stream) {
    return sort_pairs_predicted_impl(n, capacity, means_2d, depths, radii, tiles_touched, width, height, workspace,
                                     workspace_bytes, pair_workspace, pair_workspace_bytes, keys_sorted, values_sorted,
                                     tile_ranges, total_pairs_host, stream, KeySource::Built, DepthRoute::Wide, nullptr);
}

#ifdef CUGS_DEV
// Development build only: 0 = never take the direct-binning route, 1 = take it where it applies; returns the setting.
extern "C" int cugsdbg_sort_direct_route(int on) {
    if (on == 0 || on == 1) g_direct_route.store(on, std::memory_order_relaxed);
    return g_direct_route.load(std::memory_order_relaxed);
}
// Development build only: pairs per Gaussian from which the column-ordered emission is used (0: always).
extern "C" int cugsdbg_sort_column_ratio(int ratio) {
    if (ratio >= 0) g_col_min_ratio.store(ratio, std::memory_order_relaxed);
    return g_col_min_ratio.load(std::memory_order_relaxed);
}
// Debug hook (development build only, not part of the ABI header): force (0 = ballot, 1 = atomic) or query (-2) the ranking mode of the
// radix scatter; returns the mode in effect (-1 = not probed yet).
extern "C" int cugsdbg_sort_rank_mode(int mode) {
    if (mode == 0 || mode == 1 || mode == -1) g_rank_mode.store(mode, std::memory_order_relaxed);
    return g_rank_mode.load(std::memory_order_relaxed);
}
#endif
