// sort_bin.h — direct binning: the pair level as one counting sort by tile id.
#pragma once

#include "sort_bin_cover.h"
#include "sort_tile_order.h"

namespace {

// ------------------------------------------------------------------------------------
// Direct binning (round 3): steps (2)-(4) as ONE counting sort by tile id, for views of up to 2 M Gaussians on images of up
// to BIN_TILES_CAP tiles whose per-Gaussian records are the projection's packed rectangles (render()'s route).  The two
// radix passes over the pairs (emit tile id + index, histogram, scatter, histogram, scatter, range detection: eight
// launches, every pair written three times and read four) become three launches that write every pair ONCE:
//   k_bin_count    a workgroup takes a GROUP of 4096 consecutive Gaussians of the depth order and counts, in LDS, how
//                  many of them cover each tile: row b of the table [groups][tiles];
//   k_bin_scan     per tile, the exclusive prefix of its column of the table (= where group b's first pair of the tile
//                  goes inside the tile's list), the tile's total, and the totals of 64-tile chunks;
//   k_bin_scatter  a wave per (group, block of 8 x 8 tiles) scans the chunk totals into its tiles' starts, walks the
//                  group's records in depth order and writes each pair's Gaussian index straight to
//                  tile start + prefix + pairs of this group written so far; group 0's waves publish the ranges.
// What makes the last kernel a STABLE sort (ties in depth order, bit for bit what the radix passes give): every
// (group, tile) has exactly one writer, a lane that visits the records in order.
// Measured, whole sort, same box (profiles/r03_s_direct_binning.log): 1 M Gaussians / 8.4 M pairs
// 0.200 -> 0.178 ms, 45 M pairs 0.46-0.48 -> 0.355, 100 k Gaussians 0.130 -> 0.119; 6 M Gaussians / 40 M pairs 0.825 vs 0.83
// (not taken there).  What was tried on the way is in profiles/README.md (a workgroup per group with tile ownership by
// wave and 64-bit cover words for the ranking: 0.25 ms, latency-bound at one workgroup per CU; a wave per tile row or
// per band of four rows: 0.23-0.25, instruction-bound on the per-record scalar loop).
// ------------------------------------------------------------------------------------
constexpr int BIN_WAVES = 16, BIN_NT = BIN_WAVES * CUGS_WAVE;
// The scatter's workgroups: up to 8 horizontally adjacent blocks of 8 x 8 tiles, evenly filled (15 block columns: 8 + 7)
inline uint32_t bin_window_groups(int ntx) { const uint32_t nbx = ((uint32_t)ntx + 7u) / 8u; return (nbx + 7u) / 8u; }
inline uint32_t bin_window_cols(int ntx) {       // tile columns per window
    const uint32_t nbx = ((uint32_t)ntx + 7u) / 8u, gxs = bin_window_groups(ntx);
    return ((nbx + gxs - 1u) / gxs) * 8u;
}
inline uint32_t bin_windows(int ntx, int nty) { return (((uint32_t)nty + 7u) / 8u) * bin_window_groups(ntx); }

// rect: the records in INPUT order (gathered through `order` and packed here, prect_out keeps them for the scatter) unless
// prect_in holds them in depth order already (they rode through the depth passes).
// Counting costs FOUR LDS atomics per Gaussian, whatever its size: +1 / -1 at the corners of its rectangle in a grid of
// differences, then a prefix sum along the rows and one along the columns (a loop over the w x h tiles of each lane's own
// rectangle keeps a quarter of the lanes busy, and an LDS atomic instruction costs the same ~9 clocks of the CU's LDS
// pipeline with 15 active lanes as with 64: 33 us at 8.4 pairs per Gaussian, 200 at 45).
constexpr int BIN_D_MAX = BIN_TILES_CAP + 2 * CUGS_PRECT_MAX_TILES + 2;   // (ntx + 1) x (nty + 1) differences
__global__ __launch_bounds__(BIN_NT) void k_bin_count(uint32_t n, uint32_t group, const uint32_t* __restrict__ order,
                                                      const int4* __restrict__ rect, const uint32_t* __restrict__ prect_in,
                                                      uint32_t* __restrict__ prect_out, uint32_t ntx, uint32_t nty,
                                                      uint32_t* __restrict__ table, uint32_t* __restrict__ zero_pairs,
                                                      uint32_t* __restrict__ win) {
    __shared__ int32_t s_d[BIN_D_MAX];
    if (blockIdx.x == 0 && threadIdx.x < BIN_WINDOWS_MAX) win[threadIdx.x] = 0u;      // k_bin_scan adds the windows' pairs up
    __shared__ int32_t s_part[8][128];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t w2 = ntx + 1u, cells = w2 * (nty + 1u);
    for (uint32_t e = tid; e < cells; e += BIN_NT) s_d[e] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * group;
    const uint32_t end = min(n, base + group);
    for (uint32_t i = base + tid; i < end; i += BIN_NT) {
        uint32_t pr;
        if (prect_in) {
            pr = prect_in[i];
        } else {
            pr = pack_rect(rect[order[i]]);                           // the one gather per Gaussian
            prect_out[i] = pr;
        }
        if (pr & 0x80000000u) {                                       // no rectangle: nothing, or quirk Q12's zero slots
            const uint32_t z = pr & 0x7FFFFFFFu;
            if (z) atomicAdd(zero_pairs, z);
            continue;
        }
        const uint32_t x0 = pr & 127u, y0 = (pr >> 7) & 127u, w = (pr >> 14) & 127u, h = (pr >> 21) & 127u;
        atomicAdd(&s_d[y0 * w2 + x0], 1);
        atomicAdd(&s_d[y0 * w2 + x0 + w], -1);
        atomicAdd(&s_d[(y0 + h) * w2 + x0], -1);
        atomicAdd(&s_d[(y0 + h) * w2 + x0 + w], 1);
    }
    __syncthreads();
    for (uint32_t row = wave; row < nty; row += BIN_WAVES) {           // prefix along x: a wave per row
        int32_t carry = 0;
        for (uint32_t c0 = 0; c0 < ntx; c0 += CUGS_WAVE) {
            const uint32_t x = c0 + lane;
            const int32_t v = x < ntx ? s_d[row * w2 + x] : 0;
            const int32_t inc = (int32_t)wave_inclusive_scan((uint32_t)v) + carry;
            if (x < ntx) s_d[row * w2 + x] = inc;
            carry = __shfl(inc, 63);
        }
    }
    __syncthreads();
    {   // prefix along y: thread = (column, one of eight runs of rows)
        const uint32_t x = tid & 127u, seg = tid >> 7;
        const uint32_t rps = (nty + 7u) / 8u;
        const uint32_t ya = min(nty, seg * rps), yb = min(nty, ya + rps);
        int32_t sum = 0;
        if (x < ntx)
            for (uint32_t y = ya; y < yb; ++y) sum += s_d[y * w2 + x];
        s_part[seg][x] = sum;
        __syncthreads();
        int32_t run = 0;
        for (uint32_t s2 = 0; s2 < seg; ++s2) run += s_part[s2][x];
        if (x < ntx)
            for (uint32_t y = ya; y < yb; ++y) {
                run += s_d[y * w2 + x];
                s_d[y * w2 + x] = run;
            }
    }
    __syncthreads();
    uint32_t* out = table + (size_t)blockIdx.x * (ntx * nty);
    for (uint32_t row = wave; row < nty; row += BIN_WAVES)
        for (uint32_t x = lane; x < ntx; x += CUGS_WAVE) out[row * ntx + x] = (uint32_t)s_d[row * w2 + x];
}

// Workgroup = 64 tiles x 16 runs of table rows.  In place: table[b][t] becomes the number of pairs of tile t in the
// workgroups before b; ttot[t] = pairs of tile t.  Block 0 also takes the snapshots the scatter works from: the Q12 count
// k_bin_count has finished adding to (snap[0]; the counter is re-armed) and the depth range flag (snap[1]; re-armed).
// No grid-wide step here: a workgroup that waits for the others' totals must first make its own visible across the
// XCDs' L2s (a release fence = an L2 write-back with 8 MB of freshly written table in it: this kernel took 52 us that
// way).  Each workgroup leaves the prefix of its 64 tiles' totals and their sum (a chunk) instead; the scatter's waves
// finish the scan over the <= 160 chunk sums themselves.
__global__ __launch_bounds__(BIN_NT) void k_bin_scan(uint32_t rows, uint32_t tiles, uint32_t* __restrict__ table,
                                                     uint32_t* __restrict__ ttot, uint32_t* __restrict__ tpre,
                                                     uint32_t* __restrict__ csum, uint32_t* __restrict__ q12,
                                                     uint32_t* __restrict__ range_flag, uint32_t* __restrict__ snap,
                                                     uint32_t* __restrict__ win, uint32_t ntx, uint32_t win_cols,
                                                     uint32_t gxs) {
    __shared__ uint32_t s_seg[BIN_WAVES][CUGS_WAVE];
    __shared__ uint32_t s_win[BIN_WINDOWS_MAX];                       // touched by wave 0 only
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        snap[0] = q12[0]; q12[1] = q12[0]; q12[0] = 0u;
        snap[1] = *range_flag; *range_flag = 0u;
    }
    const uint32_t tl = threadIdx.x & 63u, seg = threadIdx.x >> 6;
    const uint32_t t = blockIdx.x * CUGS_WAVE + tl;
    const uint32_t rps = (rows + BIN_WAVES - 1u) / BIN_WAVES;
    const uint32_t r0 = min(rows, seg * rps), r1 = min(rows, r0 + rps);
    uint32_t sum = 0u;
    if (t < tiles) {
#pragma unroll 8
        for (uint32_t r = r0; r < r1; ++r) sum += table[(size_t)r * tiles + t];
    }
    s_seg[seg][tl] = sum;
    __syncthreads();
    uint32_t pre = 0u, tot = 0u;
#pragma unroll
    for (uint32_t s2 = 0; s2 < (uint32_t)BIN_WAVES; ++s2) {
        const uint32_t v = s_seg[s2][tl];
        pre += s2 < seg ? v : 0u;
        tot += v;
    }
    if (t < tiles) {
        uint32_t run = pre;
#pragma unroll 8
        for (uint32_t r = r0; r < r1; ++r) {
            const uint32_t v = table[(size_t)r * tiles + t];
            table[(size_t)r * tiles + t] = run;
            run += v;
        }
    }
    if (seg == 0u) {                                                  // this workgroup's 64 tiles (a CHUNK): totals, their prefix, their sum
        const uint32_t v = t < tiles ? tot : 0u;
        const uint32_t inc = wave_inclusive_scan(v);
        if (t < tiles) { ttot[t] = v; tpre[t] = inc - v; }
        if (tl == 63u) csum[blockIdx.x] = inc;
        // pairs per WINDOW of the scatter (8 tile rows x win_cols tile columns: one workgroup per group of the depth order):
        // what the scatter orders its workgroups by (win == NULL: more windows than BIN_WINDOWS_MAX, no ordering)
        if (win) {                                                    // (kernel-uniform; all of it inside this one wave)
            s_win[tl] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (v) {
                const uint32_t ty = t / ntx, tx = t - ty * ntx;
                atomicAdd(&s_win[(ty >> 3) * gxs + tx / win_cols], v);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t mine = s_win[tl];
            if (mine) atomicAdd(&win[tl], mine);
        }
    }
}

// A WAVE per (group of the depth order, block of 8 x 8 tiles): lane = tile, the next free slot of the lane's tile lives in a
// register, and the wave walks - in depth order - the records of the group whose rectangle touches its block.  STAGE: each
// one is ONE masked step, the lanes inside the rectangle take the Gaussian's index for their tile's slot and advance
// (~25 dependent, mostly scalar instructions per hit).  Direct: the hits are gathered 64 at a time, lane = hit forms the
// cover mask of the block, a bit-matrix transpose across the wave turns that into lane = tile, and every tile lane pops
// its own hits in order (bin_pop_batch below; 80 -> 64 us at 1 M Gaussians / 8.4 M pairs).
// Stable by construction (one wave per tile, records in order): no atomics, no ranking, and tens of thousands of
// independent waves that hide each other's latencies.
// A workgroup is up to eight horizontally adjacent blocks.  Its waves first share out a pre-filter - each takes a slice of the
// group's records straight from memory and lists in LDS, in order, the ones that touch the workgroup's 8-row, <= 64-column
// window (one in twelve at 1080p), with their Gaussian index - and every wave then tests only the listed ones against its
// own block.
constexpr int BIN_BLK = 8;                        // tile block edge: 64 tiles, one per lane
constexpr int BIN_WG_WAVES = 8;
constexpr int BIN_SLICE = 512;                    // records per wave and stage in the pre-filter
constexpr int BIN_SLICE_STEPS = BIN_SLICE / CUGS_WAVE;
// STAGE (dense views: from BIN_STAGE_RATIO pairs per Gaussian on): a lane collects the indices for its tile in LDS and
// writes them sixteen at a time - one 64-byte run of its tile's list - instead of one scattered 4-byte store per pair
// (45 M of those are two thirds of the kernel on the dense 1080p view).  The sparse views keep the direct stores: their
// (group, tile) runs are ~4 entries long, and the buffer's LDS would halve the resident workgroups.
constexpr int BIN_RUN = 16;                       // entries a lane collects before the wave writes (16: two workgroups per CU, sort 0.270-0.279 ms
                                                  // on the dense 1080p view; 8: three per CU, 0.277-0.285; without the buffer 0.345)
constexpr int BIN_RUN_STRIDE = BIN_RUN + 3;       // LDS row stride in dwords: odd (the lanes' rows start in different banks), and the
                                                  // flush reads up to three entries beyond `held`
// ---- the direct (not STAGE) variant's walk: lanes = hits -> lanes = tiles through a bit-matrix transpose ----
// Orders this wave's LDS traffic for the compiler: what the lanes wrote before is what any lane reads after.  (The LDS
// itself executes one wave's instructions in order; no instruction comes out of this.)
__device__ __forceinline__ void bin_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
template <int CTRL>
__device__ __forceinline__ uint32_t bin_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// One block-swap stage of the transpose inside a dword: v = this lane's row, p = the row of lane ^ S, M = the bit
// positions with (position & S) == 0.  The lane without bit S keeps those and takes the partner's from them, moved up
// by S; the lane with bit S keeps the others and takes the partner's from them, moved down.  Both are a rotation of p
// (no bit that is taken wraps) and one v_bfi with the lane's keep mask: no branch, whatever the lane.
template <int S, uint32_t M>
__device__ __forceinline__ uint32_t bin_tr_merge(uint32_t v, uint32_t p, bool upper) {
    const uint32_t keep = upper ? ~M : M;
    const uint32_t moved = __builtin_rotateright32(p, upper ? (uint32_t)S : 32u - (uint32_t)S);
    return (v & keep) | (moved & ~keep);
}
// 64 x 64 bit-matrix transpose across the wave: in, lane c holds row c (bit t of {hi, lo}); out, lane t holds column t
// (bit c).  Six block-swap stages on the two dwords: 32 is one v_permlane32_swap (lo of the upper half <-> hi of the
// lower half, exactly the two off-diagonal 32 x 32 blocks), 16 goes through ds_bpermute (a v_permlane16_swap wants a
// copy and a select per dword), 8 / 4 / 2 / 1 are DPP: row_ror:8, row_half_mirror then quad_perm [3,2,1,0] (= lane ^ 4),
// quad_perm [2,3,0,1], quad_perm [1,0,3,2].  All 64 lanes must be active.
__device__ __forceinline__ void bin_transpose64(uint32_t& lo, uint32_t& hi, uint32_t lane) {
    {
        const auto r = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);
        lo = r[0]; hi = r[1];
    }
    {
        const bool up = (lane & 16u) != 0u;
        const uint32_t pl = (uint32_t)__shfl_xor((int)lo, 16), ph = (uint32_t)__shfl_xor((int)hi, 16);
        lo = bin_tr_merge<16, 0x0000FFFFu>(lo, pl, up); hi = bin_tr_merge<16, 0x0000FFFFu>(hi, ph, up);
    }
    {
        const bool up = (lane & 8u) != 0u;
        const uint32_t pl = bin_dpp<0x128>(lo), ph = bin_dpp<0x128>(hi);
        lo = bin_tr_merge<8, 0x00FF00FFu>(lo, pl, up); hi = bin_tr_merge<8, 0x00FF00FFu>(hi, ph, up);
    }
    {
        const bool up = (lane & 4u) != 0u;
        const uint32_t pl = bin_dpp<0x1B>(bin_dpp<0x141>(lo)), ph = bin_dpp<0x1B>(bin_dpp<0x141>(hi));
        lo = bin_tr_merge<4, 0x0F0F0F0Fu>(lo, pl, up); hi = bin_tr_merge<4, 0x0F0F0F0Fu>(hi, ph, up);
    }
    {
        const bool up = (lane & 2u) != 0u;
        const uint32_t pl = bin_dpp<0x4E>(lo), ph = bin_dpp<0x4E>(hi);
        lo = bin_tr_merge<2, 0x33333333u>(lo, pl, up); hi = bin_tr_merge<2, 0x33333333u>(hi, ph, up);
    }
    {
        const bool up = (lane & 1u) != 0u;
        const uint32_t pl = bin_dpp<0xB1>(lo), ph = bin_dpp<0xB1>(hi);
        lo = bin_tr_merge<1, 0x55555555u>(lo, pl, up); hi = bin_tr_merge<1, 0x55555555u>(hi, ph, up);
    }
}
// Writes one batch of buffered hits (hits[0 .. count), count <= 64, in depth order; wave-uniform call, all lanes active).
// Lane c forms hit c's cover of the block; after the transpose lane t holds the hits that cover ITS tile and pops them in
// ascending order = depth order: the hit's Gaussian index from LDS to the tile's next slot.  A per-lane loop under EXEC,
// as long as the fullest tile of the batch; nothing per hit on the scalar unit.
__device__ __forceinline__ void bin_pop_batch(const uint2* hits, uint32_t count, uint32_t lane, uint32_t blk_tx0,
                                              uint32_t blk_ty0, bool tile_ok, char* outb, uint32_t& pos) {
    bin_wave_lds_sync();
    const uint64_t cover = lane < count ? bin_cover_mask(hits[lane].x, blk_tx0, blk_ty0) : 0ull;
    uint32_t lo = (uint32_t)cover, hi = (uint32_t)(cover >> 32);
    bin_transpose64(lo, hi, lane);
    if (!tile_ok) lo = hi = 0u;                                       // a tile outside the image never stores
    const uint32_t* const word = reinterpret_cast<const uint32_t*>(hits);     // hit b's Gaussian: word 2 b + 1
    while (lo != 0u) {
        const uint32_t b = (uint32_t)__builtin_ctz(lo);
        lo &= lo - 1u;
        *reinterpret_cast<uint32_t*>(outb + pos) = word[2u * b + 1u];
        pos += 4u;
    }
    while (hi != 0u) {
        const uint32_t b = (uint32_t)__builtin_ctz(hi);
        hi &= hi - 1u;
        *reinterpret_cast<uint32_t*>(outb + pos) = word[2u * b + 65u];
        pos += 4u;
    }
    bin_wave_lds_sync();                                              // the buffer is free again
}

template <bool STAGE>
__global__ __launch_bounds__(BIN_WG_WAVES * CUGS_WAVE) void k_bin_scatter(
    uint32_t n, uint32_t group, uint32_t nbx, uint32_t nby, uint32_t gxs, uint32_t pairs_or_cap, bool predicted,
    const uint32_t* __restrict__ order, const uint32_t* __restrict__ prect, uint32_t ntx, uint32_t nty,
    const uint32_t* __restrict__ table, const uint32_t* __restrict__ ttot, const uint32_t* __restrict__ tpre,
    const uint32_t* __restrict__ csum, const uint32_t* __restrict__ snap, uint32_t* __restrict__ tbase,
    unsigned long long* __restrict__ total, unsigned long long* __restrict__ total_mapped, uint32_t* __restrict__ out,
    int32_t* __restrict__ tile_ranges, uint32_t* __restrict__ tile_order, const uint32_t* __restrict__ win) {
    __shared__ uint2 s_cand[BIN_WG_WAVES][BIN_SLICE];                 // {packed rectangle, Gaussian} of the listed records
    __shared__ uint32_t s_cnt[BIN_WG_WAVES];
    __shared__ uint2 s_hit[STAGE ? 1 : BIN_WG_WAVES * CUGS_WAVE];     // direct: a wave's batch of hits, {packed rectangle, Gaussian}
    __shared__ uint32_t s_run[STAGE ? BIN_WG_WAVES * CUGS_WAVE * BIN_RUN_STRIDE + 4 : 1];   // (+ the read-ahead of the last row's flush)
    const uint32_t nt = blockDim.x, nw = nt >> 6, tid = threadIdx.x, wid = tid >> 6, lane = tid & 63u;
    const uint32_t per_group = nby * gxs;
    // Which (group, window) this workgroup takes.  Balanced views: group-major (the windows of one group side by side:
    // they read the same records).  When one window holds over twice the mean (a view whose splats cluster: half of every
    // group's records can fall into ONE 8 x 8 tile block, whose wave then walks them one by one for tens of microseconds):
    // window-major with the heaviest window first, so that those long workgroups all start at once instead of one per
    // group all the way to the end of the grid (k_bin_scatter 155 -> 96 us with half of the splats on 2 % of the screen).
    uint32_t blk = blockIdx.x / per_group, rem = blockIdx.x - blk * per_group;
    const uint32_t win_mine = (win && lane < per_group) ? win[lane] : 0u;     // pairs of window `lane` (k_bin_scan)
    const uint32_t zero = snap[0];                                    // quirk Q12's (tile 0, Gaussian 0) pairs: the head of tile 0's list
    const bool bad = snap[1] != 0u;                                   // a depth key outside the three-pass range: nothing is valid
    const uint32_t tiles = ntx * nty;

    // Tile starts, by every wave for itself (a kernel of its own for this scan cost 10 us of the frame): the totals of the
    // 64-tile chunks (k_bin_scan's workgroups: <= 160 of them) scanned across the lanes, + the tile's prefix inside its chunk.
    const uint32_t nch = (tiles + CUGS_WAVE - 1u) / CUGS_WAVE;
    uint32_t cpre[3] = {0u, 0u, 0u};                                  // exclusive prefix of chunk (lane + 64 i)
    uint32_t pairs = zero;                                            // the pair total, SATURATING at 2^32 - 1 (such a total never fits)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if ((uint32_t)i * CUGS_WAVE < nch) {                          // kernel-uniform: 128 chunks at 1080p = two scans
            const uint32_t c = lane + (uint32_t)i * CUGS_WAVE;
            const uint32_t v = c < nch ? csum[c] : 0u;
            uint32_t inc = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(inc, d);
                const uint32_t sum = inc + o;
                if ((int)lane >= d) inc = sum < o ? 0xFFFFFFFFu : sum;
            }
            const uint32_t with = inc + pairs;                        // + the chunks of the earlier scans (and the Q12 pairs)
            cpre[i] = (with < inc ? 0xFFFFFFFFu : with) - v;          // (meaningless once saturated: nothing is written then)
            const uint32_t last = __shfl(inc, 63), tot = last + pairs;
            pairs = tot < last ? 0xFFFFFFFFu : tot;
        }
    }
    const bool fits = !bad && (!predicted || pairs <= pairs_or_cap);
    cpre[0] -= zero; cpre[1] -= zero; cpre[2] -= zero;                // (the Q12 pairs are added to `start` below)
    // does one window hold over twice the mean?  (one compare and a ballot per wave; `pairs` is the total)
    if (__ballot((unsigned long long)win_mine * per_group > 2ull * pairs) != 0ull) {     // kernel-uniform
        uint32_t rank = 0u;                                           // (v_readlane with a scalar lane: no LDS round trips)
        for (uint32_t w2 = 0; w2 < per_group; ++w2) {
            const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)win_mine, (int)w2);
            rank += (o > win_mine || (o == win_mine && w2 < lane)) ? 1u : 0u;
        }
        const uint32_t groups = gridDim.x / per_group;
        const uint32_t slot = blockIdx.x / groups;
        blk = blockIdx.x - slot * groups;
        rem = (uint32_t)__builtin_ctzll(__ballot(lane < per_group && rank == slot));
    }
    const uint32_t by = rem / gxs, gx = rem - by * gxs;

    const uint32_t bx = gx * nw + wid;
    const bool active = bx < nbx;
    const uint32_t tx = bx * BIN_BLK + (lane & 7u), ty = by * BIN_BLK + (lane >> 3);      // this lane's tile
    const bool tile_ok = active && tx < ntx && ty < nty;
    const uint32_t t = tile_ok ? ty * ntx + tx : 0u;
    uint32_t start;                                                   // where the first REAL pair of the tile goes
    {
        const uint32_t ch = t >> 6;
        const uint32_t p0 = __shfl(cpre[0], ch & 63u), p1 = __shfl(cpre[1], ch & 63u), p2 = __shfl(cpre[2], ch & 63u);
        start = zero + (ch < 64u ? p0 : ch < 128u ? p1 : p2) + (tile_ok ? tpre[t] : 0u);
    }
    uint32_t pos = tile_ok ? (start + table[(size_t)blk * tiles + t]) * 4u : 0u;           // BYTE offset of the tile's next slot
    if (blk == 0u) {
        // group 0's waves cover every tile once: they publish what k_scan_blocksums / k_tile_ranges publish on the radix
        // route.  When the pairs do not fit the buffer (or the depth order is invalid) the result is declared invalid
        // through the total, nothing is written, and EVERY range is {0,0}: the blend queued behind this kernel then does
        // nothing instead of walking an unwritten index buffer.
        if (tile_ok) {
            const uint32_t c = fits ? ttot[t] + (t == 0u ? zero : 0u) : 0u;                 // {0,0} for untouched tiles (sorting.cu:216)
            tile_ranges[2 * t + 0] = c ? (int32_t)(t == 0u ? 0u : start) : 0;
            tile_ranges[2 * t + 1] = c ? (int32_t)(start + ttot[t]) : 0;
            tbase[t] = start;
        }
        if (rem == 0u && tid == 0u) {
            unsigned long long exact = zero;                          // in 64 bits: int32 overflow is the host's check
            for (uint32_t c = 0; c < nch; ++c) exact += csum[c];
            tbase[tiles] = pairs;
            const unsigned long long host_total = bad ? ~0ull : exact;
            total[0] = bad ? 0ull : exact;
            total[1] = host_total;
            if (total_mapped) __hip_atomic_store(total_mapped, host_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (tile_order && blockIdx.x == 0u) {                             // the blend kernels' workgroup order, by this one workgroup
        uint32_t* const s_lds = reinterpret_cast<uint32_t*>(&s_cand[0][0]);   // (the candidate lists are not in use yet)
        uint32_t* const s_chunk = s_lds + ORDER_LDS;                  // exclusive prefix of every chunk, for the tile starts
        if (wid == 0u) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (lane + (uint32_t)i * CUGS_WAVE < nch) s_chunk[lane + (uint32_t)i * CUGS_WAVE] = cpre[i];
        }
        write_tile_order(tiles, [&](uint32_t t2) { return fits ? ttot[t2] + (t2 == 0u ? zero : 0u) : 0u; },
                         [&](uint32_t t2) { return t2 == 0u ? 0u : zero + s_chunk[t2 >> 6] + tpre[t2]; },
                         reinterpret_cast<uint4*>(tile_order), s_lds);
    }
    if (!fits) return;
    if (blk == 0u)                                                    // the Q12 slots: (tile 0, Gaussian 0) pairs
        for (uint32_t k = rem * nt + tid; k < zero; k += per_group * nt) out[k] = 0u;
    // the workgroup's window, in tiles
    const uint32_t win_y0 = by * BIN_BLK, win_y1 = win_y0 + BIN_BLK;
    const uint32_t win_x0 = gx * nw * BIN_BLK, win_x1 = win_x0 + nw * BIN_BLK;
    const uint32_t blk_x0 = bx * BIN_BLK, blk_x1 = blk_x0 + BIN_BLK;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    char* const outb = reinterpret_cast<char*>(out);
    uint32_t* const run = s_run + (STAGE ? tid * BIN_RUN_STRIDE : 0u);      // STAGE: this lane's collected indices
    uint32_t held = 0u;
    uint2* const hits = s_hit + (STAGE ? 0u : wid * CUGS_WAVE);       // direct: this wave's batch and how many hits it holds
    uint32_t nhit = 0u;
    const uint32_t base = blk * group;
    const uint32_t end = min(n, base + group);                        // base < end: the grid covers ceil(n / group) groups
    const uint32_t stage = nw * BIN_SLICE;
    for (uint32_t c0 = base; c0 < end; c0 += stage) {
        __syncthreads();                                              // every wave is done with the last stage's lists
        {   // pre-filter: this wave's slice against the workgroup's window (a record without a rectangle has bit 31 set)
            const uint32_t s_begin = c0 + wid * BIN_SLICE;
            uint32_t pr[BIN_SLICE_STEPS], gq[BIN_SLICE_STEPS];
            bool ov[BIN_SLICE_STEPS];
#pragma unroll
            for (int u = 0; u < BIN_SLICE_STEPS; ++u) {               // all loads first (clamped addresses, no branches):
                const uint32_t i = s_begin + (uint32_t)u * CUGS_WAVE + lane;      // ONE memory round trip per stage
                pr[u] = prect[min(i, end - 1u)];
                gq[u] = order[min(i, end - 1u)];
                if (i >= end) pr[u] = 0x80000000u;
            }
#pragma unroll
            for (int u = 0; u < BIN_SLICE_STEPS; ++u) {
                const uint32_t x0 = pr[u] & 127u, y0 = (pr[u] >> 7) & 127u, w = (pr[u] >> 14) & 127u, h = (pr[u] >> 21) & 127u;
                ov[u] = (int32_t)pr[u] >= 0 && y0 < win_y1 && y0 + h > win_y0 && x0 < win_x1 && x0 + w > win_x0;
            }
            uint32_t found = 0u;
#pragma unroll
            for (int u = 0; u < BIN_SLICE_STEPS; ++u) {
                const unsigned long long m = __ballot(ov[u]);
                if (ov[u]) s_cand[wid][found + (uint32_t)__popcll(m & lt_mask)] = make_uint2(pr[u], gq[u]);
                found += (uint32_t)__popcll(m);
            }
            if (lane == 0u) s_cnt[wid] = found;
        }
        __syncthreads();
        if (!active) continue;
        if constexpr (!STAGE) {
            // The lists one after the other, 64 candidates at a time: the lanes whose candidate touches the block append
            // it to the wave's batch at the ballot prefix (depth order kept), and every 64 hits the batch is written by
            // bin_pop_batch.  What is left rides on to the next list, the next stage, and is written after the group.
            const uint32_t cnts = s_cnt[lane & (uint32_t)(BIN_WG_WAVES - 1)];      // all the lists' lengths in one read
            for (uint32_t w2 = 0; w2 < nw; ++w2) {
                const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cnts, (int)w2);
                for (uint32_t k0 = 0; k0 < c; k0 += CUGS_WAVE) {
                    const uint2 rec = s_cand[w2][k0 + lane];          // (k0 + lane < BIN_SLICE; beyond c: stale, not a hit)
                    const uint32_t x0v = rec.x & 127u, wv = (rec.x >> 14) & 127u;
                    const bool hit = k0 + lane < c && (int32_t)rec.x >= 0 && x0v < blk_x1 && x0v + wv > blk_x0;
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
                    const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, nhit));
                    if (hit && slot < (uint32_t)CUGS_WAVE) hits[slot] = rec;
                    nhit = (uint32_t)__builtin_amdgcn_readfirstlane((int)(nhit + (uint32_t)__popcll(m)));   // (in an SGPR)
                    if (nhit >= (uint32_t)CUGS_WAVE) {                // (wave-uniform)
                        bin_pop_batch(hits, (uint32_t)CUGS_WAVE, lane, blk_x0, win_y0, tile_ok, outb, pos);
                        if (hit && slot >= (uint32_t)CUGS_WAVE) hits[slot - (uint32_t)CUGS_WAVE] = rec;
                        nhit -= (uint32_t)CUGS_WAVE;
                    }
                }
            }
            continue;
        }
        for (uint32_t w2 = 0; w2 < nw; ++w2) {                        // the slices' lists one after the other: depth order
            const uint32_t c = s_cnt[w2];
            for (uint32_t k0 = 0; k0 < c; k0 += CUGS_WAVE) {
                uint2 rec = make_uint2(0x80000000u, 0u);
                if (k0 + lane < c) rec = s_cand[w2][k0 + lane];
                const uint32_t x0v = rec.x & 127u, wv = (rec.x >> 14) & 127u;
                unsigned long long m = __ballot((int32_t)rec.x >= 0 && x0v < blk_x1 && x0v + wv > blk_x0);
                while (m != 0ull) {
                    const int l = __builtin_ctzll(m);
                    m &= m - 1ull;
                    const uint32_t prl = (uint32_t)__builtin_amdgcn_readlane((int)rec.x, l);
                    const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)rec.y, l);
                    const uint32_t x0 = prl & 127u, y0 = (prl >> 7) & 127u, w = (prl >> 14) & 127u, h = (prl >> 21) & 127u;
                    const bool in = ((tx - x0) < w) & ((ty - y0) < h);     // unsigned: inside the rectangle
                    if constexpr (STAGE) {
                        if (in) run[held++] = g;
                        if (__ballot(held == (uint32_t)BIN_RUN) != 0ull) {
                            // one lane's row is full: EVERY lane writes the whole 16-byte pieces it holds (all lanes at
                            // once - a flush by the one or two full lanes alone is a string of nearly empty instructions)
                            // and keeps the up to three entries left over
                            const uint32_t whole = held & ~3u;
#pragma unroll
                            for (int q = 0; q < BIN_RUN; q += 4)
                                if ((uint32_t)q < whole)
                                    *reinterpret_cast<uint4*>(outb + pos + 4 * q) = make_uint4(run[q], run[q + 1], run[q + 2], run[q + 3]);
                            const uint32_t rest = held - whole;
                            const uint32_t r0 = run[whole], r1 = run[whole + 1u], r2 = run[whole + 2u];   // (reads ahead of `held`: values unused)
                            if (rest > 0u) run[0] = r0;
                            if (rest > 1u) run[1] = r1;
                            if (rest > 2u) run[2] = r2;
                            pos += 4u * whole;
                            held = rest;
                        }
                    } else if (in) {
                        *reinterpret_cast<uint32_t*>(outb + pos) = g;
                        pos += 4u;
                    }
                }
            }
        }
    }
    if constexpr (!STAGE) {
        if (nhit != 0u) bin_pop_batch(hits, nhit, lane, blk_x0, win_y0, tile_ok, outb, pos);      // the rest of the group
    }
    if constexpr (STAGE) {                                            // what the lanes still hold
        for (uint32_t q = 0; __ballot(q < held) != 0ull; ++q)
            if (q < held) *reinterpret_cast<uint32_t*>(outb + pos + 4u * q) = run[q];
    }
}

// SortingOutput::gaussian_keys_sorted for the direct route (only when the caller asks for the keys): the tile of pair i
// is the last tile whose list starts at or before i.
__global__ __launch_bounds__(CUGS_BLOCK) void k_bin_keys(uint32_t pairs_or_cap, const unsigned long long* __restrict__ dev_count,
                                                         uint32_t tiles, const uint32_t* __restrict__ tbase,
                                                         const uint32_t* __restrict__ zero_snap,
                                                         const int32_t* __restrict__ pidx, const float* __restrict__ depths,
                                                         uint64_t* __restrict__ keys_sorted) {
    if (dev_count && *dev_count > (unsigned long long)pairs_or_cap) return;   // the pairs did not fit: no indices were written
    const uint32_t total = live_count(pairs_or_cap, dev_count);
    const uint32_t i = blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (i >= total) return;
    if (i < *zero_snap) { keys_sorted[i] = 0ull; return; }            // Q12 pairs: key 0
    uint32_t lo = 0u, hi = tiles;                                     // largest t in [0, tiles) with tbase[t] <= i (tbase[0] = Z <= i)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tbase[mid] <= i) lo = mid; else hi = mid;
    }
    keys_sorted[i] = ((uint64_t)lo << 32) | (uint64_t)__float_as_uint(depths[pidx[i]]);
}

}  // namespace
