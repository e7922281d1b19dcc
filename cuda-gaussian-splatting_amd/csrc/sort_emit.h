// sort_emit.h — per-Gaussian keys and records, pair counts, pair emission (depth order / tile-column order), tile ranges.
#pragma once

#include "sort_radix.h"

namespace {

// Reference quirk Q12: a splat whose tile rectangle is empty in both axes still has
// tiles_touched = (negative) x (negative) > 0 (projection.cu:187-188); k_fill_sort_pairs writes
// nothing for it and its reserved slots keep the zero-initialised (key 0, value 0) pairs
// (sorting.cu:166-167), which sort to the front of tile 0.  Reproduced here by giving such a
// Gaussian the depth key 0 (its pairs are emitted first) and emitting (tile 0, Gaussian 0).
//
// One sequential read of the projection outputs produces the depth key and a 16-byte tile-rectangle
// record per Gaussian, so that the depth-ordered stages gather ONE record per Gaussian instead of
// tiles_touched, radius and mean separately (random 4-8 byte gathers were what bounded k_fill_pairs).
__global__ __launch_bounds__(CUGS_BLOCK) void k_depth_keys_rect(uint32_t n, const float* __restrict__ depths,
                                                                const float* __restrict__ means_2d,
                                                                const int32_t* __restrict__ radii,
                                                                const int32_t* __restrict__ tiles, int img_w,
                                                                int img_h, int ntx, int nty,
                                                                uint32_t* __restrict__ keys,
                                                                int4* __restrict__ rect,
                                                                uint32_t* __restrict__ range_flag,
                                                                uint32_t* __restrict__ zero, uint32_t nzero) {
    const uint32_t i = blockIdx.x * CUGS_BLOCK + threadIdx.x;
    for (uint32_t z = i; z < nzero; z += gridDim.x * CUGS_BLOCK) zero[z] = 0u;     // the depth passes' super tables
    if (i >= n) return;
    const int t = tiles[i];
    const int radius = t > 0 ? radii[i] : 0;
    TileRect tr{0, 0, 0, 0};
    if (t > 0 && radius > 0) tr = tile_rect_of(means_2d[i * 2 + 0], means_2d[i * 2 + 1], radius, img_w, img_h, ntx, nty);
    bool bad;
    const SortRecord r = sort_record_of(depths[i], t, radius, tr, range_flag != nullptr, &bad);
    if (bad) atomicOr(range_flag, 1u);
    keys[i] = r.key;
    rect[i] = r.rect;
}

// ------------------------------------------------------------------------------------
// Pair emission in depth order
// ------------------------------------------------------------------------------------
// Column-ordered emission, step 1: the pairs of each COL_CHUNK block of the depth order per tile column
// (colhist[column][block], digit-major like the radix histograms): a Gaussian adds its rectangle height to each
// column it covers; slots the reference leaves at zero (quirk Q12) count for column 0, where their
// (tile 0, Gaussian 0) pairs go.  One sequential read of the depth-ordered rectangle records.
__global__ __launch_bounds__(COL_CHUNK) void k_col_hist(uint32_t n, const int4* __restrict__ rect_sorted,
                                                        uint32_t* __restrict__ colhist, uint32_t ncol) {
    __shared__ uint32_t s_col[RADIX];
    const uint32_t tid = threadIdx.x;
    if (tid < RADIX) s_col[tid] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * COL_CHUNK + tid;
    if (i < n) {
        const int4 r = rect_sorted[i];
        const uint32_t t = (uint32_t)r.w;
        const int w = r.z & 0xFFFF, h = r.z >> 16;
        if ((uint32_t)(w * h) < t) atomicAdd(&s_col[0], t - (uint32_t)(w * h));
        for (int c = 0; c < w; ++c) atomicAdd(&s_col[r.x + c], (uint32_t)h);
    }
    __syncthreads();
    if (tid < RADIX) colhist[(size_t)tid * ncol + blockIdx.x] = s_col[tid];
}

// prect_sorted (when given): the packed rectangles arrive IN depth order (they rode through the passes): a sequential
// read instead of the gather.
__global__ __launch_bounds__(CUGS_BLOCK) void k_fill_blocksums(uint32_t n,
                                                               const uint32_t* __restrict__ order,
                                                               const int4* __restrict__ rect,
                                                               int4* __restrict__ rect_sorted,
                                                               uint32_t* __restrict__ blocksum,
                                                               const uint32_t* __restrict__ prect_sorted) {
    __shared__ uint32_t s_tmp[4];
    const uint32_t i = blockIdx.x * FILL_CHUNK + threadIdx.x;
    uint32_t acc = 0u;
    if (i < n) {
        const int4 r = prect_sorted ? unpack_rect(__builtin_nontemporal_load(prect_sorted + i))
                                    : rect[order[i]];             // the one gather per Gaussian
        rect_sorted[i] = r;
        acc = (uint32_t)r.w;
    }
    uint32_t total;
    block_exclusive_scan(acc, s_tmp, &total);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

// Single workgroup: exclusive scan of blocksum[0..nb) in place; *total = the 64-bit grand total =
// sum(tiles_touched), the reference's cumsum[-1].item() (sorting.cu:145-146).  16 consecutive entries per
// thread, so 16384 entries cost two barriers.  Also arms the Q12 counter (ctl[0] = 0).
// range_flag (three-pass depth sort): non-zero = some depth key lay outside the range that route covers, the order
// is not valid: the device-side total becomes 0 (every pair-level kernel then does nothing), the host-visible one
// (total[1], total_mapped) -1, and the flag is re-armed.
constexpr int SCAN_NT = 1024;                     // one workgroup, on the critical path of the pair count: as wide as it gets
__global__ __launch_bounds__(SCAN_NT) void k_scan_blocksums(uint32_t* __restrict__ blocksum, uint32_t nb,
                                                            unsigned long long* __restrict__ total,
                                                            uint32_t* __restrict__ ctl,
                                                            unsigned long long* __restrict__ total_mapped,
                                                            uint32_t* __restrict__ range_flag) {
    __shared__ uint32_t s_tmp[SCAN_NT / CUGS_WAVE];
    constexpr int PER = 16;
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < nb; base += SCAN_NT * PER) {
        const uint32_t i0 = base + threadIdx.x * PER;
        uint32_t v[PER], sum = 0;
#pragma unroll
        for (int e = 0; e < PER; ++e) { v[e] = (i0 + e < nb) ? blocksum[i0 + e] : 0u; sum += v[e]; }
        uint32_t chunk_total;
        uint32_t run = (uint32_t)carry + block_exclusive_scan<SCAN_NT / CUGS_WAVE>(sum, s_tmp, &chunk_total);
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            if (i0 + e < nb) blocksum[i0 + e] = run;      // valid whenever the total fits int32 (checked on the host)
            run += v[e];
        }
        carry += chunk_total;
    }
    if (threadIdx.x == 0) {
        bool bad = false;
        if (range_flag) { bad = *range_flag != 0u; *range_flag = 0u; }
        const unsigned long long host_total = bad ? ~0ull : carry;
        total[0] = bad ? 0ull : carry;
        total[1] = host_total;
        ctl[0] = 0u;
        // the caller's pinned host variable, when it is mapped into the device's address space: one store here
        // instead of a copy kernel on the critical path of the predicted-capacity sort (~5 us)
        if (total_mapped) __hip_atomic_store(total_mapped, host_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// k_fill_sort_pairs (sorting.cu:30-72), walked in depth order; only the tile id and the index are
// stored (the depth half of the key is implied by the order).  One Gaussian per thread computes its
// rectangle and its offset (workgroup scan); each wave then emits the pairs of its own 64 Gaussians
// COOPERATIVELY, 256 output slots at a time: the Gaussians whose span starts inside the window stamp
// their lane number at that slot, a running maximum over the window (4 consecutive slots per lane + a
// wave scan) turns the stamps into an owner per slot, and the slots are then written lane-strided -
// consecutive lanes write consecutive pairs, and a splat covering thousands of tiles does not
// serialise one thread.  No workgroup barrier inside the loop.
// Housekeeping shared out over the grid: the {0,0} ranges of untouched tiles (sorting.cu:216).
template <typename K>
__global__ __launch_bounds__(CUGS_BLOCK) void k_fill_pairs(
    uint32_t n, uint32_t pairs_or_cap, const unsigned long long* __restrict__ dev_count,
    const uint32_t* __restrict__ order, const int4* __restrict__ rect_sorted, int ntx,
    const uint32_t* __restrict__ blocksum, K* __restrict__ ptile, uint32_t* __restrict__ pidx,
    uint32_t* __restrict__ zero_pairs, int32_t* __restrict__ tile_ranges, uint32_t range_dwords,
    uint32_t* __restrict__ sup_zero, uint32_t nsup) {
    constexpr int WIN = 4 * CUGS_WAVE;                               // output slots per wave iteration
    __shared__ uint32_t s_tmp[4];
    __shared__ uint32_t s_off[CUGS_BLOCK + 1];
    __shared__ int4 s_info[CUGS_BLOCK];                              // {Gaussian, x0, y0, rect width}
    __shared__ int s_cnt[CUGS_BLOCK];
    __shared__ uint4 s_own[4][CUGS_WAVE];                            // per wave: owner lane of each window slot
    const uint32_t total_pairs = live_count(pairs_or_cap, dev_count);
    for (uint32_t z = blockIdx.x * CUGS_BLOCK + threadIdx.x; z < range_dwords; z += gridDim.x * CUGS_BLOCK)
        tile_ranges[z] = 0;
    for (uint32_t z = blockIdx.x * CUGS_BLOCK + threadIdx.x; z < nsup; z += gridDim.x * CUGS_BLOCK)
        sup_zero[z] = 0u;                                            // the pair passes' super tables (radix_pass)
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t i = blockIdx.x * FILL_CHUNK + tid;
    uint32_t g = 0, t = 0;
    int x0 = 0, y0 = 0, w = 0, real = 0;          // real = pairs the reference's loops would write
    if (i < n) {
        g = __builtin_nontemporal_load(order + i);                     // last use of both streams
        typedef int v4i_ __attribute__((ext_vector_type(4)));
        const v4i_ r = __builtin_nontemporal_load(reinterpret_cast<const v4i_*>(rect_sorted) + i);
        t = (uint32_t)r.w;
        x0 = r.x; y0 = r.y; w = r.z & 0xFFFF;
        real = w * (r.z >> 16);
        if ((uint32_t)real < t) atomicAdd(zero_pairs, t - (uint32_t)real);       // quirk Q12 slots (rare)
    }
    uint32_t blk_total;
    const uint32_t off = block_exclusive_scan(t, s_tmp, &blk_total);
    s_off[tid] = off;
    s_info[tid] = make_int4((int)g, x0, y0, w);
    s_cnt[tid] = real;
    if (tid == 0) s_off[CUGS_BLOCK] = blk_total;
    __syncthreads();

    const uint32_t out_base = blocksum[blockIdx.x];
    const uint32_t wstart = s_off[wave * CUGS_WAVE], wend = s_off[wave * CUGS_WAVE + CUGS_WAVE];
    uint4* own4 = s_own[wave];
    const uint32_t* own = reinterpret_cast<const uint32_t*>(own4);
    uint32_t carry = 0;                                              // owner of the slot before the window
    for (uint32_t base = wstart; base < wend; base += WIN) {
        own4[lane] = make_uint4(0u, 0u, 0u, 0u);
        __builtin_amdgcn_wave_barrier();
        if (t > 0 && off >= base && off - base < (uint32_t)WIN) reinterpret_cast<uint32_t*>(own4)[off - base] = lane;
        __builtin_amdgcn_wave_barrier();
        uint4 a = own4[lane];
        a.y = max(a.x, a.y); a.z = max(a.y, a.z); a.w = max(a.z, a.w);
        uint32_t inc = a.w;                                          // inclusive running maximum over lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d);
            if ((int)lane >= d) inc = max(inc, o);
        }
        uint32_t pre = __shfl_up(inc, 1);
        pre = max(lane == 0 ? 0u : pre, carry);
        a.x = max(a.x, pre); a.y = max(a.y, pre); a.z = max(a.z, pre); a.w = max(a.w, pre);
        carry = __shfl(a.w, 63);
        own4[lane] = a;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t k = base + e * CUGS_WAVE + lane;
            if (k < wend) {
                const uint32_t j = wave * CUGS_WAVE + own[e * CUGS_WAVE + lane];
                const uint32_t local = k - s_off[j];
                uint32_t tile = 0u, idx = 0u;                        // slots the reference leaves at zero (Q12)
                if ((int)local < s_cnt[j]) {
                    const int4 info = s_info[j];
                    const int row = (int)local / info.w;
                    tile = (uint32_t)((info.z + row) * ntx + info.y + ((int)local - row * info.w));
                    idx = (uint32_t)info.x;
                }
                const uint32_t dst = out_base + k;
                if (dst < total_pairs) {                             // never write past the buffers
                    ptile[dst] = (K)tile;
                    pidx[dst] = idx;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Pair emission ordered by TILE COLUMN (then depth, then row): the first pass of the stable sort by tile id,
// done while the pairs are generated.  Key written per pair: (row << 8 | column), images of <= 256 x 256 tiles.
// The unit is an ITEM = (Gaussian, column it covers), worth `height` consecutive pairs - ~3x fewer items than
// pairs at 1080p.  A workgroup takes COL_CHUNK Gaussians of the depth order and
//   (b) sets, per column, one bit per Gaussian that covers it (LDS bit matrix; OR commutes, so no ordering issue);
//   (c) counts each column's bits (prefix per 32-Gaussian word) and scans the counts over the columns;
//   (d) drops each item's record at  column start + set bits below its Gaussian  - the items are now sorted by
//       (column, depth) - with its height beside it;
//   (e) scans the heights: the local slot of every item's first pair, and per column the offset between local
//       slots and the column's run in the output (column start + pairs of the workgroups before this one, from
//       the scanned column histogram of k_col_hist);
//   (g) streams the pairs out, 64 sorted items per wave round (rounds handed out by an LDS counter), lane = item:
//       neighbouring lanes own neighbouring runs of the output, so the `height` store instructions of a round
//       complete each other's cache lines (writing from UNSORTED items cost 2x the HBM write requests; a slot-
//       parallel loop with a 6-step owner search per slot was bound by its ~136 instructions per 64 pairs).
// LDS holds ICAP items; a workgroup with more (dense views) works in batches of whole Gaussians.
// Slots the reference's loops leave at zero (tiles_touched beyond the w x h pairs of the rectangle: the Q12
// Gaussians, whose rectangle is empty) are ONE more item of the Gaussian worth that many (tile 0, Gaussian 0)
// pairs, in a pseudo column ordered before column 0 and sharing its run.  Q12 Gaussians are first in depth
// order, hence first in column 0, hence (row pass) first in tile 0, where the reference's zero pairs sort to.
__global__ __launch_bounds__(COL_CHUNK) void k_col_emit(
    uint32_t n, uint32_t pairs_or_cap, const unsigned long long* __restrict__ dev_count,
    const uint32_t* __restrict__ order, const int4* __restrict__ rect_sorted,
    const uint32_t* __restrict__ colscan, const uint32_t* __restrict__ coltot, uint32_t nblk,
    uint16_t* __restrict__ ptile, uint32_t* __restrict__ pidx,
    uint32_t* __restrict__ zero_pairs, int32_t* __restrict__ tile_ranges, uint32_t range_dwords,
    uint32_t* __restrict__ sup_zero, uint32_t nsup) {
    constexpr int NT = COL_CHUNK, NW = COL_WAVES;
    for (uint32_t z = blockIdx.x * COL_CHUNK + threadIdx.x; z < nsup; z += gridDim.x * COL_CHUNK)
        sup_zero[z] = 0u;                                            // the row pass's super table (radix_pass)
    constexpr int NWORD = NT / 32;                                   // bit-matrix words per column
    constexpr int NC = RADIX + 1, ZCOL = RADIX;                      // tile columns + the zero-slot pseudo column
    constexpr int NCP = RADIX + 4;
    constexpr int PER = 6;                                           // staged items per thread
    constexpr int ICAP = PER * NT;
    constexpr int IWIN = ICAP - (RADIX + 1);                         // a batch: the Gaussians whose first item is in one window
    static_assert(NT >= NC, "one thread per column");
    __shared__ uint32_t s_cover[NWORD][NCP];
    __shared__ uint16_t s_wpre[NWORD][NCP];
    __shared__ uint32_t s_istart[NCP];                               // first sorted item of each column (this batch)
    __shared__ uint32_t s_gpos[NCP];                                 // where the workgroup's next pair of each column goes
    __shared__ uint32_t s_delta[NCP];                                // output position - local slot, per column (this batch)
    __shared__ uint2 s_item[ICAP];                                   // {row0 << 8 | column (bit 31: zero item), Gaussian}
    __shared__ uint32_t s_poff[ICAP + 1];                            // height, then local slot of the item's first pair
    __shared__ uint32_t s_tmp[NW];
    __shared__ uint32_t s_next;
    const uint32_t total_pairs = live_count(pairs_or_cap, dev_count);
    for (uint32_t z = blockIdx.x * NT + threadIdx.x; z < range_dwords; z += gridDim.x * NT) tile_ranges[z] = 0;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t i = blockIdx.x * NT + tid;
    uint32_t g = 0, t = 0;
    int x0 = 0, y0 = 0, w = 0, h = 0;
    if (i < n) {
        g = order[i];
        const int4 r = rect_sorted[i];
        t = (uint32_t)r.w;
        x0 = r.x; y0 = r.y; w = r.z & 0xFFFF; h = r.z >> 16;
    }
    const uint32_t nzero = (uint32_t)(w * h) < t ? t - (uint32_t)(w * h) : 0u;
    if (nzero) atomicAdd(zero_pairs, nzero);                         // quirk Q12 slots (rare)
    const uint32_t ni = t == 0u ? 0u : (uint32_t)w + (nzero ? 1u : 0u);   // items of this Gaussian
    {   // where this workgroup's run of each column starts
        const bool col = tid < RADIX;
        const uint32_t col_start = block_exclusive_scan<NW>(col ? coltot[tid] : 0u, s_tmp, nullptr);
        if (col) s_gpos[tid] = col_start + colscan[(size_t)tid * nblk + blockIdx.x];
    }
    uint32_t itot;
    const uint32_t ioff = block_exclusive_scan<NW>(ni, s_tmp, &itot);
    const uint32_t my_batch = ioff / IWIN;
    const uint32_t nbatch = (itot + IWIN - 1) / IWIN;
    const uint32_t word = tid >> 5, bit = 1u << (tid & 31u);
    const uint32_t cu = tid == 0 ? (uint32_t)ZCOL : tid - 1u;        // column of thread `tid` in scan order: pseudo column first

    for (uint32_t k = 0; k < nbatch; ++k) {
        const bool mine = t > 0u && my_batch == k;
        for (uint32_t e = tid; e < NWORD * NCP; e += NT) (&s_cover[0][0])[e] = 0u;
        __syncthreads();
        if (mine) {                                                  // (b)
            for (int c = 0; c < w; ++c) atomicOr(&s_cover[word][x0 + c], bit);
            if (nzero) atomicOr(&s_cover[word][ZCOL], bit);
        }
        __syncthreads();
        uint32_t cnt = 0u;                                           // (c)
        if (tid < NC) {
            uint32_t bits[NWORD];
#pragma unroll
            for (int q = 0; q < NWORD; ++q) bits[q] = s_cover[q][cu];
#pragma unroll
            for (int q = 0; q < NWORD; ++q) {
                s_wpre[q][cu] = (uint16_t)cnt;
                cnt += __popc(bits[q]);
            }
        }
        uint32_t icount;
        const uint32_t ist = block_exclusive_scan<NW>(cnt, s_tmp, &icount);
        if (tid < NC) s_istart[cu] = ist;
        __syncthreads();
        if (mine) {                                                  // (d)
            for (int c = 0; c < w; ++c) {
                const uint32_t col = (uint32_t)(x0 + c);
                const uint32_t at = s_istart[col] + s_wpre[word][col] + __popc(s_cover[word][col] & (bit - 1u));
                s_item[at] = make_uint2(((uint32_t)y0 << 8) | col, g);
                s_poff[at] = (uint32_t)h;
            }
            if (nzero) {
                const uint32_t at = s_istart[ZCOL] + s_wpre[word][ZCOL] + __popc(s_cover[word][ZCOL] & (bit - 1u));
                s_item[at] = make_uint2(0x80000000u, 0u);
                s_poff[at] = nzero;
            }
        }
        __syncthreads();
        {                                                            // (e) heights -> local slots; s_poff[icount] = pairs of the batch
            const uint32_t e0 = tid * PER;
            uint32_t v[PER], sum = 0u;
#pragma unroll
            for (int e = 0; e < PER; ++e) { v[e] = (e0 + e < icount) ? s_poff[e0 + e] : 0u; sum += v[e]; }
            uint32_t run = block_exclusive_scan<NW>(sum, s_tmp, nullptr);
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                if (e0 + e <= icount) s_poff[e0 + e] = run;
                run += v[e];
            }
        }
        __syncthreads();
        if (tid >= 1u && tid < NC) {                                 // column cu = tid - 1; column 0 also serves the pseudo column
            const uint32_t first = (cu == 0u) ? s_istart[ZCOL] : ist;          // the pseudo column's items sit right before column 0's
            const uint32_t lo_slot = s_poff[first], hi_slot = s_poff[ist + cnt];
            const uint32_t d = s_gpos[cu] - lo_slot;
            s_delta[cu] = d;
            if (cu == 0u) s_delta[ZCOL] = d;
            s_gpos[cu] += hi_slot - lo_slot;
        }
        if (tid == 0) s_next = 0u;
        __syncthreads();
        const uint32_t nround = (icount + CUGS_WAVE - 1) / CUGS_WAVE;  // (g)
        while (true) {
            uint32_t r = 0u;
            if (lane == 0) r = atomicAdd(&s_next, 1u);
            r = __builtin_amdgcn_readfirstlane(r);
            if (r >= nround) break;
            const uint32_t it = r * CUGS_WAVE + lane;
            const bool valid = it < icount;
            uint32_t slot = 0u, cnt_it = 0u;
            uint2 rec = make_uint2(0u, 0u);
            if (valid) {
                slot = s_poff[it];
                cnt_it = s_poff[it + 1] - slot;
                rec = s_item[it];
            }
            const bool zero = rec.x >> 31;
            const uint32_t dst0 = slot + s_delta[zero ? (uint32_t)ZCOL : (rec.x & 255u)];
            // lane = item, walking down its rows: neighbouring lanes hold neighbouring runs of the output, so the
            // `height` store instructions of a round fill the same cache lines between them
            if (!zero) {
                const uint32_t room = dst0 < total_pairs ? total_pairs - dst0 : 0u;     // never write past the buffers
                const uint32_t rows = min(cnt_it, room);
                uint16_t* kp = ptile + dst0;
                uint32_t* ip = pidx + dst0;
                uint32_t key = rec.x;
                for (uint32_t y = 0; y < rows; ++y) {
                    kp[y] = (uint16_t)key;
                    ip[y] = rec.y;
                    key += 256u;
                }
            }
            for (unsigned long long m = __ballot(valid && zero); m; m &= m - 1ull) {   // zero slots: by the whole wave
                const int l = __builtin_ctzll(m);
                const uint32_t p = __shfl(dst0, l), c = __shfl(cnt_it, l);
                for (uint32_t sl = lane; sl < c; sl += CUGS_WAVE)
                    if (p + sl < total_pairs) { ptile[p + sl] = 0; pidx[p + sl] = 0u; }
            }
        }
        __syncthreads();
    }
}

// k_compute_tile_ranges (sorting.cu:82-109) on the sorted tile ids; optionally rebuilds the
// reference's sorted 64-bit keys (SortingOutput::gaussian_keys_sorted, sorting.hpp:20).
// COLKEY: the keys are (row << 8 | column) as written by k_col_emit; ntx turns them back into tile ids.
template <typename K, bool COLKEY>
__global__ __launch_bounds__(CUGS_BLOCK) void k_tile_ranges(uint32_t pairs_or_cap,
                                                            const unsigned long long* __restrict__ dev_count,
                                                            const K* __restrict__ ptile, uint32_t ntx,
                                                            const int32_t* __restrict__ pidx,
                                                            const float* __restrict__ depths,
                                                            int32_t* __restrict__ tile_ranges,
                                                            uint64_t* __restrict__ keys_sorted,
                                                            const uint32_t* __restrict__ zero_pairs) {
    constexpr int PER = 8;                                   // consecutive pairs per thread (one or two 16-byte loads)
    const uint32_t total_pairs = live_count(pairs_or_cap, dev_count);
    const uint32_t i0 = (blockIdx.x * CUGS_BLOCK + threadIdx.x) * PER;
    if (i0 >= total_pairs) return;
    uint32_t t[PER];
    if (i0 + PER <= total_pairs) {
        if (sizeof(K) == 2) {
            const uint4 q = *reinterpret_cast<const uint4*>(ptile + i0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) { t[2 * e] = w[e] & 0xFFFFu; t[2 * e + 1] = w[e] >> 16; }
        } else {
            const uint4 q0 = reinterpret_cast<const uint4*>(ptile + i0)[0], q1 = reinterpret_cast<const uint4*>(ptile + i0)[1];
            t[0] = q0.x; t[1] = q0.y; t[2] = q0.z; t[3] = q0.w; t[4] = q1.x; t[5] = q1.y; t[6] = q1.z; t[7] = q1.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < PER; ++e) t[e] = (i0 + e < total_pairs) ? (uint32_t)ptile[i0 + e] : 0u;
    }
    uint32_t prev = (i0 == 0) ? 0u : (uint32_t)ptile[i0 - 1];
    if constexpr (COLKEY) {
        prev = (prev >> 8) * ntx + (prev & 255u);
#pragma unroll
        for (int e = 0; e < PER; ++e) t[e] = (t[e] >> 8) * ntx + (t[e] & 255u);
    }
    const uint32_t nzero = keys_sorted ? *zero_pairs : 0u;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const uint32_t i = i0 + e;
        if (i >= total_pairs) break;
        const uint32_t cur = t[e];
        if (i == 0) {
            tile_ranges[cur * 2 + 0] = 0;
        } else if (cur != prev) {
            tile_ranges[prev * 2 + 1] = (int32_t)i;
            tile_ranges[cur * 2 + 0] = (int32_t)i;
        }
        if (i == total_pairs - 1) tile_ranges[cur * 2 + 1] = (int32_t)total_pairs;
        if (keys_sorted)   // Q12 pairs are the leading entries of tile 0 and carry depth bits 0
            keys_sorted[i] = (i < nzero) ? 0ull : (((uint64_t)cur << 32) | (uint64_t)__float_as_uint(depths[pidx[i]]));
        prev = cur;
    }
}

}  // namespace
