// sort_radix.h — one radix pass (histogram, row scan, stable scatter) and the scan helpers every sort kernel shares.
#pragma once

#include "sort_workspace.h"

namespace {

// ------------------------------------------------------------------------------------
// wave / workgroup scan helpers (low-frequency paths; plain shuffles)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// Exclusive scan of one value per thread over a workgroup of NW waves; *total = workgroup sum.
// s_tmp: NW dwords of LDS.  Contains two barriers.
template <int NW = 4>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* s_tmp, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = wave_inclusive_scan(v);
    if (lane == 63) s_tmp[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const uint32_t t = s_tmp[w];
        base += (w < wave) ? t : 0u;
        sum += t;
    }
    if (total) *total = sum;
    __syncthreads();
    return base + inc - v;
}

// Pair-level kernels take their item count either exactly (dev_count == nullptr: `count`) or, for the
// predicted-capacity path (cugs_sort_pairs_predicted), as min(*dev_count, count) with `count` the capacity
// of the buffers - the host has not read the total yet.
__device__ __forceinline__ uint32_t live_count(uint32_t count, const unsigned long long* __restrict__ dev_count) {
    if (!dev_count) return count;
    const unsigned long long t = *dev_count;
    return t < (unsigned long long)count ? (uint32_t)t : count;
}

// ctl: when given, block 0 hands the Q12 counter k_fill_pairs has finished adding to (ctl[0]) over to
// k_tile_ranges (ctl[1]) and re-arms it, so that cugs_sort_pairs may be repeated on one count.
template <typename K, int NT, int CHUNK, int RDX = RADIX>
__global__ __launch_bounds__(NT) void k_radix_hist(const K* __restrict__ keys, uint32_t count_or_cap,
                                                   const unsigned long long* __restrict__ dev_count, int shift,
                                                   uint32_t mask, uint32_t* __restrict__ hist, uint32_t nblk,
                                                   uint32_t* __restrict__ ctl, uint32_t* __restrict__ sup, uint32_t sb) {
    const uint32_t count = live_count(count_or_cap, dev_count);
    constexpr int PER = CHUNK / NT;                           // consecutive keys per thread (order is irrelevant here)
    constexpr int NWORDS = PER * (int)sizeof(K) / 4;          // ... fetched as dwords in 16- or 8-byte loads
    static_assert(NWORDS >= 2 && NWORDS * 4 == PER * (int)sizeof(K), "whole 8-byte loads per thread");
    static_assert(NT >= RDX, "one thread per digit");
    __shared__ uint32_t s_cnt[RDX];
    if (threadIdx.x < RDX) s_cnt[threadIdx.x] = 0;
    if (ctl && blockIdx.x == 0 && threadIdx.x == 0) { ctl[1] = ctl[0]; ctl[0] = 0u; }
    __syncthreads();
    const uint32_t bbase = blockIdx.x * CHUNK;
    if (bbase + CHUNK <= count) {
        uint32_t wds[NWORDS];
        if constexpr (NWORDS % 4 == 0) {
            const uint4* src = reinterpret_cast<const uint4*>(keys + bbase + threadIdx.x * PER);
#pragma unroll
            for (int v = 0; v < NWORDS / 4; ++v) {
                const uint4 q = src[v];
                wds[4 * v] = q.x; wds[4 * v + 1] = q.y; wds[4 * v + 2] = q.z; wds[4 * v + 3] = q.w;
            }
        } else {
            const uint2* src = reinterpret_cast<const uint2*>(keys + bbase + threadIdx.x * PER);
#pragma unroll
            for (int v = 0; v < NWORDS / 2; ++v) {
                const uint2 q = src[v];
                wds[2 * v] = q.x; wds[2 * v + 1] = q.y;
            }
        }
#pragma unroll
        for (int c = 0; c < NWORDS; ++c) {
            if (sizeof(K) == 4) {
                atomicAdd(&s_cnt[(wds[c] >> shift) & mask], 1u);
            } else {
                atomicAdd(&s_cnt[((wds[c] & 0xFFFFu) >> shift) & mask], 1u);
                atomicAdd(&s_cnt[((wds[c] >> 16) >> shift) & mask], 1u);
            }
        }
    } else {
        for (uint32_t i = bbase + threadIdx.x; i < count; i += NT)
            atomicAdd(&s_cnt[((uint32_t)keys[i] >> shift) & mask], 1u);
    }
    __syncthreads();
    if (threadIdx.x < RDX) {
        const uint32_t c = s_cnt[threadIdx.x];
        if (sup) {                                                              // scan-free pass (kernel-uniform)
            hist[(size_t)blockIdx.x * RDX + threadIdx.x] = c;                   // block-major: one contiguous row
            if (c) atomicAdd(&sup[(size_t)(blockIdx.x / sb) * RDX + threadIdx.x], c);
        } else {
            hist[(size_t)threadIdx.x * nblk + blockIdx.x] = c;                  // digit-major, for k_radix_scan_rows
        }
    }
}

// Block d: exclusive scan of row d of hist into `out` (may be hist itself); tot[d] = row sum.
__global__ __launch_bounds__(CUGS_BLOCK) void k_radix_scan_rows(const uint32_t* hist, uint32_t* out,
                                                                uint32_t nblk, uint32_t* __restrict__ tot) {
    __shared__ uint32_t s_tmp[4];
    constexpr int PER = 8;                                   // consecutive entries per thread: 2048 per iteration
    const uint32_t* row = hist + (size_t)blockIdx.x * nblk;
    uint32_t* orow = out + (size_t)blockIdx.x * nblk;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblk; base += CUGS_BLOCK * PER) {
        const uint32_t i0 = base + threadIdx.x * PER;
        uint32_t v[PER], sum = 0;
#pragma unroll
        for (int e = 0; e < PER; ++e) { v[e] = (i0 + e < nblk) ? row[i0 + e] : 0u; sum += v[e]; }
        uint32_t total;
        uint32_t run = carry + block_exclusive_scan(sum, s_tmp, &total);
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            if (i0 + e < nblk) orow[i0 + e] = run;
            run += v[e];
        }
        carry += total;
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// Stable scatter.  Ranking: each wave owns a contiguous 1024-item slice and walks it in rounds of
// 64; in a round the lanes holding the same digit find each other with one ballot per digit bit (match-any), the
// rank is the popcount below the lane, and the group's highest lane advances the wave's running
// base in LDS.  The (key, value) pairs are first placed at their position in the workgroup's LOCALLY
// sorted order in LDS and then streamed out, so that consecutive lanes write consecutive global
// addresses inside each digit's run (4 B items scattered straight to 128-256 buckets cost ~2x).
// IOTA: first pass of the depth sort, which generates the Gaussian index instead of reading a value
// array.  NB: digit width (the match-any needs one ballot per digit bit).  NT: threads per workgroup -
// 256 for the pair-level passes (thousands of workgroups), 1024 for the depth sort, whose 4096-item
// chunks are too few to fill the chip with 4 waves each.
// V2: a second dword per item travels with the first (the depth sort's packed tile rectangle, pack_rect).
template <typename K, bool IOTA, int NB, int NT, bool ARANK, int CHUNK, int RDX = RADIX, bool V2 = false>
__global__ __launch_bounds__(NT) void k_radix_scatter(
    const K* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, uint32_t count_or_cap,
    const unsigned long long* __restrict__ dev_count, int shift, uint32_t mask_rt, const uint32_t* __restrict__ hist,
    const uint32_t* __restrict__ sup, uint32_t sb, const uint32_t* __restrict__ tot, uint32_t nblk,
    K* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
    const uint32_t* __restrict__ vals2_in = nullptr, uint32_t* __restrict__ vals2_out = nullptr) {
    const uint32_t mask = ARANK ? mask_rt : ((1u << NB) - 1u);       // the ballot ranking needs the width at compile time
    const uint32_t count = live_count(count_or_cap, dev_count);
    if (blockIdx.x * CHUNK >= count) return;              // chunks beyond the live items (capacity path): nothing to move
    constexpr int NW = NT / CUGS_WAVE;                    // waves
    constexpr int PER = CHUNK / NT;                       // items per thread
    constexpr int SLICE = CUGS_WAVE * PER;                // contiguous items per wave
    static_assert(NT >= RDX && (1 << NB) <= RDX, "one thread per digit");
    __shared__ uint32_t s_lbase[NW][RDX];      // per (wave, digit): count, then running LOCAL position
    __shared__ uint32_t s_lstart[RDX];         // first local position of digit d
    __shared__ uint32_t s_gbase[RDX];          // first global position of this workgroup's digit-d run
    __shared__ K s_key[CHUNK];
    __shared__ uint32_t s_val[CHUNK];
    __shared__ uint32_t s_val2[V2 ? CHUNK : 1];
    __shared__ uint32_t s_tmp[NW];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t bbase = blockIdx.x * CHUNK;
    const uint32_t wbase = bbase + wave * SLICE;
    const uint32_t count_blk = min((uint32_t)CHUNK, count - bbase);

    // Global offsets of this workgroup's digit runs (see the note at sup_block): thread t takes digit t % RDX and every
    // (NT / RDX)-th row, partial sums meet in LDS further down.  The loads go out first thing and are consumed after the
    // local ranking.  Rows of blocks beyond the live count hold zeros (their histogram workgroups wrote them).
    constexpr int ND = ARANK ? RDX : (1 << NB);              // digits that can be non-zero (the rows are RDX wide)
    constexpr int GRP = NT / ND;                             // threads per digit
    uint32_t pre = 0u, totd = 0u;
    if (sup) {                                               // scan-free pass (kernel-uniform)
        const uint32_t d = tid % ND, part = tid / ND;
        const uint32_t mysb = blockIdx.x / sb, nsb = (nblk + sb - 1u) / sb;
#pragma unroll 4
        for (uint32_t r = part; r < nsb; r += GRP) {             // super rows: totals, and the rows before mine
            const uint32_t v = sup[(size_t)r * RDX + d];
            totd += v;
            pre += (r < mysb) ? v : 0u;
        }
#pragma unroll 4
        for (uint32_t b2 = mysb * sb + part; b2 < blockIdx.x; b2 += GRP) pre += hist[(size_t)b2 * RDX + d];   // my super-block
    } else if (tid < RDX) {                                  // k_radix_scan_rows has scanned the digit-major table
        pre = hist[(size_t)tid * nblk + blockIdx.x];
        totd = tot[tid];
    }

    for (uint32_t e = tid; e < NW * RDX; e += NT) (&s_lbase[0][0])[e] = 0;
    if (tid < RDX) { s_gbase[tid] = 0u; s_lstart[tid] = 0u; }     // accumulators of the partial sums (pre, totals)
    __syncthreads();
    if (sup && GRP > 1) {
        if (pre) atomicAdd(&s_gbase[tid % ND], pre);
        if (totd) atomicAdd(&s_lstart[tid % ND], totd);
    } else if (tid < RDX) {
        s_gbase[tid] = pre; s_lstart[tid] = totd;
    }

    uint32_t k[PER], v[PER], v2[V2 ? PER : 1];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        uint32_t i = wbase + r * CUGS_WAVE + lane;
        bool ok = i < count;
        // last use of this pass's input: streamed, so that it does not evict the output being written for the next pass
        k[r] = ok ? (uint32_t)__builtin_nontemporal_load(keys_in + i) : 0xFFFFFFFFu;
        v[r] = ok ? (IOTA ? i : __builtin_nontemporal_load(vals_in + i)) : 0u;
        if constexpr (V2) v2[r] = ok ? __builtin_nontemporal_load(vals2_in + i) : 0u;
        if (ok) atomicAdd(&s_lbase[wave][(k[r] >> shift) & mask], 1u);
    }
    __syncthreads();

    {   // digit d = tid (threads beyond the radix only take part in the barriers)
        const bool dig = tid < RDX;
        uint32_t cnt = 0;
        if (dig) {
#pragma unroll
            for (int w = 0; w < NW; ++w) cnt += s_lbase[w][tid];
        }
        const uint32_t before = dig ? s_gbase[tid] : 0u;                                           // digit d in the workgroups before this one
        const uint32_t dig_base = block_exclusive_scan<NW>(dig ? s_lstart[tid] : 0u, s_tmp, nullptr);   // global digit start
        const uint32_t lstart = block_exclusive_scan<NW>(cnt, s_tmp, nullptr);                     // local digit start
        if (dig) {
            s_gbase[tid] = dig_base + before;
            s_lstart[tid] = lstart;
            uint32_t run = lstart;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const uint32_t c = s_lbase[w][tid];
                s_lbase[w][tid] = run;
                run += c;
            }
        }
    }
    __syncthreads();

    const unsigned long long lt_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const uint32_t i = wbase + r * CUGS_WAVE + lane;
        const bool ok = i < count;
        const uint32_t d = (k[r] >> shift) & mask;
        if constexpr (ARANK) {
            // One LDS atomic with return per item: the hardware serves the lanes of a wave instruction that hit the
            // same counter in ascending lane order and a wave's LDS instructions in issue order, so the returned
            // values ARE the stable positions.  That ordering is not in the ISA manual: it is verified on the device
            // before this path is ever selected (k_probe_lds_order), and the ballot path below stays as the fallback.
            if (ok) {
                const uint32_t pos = atomicAdd(&s_lbase[wave][d], 1u);
                s_key[pos] = (K)k[r];
                s_val[pos] = v[r];
                if constexpr (V2) s_val2[pos] = v2[r];
            }
            continue;
        }
        unsigned long long peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        if (ok) {
            const uint32_t base = s_lbase[wave][d];
            const uint32_t pos = base + __popcll(peers & lt_mask);
            s_key[pos] = (K)k[r];
            s_val[pos] = v[r];
            if constexpr (V2) s_val2[pos] = v2[r];
            if ((peers >> lane) == 1ull) s_lbase[wave][d] = base + __popcll(peers);
        }
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const uint32_t j = r * NT + tid;
        if (j < count_blk) {
            const K key = s_key[j];
            const uint32_t d = ((uint32_t)key >> shift) & mask;
            const uint32_t dst = s_gbase[d] + (j - s_lstart[d]);
            keys_out[dst] = key;
            vals_out[dst] = s_val[j];
            if constexpr (V2) vals2_out[dst] = s_val2[j];
        }
    }
}

#ifdef CUGS_DEV
// ---- development build only (libcugs_hip_dev.so): ranking by one LDS atomic-with-return per item -------------
// Measured 7 % faster than the ballot ranking (sort 0.250 -> 0.232 ms at config 3), but it relies on an ordering
// of same-address LDS lanes that the ISA manual does not state.  The shipped library therefore always ranks with
// wave ballots, keeps no mode variable and reads no environment; this path, its on-device probe and the
// cugsdbg_sort_rank_mode hook exist only for experiments (tests/test_gpu_parity.py runs both modes against the
// oracle in a child process that loads the development library).
// Does an LDS atomic with return serve the lanes of one wave instruction that hit the SAME address in ascending
// lane order, and successive instructions of a wave in issue order?  Each lane checks that the value it got back
// equals the number of earlier (round, lane) items with its digit, for random, clustered, constant, same-bank and
// strided digit patterns; *violations counts the mismatches.
__device__ __forceinline__ uint32_t probe_digit(uint32_t set, uint32_t wave, uint32_t r, uint32_t lane) {
    uint32_t h = (set * 4u + wave) * 8u + r;
    h = (h ^ 61u) ^ (h >> 16); h *= 9u; h ^= h >> 4; h *= 0x27d4eb2du; h ^= h >> 15;
    uint32_t x = h + lane * 0x9E3779B9u;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    switch (set % 6u) {
        case 0: return x & 255u;
        case 1: return x & 127u;
        case 2: return x & 3u;
        case 3: return 5u;
        case 4: return (x & 1u) ? 7u : 39u;                       // same LDS bank, 32 dwords apart
        default: return (lane * 37u + (x & 1u)) & 63u;
    }
}
__global__ __launch_bounds__(CUGS_BLOCK) void k_probe_lds_order(uint32_t* __restrict__ violations) {
    __shared__ uint32_t cnt[4][RADIX];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, set = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < 4 * RADIX; i += CUGS_BLOCK) (&cnt[0][0])[i] = 0;
    __syncthreads();
    uint32_t d[8], got[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = probe_digit(set, wave, r, lane);
#pragma unroll
    for (int r = 0; r < 8; ++r) got[r] = atomicAdd(&cnt[wave][d[r]], 1u);
    uint32_t bad = 0;
    for (int r = 0; r < 8; ++r) {
        uint32_t expect = 0;
        for (int rr = 0; rr <= r; ++rr)
            for (uint32_t l = 0; l < 64u && !(rr == r && l >= lane); ++l) expect += probe_digit(set, wave, rr, l) == d[r];
        bad += expect != got[r];
    }
    if (bad) atomicAdd(violations, bad);
}
#endif

// One pass: histogram, (row scan,) stable scatter.
template <typename K, bool IOTA, int NT, int CHUNK, int RDX = RADIX>
int radix_pass(const K* kin, const uint32_t* vin, uint32_t count, const unsigned long long* dev_count, int shift, int bits,
               uint32_t* hist, uint32_t* sup, uint32_t* tot, K* kout, uint32_t* vout, uint32_t* ctl, hipStream_t st,
               const uint32_t* v2in = nullptr, uint32_t* v2out = nullptr) {
    // `sup`: this pass's super-block table, ZEROED by an earlier kernel of the stream (the key kernel / the projection for
    // the depth passes, the pair emission for the pair passes); used for passes of up to SCANFREE_MAX_BLOCKS workgroups
    const uint32_t nblk = nblocks_for(count, CHUNK);
    const uint32_t sb = sup_block(nblk);
    static_assert(NT % RDX == 0, "whole thread groups per digit");
    if (!scan_free(nblk, (uint32_t)NT >> bits)) sup = nullptr;
    hipLaunchKernelGGL((k_radix_hist<K, NT, CHUNK, RDX>), dim3(nblk), dim3(NT), 0, st, kin, count, dev_count, shift,
                       (1u << bits) - 1u, hist, nblk, ctl, sup, sb);
    CUGS_LAUNCH_CHECK();
    if (!sup) {
        hipLaunchKernelGGL(k_radix_scan_rows, dim3(RDX), dim3(CUGS_BLOCK), 0, st, hist, hist, nblk, tot);
        CUGS_LAUNCH_CHECK();
    }
    if constexpr (RDX == RADIX_DEPTH) {                    // the 9-bit passes of the depth sort: ballot ranking only
        if (v2in)                                          // the packed tile rectangle rides along
            hipLaunchKernelGGL((k_radix_scatter<K, IOTA, DEPTH_BITS, NT, false, CHUNK, RDX, true>), dim3(nblk), dim3(NT), 0, st, kin,
                               vin, count, dev_count, shift, 0u, hist, sup, sb, tot, nblk, kout, vout, v2in, v2out);
        else
            hipLaunchKernelGGL((k_radix_scatter<K, IOTA, DEPTH_BITS, NT, false, CHUNK, RDX>), dim3(nblk), dim3(NT), 0, st, kin, vin, count,
                               dev_count, shift, 0u, hist, sup, sb, tot, nblk, kout, vout);
        CUGS_LAUNCH_CHECK();
        return 0;
    }
    if (v2in) return CUGS_EINVAL;
#ifdef CUGS_DEV
    if (rank_mode() == 1) {               // digit width only matters to the ballot ranking: one instantiation
        hipLaunchKernelGGL((k_radix_scatter<K, IOTA, 8, NT, true, CHUNK>), dim3(nblk), dim3(NT), 0, st, kin, vin, count, dev_count,
                           shift, (1u << bits) - 1u, hist, sup, sb, tot, nblk, kout, vout);
        CUGS_LAUNCH_CHECK();
        return 0;
    }
#endif
#define CUGS_SCATTER(NB)                                                                                          \
    hipLaunchKernelGGL((k_radix_scatter<K, IOTA, NB, NT, false, CHUNK>), dim3(nblk), dim3(NT), 0, st, kin, vin, count, dev_count, \
                       shift, 0u, hist, sup, sb, tot, nblk, kout, vout)
    switch (bits) {
        case 1: CUGS_SCATTER(1); break;
        case 2: CUGS_SCATTER(2); break;
        case 3: CUGS_SCATTER(3); break;
        case 4: CUGS_SCATTER(4); break;
        case 5: CUGS_SCATTER(5); break;
        case 6: CUGS_SCATTER(6); break;
        case 7: CUGS_SCATTER(7); break;
        default: CUGS_SCATTER(8); break;
    }
#undef CUGS_SCATTER
    CUGS_LAUNCH_CHECK();
    return 0;
}

}  // namespace
