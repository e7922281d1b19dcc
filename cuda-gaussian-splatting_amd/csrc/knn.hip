// knn.hip — a model from a point cloud: init_gaussians_from_sparse (core/gaussian_init.cpp:25-152) on the device.
//
// The reference's scale initialisation is a brute-force k-nearest-neighbour search on one CPU thread
// (gaussian_init.cpp:38-65: n^2 distances, an nth_element per point).  Here the search is exact on the device, by two routes
// that give the same bits:
//   * exhaustive: one query per lane, every candidate streamed through LDS, the k best d^2 kept sorted in registers;
//   * tree: 63-bit Morton keys over the bounding box, the stable radix sort of sort_radix.h, buckets of 32 consecutive
//     sorted points with their boxes, an implicit 8-ary tree of boxes over the buckets, and a stackless depth-first walk per
//     query that skips a node only when its lower bound is STRICTLY greater than the k-th best d^2 so far.
// The contract both meet: d^2 = (dx*dx + dy*dy) + dz*dz with dx = p_j.x - p_i.x, one fp32 rounding per operation (the library
// is built without contraction); the point itself is excluded by index; m_i = (sum of sqrt(d^2), ascending d^2) / float(k).
// No float atomics, no host read-back, nothing allocated: same bits from run to run.
#include "cugs_common.h"
#include "sort_radix.h"

namespace {

constexpr int KNN_BUCKET = 32;                    // consecutive sorted points per leaf
constexpr int KNN_FAN_BITS = 3;                   // 8 children per inner node
constexpr int KNN_TILE = 1024;                    // candidates per LDS tile of the exhaustive route (16 KB)
constexpr int KNN_BBOX_BLOCKS = 256;              // partial boxes of the bounding-box reduction
constexpr int KNN_CHUNK = CHUNK_MIN;              // items per workgroup in the radix passes
constexpr int KNN_MAX_LEVELS = 10;                // n <= 2^30: 2^25 buckets, 8^9 > 2^25
constexpr int64_t KNN_MAX_N = 1ll << 30;
// CUGS_KNN_AUTO takes the tree from this many points on (provisional, from the instruction-count estimate: DESIGN.md §4.15;
// tools/bench_init.py measures the crossover)
constexpr int64_t KNN_AUTO_TREE_FROM = 16384;
constexpr float KNN_INF = __builtin_inff();

// ---- the k best d^2, ascending, in registers ------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void knn_insert(float (&b)[K], float v) {          // caller has checked v < b[K - 1]
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const float lo = fminf(b[j], v);
        v = fmaxf(b[j], v);
        b[j] = lo;
    }
}

template <int K>
__device__ __forceinline__ float knn_mean(const float (&b)[K]) {
    float s = sqrtf(b[0]);
#pragma unroll
    for (int j = 1; j < K; ++j) s = s + sqrtf(b[j]);
    return s / (float)K;
}

__device__ __forceinline__ float knn_d2(float cx, float cy, float cz, float qx, float qy, float qz) {
    const float dx = cx - qx, dy = cy - qy, dz = cz - qz;                       // gaussian_init.cpp:48-51
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- exhaustive route ---------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(CUGS_BLOCK) void k_knn_exhaustive(uint32_t n, const float* __restrict__ pos,
                                                               float* __restrict__ mean) {
    __shared__ float4 s_c[KNN_TILE];
    const uint32_t i = blockIdx.x * CUGS_BLOCK + threadIdx.x;
    const bool live = i < n;
    const float qx = live ? pos[3 * (size_t)i] : 0.0f, qy = live ? pos[3 * (size_t)i + 1] : 0.0f,
                qz = live ? pos[3 * (size_t)i + 2] : 0.0f;
    float b[K];
#pragma unroll
    for (int j = 0; j < K; ++j) b[j] = KNN_INF;
    for (uint32_t base = 0; base < n; base += KNN_TILE) {
        const uint32_t cnt = min((uint32_t)KNN_TILE, n - base);
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < cnt; t += CUGS_BLOCK) {
            const float* p = pos + 3 * (size_t)(base + t);
            s_c[t] = make_float4(p[0], p[1], p[2], 0.0f);
        }
        __syncthreads();
        const uint32_t self = i - base;                                          // >= cnt when the query is not in this tile
#pragma unroll 4
        for (uint32_t t = 0; t < cnt; ++t) {
            const float4 c = s_c[t];                                             // one address per wave: an LDS broadcast
            const float d2 = knn_d2(c.x, c.y, c.z, qx, qy, qz);
            if (d2 < b[K - 1] && t != self) knn_insert<K>(b, d2);
        }
    }
    if (live) mean[i] = knn_mean<K>(b);
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_knn_constant(uint32_t n, float* __restrict__ mean, float v) {
    const uint32_t i = blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (i < n) mean[i] = v;
}

// ---- tree route: bounding box, keys ---------------------------------------------------------------------------------
// min / max are exact and commutative: any reduction order gives the same box.
__device__ __forceinline__ void knn_block_minmax(float (&lo)[3], float (&hi)[3], float (*s_red)[6]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], d));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_red[wave][a] = lo[a]; s_red[wave][3 + a] = hi[a]; }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(fminf(s_red[0][a], s_red[1][a]), fminf(s_red[2][a], s_red[3][a]));
        hi[a] = fmaxf(fmaxf(s_red[0][3 + a], s_red[1][3 + a]), fmaxf(s_red[2][3 + a], s_red[3][3 + a]));
    }
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_knn_bbox_partial(uint32_t n, const float* __restrict__ pos,
                                                                 float* __restrict__ part) {
    static_assert(CUGS_BLOCK == 256, "four waves per workgroup");
    __shared__ float s_red[4][6];
    float lo[3] = {KNN_INF, KNN_INF, KNN_INF}, hi[3] = {-KNN_INF, -KNN_INF, -KNN_INF};
    for (uint32_t i = blockIdx.x * CUGS_BLOCK + threadIdx.x; i < n; i += gridDim.x * CUGS_BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pos[3 * (size_t)i + a];
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
    }
    knn_block_minmax(lo, hi, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[blockIdx.x * 6 + a] = lo[a]; part[blockIdx.x * 6 + 3 + a] = hi[a]; }
    }
}

// bbox[0..2] = lower corner, bbox[3..5] = cells per unit length (0 along an axis of no extent: every key bit of it is 0)
__global__ __launch_bounds__(CUGS_BLOCK) void k_knn_bbox_final(uint32_t nparts, const float* __restrict__ part,
                                                               float* __restrict__ bbox) {
    __shared__ float s_red[4][6];
    float lo[3] = {KNN_INF, KNN_INF, KNN_INF}, hi[3] = {-KNN_INF, -KNN_INF, -KNN_INF};
    for (uint32_t p = threadIdx.x; p < nparts; p += CUGS_BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], part[p * 6 + a]);
            hi[a] = fmaxf(hi[a], part[p * 6 + 3 + a]);
        }
    }
    knn_block_minmax(lo, hi, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float ext = hi[a] - lo[a];
            bbox[a] = lo[a];
            bbox[3 + a] = (ext > 0.0f && ext < KNN_INF) ? 2097151.0f / ext : 0.0f;
        }
    }
}

__device__ __forceinline__ unsigned long long knn_spread3(uint32_t v) {       // 21 bits -> every third bit of 63
    unsigned long long x = v & 0x1FFFFFu;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__device__ __forceinline__ uint32_t knn_cell(float v, float lo, float inv) {
    const float t = fminf(fmaxf((v - lo) * inv, 0.0f), 2097151.0f);            // fmaxf / fminf drop a NaN: always in range
    return min((uint32_t)t, 2097151u);
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_knn_keys(uint32_t n, const float* __restrict__ pos,
                                                         const float* __restrict__ bbox, uint32_t* __restrict__ klo,
                                                         uint32_t* __restrict__ khi) {
    const uint32_t i = blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = knn_spread3(knn_cell(pos[3 * (size_t)i], bbox[0], bbox[3])) |
                                   knn_spread3(knn_cell(pos[3 * (size_t)i + 1], bbox[1], bbox[4])) << 1 |
                                   knn_spread3(knn_cell(pos[3 * (size_t)i + 2], bbox[2], bbox[5])) << 2;
    klo[i] = (uint32_t)key;
    khi[i] = (uint32_t)(key >> 32);
}

// ---- tree route: leaves and inner nodes -----------------------------------------------------------------------------
// Sorted points as (x, y, z, input index); leaf b = sorted points [32 b, 32 b + 32) with its box.  nodes: two float4 per
// node (lower corner, upper corner), level 0 = the leaves, level l + 1 = groups of 8 consecutive nodes of level l.
__global__ __launch_bounds__(CUGS_BLOCK) void k_knn_leaves(uint32_t n, const float* __restrict__ pos,
                                                           const uint32_t* __restrict__ sidx, float4* __restrict__ spos,
                                                           float4* __restrict__ nodes) {
    const uint32_t s = blockIdx.x * CUGS_BLOCK + threadIdx.x;
    float lo[3] = {KNN_INF, KNN_INF, KNN_INF}, hi[3] = {-KNN_INF, -KNN_INF, -KNN_INF};
    if (s < n) {
        const uint32_t i = sidx[s];
        const float x = pos[3 * (size_t)i], y = pos[3 * (size_t)i + 1], z = pos[3 * (size_t)i + 2];
        spos[s] = make_float4(x, y, z, __uint_as_float(i));
        lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int d = KNN_BUCKET / 2; d >= 1; d >>= 1) {                          // stays inside the aligned group of 32 lanes
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], d));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d));
        }
    }
    if ((threadIdx.x & (KNN_BUCKET - 1)) == 0 && s < n) {
        const uint32_t bkt = s / KNN_BUCKET;
        nodes[2 * (size_t)bkt] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        nodes[2 * (size_t)bkt + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_knn_level(uint32_t nchild, const float4* __restrict__ child,
                                                          uint32_t nparent, float4* __restrict__ parent) {
    const uint32_t p = blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (p >= nparent) return;
    float4 lo = make_float4(KNN_INF, KNN_INF, KNN_INF, 0.0f), hi = make_float4(-KNN_INF, -KNN_INF, -KNN_INF, 0.0f);
    const uint32_t c0 = p << KNN_FAN_BITS, c1 = min(c0 + (1u << KNN_FAN_BITS), nchild);
    for (uint32_t c = c0; c < c1; ++c) {
        const float4 l = child[2 * (size_t)c], h = child[2 * (size_t)c + 1];
        lo.x = fminf(lo.x, l.x); lo.y = fminf(lo.y, l.y); lo.z = fminf(lo.z, l.z);
        hi.x = fmaxf(hi.x, h.x); hi.y = fmaxf(hi.y, h.y); hi.z = fmaxf(hi.z, h.z);
    }
    parent[2 * (size_t)p] = lo;
    parent[2 * (size_t)p + 1] = hi;
}

// ---- tree route: the search -----------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void knn_scan_leaf(float (&b)[K], const float4* __restrict__ spos, uint32_t n, uint32_t bkt,
                                              uint32_t self, float qx, float qy, float qz) {
    const uint32_t base = bkt * KNN_BUCKET, cnt = min((uint32_t)KNN_BUCKET, n - base);
    for (uint32_t t = 0; t < cnt; ++t) {
        const float4 c = spos[base + t];
        const float d2 = knn_d2(c.x, c.y, c.z, qx, qy, qz);
        if (d2 < b[K - 1] && base + t != self) knn_insert<K>(b, d2);
    }
}

// Lower bound of d^2 over a box, in the contract's own operation order.  For a point p of the box and an axis where the
// query lies below the box, p.x - q.x >= lo.x - q.x as real numbers, and rounding to nearest keeps that order; likewise
// above the box; products and sums of non-negative values keep it too.  So this never exceeds the d^2 computed for p.
__device__ __forceinline__ float knn_box_bound(float4 lo, float4 hi, float qx, float qy, float qz) {
    const float gx = fmaxf(fmaxf(lo.x - qx, qx - hi.x), 0.0f);
    const float gy = fmaxf(fmaxf(lo.y - qy, qy - hi.y), 0.0f);
    const float gz = fmaxf(fmaxf(lo.z - qz, qz - hi.z), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

template <int K>
__global__ __launch_bounds__(CUGS_BLOCK) void k_knn_tree(uint32_t n, const float4* __restrict__ spos,
                                                         const float4* __restrict__ nodes, int top,
                                                         float* __restrict__ mean) {
    __shared__ uint32_t s_cnt[KNN_MAX_LEVELS], s_off[KNN_MAX_LEVELS];             // nodes of level l, first node of level l
    if (threadIdx.x == 0) {
        const uint32_t nb = (n + KNN_BUCKET - 1) / KNN_BUCKET;
        uint32_t off = 0;
        for (int l = 0; l <= top; ++l) {
            const uint32_t c = (nb + (1u << (KNN_FAN_BITS * l)) - 1u) >> (KNN_FAN_BITS * l);
            s_cnt[l] = c;
            s_off[l] = off;
            off += c;
        }
    }
    __syncthreads();
    const uint32_t s = blockIdx.x * CUGS_BLOCK + threadIdx.x;                     // queries in sorted order: a wave walks
    if (s >= n) return;                                                          // neighbouring paths
    const float4 q = spos[s];
    const uint32_t own = s / KNN_BUCKET;
    float b[K];
#pragma unroll
    for (int j = 0; j < K; ++j) b[j] = KNN_INF;
    knn_scan_leaf<K>(b, spos, n, own, s, q.x, q.y, q.z);                         // a tight bound before the walk starts
    int l = top;
    uint32_t i = 0;
    const uint32_t ntop = s_cnt[top];
    while (b[K - 1] > 0.0f) {                                                    // a k-th best of 0 cannot improve
        bool descend = false;
        if (l != 0 || i != own) {
            const size_t node = (size_t)s_off[l] + i;
            const float bound = knn_box_bound(nodes[2 * node], nodes[2 * node + 1], q.x, q.y, q.z);
            if (!(bound > b[K - 1])) {                                           // skipped only if STRICTLY farther
                if (l == 0) knn_scan_leaf<K>(b, spos, n, i, s, q.x, q.y, q.z);
                else descend = true;
            }
        }
        if (descend) { --l; i <<= KNN_FAN_BITS; continue; }
        ++i;                                                                     // next sibling, or up past finished groups
        while (l < top && ((i & ((1u << KNN_FAN_BITS) - 1u)) == 0u || i >= s_cnt[l])) {
            i = ((i - 1u) >> KNN_FAN_BITS) + 1u;
            ++l;
        }
        if (l == top && i >= ntop) break;
    }
    mean[__float_as_uint(q.w)] = knn_mean<K>(b);                                 // back to input order
}

// ---- fill -----------------------------------------------------------------------------------------------------------
// Element e of the widest array (sh_coeffs, or rotations at one coefficient) also writes element e of the narrower ones.
__global__ __launch_bounds__(CUGS_BLOCK) void k_init_from_points(int64_t n, int C, const float* __restrict__ pos,
                                                                 const uint8_t* __restrict__ col, const float* __restrict__ m,
                                                                 float* __restrict__ opos, float* __restrict__ osh,
                                                                 float* __restrict__ oopa, float* __restrict__ orot,
                                                                 float* __restrict__ oscl) {
    const int64_t e = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (e < n * 3 * C) {
        const int64_t pc = e / C;                                                // point * 3 + channel
        float v = 0.0f;
        if (e - pc * C == 0) {
            const float colour = (float)col[pc] / 255.0f;                        // gaussian_init.cpp:115-116
            v = (colour - 0.5f) / 0.28209479177387814f;
        }
        cugs_stnt(osh + e, v);
    }
    if (e < n * 3) {
        cugs_stnt(opos + e, cugs_ldnt(pos + e));                                 // :98-104
        cugs_stnt(oscl + e, logf(fmaxf(m[e / 3], 1e-7f)));                       // :140
    }
    if (e < n * 4) cugs_stnt(orot + e, (e & 3) == 0 ? 1.0f : 0.0f);              // :129-130
    if (e < n) cugs_stnt(oopa + e, -2.1972245773362196f);                        // :125-126
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct KnnWs {
    float* part;                 // [KNN_BBOX_BLOCKS][6]
    float* bbox;                 // [8]
    uint32_t* tot;               // [RADIX]
    uint32_t* hist;              // [RADIX][nblk]
    uint32_t *klo[2], *khi[2], *idx[2];
    float4* spos;                // [n]
    float4* nodes;               // two per node, all levels
    size_t bytes;
};

struct KnnCarve {
    char* p;
    size_t used = 0;
    template <typename T> T* take(size_t count) {
        used = align_up(used, 256);
        T* r = p ? reinterpret_cast<T*>(p + used) : nullptr;
        used += count * sizeof(T);
        return r;
    }
};

inline int knn_top_level(uint32_t nb) {
    int top = 0;
    while (((nb + (1u << (KNN_FAN_BITS * top)) - 1u) >> (KNN_FAN_BITS * top)) > (1u << KNN_FAN_BITS)) ++top;
    return top;
}

inline KnnWs knn_carve(void* base, int64_t n) {
    KnnWs w;
    char* b = static_cast<char*>(base);
    const size_t skew = b ? (size_t)(align_up(reinterpret_cast<uintptr_t>(b), 256) - reinterpret_cast<uintptr_t>(b)) : 0;
    KnnCarve c{b ? b + skew : nullptr};
    const size_t np = (size_t)(n > 0 ? n : 0);
    const size_t nb = (np + KNN_BUCKET - 1) / KNN_BUCKET;
    w.part = c.take<float>(KNN_BBOX_BLOCKS * 6);
    w.bbox = c.take<float>(8);
    w.tot = c.take<uint32_t>(RADIX);
    w.hist = c.take<uint32_t>((size_t)RADIX * (nblocks_for((int64_t)np, KNN_CHUNK) + 1));
    for (int h = 0; h < 2; ++h) {
        w.klo[h] = c.take<uint32_t>(np + 4);
        w.khi[h] = c.take<uint32_t>(np + 4);
        w.idx[h] = c.take<uint32_t>(np + 4);
    }
    w.spos = c.take<float4>(np + 1);
    w.nodes = c.take<float4>(2 * (nb + nb / 7 + 2 * KNN_MAX_LEVELS));          // sum of ceil(nb / 8^l) <= 8 nb / 7 + levels
    w.bytes = c.used + 256;                                                     // room for aligning the caller's pointer
    return w;
}

// One stable 8-bit pass on a 32-bit half of the key; the index and the other half ride along.
template <bool IOTA>
int knn_radix_pass(const uint32_t* kin, const uint32_t* vin, const uint32_t* v2in, uint32_t* kout, uint32_t* vout,
                   uint32_t* v2out, uint32_t n, int shift, uint32_t* hist, uint32_t* tot, hipStream_t st) {
    const uint32_t nblk = nblocks_for(n, KNN_CHUNK);
    hipLaunchKernelGGL((k_radix_hist<uint32_t, CUGS_BLOCK, KNN_CHUNK>), dim3(nblk), dim3(CUGS_BLOCK), 0, st, kin, n, nullptr,
                       shift, 255u, hist, nblk, nullptr, nullptr, 0u);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_radix_scan_rows, dim3(RADIX), dim3(CUGS_BLOCK), 0, st, hist, hist, nblk, tot);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_radix_scatter<uint32_t, IOTA, 8, CUGS_BLOCK, false, KNN_CHUNK, RADIX, true>), dim3(nblk),
                       dim3(CUGS_BLOCK), 0, st, kin, vin, n, nullptr, shift, 0u, hist, nullptr, 0u, tot, nblk, kout, vout, v2in,
                       v2out);
    CUGS_LAUNCH_CHECK();
    return 0;
}

template <int K>
int knn_launch_exhaustive(uint32_t n, const float* pos, float* mean, hipStream_t st) {
    hipLaunchKernelGGL(k_knn_exhaustive<K>, dim3(nblocks_for(n, CUGS_BLOCK)), dim3(CUGS_BLOCK), 0, st, n, pos, mean);
    CUGS_LAUNCH_CHECK();
    return 0;
}

template <int K>
int knn_launch_tree(uint32_t n, const KnnWs& w, int top, float* mean, hipStream_t st) {
    hipLaunchKernelGGL(k_knn_tree<K>, dim3(nblocks_for(n, CUGS_BLOCK)), dim3(CUGS_BLOCK), 0, st, n, w.spos, w.nodes, top, mean);
    CUGS_LAUNCH_CHECK();
    return 0;
}

#define KNN_DISPATCH(k, call)                                                                        \
    switch (k) {                                                                                     \
        case 1: return call(1);   case 2: return call(2);   case 3: return call(3);   case 4: return call(4);     \
        case 5: return call(5);   case 6: return call(6);   case 7: return call(7);   case 8: return call(8);     \
        case 9: return call(9);   case 10: return call(10); case 11: return call(11); case 12: return call(12);   \
        case 13: return call(13); case 14: return call(14); case 15: return call(15); case 16: return call(16);   \
        default: return CUGS_EINVAL;                                                                 \
    }

int knn_exhaustive(uint32_t n, int k, const float* pos, float* mean, hipStream_t st) {
#define KNN_CALL(K) knn_launch_exhaustive<K>(n, pos, mean, st)
    KNN_DISPATCH(k, KNN_CALL)
#undef KNN_CALL
}

int knn_tree_search(uint32_t n, int k, const KnnWs& w, int top, float* mean, hipStream_t st) {
#define KNN_CALL(K) knn_launch_tree<K>(n, w, top, mean, st)
    KNN_DISPATCH(k, KNN_CALL)
#undef KNN_CALL
}

int knn_tree(uint32_t n, int k, const float* pos, float* mean, const KnnWs& w, hipStream_t st) {
    const uint32_t nblk = nblocks_for(n, CUGS_BLOCK);
    const uint32_t nparts = nblk < (uint32_t)KNN_BBOX_BLOCKS ? nblk : (uint32_t)KNN_BBOX_BLOCKS;
    hipLaunchKernelGGL(k_knn_bbox_partial, dim3(nparts), dim3(CUGS_BLOCK), 0, st, n, pos, w.part);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_knn_bbox_final, dim3(1), dim3(CUGS_BLOCK), 0, st, nparts, w.part, w.bbox);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_knn_keys, dim3(nblk), dim3(CUGS_BLOCK), 0, st, n, pos, w.bbox, w.klo[0], w.khi[0]);
    CUGS_LAUNCH_CHECK();
    int cur = 0;
    for (int pass = 0; pass < 8; ++pass, cur ^= 1) {                            // low half first: least significant digit first
        const bool low = pass < 4;
        const uint32_t* kin = low ? w.klo[cur] : w.khi[cur];
        const uint32_t* v2in = low ? w.khi[cur] : w.klo[cur];
        uint32_t* kout = low ? w.klo[cur ^ 1] : w.khi[cur ^ 1];
        uint32_t* v2out = low ? w.khi[cur ^ 1] : w.klo[cur ^ 1];
        const int shift = 8 * (pass & 3);
        const int rc = pass == 0 ? knn_radix_pass<true>(kin, nullptr, v2in, kout, w.idx[cur ^ 1], v2out, n, shift, w.hist, w.tot, st)
                                 : knn_radix_pass<false>(kin, w.idx[cur], v2in, kout, w.idx[cur ^ 1], v2out, n, shift, w.hist, w.tot, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_knn_leaves, dim3(nblk), dim3(CUGS_BLOCK), 0, st, n, pos, w.idx[cur], w.spos, w.nodes);
    CUGS_LAUNCH_CHECK();
    const uint32_t nb = nblocks_for(n, KNN_BUCKET);
    const int top = knn_top_level(nb);
    uint32_t off = 0, cnt = nb;
    for (int l = 1; l <= top; ++l) {
        const uint32_t pcnt = (cnt + (1u << KNN_FAN_BITS) - 1u) >> KNN_FAN_BITS;
        hipLaunchKernelGGL(k_knn_level, dim3(nblocks_for(pcnt, CUGS_BLOCK)), dim3(CUGS_BLOCK), 0, st, cnt, w.nodes + 2 * (size_t)off,
                           pcnt, w.nodes + 2 * (size_t)(off + cnt));
        CUGS_LAUNCH_CHECK();
        off += cnt;
        cnt = pcnt;
    }
    return knn_tree_search(n, k, w, top, mean, st);
}

}  // namespace

extern "C" size_t cugs_knn_workspace_bytes(int64_t n, int k) {
    if (n < 0 || n > KNN_MAX_N || k < 1 || k > 16) return 0;
    return knn_carve(nullptr, n).bytes;
}

extern "C" int cugs_knn_mean_distances(int64_t n, int k, const float* positions, float* mean_dist, void* workspace,
                                       size_t workspace_bytes, int route, void* stream) {
    if (n < 0 || n > KNN_MAX_N || k < 1 || k > 16) return CUGS_EINVAL;
    if (route != CUGS_KNN_AUTO && route != CUGS_KNN_EXHAUSTIVE && route != CUGS_KNN_TREE) return CUGS_EINVAL;
    if (n == 0) return 0;
    if (!positions || !mean_dist) return CUGS_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 1) {                                                               // gaussian_init.cpp:29-33
        hipLaunchKernelGGL(k_knn_constant, dim3(1), dim3(CUGS_BLOCK), 0, st, 1u, mean_dist, 1.0f);
        CUGS_LAUNCH_CHECK();
        return 0;
    }
    if (k > n - 1) k = (int)(n - 1);                                            // :36
    if (route == CUGS_KNN_EXHAUSTIVE) return knn_exhaustive((uint32_t)n, k, positions, mean_dist, st);
    if (workspace_bytes < knn_carve(nullptr, n).bytes) return CUGS_EWORKSPACE;
    if (!workspace) return CUGS_EINVAL;
    if (route == CUGS_KNN_AUTO && n < KNN_AUTO_TREE_FROM) return knn_exhaustive((uint32_t)n, k, positions, mean_dist, st);
    return knn_tree((uint32_t)n, k, positions, mean_dist, knn_carve(workspace, n), st);
}

extern "C" int cugs_init_from_points(int64_t n, int num_coeffs, const float* positions, const uint8_t* colors,
                                     const float* mean_dist, float* out_positions, float* out_sh, float* out_opacities,
                                     float* out_rotations, float* out_scales, void* stream) {
    if (n < 0 || n > KNN_MAX_N) return CUGS_EINVAL;
    if (num_coeffs != 1 && num_coeffs != 4 && num_coeffs != 9 && num_coeffs != 16) return CUGS_EINVAL;
    if (n == 0) return 0;
    if (!positions || !colors || !mean_dist || !out_positions || !out_sh || !out_opacities || !out_rotations || !out_scales)
        return CUGS_EINVAL;
    const int64_t total = n * (num_coeffs == 1 ? 4 : 3 * num_coeffs);
    hipLaunchKernelGGL(k_init_from_points, dim3((unsigned)((total + CUGS_BLOCK - 1) / CUGS_BLOCK)), dim3(CUGS_BLOCK), 0,
                       static_cast<hipStream_t>(stream), n, num_coeffs, positions, colors, mean_dist, out_positions, out_sh,
                       out_opacities, out_rotations, out_scales);
    CUGS_LAUNCH_CHECK();
    return 0;
}
