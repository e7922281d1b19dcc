// mcmc.hip — MCMC densification on the device (Kheradmand et al., NeurIPS 2024).
//
// Replaces optimizer/mcmc_densification.cpp, which runs on libtorch ops:
//   compute_regularization (:167-186): two clones, an autograd pass over ~10 ops and a host sync (.item()) per
//     iteration -> k_reg_partials + k_reg_final: one pass over opacity and scales, the value stays on the device;
//   inject_noise (:144-161): ~8 elementwise ops over N x 3 and a randn_like per iteration -> k_inject_noise;
//   relocate (:56-138): sum().item(), two nonzero(), a multinomial and five index_put_ every ~100 iterations ->
//     count / scan / build / apply, four launches and no read-back (grids are sized by the host-known N).
// The per-element arithmetic is in cugs_mcmc.h, shared with the fused route of project_backward.hip.
#include "cugs_mcmc.h"

namespace {

constexpr int ITEMS = 4;                                  // Gaussians per thread in the count / build kernels
constexpr int SCAN_CHUNK = CUGS_BLOCK * ITEMS;            // 1024 per workgroup
constexpr int REG_GRID = 1024;                            // fixed grid of the regulariser: a fixed summation order
constexpr size_t REG_BYTES = sizeof(double) * 2 * REG_GRID;  // its partials: all the workspace it needs, whatever n
constexpr float LOG_TEN = 0x1.26bb1cp+1f;                 // std::log(10.0f) (:121)
constexpr float LOW_OPACITY = -0x1.261672p+2f;            // std::log(0.01f / 0.99f) (:125)
constexpr float WEIGHT_ONE = 16777216.0f;                 // 2^24: sampling weights are exact integers

struct RelocWs {
    double* reg_partials;            // [2 * REG_GRID] the regulariser's per-workgroup sums (at offset 0)
    unsigned long long* totals;      // [4] num_dead, total weight, M, reserved
    uint32_t* blk_dead;              // [nb] exclusive-scanned in place
    unsigned long long* blk_w;       // [nb] exclusive-scanned in place
    unsigned long long* cdf;         // [n] inclusive scan of the weights
    int32_t* dead_list;              // [n] dead rows in index order
    int32_t* src_list;               // [n] source of the j-th relocated row
    size_t bytes;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline uint32_t nblocks(int64_t n) { return (uint32_t)((n + SCAN_CHUNK - 1) / SCAN_CHUNK); }
inline int grid_for(int64_t n) { return (int)((n + CUGS_BLOCK - 1) / CUGS_BLOCK); }

RelocWs carve(void* base, int64_t n) {
    char* p = static_cast<char*>(base);
    size_t off = 0;
    RelocWs w;
    const size_t nb = (size_t)nblocks(n) + 1;
    w.reg_partials = reinterpret_cast<double*>(p + off); off = align_up(off + REG_BYTES, 256);     // first: the regulariser
    w.totals = reinterpret_cast<unsigned long long*>(p + off); off = align_up(off + 4 * sizeof(unsigned long long), 256);
    w.blk_dead = reinterpret_cast<uint32_t*>(p + off); off = align_up(off + sizeof(uint32_t) * nb, 256);
    w.blk_w = reinterpret_cast<unsigned long long*>(p + off); off = align_up(off + sizeof(unsigned long long) * nb, 256);
    w.cdf = reinterpret_cast<unsigned long long*>(p + off); off = align_up(off + sizeof(unsigned long long) * (size_t)n, 256);
    w.dead_list = reinterpret_cast<int32_t*>(p + off); off = align_up(off + sizeof(int32_t) * (size_t)n, 256);
    w.src_list = reinterpret_cast<int32_t*>(p + off); off = align_up(off + sizeof(int32_t) * (size_t)n, 256);
    w.bytes = off;
    return w;
}

// ---- generator ----
__global__ __launch_bounds__(CUGS_BLOCK) void k_random_bits(uint64_t seed, uint32_t stream_id, uint32_t step,
                                                            uint64_t first, int64_t count, uint4* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (j >= count) return;
    out[j] = cugs_mcmc_bits(seed, stream_id, step, first + (uint64_t)j);
}

// ---- regulariser ----
__device__ __forceinline__ double block_sum(double v, double* s_tmp) {
    s_tmp[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = CUGS_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_tmp[threadIdx.x] += s_tmp[threadIdx.x + s];
        __syncthreads();
    }
    const double r = s_tmp[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_reg_partials(int64_t n, const float* __restrict__ opa,
                                                             const float* __restrict__ scl, float coef_o, float coef_s,
                                                             // base == out is the documented in-place add: no
                                                             // __restrict__ on these four
                                                             const float* base_o, const float* base_s, float* out_o,
                                                             float* out_s, double* __restrict__ partials) {
    __shared__ double s_tmp[CUGS_BLOCK];
    double sy = 0.0, se = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CUGS_BLOCK) {
        const float o = opa[i];
        sy += (double)cugs_sigmoidf(o);
        if (out_o) {
            const float r = cugs_mcmc_reg_opacity(coef_o, o);
            out_o[i] = base_o ? base_o[i] + r : r;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float s = scl[i * 3 + k];
            se += (double)cugs_expf(s);
            if (out_s) {
                const float r = cugs_mcmc_reg_scale(coef_s, s);
                out_s[i * 3 + k] = base_s ? base_s[i * 3 + k] + r : r;
            }
        }
    }
    sy = block_sum(sy, s_tmp);
    se = block_sum(se, s_tmp);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = sy; partials[2 * blockIdx.x + 1] = se; }
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_reg_final(int64_t n, int nparts, const double* __restrict__ partials,
                                                          float lambda_o, float lambda_s, float* __restrict__ value) {
    __shared__ double s_tmp[CUGS_BLOCK];
    double sy = 0.0, se = 0.0;
    for (int b = threadIdx.x; b < nparts; b += CUGS_BLOCK) { sy += partials[2 * b]; se += partials[2 * b + 1]; }
    sy = block_sum(sy, s_tmp);
    se = block_sum(se, s_tmp);
    if (threadIdx.x == 0)
        *value = (float)((double)lambda_o * (sy / (double)n) + (double)lambda_s * (se / (3.0 * (double)n)));
}

// ---- noise ----
__global__ __launch_bounds__(CUGS_BLOCK) void k_inject_noise(int64_t n, float* __restrict__ pos,
                                                             const float* __restrict__ scl, const float* __restrict__ opa,
                                                             float lr, float gate_k, float gate_t,
                                                             const float* __restrict__ noise, uint64_t seed,
                                                             uint32_t step) {
    const int64_t i = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (i >= n) return;
    float z[3];
    if (noise) { z[0] = noise[i * 3 + 0]; z[1] = noise[i * 3 + 1]; z[2] = noise[i * 3 + 2]; }
    else cugs_mcmc_normals3(seed, CUGS_MCMC_STREAM_NOISE, step, (uint64_t)i, z);
    const float gate = cugs_mcmc_gate(opa[i], gate_k, gate_t);
#pragma unroll
    for (int k = 0; k < 3; ++k) pos[i * 3 + k] = cugs_mcmc_noisy(pos[i * 3 + k], scl[i * 3 + k], gate, lr, z[k]);
}

// ---- relocation ----
// dead flag and sampling weight of row i (weight 0 for dead rows and past the end)
__device__ __forceinline__ void classify(int64_t i, int64_t n, const float* opa, float thr, uint32_t& dead,
                                         unsigned long long& w) {
    dead = 0u; w = 0ull;
    if (i >= n) return;
    const float y = cugs_sigmoidf(opa[i]);
    if (y < thr) dead = 1u;                                                    // :74-75
    else w = (unsigned long long)rintf(y * WEIGHT_ONE);
}

__device__ __forceinline__ uint32_t wave_incl(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_incl(unsigned long long v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive scan over the 256-thread workgroup of a (dead count, weight) pair; totals optional
__device__ __forceinline__ void block_excl2(uint32_t a, unsigned long long b, uint32_t* s_a, unsigned long long* s_b,
                                            uint32_t& ea, unsigned long long& eb, uint32_t* ta, unsigned long long* tb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ia = wave_incl(a);
    const unsigned long long ib = wave_incl(b);
    if (lane == 63) { s_a[wave] = ia; s_b[wave] = ib; }
    __syncthreads();
    uint32_t ba = 0, sa = 0;
    unsigned long long bb = 0, sb = 0;
#pragma unroll
    for (int w = 0; w < CUGS_BLOCK / 64; ++w) {
        if (w < wave) { ba += s_a[w]; bb += s_b[w]; }
        sa += s_a[w]; sb += s_b[w];
    }
    ea = ba + ia - a;
    eb = bb + ib - b;
    if (ta) *ta = sa;
    if (tb) *tb = sb;
    __syncthreads();
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_reloc_count(int64_t n, const float* __restrict__ opa, float thr,
                                                            uint32_t* __restrict__ blk_dead,
                                                            unsigned long long* __restrict__ blk_w) {
    __shared__ uint32_t s_a[CUGS_BLOCK / 64];
    __shared__ unsigned long long s_b[CUGS_BLOCK / 64];
    uint32_t d = 0;
    unsigned long long w = 0;
    const int64_t i0 = (int64_t)blockIdx.x * SCAN_CHUNK + threadIdx.x * ITEMS;
#pragma unroll
    for (int e = 0; e < ITEMS; ++e) {
        uint32_t de;
        unsigned long long we;
        classify(i0 + e, n, opa, thr, de, we);
        d += de; w += we;
    }
    uint32_t ea, ta;
    unsigned long long eb, tb;
    block_excl2(d, w, s_a, s_b, ea, eb, &ta, &tb);
    if (threadIdx.x == 0) { blk_dead[blockIdx.x] = ta; blk_w[blockIdx.x] = tb; }
}

// One workgroup: exclusive scan of the block sums; totals = {num_dead, total weight, M}; stats = {num_dead, M}.
__global__ __launch_bounds__(CUGS_BLOCK) void k_reloc_scan(int64_t n, uint32_t nb, uint32_t* __restrict__ blk_dead,
                                                           unsigned long long* __restrict__ blk_w, int64_t cap_rows,
                                                           unsigned long long* __restrict__ totals,
                                                           int32_t* __restrict__ stats) {
    __shared__ uint32_t s_a[CUGS_BLOCK / 64];
    __shared__ unsigned long long s_b[CUGS_BLOCK / 64];
    unsigned long long ca = 0, cb = 0;
    for (uint32_t base = 0; base < nb; base += CUGS_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t a = i < nb ? blk_dead[i] : 0u;
        const unsigned long long b = i < nb ? blk_w[i] : 0ull;
        uint32_t ea, ta;
        unsigned long long eb, tb;
        block_excl2(a, b, s_a, s_b, ea, eb, &ta, &tb);
        if (i < nb) { blk_dead[i] = (uint32_t)ca + ea; blk_w[i] = cb + eb; }
        ca += ta; cb += tb;
    }
    if (threadIdx.x == 0) {
        const int64_t dead = (int64_t)ca, alive = n - dead;
        // :88-90 (num_dead == 0 || num_alive == 0); a zero total weight (alive rows that all round to 0) likewise
        const int64_t m = (dead == 0 || alive == 0 || cb == 0ull) ? 0 : (dead < cap_rows ? dead : cap_rows);
        totals[0] = ca; totals[1] = cb; totals[2] = (unsigned long long)m;
        if (stats) { stats[0] = (int32_t)dead; stats[1] = (int32_t)m; }
    }
}

// cdf (inclusive) and the list of dead rows in index order
__global__ __launch_bounds__(CUGS_BLOCK) void k_reloc_build(int64_t n, const float* __restrict__ opa, float thr,
                                                            const uint32_t* __restrict__ blk_dead,
                                                            const unsigned long long* __restrict__ blk_w,
                                                            unsigned long long* __restrict__ cdf,
                                                            int32_t* __restrict__ dead_list) {
    __shared__ uint32_t s_a[CUGS_BLOCK / 64];
    __shared__ unsigned long long s_b[CUGS_BLOCK / 64];
    uint32_t de[ITEMS], d = 0;
    unsigned long long we[ITEMS], w = 0;
    const int64_t i0 = (int64_t)blockIdx.x * SCAN_CHUNK + threadIdx.x * ITEMS;
#pragma unroll
    for (int e = 0; e < ITEMS; ++e) {
        classify(i0 + e, n, opa, thr, de[e], we[e]);
        d += de[e]; w += we[e];
    }
    uint32_t ea;
    unsigned long long eb;
    block_excl2(d, w, s_a, s_b, ea, eb, nullptr, nullptr);
    uint32_t rd = blk_dead[blockIdx.x] + ea;
    unsigned long long c = blk_w[blockIdx.x] + eb;
#pragma unroll
    for (int e = 0; e < ITEMS; ++e) {
        if (i0 + e >= n) break;
        c += we[e];
        cdf[i0 + e] = c;
        if (de[e]) dead_list[rd++] = (int32_t)(i0 + e);
    }
}

// One relocated row per thread: draw the source, write the geometry rows (:104-126).
__global__ __launch_bounds__(CUGS_BLOCK) void k_reloc_apply(int64_t n, int64_t cap_rows,
                                                            const unsigned long long* __restrict__ totals,
                                                            const unsigned long long* __restrict__ cdf,
                                                            const int32_t* __restrict__ dead_list,
                                                            int32_t* __restrict__ src_list, int32_t* __restrict__ src_out,
                                                            float* __restrict__ pos, float* __restrict__ rot,
                                                            float* __restrict__ scl, float* __restrict__ opa,
                                                            float extent, uint64_t seed, uint32_t step) {
    const int64_t j = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (j >= cap_rows || j >= (int64_t)totals[2]) return;
    const unsigned long long total = totals[1];
    const uint4 r = cugs_mcmc_bits(seed, CUGS_MCMC_STREAM_SAMPLE, step, (uint64_t)j);
    const unsigned long long x = __umul64hi(((unsigned long long)r.y << 32) | r.x, total);     // [0, total)
    int64_t lo = 0, hi = n - 1;                                  // the first i with cdf[i] > x (cdf[n - 1] == total)
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > x) hi = mid; else lo = mid + 1;
    }
    const int64_t src = lo, dst = dead_list[j];
    src_list[j] = (int32_t)src;
    if (src_out) src_out[j] = (int32_t)src;
    float z[3];
    cugs_mcmc_normals3(seed, CUGS_MCMC_STREAM_JITTER, step, (uint64_t)dst, z);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        pos[dst * 3 + k] = pos[src * 3 + k] + (z[k] * extent) * 0.01f;      // :113-115
        scl[dst * 3 + k] = scl[src * 3 + k] - LOG_TEN;                       // :118-121
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) rot[dst * 4 + k] = rot[src * 4 + k];        // :108-109
    opa[dst] = LOW_OPACITY;                                                  // :124-127
}

// Whole rows of one array for the relocated rows: copied from the source (SH coefficients) or zeroed (moments).
__global__ __launch_bounds__(CUGS_BLOCK) void k_reloc_rows(int64_t cap_rows, int row_floats,
                                                           const unsigned long long* __restrict__ totals,
                                                           const int32_t* __restrict__ dead_list,
                                                           const int32_t* __restrict__ src_list, float* __restrict__ a,
                                                           int zero) {
    const int64_t e = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (e >= cap_rows * row_floats) return;
    const int64_t j = e / row_floats;
    const int col = (int)(e - j * row_floats);
    if (j >= (int64_t)totals[2]) return;
    const int64_t dst = dead_list[j];
    a[dst * row_floats + col] = zero ? 0.0f : a[(int64_t)src_list[j] * row_floats + col];
}

}  // namespace

extern "C" int cugs_mcmc_random_bits(uint64_t seed, uint32_t stream_id, uint32_t step, uint64_t first_index,
                                     int64_t count, uint32_t* out, void* stream) {
    if (count < 0) return CUGS_EINVAL;
    if (count == 0) return 0;
    if (!out) return CUGS_EINVAL;
    if (!cugs_aligned16(out)) return CUGS_EALIGN;
    hipLaunchKernelGGL(k_random_bits, dim3(grid_for(count)), dim3(CUGS_BLOCK), 0, static_cast<hipStream_t>(stream),
                       seed, stream_id, step, first_index, count, reinterpret_cast<uint4*>(out));
    CUGS_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t cugs_mcmc_relocate_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    return carve(nullptr, n).bytes;
}

extern "C" int cugs_mcmc_regularization(int64_t n, const float* opacities, const float* scales, float lambda_opacity,
                                        float lambda_scale, const float* base_dL_dopacities,
                                        const float* base_dL_dscales, float* dL_dopacities, float* dL_dscales,
                                        float* value_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0) return CUGS_EINVAL;
    if (n == 0) return 0;
    if (!opacities || !scales || !workspace) return CUGS_EINVAL;
    if ((base_dL_dopacities && !dL_dopacities) || (base_dL_dscales && !dL_dscales)) return CUGS_EINVAL;
    if (n > 2147483647ll / 3) return CUGS_EOVERFLOW;
    if (workspace_bytes < REG_BYTES) return CUGS_EWORKSPACE;
    RelocWs ws = carve(workspace, 0);                               // only reg_partials (offset 0) is used
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float coef_o = lambda_opacity / (float)n, coef_s = lambda_scale / (float)(3 * n);   // mean's 1 / numel
    const int grid = grid_for(n) < REG_GRID ? grid_for(n) : REG_GRID;
    hipLaunchKernelGGL(k_reg_partials, dim3(grid), dim3(CUGS_BLOCK), 0, st, n, opacities, scales, coef_o, coef_s,
                       base_dL_dopacities, base_dL_dscales, dL_dopacities, dL_dscales, ws.reg_partials);
    CUGS_LAUNCH_CHECK();
    if (value_out) {
        hipLaunchKernelGGL(k_reg_final, dim3(1), dim3(CUGS_BLOCK), 0, st, n, grid, ws.reg_partials, lambda_opacity,
                           lambda_scale, value_out);
        CUGS_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int cugs_mcmc_inject_noise(int64_t n, float* positions, const float* scales, const float* opacities,
                                      float noise_lr, float gate_k, float gate_t, const float* noise, uint64_t seed,
                                      uint32_t step, void* stream) {
    if (n < 0) return CUGS_EINVAL;
    if (n == 0) return 0;
    if (!positions || !scales || !opacities) return CUGS_EINVAL;
    hipLaunchKernelGGL(k_inject_noise, dim3(grid_for(n)), dim3(CUGS_BLOCK), 0, static_cast<hipStream_t>(stream), n,
                       positions, scales, opacities, noise_lr, gate_k, gate_t, noise, seed, step);
    CUGS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cugs_mcmc_relocate(int64_t n, int num_coeffs, float* positions, float* rotations, float* scales,
                                  float* opacities, float* sh_coeffs, float dead_threshold, float relocate_cap,
                                  float scene_extent, uint64_t seed, uint32_t step, float* const m[5],
                                  float* const v[5], void* workspace, size_t workspace_bytes, int32_t* stats,
                                  int32_t* src_out, void* stream) {
    if (n < 0 || num_coeffs < 1 || num_coeffs > 16) return CUGS_EINVAL;
    if ((m == nullptr) != (v == nullptr)) return CUGS_EINVAL;
    if (n == 0) return 0;
    if (!positions || !rotations || !scales || !opacities || !sh_coeffs || !workspace || !stats) return CUGS_EINVAL;
    if (n > 2147483647ll / 48) return CUGS_EOVERFLOW;               // int32 row indices, SH rows addressed in int64
    if (m)
        for (int g = 0; g < 5; ++g)
            if (!m[g] || !v[g]) return CUGS_EINVAL;
    RelocWs ws = carve(workspace, n);
    if (workspace_bytes < ws.bytes) return CUGS_EWORKSPACE;
    // the reference's (int)(relocate_cap * n) in float (:93), clamped to [0, n]
    const float capf = relocate_cap * (float)n;
    const int64_t cap_rows = !(capf > 0.0f) ? 0 : (capf >= (float)n ? n : (int64_t)capf);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t nb = nblocks(n);
    hipLaunchKernelGGL(k_reloc_count, dim3(nb), dim3(CUGS_BLOCK), 0, st, n, opacities, dead_threshold, ws.blk_dead,
                       ws.blk_w);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_reloc_scan, dim3(1), dim3(CUGS_BLOCK), 0, st, n, nb, ws.blk_dead, ws.blk_w, cap_rows, ws.totals,
                       stats);
    CUGS_LAUNCH_CHECK();
    if (cap_rows == 0) return 0;
    hipLaunchKernelGGL(k_reloc_build, dim3(nb), dim3(CUGS_BLOCK), 0, st, n, opacities, dead_threshold, ws.blk_dead,
                       ws.blk_w, ws.cdf, ws.dead_list);
    CUGS_LAUNCH_CHECK();
    // k_reloc_apply writes src_list, which the row copies read; sources are alive rows, never relocated ones
    hipLaunchKernelGGL(k_reloc_apply, dim3(grid_for(cap_rows)), dim3(CUGS_BLOCK), 0, st, n, cap_rows, ws.totals, ws.cdf,
                       ws.dead_list, ws.src_list, src_out, positions, rotations, scales, opacities, scene_extent, seed,
                       step);
    CUGS_LAUNCH_CHECK();
    const int sh_floats = 3 * num_coeffs;
    hipLaunchKernelGGL(k_reloc_rows, dim3(grid_for(cap_rows * sh_floats)), dim3(CUGS_BLOCK), 0, st, cap_rows, sh_floats,
                       ws.totals, ws.dead_list, ws.src_list, sh_coeffs, 0);
    CUGS_LAUNCH_CHECK();
    if (m) {
        const int rows[5] = {3, sh_floats, 1, 3, 4};                 // ParamGroup order
        for (int g = 0; g < 5; ++g)
            for (int s = 0; s < 2; ++s) {
                hipLaunchKernelGGL(k_reloc_rows, dim3(grid_for(cap_rows * rows[g])), dim3(CUGS_BLOCK), 0, st, cap_rows,
                                   rows[g], ws.totals, ws.dead_list, ws.src_list, s ? v[g] : m[g], 1);
                CUGS_LAUNCH_CHECK();
            }
    }
    return 0;
}
