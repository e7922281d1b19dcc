// vq.hip — vector quantisation of rows of up to 48 floats: nearest-code assignment on the matrix pipe and a
// deterministic Lloyd update in 64-bit fixed point (not in the reference).
//
// k_vq_prepare     once per assign call: h[j] = 0.5 |c_j|^2 as an ascending fmaf chain, and the codebook repacked for
//                  the assign kernel - rows of 48 floats, even t in floats 0..23, odd t in 24..47, zero beyond d, and
//                  rows k.. of the last chunk zero with h = +inf, so a padding code never wins a strict comparison.
// k_vq_assign<KS>  a workgroup owns 256 data rows, a wave 64 of them as two groups of 32.  The wave's rows are the
//                  B operand of v_mfma_f32_32x32x2_f32 and stay in 2 KS registers for the whole kernel; the codebook is
//                  the A operand and streams through LDS in chunks of 128 codes (four tiles of 32).  In the result tile
//                  a lane holds ONE data row (column lane & 31) and 16 codes (rows (reg & 3) + 8 (reg >> 2) +
//                  4 (lane >> 5)) in its accumulator registers, so the running (min, argmin) is lane-private and the
//                  only merge is the one between the two lane halves at the end.  Per the hardware the accumulator is
//                  the k-ordered chain acc = fmaf(a_k, b_k, acc), which is the contract of the header.
//                  Order: a lane meets its codes in ascending index (registers ascending in a tile, tiles and chunks
//                  ascending), compares with a strict <, and the half merge is lexicographic in (score, index); so the
//                  lowest index among equal scores wins everywhere.  No wave shares a row with another wave.
// k_vq_dist        optional, one lane per row: sum_t (x - c)^2 of the winner, every operation rounded on its own.
// k_vq_clear / k_vq_accumulate / k_vq_finalize   the update: int64 sums through 64-bit integer atomics - any order gives
//                  the same bits - then one division per codebook element.
// Every loop is bounded by n, k or d; nothing waits on another workgroup.
#include "cugs_common.h"

#include <math.h>

namespace {

typedef float vq_v16f __attribute__((ext_vector_type(16)));

constexpr int VQ_DP = 48;              // floats of a packed codebook row (d padded)
constexpr int VQ_HALF = VQ_DP / 2;     // k-steps of two at the most
constexpr int VQ_ROWS = 256;           // data rows of a workgroup: 4 waves x 2 groups x 32
constexpr int VQ_CHUNK = 128;          // codes staged in LDS at a time
constexpr int VQ_SX = VQ_DP + 1;       // LDS stride of a staged data row: odd, lanes on different rows hit different banks
constexpr int VQ_SC = VQ_DP + 4;       // LDS stride of a staged code: 13 x 16 bytes, 16 lanes' 16-byte reads cover all banks

struct VqLayout {
    size_t num, den, h, packed, total;   // byte offsets into the workspace
    int kp;                              // k rounded up to whole chunks
};

VqLayout vq_layout(int k, int d) {
    VqLayout L;
    L.kp = (k + VQ_CHUNK - 1) / VQ_CHUNK * VQ_CHUNK;
    L.num = 0;
    L.den = L.num + (size_t)k * d * sizeof(int64_t);
    L.packed = L.den + (size_t)k * sizeof(int64_t);
    L.h = L.packed + (size_t)L.kp * VQ_DP * sizeof(float);
    L.total = (L.h + (size_t)L.kp * sizeof(float) + 255) / 256 * 256;
    return L;
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_vq_prepare(int k, int kp, int d, const float* __restrict__ codebook,
                                                           float* __restrict__ packed, float* __restrict__ h) {
    const int e = (int)(blockIdx.x * CUGS_BLOCK + threadIdx.x);
    if (e >= kp * VQ_DP) return;
    const int code = e / VQ_DP, p = e - code * VQ_DP;
    const int t = 2 * (p % VQ_HALF) + p / VQ_HALF;
    packed[e] = (code < k && t < d) ? codebook[(int64_t)code * d + t] : 0.0f;
    if (p == 0) {
        float acc = 0.0f;
        if (code < k)
            for (int u = 0; u < d; ++u) {
                const float c = codebook[(int64_t)code * d + u];
                acc = __builtin_fmaf(c, c, acc);
            }
        h[code] = code < k ? 0.5f * acc : __builtin_inff();
    }
}

template <int KS>
__global__ __launch_bounds__(CUGS_BLOCK) void k_vq_assign(int64_t n, int d, int k, const float* __restrict__ x,
                                                          int64_t ldx, const float* __restrict__ packed,
                                                          const float* __restrict__ h, int32_t* __restrict__ assign) {
    static_assert(CUGS_BLOCK == 256, "k_vq_assign is laid out for four waves");
    __shared__ __attribute__((aligned(16))) float lds[VQ_ROWS * VQ_SX];       // data rows first, code chunks afterwards
    __shared__ __attribute__((aligned(16))) float hh[VQ_CHUNK];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hf = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * VQ_ROWS;

    // the workgroup's rows, one row per wave instruction (consecutive lanes on consecutive floats), zero beyond d and n
    if (lane < VQ_DP)
        for (int rr = wave; rr < VQ_ROWS; rr += 4) {
            const int64_t row = row0 + rr;
            lds[rr * VQ_SX + lane] = (row < n && lane < d) ? cugs_ldnt(x + row * ldx + lane) : 0.0f;
        }
    __syncthreads();
    float b0[KS], b1[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        b0[s] = lds[(wave * 64 + r) * VQ_SX + 2 * s + hf];
        b1[s] = lds[(wave * 64 + 32 + r) * VQ_SX + 2 * s + hf];
    }
    __syncthreads();

    float best0 = __builtin_inff(), best1 = __builtin_inff();
    int bi0 = 0, bi1 = 0;
    for (int c0 = 0; c0 < k; c0 += VQ_CHUNK) {
        const float2* src = reinterpret_cast<const float2*>(packed + (int64_t)c0 * VQ_DP);
        for (int v = tid; v < VQ_CHUNK * VQ_HALF; v += CUGS_BLOCK) {
            const int code = v / VQ_HALF, q = v - code * VQ_HALF;
            *reinterpret_cast<float2*>(lds + code * VQ_SC + 2 * q) = src[v];
        }
        if (tid < VQ_CHUNK) hh[tid] = h[c0 + tid];
        __syncthreads();
        for (int tile = 0; tile < VQ_CHUNK / 32 && c0 + tile * 32 < k; ++tile) {
            const float4* ar = reinterpret_cast<const float4*>(lds + (tile * 32 + r) * VQ_SC + hf * VQ_HALF);
            float a[(KS + 3) / 4 * 4];
#pragma unroll
            for (int q = 0; q < (KS + 3) / 4; ++q) {
                const float4 t = ar[q];
                a[4 * q] = t.x; a[4 * q + 1] = t.y; a[4 * q + 2] = t.z; a[4 * q + 3] = t.w;
            }
            vq_v16f acc0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            vq_v16f acc1 = acc0;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b0[s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b1[s], acc1, 0, 0, 0);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 h4 = *reinterpret_cast<const float4*>(hh + tile * 32 + 8 * g + 4 * hf);
                const float hv[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int code = c0 + tile * 32 + 8 * g + 4 * hf + j;
                    const float s0 = hv[j] - acc0[4 * g + j];
                    const float s1 = hv[j] - acc1[4 * g + j];
                    if (s0 < best0) { best0 = s0; bi0 = code; }
                    if (s1 < best1) { best1 = s1; bi1 = code; }
                }
            }
        }
        __syncthreads();
    }
    // the two lane halves hold the same rows and disjoint codes: (score, index) pairs merge lexicographically
    const float o0 = __shfl_xor(best0, 32), o1 = __shfl_xor(best1, 32);
    const int oi0 = __shfl_xor(bi0, 32), oi1 = __shfl_xor(bi1, 32);
    if (o0 < best0 || (o0 == best0 && oi0 < bi0)) bi0 = oi0;
    if (o1 < best1 || (o1 == best1 && oi1 < bi1)) bi1 = oi1;
    const int64_t row = row0 + wave * 64 + hf * 32 + r;
    if (row < n) assign[row] = hf ? bi1 : bi0;
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_vq_dist(int64_t n, int d, int k, const float* __restrict__ x, int64_t ldx,
                                                        const float* __restrict__ codebook,
                                                        const int32_t* __restrict__ assign, float* __restrict__ dist) {
    const int64_t row = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (row >= n) return;
    const int a = assign[row];
    if ((unsigned)a >= (unsigned)k) return;
    const float* xr = x + row * ldx;
    const float* cr = codebook + (int64_t)a * d;
    float acc = 0.0f;
    for (int t = 0; t < d; ++t) {
        const float df = xr[t] - cr[t];
        acc = acc + df * df;
    }
    dist[row] = acc;
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_vq_clear(int64_t words, unsigned long long* __restrict__ sums, int k,
                                                         int32_t* __restrict__ counts) {
    const int64_t e = (int64_t)blockIdx.x * CUGS_BLOCK + threadIdx.x;
    if (e < words) sums[e] = 0ull;
    if (counts && e < k) counts[e] = 0;
}

// One wave per row and turn: lanes 0..d-1 add the row's scaled elements, lane d its scaled weight, lane d+1 counts it.
__global__ __launch_bounds__(CUGS_BLOCK) void k_vq_accumulate(int64_t n, int d, int k, const float* __restrict__ x,
                                                              int64_t ldx, const float* __restrict__ weights,
                                                              const int32_t* __restrict__ assign, double scale,
                                                              unsigned long long* __restrict__ num,
                                                              unsigned long long* __restrict__ den,
                                                              int32_t* __restrict__ counts) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * (CUGS_BLOCK / 64);
    for (int64_t row = (int64_t)blockIdx.x * (CUGS_BLOCK / 64) + (threadIdx.x >> 6); row < n; row += stride) {
        const int a = assign[row];
        if ((unsigned)a >= (unsigned)k) continue;                 // -1: the row is left out
        const double w = weights ? (double)weights[row] : 1.0;
        if (lane < d) {
            const long long v = __double2ll_rn(w * (double)x[row * ldx + lane] * scale);
            if (v != 0) atomicAdd(num + (int64_t)a * d + lane, (unsigned long long)v);
        } else if (lane == d) {
            const long long v = __double2ll_rn(w * scale);
            if (v != 0) atomicAdd(den + a, (unsigned long long)v);
        } else if (lane == d + 1 && counts) {
            atomicAdd(counts + a, 1);
        }
    }
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_vq_finalize(int k, int d, const long long* __restrict__ num,
                                                            const long long* __restrict__ den,
                                                            float* __restrict__ codebook) {
    const int e = (int)(blockIdx.x * CUGS_BLOCK + threadIdx.x);
    if (e >= k * d) return;
    const long long dn = den[e / d];
    if (dn > 0) codebook[e] = (float)((double)num[e] / (double)dn);
}

bool vq_aligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

bool vq_sizes_ok(int64_t n, int d, int k, int64_t ldx) {
    return n >= 0 && n <= 2147483647ll && d >= 1 && d <= VQ_DP && k >= 1 && k <= 65536 && ldx >= d;
}

}  // namespace

extern "C" size_t cugs_vq_workspace_bytes(int k, int d) {
    if (d < 1 || d > VQ_DP || k < 1 || k > 65536) return 0;
    return vq_layout(k, d).total;
}

extern "C" int cugs_vq_assign(int64_t n, int d, int k, const float* x, int64_t ldx, const float* codebook,
                              int32_t* assign, float* dist, void* workspace, size_t workspace_bytes, void* stream) {
    if (!vq_sizes_ok(n, d, k, ldx)) return CUGS_EINVAL;
    if (n > 0 && (!x || !codebook || !assign || !workspace)) return CUGS_EINVAL;
    const VqLayout L = vq_layout(k, d);
    if (workspace_bytes < L.total) return CUGS_EWORKSPACE;
    if (!vq_aligned(x, 3) || !vq_aligned(codebook, 3) || !vq_aligned(assign, 3) || !vq_aligned(dist, 3) ||
        !vq_aligned(workspace, 7))
        return CUGS_EALIGN;
    if (n == 0) return 0;

    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    float* packed = reinterpret_cast<float*>(ws + L.packed);
    float* h = reinterpret_cast<float*>(ws + L.h);
    const dim3 block(CUGS_BLOCK);
    hipLaunchKernelGGL(k_vq_prepare, dim3((unsigned)((L.kp * VQ_DP + CUGS_BLOCK - 1) / CUGS_BLOCK)), block, 0, st, k, L.kp,
                       d, codebook, packed, h);
    CUGS_LAUNCH_CHECK();
    const dim3 grid((unsigned)((n + VQ_ROWS - 1) / VQ_ROWS));
    const int steps = (d + 1) / 2;                                // the SH widths 9, 24 and 45 get their own trip count
    if (steps <= 5) hipLaunchKernelGGL(k_vq_assign<5>, grid, block, 0, st, n, d, k, x, ldx, packed, h, assign);
    else if (steps <= 12) hipLaunchKernelGGL(k_vq_assign<12>, grid, block, 0, st, n, d, k, x, ldx, packed, h, assign);
    else if (steps <= 23) hipLaunchKernelGGL(k_vq_assign<23>, grid, block, 0, st, n, d, k, x, ldx, packed, h, assign);
    else hipLaunchKernelGGL(k_vq_assign<24>, grid, block, 0, st, n, d, k, x, ldx, packed, h, assign);
    CUGS_LAUNCH_CHECK();
    if (dist) {
        hipLaunchKernelGGL(k_vq_dist, dim3((unsigned)((n + CUGS_BLOCK - 1) / CUGS_BLOCK)), block, 0, st, n, d, k, x, ldx,
                           codebook, assign, dist);
        CUGS_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int cugs_vq_update(int64_t n, int d, int k, const float* x, int64_t ldx, const float* weights,
                              const int32_t* assign, int frac_bits, float* codebook, int32_t* counts, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!vq_sizes_ok(n, d, k, ldx) || frac_bits < 0 || frac_bits > 62) return CUGS_EINVAL;
    if (n > 0 && (!x || !assign || !codebook || !workspace)) return CUGS_EINVAL;
    const VqLayout L = vq_layout(k, d);
    if (workspace_bytes < L.total) return CUGS_EWORKSPACE;
    if (!vq_aligned(x, 3) || !vq_aligned(weights, 3) || !vq_aligned(assign, 3) || !vq_aligned(codebook, 3) ||
        !vq_aligned(counts, 3) || !vq_aligned(workspace, 7))
        return CUGS_EALIGN;
    if (n == 0) return 0;

    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    unsigned long long* num = reinterpret_cast<unsigned long long*>(ws + L.num);
    unsigned long long* den = reinterpret_cast<unsigned long long*>(ws + L.den);
    const dim3 block(CUGS_BLOCK);
    const int64_t words = (int64_t)k * d + k;                     // num and den are adjacent
    hipLaunchKernelGGL(k_vq_clear, dim3((unsigned)((words + CUGS_BLOCK - 1) / CUGS_BLOCK)), block, 0, st, words, num, k,
                       counts);
    CUGS_LAUNCH_CHECK();
    const int64_t want = (n + CUGS_BLOCK / 64 - 1) / (CUGS_BLOCK / 64);
    hipLaunchKernelGGL(k_vq_accumulate, dim3((unsigned)(want < 8192 ? want : 8192)), block, 0, st, n, d, k, x, ldx, weights,
                       assign, ldexp(1.0, frac_bits), num, den, counts);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vq_finalize, dim3((unsigned)((k * d + CUGS_BLOCK - 1) / CUGS_BLOCK)), block, 0, st, k, d,
                       reinterpret_cast<const long long*>(num), reinterpret_cast<const long long*>(den), codebook);
    CUGS_LAUNCH_CHECK();
    return 0;
}
