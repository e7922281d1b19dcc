// cugs_mcmc.h — the per-Gaussian arithmetic of MCMC densification, shared by mcmc.hip (the
// stand-alone kernels) and project_backward.hip (the fused route, k_project_backward_mcmc), so that the two routes
// give identical bits.  Reference: optimizer/mcmc_densification.cpp.
#pragma once

#include "cugs_common.h"

// ---- counter-based generator: Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) ----------------------
// key = (seed_lo, seed_hi), counter = (index_lo, index_hi, stream_id, step): every draw is a pure function of where it
// is used, so the route (fused or not), the launch geometry and the replica (data-parallel) do not change it.
#define CUGS_MCMC_PHILOX_M0 0xD2511F53u
#define CUGS_MCMC_PHILOX_M1 0xCD9E8D57u
#define CUGS_MCMC_PHILOX_W0 0x9E3779B9u
#define CUGS_MCMC_PHILOX_W1 0xBB67AE85u

__device__ __forceinline__ uint4 cugs_philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(CUGS_MCMC_PHILOX_M0, c.x), lo0 = CUGS_MCMC_PHILOX_M0 * c.x;
        const uint32_t hi1 = __umulhi(CUGS_MCMC_PHILOX_M1, c.z), lo1 = CUGS_MCMC_PHILOX_M1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += CUGS_MCMC_PHILOX_W0;
        k1 += CUGS_MCMC_PHILOX_W1;
    }
    return c;
}

__device__ __forceinline__ uint4 cugs_mcmc_bits(uint64_t seed, uint32_t stream_id, uint32_t step, uint64_t index) {
    return cugs_philox4x32_10(make_uint4((uint32_t)index, (uint32_t)(index >> 32), stream_id, step), (uint32_t)seed,
                              (uint32_t)(seed >> 32));
}

// a word -> uniform in (0, 1]: ((x >> 8) + 1) * 2^-24, exact
__device__ __forceinline__ float cugs_mcmc_uniform(uint32_t x) { return (float)((x >> 8) + 1u) * 0x1.0p-24f; }

// Three standard normals from one Philox call: Box-Muller on the word pairs (0, 1) and (2, 3), the first three used.
__device__ __forceinline__ void cugs_mcmc_normals3(uint64_t seed, uint32_t stream_id, uint32_t step, uint64_t index,
                                                   float out[3]) {
    const uint4 x = cugs_mcmc_bits(seed, stream_id, step, index);
    const float r0 = sqrtf(-2.0f * logf(cugs_mcmc_uniform(x.x)));
    const float r1 = sqrtf(-2.0f * logf(cugs_mcmc_uniform(x.z)));
    float s0, c0;
    sincospif(2.0f * cugs_mcmc_uniform(x.y), &s0, &c0);
    out[0] = r0 * c0;
    out[1] = r0 * s0;
    out[2] = r1 * cospif(2.0f * cugs_mcmc_uniform(x.w));
}

// ---- regulariser gradients (mcmc_densification.cpp:167-186: torch's mul, mean, sigmoid_backward and exp_backward in
// torch's order, float32).  coef_o = lambda_o / (float)N, coef_s = lambda_s / (float)(3N), formed once on the host.
__device__ __forceinline__ float cugs_mcmc_reg_opacity(float coef_o, float opa_logit) {
    const float y = cugs_sigmoidf(opa_logit);
    return (coef_o * (1.0f - y)) * y;
}
__device__ __forceinline__ float cugs_mcmc_reg_scale(float coef_s, float log_scale) {
    return coef_s * cugs_expf(log_scale);
}

// ---- position noise (mcmc_densification.cpp:144-161): pos += ((lr * exp(s)) * gate) * n,
// gate = sigmoid(-k * (sigmoid(opa) - t)), on the CURRENT (post-step) opacity and scales.
__device__ __forceinline__ float cugs_mcmc_gate(float opa_logit, float gate_k, float gate_t) {
    return cugs_sigmoidf(-gate_k * (cugs_sigmoidf(opa_logit) - gate_t));
}
__device__ __forceinline__ float cugs_mcmc_noisy(float pos, float log_scale, float gate, float lr, float n) {
    return pos + ((lr * cugs_expf(log_scale)) * gate) * n;
}

// The fused route's arguments (cugs_mcmc_fused with the regulariser's two coefficients formed).
struct McmcFusedArgs {
    float coef_o, coef_s, noise_lr, gate_k, gate_t;
    uint32_t step;
    uint64_t seed;
    const float* noise;      // [n, 3] explicit normals, or NULL: the generator's stream CUGS_MCMC_STREAM_NOISE
};
