// transform.hip — a similarity x' = s R x + t applied to a Gaussian model in place (not in the reference).
//
// Host half: cugs_similarity_init derives, in fp64 from the nearest rotation to the given matrix, everything the kernel
// multiplies by - M = s R, t, log s, the quaternion of R and the per-band SH rotation matrices D_1..D_3 in the basis of
// sh_basis (cugs_gaussian_math.h) - and rounds each value to fp32 once.
// Device half: k_transform_gaussians<C>, one launch.  The work of a launch is cut into chunks of CUGS_BLOCK items that
// the workgroups take in turn; the items are, in this order,
//   3n    one (row, channel) of the SH tensor: the C coefficients are read into registers, bands 1.. are multiplied by
//         D_l, the row of the channel is written back (absent for C = 1 or R = I); a chunk is staged through LDS so that
//         global memory sees consecutive lanes on consecutive words (transform_sh_chunk)
//   n     one row of positions, rotations and scales (10 floats in, 10 out)
//   Z n   one row of one of the Z arrays to clear (the optimizer's moments)
// A lane owns its item: every float of it is on chip before the first store of its chunk, so the update is in place
// without a workspace.  Where the mask byte of a row is 0 nothing else of the row is loaded and nothing is stored.  The
// transform is a kernel argument (wave-uniform, in scalar registers); every sum is the fixed left-to-right order the
// header states.
#include "cugs_common.h"

#include <math.h>

#define XF_MAX_ZERO CUGS_TRANSFORM_MAX_ZERO

namespace {

// ---- host: SH rotation matrices from polynomial substitution ---------------------------------------------------------
// A band's basis functions are K_i q_i(d) with q_i a homogeneous polynomial with small integer coefficients.  q_i(R d) is
// expanded by multiplying linear forms (rows of R), and its coordinates y_j in the q_j are read off single monomial
// coefficients (each q_j owns a monomial, or a difference of two, that no other q of the band contains with another
// ratio).  D[i][j] = (K_i / K_j) y_j: Y_l(R d) = D_l Y_l(d).  For a signed permutation R every product is exact, so D is
// an exact signed permutation as well.
struct Poly { double c[4][4]; };      // c[i][j]: coefficient of x^i y^j z^(deg - i - j)

Poly poly_one() { Poly p{}; p.c[0][0] = 1.0; return p; }

// p (degree deg) times the linear form r0 x + r1 y + r2 z
Poly poly_times_linear(const Poly& p, int deg, const double* r) {
    Poly o{};
    for (int i = 0; i <= deg; ++i)
        for (int j = 0; i + j <= deg; ++j) {
            const double v = p.c[i][j];
            if (v == 0.0) continue;
            o.c[i + 1][j] += v * r[0];
            o.c[i][j + 1] += v * r[1];
            o.c[i][j] += v * r[2];
        }
    return o;
}

// (R d)_x^a (R d)_y^b (R d)_z^c as a polynomial in d
Poly rotated_monomial(const double* R, int a, int b, int c) {
    Poly p = poly_one();
    int deg = 0;
    for (int k = 0; k < a; ++k) p = poly_times_linear(p, deg++, R + 0);
    for (int k = 0; k < b; ++k) p = poly_times_linear(p, deg++, R + 3);
    for (int k = 0; k < c; ++k) p = poly_times_linear(p, deg++, R + 6);
    return p;
}

struct Term { int coef, a, b, c; };
struct Basis { double K; int nterms; Term t[3]; };

void poly_axpy(Poly& acc, double s, const Poly& p) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) acc.c[i][j] += s * p.c[i][j];
}

Poly rotated_basis(const double* R, const Basis& b) {
    Poly acc{};
    for (int k = 0; k < b.nterms; ++k)
        poly_axpy(acc, (double)b.t[k].coef, rotated_monomial(R, b.t[k].a, b.t[k].b, b.t[k].c));
    return acc;
}

constexpr double K1 = 0.4886025119029199;
constexpr double K2a = 1.0925484305920792, K2b = 0.31539156525252005, K2c = 0.5462742152960396;
constexpr double K3a = 0.5900435899266435, K3b = 2.890611442640554, K3c = 0.4570457994644658,
                 K3d = 0.3731763325901154, K3e = 1.4453057213202769;

void sh_rotation_band1(const double* R, double* D) {
    const Basis B[3] = {{-K1, 1, {{1, 0, 1, 0}}}, {K1, 1, {{1, 0, 0, 1}}}, {-K1, 1, {{1, 1, 0, 0}}}};
    for (int i = 0; i < 3; ++i) {
        const Poly g = rotated_basis(R, B[i]);
        const double y[3] = {g.c[0][1], g.c[0][0], g.c[1][0]};
        for (int j = 0; j < 3; ++j) D[3 * i + j] = (B[i].K / B[j].K) * y[j];
    }
}

void sh_rotation_band2(const double* R, double* D) {
    const Basis B[5] = {{K2a, 1, {{1, 1, 1, 0}}},
                        {K2a, 1, {{1, 0, 1, 1}}},
                        {K2b, 3, {{2, 0, 0, 2}, {-1, 2, 0, 0}, {-1, 0, 2, 0}}},
                        {K2a, 1, {{1, 1, 0, 1}}},
                        {K2c, 2, {{1, 2, 0, 0}, {-1, 0, 2, 0}}}};
    for (int i = 0; i < 5; ++i) {
        const Poly g = rotated_basis(R, B[i]);
        const double y[5] = {g.c[1][1], g.c[0][1], g.c[0][0] / 2.0, g.c[1][0], (g.c[2][0] - g.c[0][2]) / 2.0};
        for (int j = 0; j < 5; ++j) D[5 * i + j] = (B[i].K / B[j].K) * y[j];
    }
}

void sh_rotation_band3(const double* R, double* D) {
    const Basis B[7] = {{K3a, 2, {{3, 2, 1, 0}, {-1, 0, 3, 0}}},
                        {K3b, 1, {{1, 1, 1, 1}}},
                        {K3c, 3, {{4, 0, 1, 2}, {-1, 2, 1, 0}, {-1, 0, 3, 0}}},
                        {K3d, 3, {{2, 0, 0, 3}, {-3, 2, 0, 1}, {-3, 0, 2, 1}}},
                        {K3c, 3, {{4, 1, 0, 2}, {-1, 3, 0, 0}, {-1, 1, 2, 0}}},
                        {K3e, 2, {{1, 2, 0, 1}, {-1, 0, 2, 1}}},
                        {K3a, 2, {{1, 3, 0, 0}, {-3, 1, 2, 0}}}};
    for (int i = 0; i < 7; ++i) {
        const Poly g = rotated_basis(R, B[i]);
        const double y[7] = {(g.c[2][1] - g.c[0][3]) / 4.0,      // x^2 y - y^3
                             g.c[1][1],                           // x y z
                             g.c[0][1] / 4.0,                     // y z^2
                             g.c[0][0] / 2.0,                     // z^3
                             g.c[1][0] / 4.0,                     // x z^2
                             (g.c[2][0] - g.c[0][2]) / 2.0,       // x^2 z - y^2 z
                             (g.c[3][0] - g.c[1][2]) / 4.0};      // x^3 - x y^2
        for (int j = 0; j < 7; ++j) D[7 * i + j] = (B[i].K / B[j].K) * y[j];
    }
}

double det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// Nearest rotation: the orthogonal polar factor by Newton's iteration X <- (X + X^-T) / 2, which a matrix within 1e-4
// of orthogonal reaches to the last bit in a few steps; an exactly orthogonal input with exact cofactors is a fixed point.
void nearest_rotation(const double* in, double* X) {
    for (int i = 0; i < 9; ++i) X[i] = in[i];
    for (int it = 0; it < 12; ++it) {
        const double d = det3(X);
        const double cof[9] = {X[4] * X[8] - X[5] * X[7], X[5] * X[6] - X[3] * X[8], X[3] * X[7] - X[4] * X[6],
                               X[2] * X[7] - X[1] * X[8], X[0] * X[8] - X[2] * X[6], X[1] * X[6] - X[0] * X[7],
                               X[1] * X[5] - X[2] * X[4], X[2] * X[3] - X[0] * X[5], X[0] * X[4] - X[1] * X[3]};
        double change = 0.0;
        for (int i = 0; i < 9; ++i) {
            const double nx = 0.5 * (X[i] + cof[i] / d);       // X^-T = cofactor matrix / det
            change = fmax(change, fabs(nx - X[i]));
            X[i] = nx;
        }
        if (change < 1e-17) break;
    }
}

// Unit quaternion (wxyz, w >= 0) of a rotation matrix, by the branch with the largest pivot.
void quaternion_of(const double* R, double* q) {
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) {
        const double s = 2.0 * sqrt(1.0 + tr);
        q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
        q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
    } else if (R[4] > R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
        q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
        q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
    }
    const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double sign = q[0] < 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < 4; ++i) q[i] = sign * q[i] / nrm + 0.0;      // + 0.0: no negative zero
}

// ---- device ----------------------------------------------------------------------------------------------------------
struct XfArgs {
    CugsSimilarity xf;
    int64_t n;
    int64_t sh_items, geo_items;        // 3n or 0; n or 0
    float* positions; float* rotations; float* scales; float* sh;
    const uint8_t* mask;
    float* zero[XF_MAX_ZERO];
    int32_t zero_floats[XF_MAX_ZERO];
    int32_t zero_vec4[XF_MAX_ZERO];
    int32_t num_zero;
    int32_t sh_vec4, rot_vec4;          // 16-byte accesses are safe for the SH rows of a channel / the quaternions
};

// out[i] = sum_j A[i][j] x[j], j ascending, product and sum rounded separately (-ffp-contract=off)
template <int L>
__device__ __forceinline__ void band_times(const float (&A)[L * L], const float* x, float* out) {
#pragma unroll
    for (int i = 0; i < L; ++i) {
        float acc = A[i * L] * x[0];
#pragma unroll
        for (int j = 1; j < L; ++j) acc = acc + A[i * L + j] * x[j];
        out[i] = acc;
    }
}

// One chunk of CUGS_BLOCK consecutive (row, channel) items = CUGS_BLOCK * C consecutive floats of the SH tensor.  The
// workgroup loads them with consecutive lanes on consecutive dwords (or 16-byte words), parks them in LDS at a row
// stride of C + 1 floats (conflict-free when every lane then reads its own row), lane i transforms item i in registers
// and writes it back to LDS, and the chunk is stored the way it was loaded.  Every load of the chunk precedes every
// store (two barriers), so the update is in place; the loads and stores of a float are predicated on the mask byte of
// its row, which one lane reads for the whole chunk.  A lane-per-row access without the staging reads 64 rows at a
// 4 C byte stride per instruction and ran at a third of a copy's rate.
template <int C>
__device__ __forceinline__ void transform_sh_chunk(const XfArgs& a, int64_t chunk, float* lds, int* live) {
    constexpr int S = C + 1;
    const int64_t first = chunk * CUGS_BLOCK;                     // first item of the chunk
    const int64_t left = a.sh_items - first;
    const int items = (int)(left < CUGS_BLOCK ? left : CUGS_BLOCK);
    float* g = a.sh + first * C;
    const int tid = (int)threadIdx.x;
    const bool vec = (C & 3) == 0 && a.sh_vec4;
    const bool masked = a.mask != nullptr;
    if (masked) {                                                 // one mask byte per item, read once, shared through LDS
        live[tid] = (tid < items && a.mask[(first + tid) / 3] != 0) ? 1 : 0;
        __syncthreads();
    }
    if (vec) {
        for (int v = tid; v < items * (C / 4); v += CUGS_BLOCK) {
            const int item = v / (C / 4), k = (v % (C / 4)) * 4;
            if (masked && !live[item]) continue;
            const float4 x = cugs_ldnt(reinterpret_cast<const float4*>(g) + v);
            float* d = lds + item * S + k;
            d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
        }
    } else {
        for (int e = tid; e < items * C; e += CUGS_BLOCK) {
            const int item = e / C;
            if (masked && !live[item]) continue;
            lds[item * S + (e - item * C)] = cugs_ldnt(g + e);
        }
    }
    __syncthreads();
    if (tid < items && !(masked && !live[tid])) {
        float* r = lds + tid * S;
        float c[C], o[C];
#pragma unroll
        for (int k = 0; k < C; ++k) c[k] = r[k];
        if (C >= 4) band_times<3>(a.xf.d1, c + 1, o + 1);
        if (C >= 9) band_times<5>(a.xf.d2, c + 4, o + 4);
        if (C >= 16) band_times<7>(a.xf.d3, c + 9, o + 9);
#pragma unroll
        for (int k = 1; k < C; ++k) r[k] = o[k];                  // the DC term stays as loaded
    }
    __syncthreads();
    if (vec) {
        for (int v = tid; v < items * (C / 4); v += CUGS_BLOCK) {
            const int item = v / (C / 4), k = (v % (C / 4)) * 4;
            if (masked && !live[item]) continue;
            const float* d = lds + item * S + k;
            cugs_stnt(reinterpret_cast<float4*>(g) + v, make_float4(d[0], d[1], d[2], d[3]));
        }
    } else {
        for (int e = tid; e < items * C; e += CUGS_BLOCK) {
            const int item = e / C, k = e - item * C;
            if (k == 0 || (masked && !live[item])) continue;   // the DC term is not rewritten
            cugs_stnt(g + e, lds[item * S + k]);
        }
    }
    __syncthreads();                                              // the next chunk's loads overwrite the staging rows
}

__device__ __forceinline__ void transform_geometry_row(const XfArgs& a, int64_t row) {
    if (a.mask && a.mask[row] == 0) return;
    const CugsSimilarity& f = a.xf;
    const bool rotate = !(f.flags & CUGS_SIMILARITY_ROTATION_IS_IDENTITY);
    const bool rescale = !(f.flags & CUGS_SIMILARITY_SCALE_IS_ONE);
    float* pp = a.positions + row * 3;
    float* pq = a.rotations + row * 4;
    float* ps = a.scales + row * 3;
    const float x = cugs_ldnt(pp), y = cugs_ldnt(pp + 1), z = cugs_ldnt(pp + 2);
    float qw = 0.f, qx = 0.f, qy = 0.f, qz = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (rotate) {
        if (a.rot_vec4) {
            const float4 q = cugs_ldnt(reinterpret_cast<const float4*>(pq));
            qw = q.x; qx = q.y; qy = q.z; qz = q.w;
        } else {
            qw = cugs_ldnt(pq); qx = cugs_ldnt(pq + 1); qy = cugs_ldnt(pq + 2); qz = cugs_ldnt(pq + 3);
        }
    }
    if (rescale) { s0 = cugs_ldnt(ps); s1 = cugs_ldnt(ps + 1); s2 = cugs_ldnt(ps + 2); }

    float acc;
    acc = f.m[0] * x; acc = acc + f.m[1] * y; acc = acc + f.m[2] * z; const float ox = acc + f.t[0];
    acc = f.m[3] * x; acc = acc + f.m[4] * y; acc = acc + f.m[5] * z; const float oy = acc + f.t[1];
    acc = f.m[6] * x; acc = acc + f.m[7] * y; acc = acc + f.m[8] * z; const float oz = acc + f.t[2];
    cugs_stnt(pp, ox); cugs_stnt(pp + 1, oy); cugs_stnt(pp + 2, oz);
    if (rotate) {                                                 // q_R (x) q, Hamilton, wxyz
        const float aw = f.q[0], ax = f.q[1], ay = f.q[2], az = f.q[3];
        const float ow = aw * qw - ax * qx - ay * qy - az * qz;
        const float oxq = aw * qx + ax * qw + ay * qz - az * qy;
        const float oyq = aw * qy - ax * qz + ay * qw + az * qx;
        const float ozq = aw * qz + ax * qy - ay * qx + az * qw;
        if (a.rot_vec4) {
            cugs_stnt(reinterpret_cast<float4*>(pq), make_float4(ow, oxq, oyq, ozq));
        } else {
            cugs_stnt(pq, ow); cugs_stnt(pq + 1, oxq); cugs_stnt(pq + 2, oyq); cugs_stnt(pq + 3, ozq);
        }
    }
    if (rescale) {
        cugs_stnt(ps, s0 + f.log_scale); cugs_stnt(ps + 1, s1 + f.log_scale); cugs_stnt(ps + 2, s2 + f.log_scale);
    }
}

__device__ __forceinline__ void zero_row(const XfArgs& a, int64_t item) {
    int k = 0;
    int64_t row = item;
#pragma unroll
    for (int j = 1; j < XF_MAX_ZERO; ++j)
        if (j < a.num_zero && item >= (int64_t)j * a.n) { k = j; row = item - (int64_t)j * a.n; }
    if (a.mask && a.mask[row] == 0) return;
    float* base = a.zero[0];
    int32_t nf = a.zero_floats[0], v4 = a.zero_vec4[0];
#pragma unroll
    for (int j = 1; j < XF_MAX_ZERO; ++j)                         // no run-time index into a kernel argument
        if (j == k) { base = a.zero[j]; nf = a.zero_floats[j]; v4 = a.zero_vec4[j]; }
    float* p = base + row * nf;
    if (v4) {
        for (int j = 0; j < (nf >> 2); ++j) cugs_stnt(reinterpret_cast<float4*>(p) + j, make_float4(0.f, 0.f, 0.f, 0.f));
    } else {
        for (int j = 0; j < nf; ++j) cugs_stnt(p + j, 0.0f);
    }
}

template <int C>
__global__ __launch_bounds__(CUGS_BLOCK) void k_transform_gaussians(const XfArgs a) {
    __shared__ float lds[C > 1 ? CUGS_BLOCK * (C + 1) : 1];
    __shared__ int live[CUGS_BLOCK];
    // chunks of CUGS_BLOCK items, taken workgroup by workgroup: the trip count and the kind of a chunk are uniform over
    // the workgroup, as the barriers of the SH chunks need
    const int64_t sh_chunks = (a.sh_items + CUGS_BLOCK - 1) / CUGS_BLOCK;
    const int64_t geo_chunks = (a.geo_items + CUGS_BLOCK - 1) / CUGS_BLOCK;
    const int64_t zero_items = (int64_t)a.num_zero * a.n;
    const int64_t total = sh_chunks + geo_chunks + (zero_items + CUGS_BLOCK - 1) / CUGS_BLOCK;
    for (int64_t chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
        if (chunk < sh_chunks) {
            if (C > 1) transform_sh_chunk<C>(a, chunk, lds, live);
        } else if (chunk < sh_chunks + geo_chunks) {
            const int64_t row = (chunk - sh_chunks) * CUGS_BLOCK + threadIdx.x;
            if (row < a.geo_items) transform_geometry_row(a, row);
        } else {
            const int64_t item = (chunk - sh_chunks - geo_chunks) * CUGS_BLOCK + threadIdx.x;
            if (item < zero_items) zero_row(a, item);
        }
    }
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int cugs_similarity_init(CugsSimilarity* out, const double rotation[9], const double translation[3],
                                    double scale) {
    if (!out || !rotation || !translation) return CUGS_EINVAL;
    for (int i = 0; i < 9; ++i)
        if (!isfinite(rotation[i])) return CUGS_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (!isfinite(translation[i])) return CUGS_EINVAL;
    if (!isfinite(scale) || !(scale > 0.0)) return CUGS_EINVAL;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double g = 0.0;
            for (int k = 0; k < 3; ++k) g += rotation[3 * k + i] * rotation[3 * k + j];
            if (!(fabs(g - (i == j ? 1.0 : 0.0)) <= 1e-4)) return CUGS_EINVAL;
        }
    if (det3(rotation) < 0.0) return CUGS_EINVAL;

    double R[9], q[4], D1[9], D2[25], D3[49];
    nearest_rotation(rotation, R);
    quaternion_of(R, q);
    sh_rotation_band1(R, D1);
    sh_rotation_band2(R, D2);
    sh_rotation_band3(R, D3);
    bool identity = true;
    for (int i = 0; i < 9; ++i) {
        out->m[i] = (float)(scale * R[i]);
        identity = identity && R[i] == ((i % 4 == 0) ? 1.0 : 0.0);
    }
    for (int i = 0; i < 3; ++i) out->t[i] = (float)translation[i];
    out->log_scale = (float)log(scale);
    for (int i = 0; i < 4; ++i) out->q[i] = (float)q[i];
    for (int i = 0; i < 9; ++i) out->d1[i] = (float)D1[i];
    for (int i = 0; i < 25; ++i) out->d2[i] = (float)D2[i];
    for (int i = 0; i < 49; ++i) out->d3[i] = (float)D3[i];
    out->flags = (identity ? CUGS_SIMILARITY_ROTATION_IS_IDENTITY : 0u) | (scale == 1.0 ? CUGS_SIMILARITY_SCALE_IS_ONE : 0u);
    return 0;
}

extern "C" int cugs_transform_gaussians(int64_t n, int sh_coeffs, float* positions, float* rotations, float* scales,
                                        float* sh, const uint8_t* mask, float* const* zero_rows_host,
                                        const int* zero_row_floats_host, int num_zero, const CugsSimilarity* xf_host,
                                        void* stream) {
    if (n < 0 || !(sh_coeffs == 1 || sh_coeffs == 4 || sh_coeffs == 9 || sh_coeffs == 16) || !xf_host) return CUGS_EINVAL;
    if (num_zero < 0 || num_zero > XF_MAX_ZERO || (num_zero > 0 && (!zero_rows_host || !zero_row_floats_host)))
        return CUGS_EINVAL;
    for (int k = 0; k < num_zero; ++k)
        if (zero_row_floats_host[k] <= 0 || (n > 0 && !zero_rows_host[k])) return CUGS_EINVAL;
    if (n > 0 && (!positions || !rotations || !scales || !sh)) return CUGS_EINVAL;
    if (!aligned4(positions) || !aligned4(rotations) || !aligned4(scales) || !aligned4(sh)) return CUGS_EALIGN;
    for (int k = 0; k < num_zero; ++k)
        if (!aligned4(zero_rows_host[k])) return CUGS_EALIGN;
    if (n == 0) return 0;

    XfArgs a;
    a.xf = *xf_host;
    const bool rot_id = (a.xf.flags & CUGS_SIMILARITY_ROTATION_IS_IDENTITY) != 0;
    const bool identity = rot_id && (a.xf.flags & CUGS_SIMILARITY_SCALE_IS_ONE) && a.xf.t[0] == 0.0f &&
                          a.xf.t[1] == 0.0f && a.xf.t[2] == 0.0f;
    a.n = n;
    a.sh_items = (sh_coeffs > 1 && !rot_id) ? 3 * n : 0;
    a.geo_items = identity ? 0 : n;                              // the identity keeps every bit (a -0.0 too)
    a.positions = positions; a.rotations = rotations; a.scales = scales; a.sh = sh;
    a.mask = mask;
    a.num_zero = num_zero;
    for (int k = 0; k < XF_MAX_ZERO; ++k) {
        const bool used = k < num_zero;
        a.zero[k] = used ? zero_rows_host[k] : nullptr;
        a.zero_floats[k] = used ? zero_row_floats_host[k] : 1;
        a.zero_vec4[k] = (used && (zero_row_floats_host[k] & 3) == 0 && cugs_aligned16(zero_rows_host[k])) ? 1 : 0;
    }
    a.sh_vec4 = cugs_aligned16(sh) ? 1 : 0;                       // with C % 4 == 0 every (row, channel) then is aligned
    a.rot_vec4 = cugs_aligned16(rotations) ? 1 : 0;
    const auto chunks = [](int64_t items) { return (items + CUGS_BLOCK - 1) / CUGS_BLOCK; };
    const int64_t want = chunks(a.sh_items) + chunks(a.geo_items) + chunks((int64_t)num_zero * n);
    if (want == 0) return 0;
    const dim3 grid((unsigned)(want < 1024 ? want : 1024)), block(CUGS_BLOCK);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (sh_coeffs) {
        case 1: hipLaunchKernelGGL(k_transform_gaussians<1>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(k_transform_gaussians<4>, grid, block, 0, st, a); break;
        case 9: hipLaunchKernelGGL(k_transform_gaussians<9>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(k_transform_gaussians<16>, grid, block, 0, st, a); break;
    }
    CUGS_LAUNCH_CHECK();
    return 0;
}
