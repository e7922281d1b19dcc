// tsdf.hip — mesh export (not in the reference): fusion of render()'s depth and alpha maps into a dense
// truncated signed distance volume, and surface-net extraction of its zero level set.  The per-voxel, per-cell and
// per-edge rules are the functions of cugs_tsdf.h; this file is their launch structure.
//
//   k_tsdf_integrate   one pass over the volume for up to 16 views, brick by brick (cugs_tsdf.h: TsdfWalk).  A thread owns
//                      four x-neighbours of one row; it walks the views in the order given, loads its voxels from every plane the first time a view
//                      touches one of them, updates them in registers and stores them once at the end.  A group that
//                      no view touches moves no volume bytes.  VEC: one 16-byte access per plane (base 16-byte aligned
//                      and nx % 4 == 0); otherwise 4-byte accesses of the touched voxels only.  The arithmetic per voxel
//                      is the same on both routes.  The view table travels as a kernel argument.
//   k_mesh_classify    per cell: active or not -> one byte.
//   k_mesh_count       per chunk of 1024 cells (four per thread): the code byte of each cell (bit 0 active, bits 1-3 the
//                      lattice edges along x, y, z that give faces) and the chunk's {vertices, triangles}.
//   k_mesh_scan2       256 chunk rows per workgroup -> exclusive prefixes in place, the block's sum to level 3.
//   k_mesh_scan3       one workgroup: level 3 in strides of 256 with a carry, and the totals.
//   k_mesh_vertices    per chunk: the local scan again, vertex index per cell, vertices and colours.
//   k_mesh_faces       per chunk: the local scan again, two triangles per coded edge.
// Integer scans only: no float atomics, the same bytes from run to run.
#include "cugs_common.h"
#include "cugs_tsdf.h"

namespace {

struct TsdfViews {
    TsdfView v[CUGS_TSDF_MAX_VIEWS];
};

template <bool COLOR, bool VEC>
__global__ __launch_bounds__(CUGS_BLOCK) void k_tsdf_integrate(TsdfGrid g, TsdfViews views, int num_views, TsdfWalk walk,
                                                               float* __restrict__ vol) {
    constexpr int P = COLOR ? 5 : 2;
    const uint64_t gid = (uint64_t)blockIdx.x * (uint64_t)CUGS_BLOCK + threadIdx.x;
    int ix0, iy, iz;
    if (!tsdf_group_coords(walk, g.nx, g.ny, g.nz, gid, &ix0, &iy, &iz)) return;
    const size_t plane = (size_t)g.nx * (size_t)g.ny * (size_t)g.nz;
    const size_t base = mesh_voxel(g.nx, g.ny, ix0, iy, iz);
    const int nvox = (g.nx - ix0 < 4) ? g.nx - ix0 : 4;             // VEC: always 4

    float val[P][4];
    bool loaded = false;
    unsigned touched = 0;
    for (int s = 0; s < num_views; ++s) {
        const TsdfView& v = views.v[s];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= nvox) continue;
            float tn, w;
            size_t pix;
            if (!tsdf_sample(g, v, ix0 + k, iy, iz, &tn, &w, &pix)) continue;
            if (!loaded) {
                loaded = true;
                if constexpr (VEC) {
#pragma unroll
                    for (int p = 0; p < P; ++p) {
                        const float4 t = *reinterpret_cast<const float4*>(vol + p * plane + base);
                        val[p][0] = t.x; val[p][1] = t.y; val[p][2] = t.z; val[p][3] = t.w;
                    }
                } else {
#pragma unroll
                    for (int p = 0; p < P; ++p)
#pragma unroll
                        for (int j = 0; j < 4; ++j) val[p][j] = (j < nvox) ? vol[p * plane + base + j] : 0.0f;
                }
            }
            touched |= 1u << k;
            const float wo = val[1][k], wn = wo + w;
            val[0][k] = tsdf_blend(val[0][k], wo, tn, w, wn);
            if constexpr (COLOR) {
                const float* c = v.color + 3 * pix;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) val[2 + ch][k] = tsdf_blend(val[2 + ch][k], wo, c[ch], w, wn);
            }
            val[1][k] = fminf(wn, g.max_weight);
        }
    }
    if (!touched) return;
    if constexpr (VEC) {
#pragma unroll
        for (int p = 0; p < P; ++p)
            *reinterpret_cast<float4*>(vol + p * plane + base) = make_float4(val[p][0], val[p][1], val[p][2], val[p][3]);
    } else {
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (touched >> j & 1u) vol[p * plane + base + j] = val[p][j];
    }
}

// ---- extraction --------------------------------------------------------------------------------------------------------
constexpr int CELLS_PER_THREAD = 4;
constexpr unsigned CHUNK = CUGS_BLOCK * CELLS_PER_THREAD;       // 1024 cells
constexpr unsigned L2 = CUGS_BLOCK;                             // chunk rows per level-2 workgroup

struct MeshDims {
    int nx, ny, nz;             // voxels
    unsigned cnx, cny, cnz;     // cells
    unsigned ncells;
};

struct MeshWs {
    uint8_t* active;            // [nchunks * CHUNK]
    uint8_t* code;              // [nchunks * CHUNK]
    int32_t* vid;               // [nchunks * CHUNK]
    uint2* chunk;               // [nchunks]: {vertices, triangles}, then their exclusive prefix within the level-2 block
    unsigned long long* l3;     // [2 * nl3]: level-2 block sums, then their exclusive prefix
    unsigned long long* totals; // [2]
    size_t nchunks, nl3, bytes;
};

size_t round256(size_t b) { return (b + 255) / 256 * 256; }

MeshWs mesh_layout(void* workspace, size_t ncells) {
    MeshWs w;
    w.nchunks = (ncells + CHUNK - 1) / CHUNK;
    w.nl3 = (w.nchunks + L2 - 1) / L2;
    char* p = static_cast<char*>(workspace);
    size_t off = 0;
    const size_t padded = w.nchunks * CHUNK;
    w.active = reinterpret_cast<uint8_t*>(p + off); off += round256(padded);
    w.code = reinterpret_cast<uint8_t*>(p + off); off += round256(padded);
    w.vid = reinterpret_cast<int32_t*>(p + off); off += round256(padded * sizeof(int32_t));
    w.chunk = reinterpret_cast<uint2*>(p + off); off += round256(w.nchunks * sizeof(uint2));
    w.l3 = reinterpret_cast<unsigned long long*>(p + off); off += round256(2 * w.nl3 * sizeof(unsigned long long));
    w.totals = reinterpret_cast<unsigned long long*>(p + off); off += 256;
    w.bytes = off;
    return w;
}

__device__ __forceinline__ void cell_coords(const MeshDims& d, unsigned c, int* x, int* y, int* z) {
    const unsigned row = c / d.cnx;
    *x = (int)(c - row * d.cnx);
    *z = (int)(row / d.cny);
    *y = (int)(row - (unsigned)*z * d.cny);
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_mesh_classify(MeshDims d, const float* __restrict__ tsdf,
                                                              const float* __restrict__ weight, float min_weight,
                                                              uint8_t* __restrict__ active) {
    const unsigned c = blockIdx.x * (unsigned)CUGS_BLOCK + threadIdx.x;
    if (c >= d.ncells) return;
    int x, y, z;
    cell_coords(d, c, &x, &y, &z);
    active[c] = mesh_cell_active(tsdf, weight, d.nx, d.ny, x, y, z, min_weight);
}

// Exclusive scan of one uint2 per thread over the workgroup; *total = the workgroup's sum.
__device__ __forceinline__ uint2 block_scan(uint2 v, uint2* total) {
    __shared__ uint2 s[2][CUGS_BLOCK];
    const int tid = threadIdx.x;
    int cur = 0;
    s[0][tid] = v;
    __syncthreads();
#pragma unroll
    for (int step = 1; step < CUGS_BLOCK; step <<= 1) {
        uint2 a = s[cur][tid];
        if (tid >= step) { const uint2 b = s[cur][tid - step]; a.x += b.x; a.y += b.y; }
        s[cur ^ 1][tid] = a;
        cur ^= 1;
        __syncthreads();
    }
    const uint2 incl = s[cur][tid];
    *total = s[cur][CUGS_BLOCK - 1];
    __syncthreads();                                            // s is reused by the next call
    return make_uint2(incl.x - v.x, incl.y - v.y);
}

__device__ __forceinline__ uint2 code_counts(unsigned code) {
    return make_uint2(code & 1u, 2u * (unsigned)__popc(code >> 1));
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_mesh_count(MeshDims d, const float* __restrict__ tsdf,
                                                           const uint8_t* __restrict__ active, uint8_t* __restrict__ code,
                                                           uint2* __restrict__ chunk) {
    const unsigned c0 = blockIdx.x * CHUNK + threadIdx.x * (unsigned)CELLS_PER_THREAD;
    uint2 mine = make_uint2(0u, 0u);
    unsigned packed = 0;
#pragma unroll
    for (int j = 0; j < CELLS_PER_THREAD; ++j) {
        const unsigned c = c0 + (unsigned)j;
        unsigned cd = 0;
        if (c < d.ncells && active[c]) {
            int x, y, z;
            cell_coords(d, c, &x, &y, &z);
            cd = 1u;
#pragma unroll
            for (int axis = 0; axis < 3; ++axis)
                if (mesh_edge_faces(tsdf, active, d.nx, d.ny, x, y, z, axis)) cd |= 2u << axis;
        }
        packed |= cd << (8 * j);
        const uint2 n = code_counts(cd);
        mine.x += n.x; mine.y += n.y;
    }
    *reinterpret_cast<uint32_t*>(code + c0) = packed;          // the array is padded to whole chunks, 256-byte aligned
    uint2 total;
    block_scan(mine, &total);
    if (threadIdx.x == 0) chunk[blockIdx.x] = total;
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_mesh_scan2(unsigned nchunks, uint2* __restrict__ chunk,
                                                           unsigned long long* __restrict__ l3) {
    const unsigned i = blockIdx.x * L2 + threadIdx.x;
    const uint2 v = i < nchunks ? chunk[i] : make_uint2(0u, 0u);
    uint2 total;
    const uint2 ex = block_scan(v, &total);
    if (i < nchunks) chunk[i] = ex;
    if (threadIdx.x == 0) { l3[2 * blockIdx.x] = total.x; l3[2 * blockIdx.x + 1] = total.y; }
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_mesh_scan3(unsigned nl3, unsigned long long* __restrict__ l3,
                                                           unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long s[2][2][CUGS_BLOCK];
    const int tid = threadIdx.x;
    unsigned long long carry_v = 0, carry_f = 0;
    for (unsigned base = 0; base < nl3; base += CUGS_BLOCK) {
        const unsigned i = base + tid;
        const unsigned long long v = i < nl3 ? l3[2 * i] : 0ull, f = i < nl3 ? l3[2 * i + 1] : 0ull;
        int cur = 0;
        s[0][0][tid] = v; s[0][1][tid] = f;
        __syncthreads();
        for (int step = 1; step < CUGS_BLOCK; step <<= 1) {
            unsigned long long a = s[cur][0][tid], b = s[cur][1][tid];
            if (tid >= step) { a += s[cur][0][tid - step]; b += s[cur][1][tid - step]; }
            s[cur ^ 1][0][tid] = a; s[cur ^ 1][1][tid] = b;
            cur ^= 1;
            __syncthreads();
        }
        if (i < nl3) { l3[2 * i] = carry_v + s[cur][0][tid] - v; l3[2 * i + 1] = carry_f + s[cur][1][tid] - f; }
        carry_v += s[cur][0][CUGS_BLOCK - 1]; carry_f += s[cur][1][CUGS_BLOCK - 1];
        __syncthreads();
    }
    if (tid == 0) { totals[0] = carry_v; totals[1] = carry_f; }
}

// The first vertex and the first triangle of each of the thread's four cells.
__device__ __forceinline__ void chunk_offsets(const uint8_t* __restrict__ code, const uint2* __restrict__ chunk,
                                              const unsigned long long* __restrict__ l3, unsigned* codes,
                                              unsigned long long* v0, unsigned long long* f0) {
    const unsigned c0 = blockIdx.x * CHUNK + threadIdx.x * (unsigned)CELLS_PER_THREAD;
    const uint32_t packed = *reinterpret_cast<const uint32_t*>(code + c0);
    uint2 mine = make_uint2(0u, 0u);
#pragma unroll
    for (int j = 0; j < CELLS_PER_THREAD; ++j) {
        codes[j] = (packed >> (8 * j)) & 0xffu;
        const uint2 n = code_counts(codes[j]);
        mine.x += n.x; mine.y += n.y;
    }
    uint2 total;
    const uint2 ex = block_scan(mine, &total);
    const uint2 cb = chunk[blockIdx.x];
    const unsigned b3 = blockIdx.x / L2;
    *v0 = l3[2 * b3] + cb.x + ex.x;
    *f0 = l3[2 * b3 + 1] + cb.y + ex.y;
}

template <bool COLOR>
__global__ __launch_bounds__(CUGS_BLOCK) void k_mesh_vertices(MeshDims d, TsdfGrid g, const float* __restrict__ vol,
                                                              const uint8_t* __restrict__ code, const uint2* __restrict__ chunk,
                                                              const unsigned long long* __restrict__ l3, long long nvert,
                                                              int32_t* __restrict__ vid, float* __restrict__ vertices,
                                                              float* __restrict__ colors) {
    unsigned codes[CELLS_PER_THREAD];
    unsigned long long v, f;
    chunk_offsets(code, chunk, l3, codes, &v, &f);
    const unsigned c0 = blockIdx.x * CHUNK + threadIdx.x * (unsigned)CELLS_PER_THREAD;
    const size_t plane = (size_t)d.nx * (size_t)d.ny * (size_t)d.nz;
#pragma unroll
    for (int j = 0; j < CELLS_PER_THREAD; ++j) {
        if (!(codes[j] & 1u)) continue;
        const unsigned c = c0 + (unsigned)j;                    // < ncells after a plan: padding cells carry code 0
        if (c < d.ncells && v < (unsigned long long)nvert) {    // never past the caller's arrays, whatever the workspace holds
            int x, y, z;
            cell_coords(d, c, &x, &y, &z);
            float p[3], rgb[3];
            mesh_cell_vertex(vol, COLOR ? vol + 2 * plane : nullptr, plane, d.nx, d.ny, x, y, z, g.ox, g.oy, g.oz, g.vs, p, rgb);
            vid[c] = (int32_t)v;
            vertices[3 * v] = p[0]; vertices[3 * v + 1] = p[1]; vertices[3 * v + 2] = p[2];
            if constexpr (COLOR) { colors[3 * v] = rgb[0]; colors[3 * v + 1] = rgb[1]; colors[3 * v + 2] = rgb[2]; }
        }
        ++v;
    }
}

__global__ __launch_bounds__(CUGS_BLOCK) void k_mesh_faces(MeshDims d, const float* __restrict__ tsdf,
                                                           const uint8_t* __restrict__ code, const uint2* __restrict__ chunk,
                                                           const unsigned long long* __restrict__ l3, long long nfaces,
                                                           const int32_t* __restrict__ vid, int32_t* __restrict__ faces) {
    unsigned codes[CELLS_PER_THREAD];
    unsigned long long v, f;
    chunk_offsets(code, chunk, l3, codes, &v, &f);
    const unsigned c0 = blockIdx.x * CHUNK + threadIdx.x * (unsigned)CELLS_PER_THREAD;
#pragma unroll
    for (int j = 0; j < CELLS_PER_THREAD; ++j) {
        if (!(codes[j] >> 1)) continue;
        if (c0 + (unsigned)j >= d.ncells) continue;
        int x, y, z;
        cell_coords(d, c0 + (unsigned)j, &x, &y, &z);
        const int p[3] = {x, y, z};
#pragma unroll
        for (int axis = 0; axis < 3; ++axis) {
            if (!(codes[j] >> (1 + axis) & 1u)) continue;
            // never past the caller's array or before the box, whatever the workspace holds
            const bool inside = p[(axis + 1) % 3] >= 1 && p[(axis + 2) % 3] >= 1;
            const unsigned long long nf = (unsigned long long)nfaces;
            if (inside && f < nf && nf - f >= 2) {
                size_t q[4];
                mesh_edge_quad(tsdf, d.nx, d.ny, x, y, z, axis, q);
                const int32_t i0 = vid[q[0]], i1 = vid[q[1]], i2 = vid[q[2]], i3 = vid[q[3]];
                int32_t* o = faces + 3 * f;
                o[0] = i0; o[1] = i1; o[2] = i2;
                o[3] = i0; o[4] = i2; o[5] = i3;
            }
            f += 2;
        }
    }
}

bool pos_finite(float x) { return x > 0.0f && x < INFINITY; }

// What plan and emit ask of the volume (CUGS_EINVAL otherwise).
bool volume_ok(const cugs_tsdf_volume* vol) {
    return vol && vol->nx > 0 && vol->ny > 0 && vol->nz > 0 && vol->planes && pos_finite(vol->voxel_size) && pos_finite(vol->trunc);
}

// nx ny nz, or -1 when it does not fit int32 (CUGS_EOVERFLOW).
int64_t voxel_count(const cugs_tsdf_volume* vol) {
    const int64_t nxy = (int64_t)vol->nx * vol->ny;             // < 2^62
    if (nxy > 2147483647ll || nxy * vol->nz > 2147483647ll) return -1;
    return nxy * vol->nz;
}

size_t cell_count(int nx, int ny, int nz) { return (size_t)(nx - 1) * (size_t)(ny - 1) * (size_t)(nz - 1); }

MeshDims mesh_dims(const cugs_tsdf_volume* vol) {
    MeshDims d;
    d.nx = vol->nx; d.ny = vol->ny; d.nz = vol->nz;
    d.cnx = (unsigned)(vol->nx - 1); d.cny = (unsigned)(vol->ny - 1); d.cnz = (unsigned)(vol->nz - 1);
    d.ncells = (unsigned)cell_count(vol->nx, vol->ny, vol->nz);
    return d;
}

}  // namespace

extern "C" int cugs_tsdf_integrate(const cugs_tsdf_volume* vol, const cugs_tsdf_view* views, int num_views,
                                   const cugs_tsdf_opts* opts, void* stream) {
    if (!vol || !views || !opts) return CUGS_EINVAL;
    if (vol->nx <= 0 || vol->ny <= 0 || vol->nz <= 0) return CUGS_EINVAL;
    if (num_views < 1 || num_views > CUGS_TSDF_MAX_VIEWS) return CUGS_EINVAL;
    if (!vol->planes) return CUGS_EINVAL;
    if (!pos_finite(vol->voxel_size) || !pos_finite(vol->trunc)) return CUGS_EINVAL;
    if (!pos_finite(opts->min_depth) || !pos_finite(opts->min_alpha) || !pos_finite(opts->max_weight)) return CUGS_EINVAL;
    for (int s = 0; s < num_views; ++s) {
        const cugs_tsdf_view& v = views[s];
        if (!pos_finite(v.camera.fx) || !pos_finite(v.camera.fy)) return CUGS_EINVAL;
        if (v.camera.width <= 0 || v.camera.height <= 0) return CUGS_EINVAL;
        if (!v.depth_map || !v.alpha) return CUGS_EINVAL;
        if (vol->color && !v.color) return CUGS_EINVAL;
    }
    if (voxel_count(vol) < 0) return CUGS_EOVERFLOW;

    TsdfGrid g;
    g.ox = vol->origin[0]; g.oy = vol->origin[1]; g.oz = vol->origin[2];
    g.vs = vol->voxel_size; g.trunc = vol->trunc;
    g.min_depth = opts->min_depth; g.min_alpha = opts->min_alpha; g.max_weight = opts->max_weight;
    g.nx = vol->nx; g.ny = vol->ny; g.nz = vol->nz;
    TsdfViews t;
    for (int s = 0; s < CUGS_TSDF_MAX_VIEWS; ++s) {
        const cugs_tsdf_view& v = views[s < num_views ? s : 0];
        TsdfView& o = t.v[s];
        for (int i = 0; i < 12; ++i) o.m[i] = v.camera.view[i];
        o.fx = v.camera.fx; o.fy = v.camera.fy; o.cx = v.camera.cx; o.cy = v.camera.cy;
        o.W = v.camera.width; o.H = v.camera.height;
        o.D = v.depth_map; o.A = v.alpha; o.color = vol->color ? v.color : nullptr; o.weight = v.weight;
    }
    const TsdfWalk walk = tsdf_make_walk(vol->nx, vol->ny, vol->nz);
    const uint64_t ngroups = tsdf_walk_groups(walk, vol->nz);                           // <= 8 (2^31 - 1)
    const unsigned nblk = (unsigned)((ngroups + CUGS_BLOCK - 1) / CUGS_BLOCK);          // <= 2^26
    const bool vec = cugs_aligned16(vol->planes) && vol->nx % 4 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define CUGS_TSDF(C, V) \
    hipLaunchKernelGGL((k_tsdf_integrate<C, V>), dim3(nblk), dim3(CUGS_BLOCK), 0, st, g, t, num_views, walk, vol->planes)
    if (vol->color) { if (vec) CUGS_TSDF(true, true); else CUGS_TSDF(true, false); }
    else { if (vec) CUGS_TSDF(false, true); else CUGS_TSDF(false, false); }
#undef CUGS_TSDF
    CUGS_LAUNCH_CHECK();
    return 0;
}

// Per cell: two bytes (active, code) and one int32 (vertex index), padded to whole chunks of 1024 cells; per chunk 8
// bytes; per 256 chunks 16 bytes; the totals.
extern "C" size_t cugs_mesh_workspace_bytes(int nx, int ny, int nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    if ((int64_t)nx * ny > 2147483647ll || (int64_t)nx * ny * nz > 2147483647ll) return 0;
    return mesh_layout(nullptr, cell_count(nx, ny, nz)).bytes;
}

extern "C" int cugs_mesh_plan(const cugs_tsdf_volume* vol, float min_weight, void* workspace, size_t workspace_bytes,
                              int64_t* counts_host, void* stream) {
    if (!volume_ok(vol) || !(min_weight >= 0.0f && min_weight < INFINITY) || !workspace || !counts_host) return CUGS_EINVAL;
    const int64_t nvox = voxel_count(vol);
    if (nvox < 0) return CUGS_EOVERFLOW;
    if (workspace_bytes < cugs_mesh_workspace_bytes(vol->nx, vol->ny, vol->nz)) return CUGS_EWORKSPACE;
    if (!cugs_aligned16(workspace)) return CUGS_EALIGN;
    const MeshDims d = mesh_dims(vol);
    const MeshWs ws = mesh_layout(workspace, d.ncells);
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long t[2] = {0, 0};
    if (d.ncells == 0) {                                        // a box one voxel thin has no cells: nothing queued
        counts_host[0] = counts_host[1] = 0;
        return 0;
    }
    const float* tsdf = vol->planes;
    const float* weight = vol->planes + (size_t)nvox;
    const dim3 block(CUGS_BLOCK);
    hipLaunchKernelGGL(k_mesh_classify, dim3((d.ncells + CUGS_BLOCK - 1) / CUGS_BLOCK), block, 0, st, d, tsdf, weight,
                       min_weight, ws.active);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_count, dim3((unsigned)ws.nchunks), block, 0, st, d, tsdf, ws.active, ws.code, ws.chunk);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_scan2, dim3((unsigned)ws.nl3), block, 0, st, (unsigned)ws.nchunks, ws.chunk, ws.l3);
    CUGS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_scan3, dim3(1), block, 0, st, (unsigned)ws.nl3, ws.l3, ws.totals);
    CUGS_LAUNCH_CHECK();
    CUGS_RETURN_IF_HIP(hipMemcpyAsync(t, ws.totals, sizeof(t), hipMemcpyDeviceToHost, st));
    CUGS_RETURN_IF_HIP(hipStreamSynchronize(st));
    counts_host[0] = (int64_t)t[0];
    counts_host[1] = (int64_t)t[1];
    return 0;
}

extern "C" int cugs_mesh_emit(const cugs_tsdf_volume* vol, void* workspace, size_t workspace_bytes, int64_t num_vertices,
                              int64_t num_faces, float* vertices, float* colors, int32_t* faces, void* stream) {
    if (!volume_ok(vol) || !workspace || num_vertices < 0 || num_faces < 0) return CUGS_EINVAL;
    if ((num_vertices > 0 && !vertices) || (num_faces > 0 && !faces) || (colors && !vol->color)) return CUGS_EINVAL;
    if (voxel_count(vol) < 0) return CUGS_EOVERFLOW;
    if (workspace_bytes < cugs_mesh_workspace_bytes(vol->nx, vol->ny, vol->nz)) return CUGS_EWORKSPACE;
    if (!cugs_aligned16(workspace)) return CUGS_EALIGN;
    const MeshDims d = mesh_dims(vol);
    if (num_vertices > (int64_t)d.ncells || num_faces > 6 * (int64_t)d.ncells) return CUGS_EINVAL;   // not a plan's counts
    if (num_vertices == 0 && num_faces == 0) return 0;
    const MeshWs ws = mesh_layout(workspace, d.ncells);
    TsdfGrid g = {};
    g.ox = vol->origin[0]; g.oy = vol->origin[1]; g.oz = vol->origin[2];
    g.vs = vol->voxel_size; g.trunc = vol->trunc;
    g.nx = vol->nx; g.ny = vol->ny; g.nz = vol->nz;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)ws.nchunks), block(CUGS_BLOCK);
    if (num_vertices > 0) {
        if (colors)
            hipLaunchKernelGGL(k_mesh_vertices<true>, grid, block, 0, st, d, g, vol->planes, ws.code, ws.chunk, ws.l3,
                               (long long)num_vertices, ws.vid, vertices, colors);
        else
            hipLaunchKernelGGL(k_mesh_vertices<false>, grid, block, 0, st, d, g, vol->planes, ws.code, ws.chunk, ws.l3,
                               (long long)num_vertices, ws.vid, vertices, colors);
        CUGS_LAUNCH_CHECK();
    }
    if (num_faces > 0) {
        hipLaunchKernelGGL(k_mesh_faces, grid, block, 0, st, d, vol->planes, ws.code, ws.chunk, ws.l3, (long long)num_faces,
                           ws.vid, faces);
        CUGS_LAUNCH_CHECK();
    }
    return 0;
}
