// cugs_tsdf.h — the per-voxel, per-cell and per-edge rules of tsdf.hip as plain functions that the
// kernels call and that a host program can call too: every index these rules form is formed here, so a host build
// under a sanitizer walks the same bounds the GPU will.  No HIP header is needed to include this file.
//
// Every float step is one correctly rounded operation (-ffp-contract=off); tests/tsdf_ref.py mirrors them op for op.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CUGS_HD __host__ __device__ __forceinline__
#else
#define CUGS_HD inline
#endif

#define CUGS_TSDF_MAX_VIEWS 16

// One view of cugs_tsdf_integrate: rows 0..2 of the row-major world-to-camera matrix, the pinhole, the maps.
struct TsdfView {
    float m[12];
    float fx, fy, cx, cy;
    int W, H;
    const float* D;
    const float* A;
    const float* color;     // [H,W,3] or NULL
    const float* weight;    // [H*W] or NULL: all ones
};

struct TsdfGrid {
    float ox, oy, oz, vs, trunc;
    float min_depth, min_alpha, max_weight;
    int nx, ny, nz;
};

// Steps 1-6 of the rule for the voxel (ix, iy, iz) and one view: true when the view touches the voxel, with the
// truncated distance tn, the weight w and the pixel.  Every decision comes before the load that depends on it; no index
// is formed from a value that failed its test.
CUGS_HD bool tsdf_sample(const TsdfGrid& g, const TsdfView& v, int ix, int iy, int iz, float* tn, float* w, size_t* pix) {
    const float px = g.ox + (float)ix * g.vs, py = g.oy + (float)iy * g.vs, pz = g.oz + (float)iz * g.vs;
    const float zc = ((v.m[8] * px + v.m[9] * py) + v.m[10] * pz) + v.m[11];
    if (!(zc > g.min_depth)) return false;
    const float xc = ((v.m[0] * px + v.m[1] * py) + v.m[2] * pz) + v.m[3];
    const float yc = ((v.m[4] * px + v.m[5] * py) + v.m[6] * pz) + v.m[7];
    const float fu = floorf((v.fx * xc) / zc + v.cx), fv = floorf((v.fy * yc) / zc + v.cy);
    // in float: a cast truncates towards zero and would let u in (-1, 0) through; NaN and inf fail
    if (!(fu >= 0.0f && fu < (float)v.W && fv >= 0.0f && fv < (float)v.H)) return false;
    const size_t p = (size_t)(int)fv * (size_t)v.W + (size_t)(int)fu;
    const float a = v.A[p];
    if (!(a > g.min_alpha)) return false;
    const float d = v.D[p] / a;
    const float wv = v.weight ? v.weight[p] : 1.0f;
    if (!(wv > 0.0f)) return false;
    const float sdf = d - zc;
    if (!(sdf >= -g.trunc)) return false;
    *tn = fminf(sdf / g.trunc, 1.0f);
    *w = wv;
    *pix = p;
    return true;
}

// The order the integrate kernel walks the volume in: groups of four x-neighbours, brick by brick.  A brick is
// (4 << lbx) x (1 << lby) x (1 << lbz) voxels (at most 64^3, less where the volume is smaller); groups run x-fastest
// inside a brick and bricks x-fastest over the volume, so the workgroups in flight at any time cover a compact block whose
// projections stay cache-resident in every view (a z-slab would project onto the whole image of each view).  False for
// a group outside the volume (the last brick of an axis may be partial).
struct TsdfWalk {
    unsigned lbx, lby, lbz, bricks_x, bricks_y;
};
CUGS_HD unsigned tsdf_ceil_log2(unsigned n, unsigned cap) {
    unsigned l = 0;
    while (l < cap && (1u << l) < n) ++l;
    return l;
}
CUGS_HD TsdfWalk tsdf_make_walk(int nx, int ny, int nz) {
    TsdfWalk w;
    const unsigned nx4 = ((unsigned)nx + 3u) / 4u;
    w.lbx = tsdf_ceil_log2(nx4, 4u); w.lby = tsdf_ceil_log2((unsigned)ny, 6u); w.lbz = tsdf_ceil_log2((unsigned)nz, 6u);
    w.bricks_x = (nx4 + (1u << w.lbx) - 1u) >> w.lbx;
    w.bricks_y = ((unsigned)ny + (1u << w.lby) - 1u) >> w.lby;
    return w;
}
// Groups in the walk, padding included: at most 8 times the groups of the volume.
CUGS_HD uint64_t tsdf_walk_groups(const TsdfWalk& w, int nz) {
    const uint64_t bricks_z = ((uint64_t)(unsigned)nz + (1u << w.lbz) - 1u) >> w.lbz;
    return ((uint64_t)w.bricks_x * w.bricks_y * bricks_z) << (w.lbx + w.lby + w.lbz);
}
CUGS_HD bool tsdf_group_coords(const TsdfWalk& w, int nx, int ny, int nz, uint64_t gid, int* ix0, int* iy, int* iz) {
    const unsigned bits = w.lbx + w.lby + w.lbz;
    const uint64_t brick = gid >> bits;
    const unsigned r = (unsigned)(gid & ((1ull << bits) - 1ull));
    const unsigned lx = r & ((1u << w.lbx) - 1u), ly = (r >> w.lbx) & ((1u << w.lby) - 1u), lz = r >> (w.lbx + w.lby);
    const unsigned bx = (unsigned)(brick % w.bricks_x);
    const uint64_t t = brick / w.bricks_x;
    const unsigned by = (unsigned)(t % w.bricks_y);
    const uint64_t bz = t / w.bricks_y;
    const uint64_t x = 4ull * (((uint64_t)bx << w.lbx) + lx), y = ((uint64_t)by << w.lby) + ly, z = (bz << w.lbz) + lz;
    if (x >= (uint64_t)nx || y >= (uint64_t)ny || z >= (uint64_t)nz) return false;
    *ix0 = (int)x; *iy = (int)y; *iz = (int)z;
    return true;
}

// Step 7 for one plane: the running weighted mean.  wn = wo + w, formed once by the caller.
CUGS_HD float tsdf_blend(float old_value, float wo, float value, float w, float wn) { return (wo * old_value + w * value) / wn; }

// ---- surface nets ----------------------------------------------------------------------------------------------------
// Corner k of a cell is the voxel at (cx + (k & 1), cy + ((k >> 1) & 1), cz + (k >> 2)).  The twelve edges in their
// fixed order: the four along x (a = 0, 2, 4, 6; b = a + 1), the four along y (a = 0, 1, 4, 5; b = a + 2), the four along
// z (a = 0, 1, 2, 3; b = a + 4).
#define CUGS_MESH_EDGE_A(e) ((e) < 4 ? 2 * (e) : (e) < 8 ? ((e) - 4) + 2 * (((e) - 4) >> 1) : (e) - 8)
#define CUGS_MESH_EDGE_AXIS(e) ((e) >> 2)

CUGS_HD size_t mesh_voxel(int nx, int ny, int x, int y, int z) { return ((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x; }

// A cell is active when all eight corners are valid (weight > min_weight) and their signs (tsdf < 0) differ.  The
// caller guarantees 0 <= c < n - 1 on every axis.
CUGS_HD bool mesh_cell_active(const float* tsdf, const float* weight, int nx, int ny, int cx, int cy, int cz, float min_weight) {
    int neg = 0;
    for (int k = 0; k < 8; ++k) {
        const size_t i = mesh_voxel(nx, ny, cx + (k & 1), cy + ((k >> 1) & 1), cz + (k >> 2));
        if (!(weight[i] > min_weight)) return false;
        neg += tsdf[i] < 0.0f;
    }
    return neg > 0 && neg < 8;
}

// The lattice edge from voxel (x, y, z) to its +axis neighbour belongs to cell (x, y, z).  It gives two triangles when
// its ends differ in sign and the four cells around it exist and are active; `active` is the per-cell byte array
// [(nz-1), (ny-1), (nx-1)].  The caller guarantees that cell (x, y, z) exists and is active.
CUGS_HD bool mesh_edge_faces(const float* tsdf, const uint8_t* active, int nx, int ny, int x, int y, int z, int axis) {
    const int b = (axis + 1) % 3, c = (axis + 2) % 3;            // the other two axes, b x c = axis
    const int p[3] = {x, y, z};
    if (p[b] < 1 || p[c] < 1) return false;                       // on the box boundary: a cell is missing
    int q[3] = {x, y, z};
    q[axis] += 1;
    const bool na = tsdf[mesh_voxel(nx, ny, x, y, z)] < 0.0f, nb = tsdf[mesh_voxel(nx, ny, q[0], q[1], q[2])] < 0.0f;
    if (na == nb) return false;
    const int cnx = nx - 1, cny = ny - 1;
    for (int k = 1; k < 4; ++k) {                                 // k = 0 is the cell itself
        int r[3] = {x, y, z};
        r[b] -= k & 1;
        r[c] -= k >> 1;
        if (!active[mesh_voxel(cnx, cny, r[0], r[1], r[2])]) return false;
    }
    return true;
}

// The four cells around that edge, counter-clockwise seen from +axis: offsets (-1,-1), (0,-1), (0,0), (-1,0) on the
// axes (b, c).  Returned as cell indices, reversed when the edge runs from positive to negative tsdf, so that the
// triangles (q0,q1,q2), (q0,q2,q3) have their normal towards positive tsdf.
CUGS_HD void mesh_edge_quad(const float* tsdf, int nx, int ny, int x, int y, int z, int axis, size_t q[4]) {
    const int b = (axis + 1) % 3, c = (axis + 2) % 3;
    const int ob[4] = {-1, 0, 0, -1}, oc[4] = {-1, -1, 0, 0};
    const bool neg_first = tsdf[mesh_voxel(nx, ny, x, y, z)] < 0.0f;
    for (int k = 0; k < 4; ++k) {
        int r[3] = {x, y, z};
        r[b] += ob[k];
        r[c] += oc[k];
        q[neg_first ? k : 3 - k] = mesh_voxel(nx - 1, ny - 1, r[0], r[1], r[2]);
    }
}

// The vertex of an active cell: the mean of the crossings of its twelve edges, summed in the edge order above, in
// cell-local voxel units, then world = origin + ((float)c + m) * vs.  With colour planes (col != NULL, three planes
// `plane` floats apart) the same interpolation ca + t (cb - ca), averaged the same way.
CUGS_HD void mesh_cell_vertex(const float* tsdf, const float* col, size_t plane, int nx, int ny, int cx, int cy, int cz,
                              float ox, float oy, float oz, float vs, float vert[3], float rgb[3]) {
    float f[8];
    size_t idx[8];
    for (int k = 0; k < 8; ++k) {
        idx[k] = mesh_voxel(nx, ny, cx + (k & 1), cy + ((k >> 1) & 1), cz + (k >> 2));
        f[k] = tsdf[idx[k]];
    }
    float s[3] = {0.0f, 0.0f, 0.0f}, sc[3] = {0.0f, 0.0f, 0.0f};
    int count = 0;
    for (int e = 0; e < 12; ++e) {
        const int axis = CUGS_MESH_EDGE_AXIS(e), a = CUGS_MESH_EDGE_A(e), b = a + (1 << axis);
        const float fa = f[a], fb = f[b];
        if ((fa < 0.0f) == (fb < 0.0f)) continue;
        const float t = fa / (fa - fb);
        for (int k = 0; k < 3; ++k) s[k] = s[k] + (k == axis ? t : (float)((a >> k) & 1));
        if (col) {
            for (int k = 0; k < 3; ++k) {
                const float ca = col[k * plane + idx[a]], cb = col[k * plane + idx[b]];
                sc[k] = sc[k] + (ca + t * (cb - ca));
            }
        }
        ++count;
    }
    const float n = (float)count;
    vert[0] = ox + ((float)cx + s[0] / n) * vs;
    vert[1] = oy + ((float)cy + s[1] / n) * vs;
    vert[2] = oz + ((float)cz + s[2] / n) * vs;
    if (col) { rgb[0] = sc[0] / n; rgb[1] = sc[1] / n; rgb[2] = sc[2] / n; }
}
