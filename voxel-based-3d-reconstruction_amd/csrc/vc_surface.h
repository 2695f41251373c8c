// gfx950 kernels of the silhouette-refined surface mesh (vc_surface_mesh; contract in include/voxcarve.h, DESIGN.md section 8
// item 10).  Restated in tests/surface_np.py.
//
// The topology is vc_marching_cubes' own (vc_mc.h) on the occupancy words viewed as (nz, nx, ny): k_mc_count, the two-level
// scans, k_mc_faces.  In between, k_surf_edges walks the crossing masks in k_mc_verts' vertex order and writes one edge entry
// per vertex instead of a position, then
//
//   k_surf_refine   lane = vertex: the ON and OFF voxel centres, the point test at both ends, `steps` bisection rounds along
//                   the edge (each a float64 projection + mask bit per camera until the count is decided), the world position,
//                   and the ON voxel's colour by a binary search of the records (ascending index).  Refined vertices and
//                   camera tests: wave sums, one atomic per wave.
//
// A lane stops testing a point as soon as T >= m or T < m is decided.  Option surface_order (1): the cameras that rejected
// P_off are tried first in every later round (a point near the OFF end usually fails in one of them); 0: camera order.
#pragma once
#include "vc_device.h"
#include "vc_mc.h"

#pragma clang fp contract(off)

namespace vc {

constexpr uint32_t kSurfBlock = 256;
constexpr uint32_t kSurfMaxSteps = 24;

// edge entry of a vertex: element e (the edge's lower element) | axis << 32 | (the lower element is ON) << 34
__device__ __forceinline__ uint64_t surf_edge(uint64_t e, uint32_t axis, bool on_low)
{
    return e | ((uint64_t)axis << 32) | ((uint64_t)(on_low ? 1u : 0u) << 34);
}

// k_mc_verts with an edge entry in place of the vertex position (same word bases, same order; wbase for k_mc_faces)
__global__ __launch_bounds__(kBlock) void k_surf_edges(const McParams p, uint64_t *__restrict__ edges)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = (blockIdx.x * kBlock + threadIdx.x) >> 6;
    if (g >= p.ngroups) return;
    const uint32_t w = g * 64 + lane;
    uint64_t x[3] = {0, 0, 0};
    if (w < p.nwords) { x[0] = p.x[w]; x[1] = p.x[(size_t)p.nwords + w]; x[2] = p.x[2 * (size_t)p.nwords + w]; }
    const uint32_t c = (uint32_t)(__popcll(x[0]) + __popcll(x[1]) + __popcll(x[2]));
    const uint64_t base = p.bvoff[g / kScanBlock] + p.gvoff[g] + (wave_inclusive_scan(c, lane) - c);
    if (w >= p.nwords) return;
    p.wbase[w] = (uint32_t)base;
    if (c == 0) return;
    const uint64_t b = p.bits[w];
    uint64_t id = base;
    for (uint32_t axis = 0; axis < 3; ++axis)
        for (uint64_t m = x[axis]; m; m &= m - 1, ++id) {
            const uint32_t k = (uint32_t)__builtin_ctzll(m);
            if (id < p.vcap) edges[id] = surf_edge(((uint64_t)w << 6) + k, axis, (b >> k) & 1ull);
        }
}

struct SurfParams {
    const uint64_t *edges;          // [V] entries of k_surf_edges
    const uint64_t *records;        // [S] ascending index
    uint64_t S, V;
    const double *xs, *ys, *zs;     // the carve's linspace axes
    const uint32_t *bits;           // [C][mwords] the carve's post-filtered masks
    uint32_t mwords, C, H, W, m, steps, order;
    uint32_t nx, ny;                // element e = (iz nx + ix) ny + iy
    double *verts;                  // [V][3] world x, y, z
    uint8_t *rgb;                   // [V][3]
    uint8_t *refined;               // [V]
    unsigned long long *ctr;        // [2] refined vertices, camera tests
    CamDev cam[kMaxCameras];
};

// T(X, Y, Z) >= m, decided as early as the count allows.  Cameras in `first` are tried before the others; `rej` collects the
// cameras that were tried and rejected the point; `tests` counts the cameras tried.  The camera index is the same in every
// lane of the wave (the loops are uniform; a lane that has decided sits them out), so the parameters stay in scalar registers.
__device__ __forceinline__ bool surf_inside(const SurfParams &p, double X, double Y, double Z, uint32_t first, uint32_t &rej,
                                            uint32_t &tests)
{
    if (p.m > p.C) return false;
    const uint32_t max_fail = p.C - p.m;
    uint32_t pass = 0, fail = 0;
    bool done = false, inside = false;
    for (uint32_t round = 0; round < 2; ++round) {
        for (uint32_t c = 0; c < p.C; ++c) {
            const bool want = (((first >> c) & 1u) != 0) == (round == 0);
            if (done || !want) continue;
            const CamDev &cam = p.cam[c];
            double u, v;
            project_point(cam, X, Y, Z, u, v);
            const int32_t off = pixel_offset(u, v, p.H, p.W);
            const bool ok = off >= 0 && mask_bit(p.bits + (size_t)c * p.mwords, off);
            ++tests;
            if (ok) {
                if (++pass >= p.m) { inside = true; done = true; }
            } else {
                rej |= 1u << c;
                if (++fail > max_fail) done = true;
            }
        }
    }
    return inside;
}

__global__ __launch_bounds__(kSurfBlock) void k_surf_refine(const SurfParams p)
{
    const uint64_t v = (uint64_t)blockIdx.x * kSurfBlock + threadIdx.x;
    uint32_t refined = 0, tests = 0;
    if (v < p.V) {
        const uint64_t ent = p.edges[v];
        const uint32_t e = (uint32_t)ent, axis = (uint32_t)(ent >> 32) & 3u;
        const bool on_low = (ent >> 34) & 1ull;
        // (nz, nx, ny) axes 0, 1, 2 = world z, x, y
        const uint32_t iy = e % p.ny, t = e / p.ny;
        const uint32_t ix = t % p.nx, iz = t / p.nx;
        // the lower element's centre; the edge runs along world axis x (axis 1), y (axis 2) or z (axis 0)
        const double X0 = p.xs[ix], Y0 = p.ys[iy], Z0 = p.zs[iz];
        const bool ex = axis == 1, ey = axis == 2, ez = axis == 0;
        const double upper = ex ? p.xs[ix + 1] : (ey ? p.ys[iy + 1] : p.zs[iz + 1]);
        const double lower = ex ? X0 : (ey ? Y0 : Z0);
        const double a_on = on_low ? lower : upper, a_off = on_low ? upper : lower;
        const double d = a_off - a_on;
        uint32_t rej_on = 0, rej_off = 0;
        const bool in_on = surf_inside(p, ex ? a_on : X0, ey ? a_on : Y0, ez ? a_on : Z0, 0u, rej_on, tests);
        const bool in_off = in_on && surf_inside(p, ex ? a_off : X0, ey ? a_off : Y0, ez ? a_off : Z0, 0u, rej_off, tests);
        double s = 0.5;
        if (in_on && !in_off) {
            refined = 1;
            const uint32_t first = p.order ? rej_off : 0u;
            double lo = 0.0, hi = 1.0;
            for (uint32_t k = 0; k < p.steps; ++k) {
                const double mid = (lo + hi) * 0.5;
                const double q = a_on + mid * d;
                uint32_t unused = 0;
                if (surf_inside(p, ex ? q : X0, ey ? q : Y0, ez ? q : Z0, first, unused, tests)) lo = mid; else hi = mid;
            }
            s = (lo + hi) * 0.5;
        }
        const double q = a_on + s * d;
        p.verts[3 * v] = ex ? q : X0; p.verts[3 * v + 1] = ey ? q : Y0; p.verts[3 * v + 2] = ez ? q : Z0;
        p.refined[v] = (uint8_t)refined;
        // the ON element's record: the first with index >= it (it is a survivor, so the index is equal)
        const uint32_t ion = on_low ? e : e + (axis == 0 ? p.nx * p.ny : (axis == 1 ? p.ny : 1u));
        uint64_t lo = 0, hi = p.S;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((uint32_t)p.records[mid] < ion) lo = mid + 1; else hi = mid;
        }
        const uint64_t rec = lo < p.S ? p.records[lo] : 0ull;
        p.rgb[3 * v] = (uint8_t)(rec >> 32); p.rgb[3 * v + 1] = (uint8_t)(rec >> 40); p.rgb[3 * v + 2] = (uint8_t)(rec >> 48);
    }
    const uint32_t wr = wave_sum_u32(refined), wt = wave_sum_u32(tests);
    if ((threadIdx.x & 63u) == 0 && (wr | wt)) {
        atomicAdd(p.ctr + 0, (unsigned long long)wr);
        atomicAdd(p.ctr + 1, (unsigned long long)wt);
    }
}

}  // namespace vc
