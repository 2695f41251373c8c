// gfx950 kernels of the ray caster (vc_render; contract in include/voxcarve.h): images of the
// current carve result from any pinhole camera with the 5-coefficient lens model.  Restated in tests/render_np.py (walk_voxels
// is the contract's walk, walk_blocks the block-skipping walk below).
//
//   k_render_map   lane = block of 8^3 voxels (linear block index (bz nbx + bx) nby + by): ORs the block's 64 column segments
//                  of 8 bits out of the occupancy words; a wave's 64 block bits are one map word (ballot), written by lane 0.
//                  No atomics: the map word of a wave is the wave's alone.
//   k_render       wave = 8 x 8 pixel tile, lane = pixel: the ray (float64, the contract's operation order), its slab entry,
//                  then the walk.  A cell of a block with survivors takes one voxel step; an empty block is left in one step
//                  by its (t, axis)-least boundary event, every other axis advancing past its own events before that one
//                  (each axis's events are non-decreasing in t, so the voxel walk takes all events in (t, axis) order, and
//                  inside an empty block it can only end at the block's exit).  A hit's colour comes from a binary search of
//                  the records (ascending index).  Hits, cells looked at and blocks skipped: wave sums, one atomic per wave.
// The ray, the entry and the walk are functions of their own (rpixel, rentry, rwalk): vc_texture.h takes the ray, vc_light.h all
// three for its secondary rays.
#pragma once
#include "vc_kernels.h"          // wave_sum_u32

#pragma clang fp contract(off)

namespace vc {

constexpr uint32_t kRenderBlock = 256;       // 4 waves, an 8 x 8 pixel tile each
constexpr uint32_t kRenderShift = 3;         // skip blocks of 8^3 voxels
constexpr uint32_t kRenderB = 1u << kRenderShift;
constexpr uint32_t kRenderMiss = 0xFFFFFFFFu;

struct RenderView {                          // = vc_view_t
    double K[4], dist[5], R[9], t[3];
};

struct RenderParams {
    const uint64_t *words;                   // occupancy of the current result (dense)
    const uint64_t *bmap;                    // block map, bit per 8^3 block
    const uint64_t *records;                 // [S] ascending index
    uint64_t S;
    const RenderView *views;                 // [V]
    uint32_t *idx;                           // [V H W]
    float *depth;                            // [V H W]
    uint32_t *rgbf;                          // [V H W] R | G << 8 | B << 16 | face << 24
    unsigned long long *ctr;                 // [3] hits, cells looked at, blocks skipped
    double e[3], s[3];                       // b(k) = e + (double)k s
    uint32_t n[3];                           // nx, ny, nz
    uint32_t nb[3];                          // blocks per axis
    uint32_t H, W, tiles_x, tiles_per_view, n_tiles;
    uint32_t shade[7];
    uint32_t bg;                             // R | G << 8 | B << 16
    uint32_t skip;                           // 1: skip empty blocks (same results)
};

__global__ __launch_bounds__(kRenderBlock) void k_render_map(const uint64_t *__restrict__ words, uint64_t *__restrict__ bmap,
                                                             uint32_t nx, uint32_t ny, uint32_t nz, uint32_t nbx, uint32_t nby,
                                                             uint64_t nblocks)
{
    const uint64_t lb = (uint64_t)blockIdx.x * kRenderBlock + threadIdx.x;
    bool any = false;
    if (lb < nblocks) {
        const uint32_t by = (uint32_t)(lb % nby);
        const uint64_t r = lb / nby;
        const uint32_t bx = (uint32_t)(r % nbx), bz = (uint32_t)(r / nbx);
        const uint32_t y0 = by * kRenderB, L = min(kRenderB, ny - y0);
        const uint32_t x1 = min(bx * kRenderB + kRenderB, nx), z1 = min(bz * kRenderB + kRenderB, nz);
        const uint64_t m = (1ull << L) - 1ull;
        for (uint32_t z = bz * kRenderB; z < z1 && !any; ++z)
            for (uint32_t x = bx * kRenderB; x < x1 && !any; ++x) {
                const uint64_t i0 = ((uint64_t)z * nx + x) * ny + y0;
                const uint64_t w0 = i0 >> 6;
                const uint32_t sh = (uint32_t)(i0 & 63);
                uint64_t v = words[w0] >> sh;
                if (sh + L > 64) v |= words[w0 + 1] << (64 - sh);      // the segment's bits run into the next word (which exists)
                any = (v & m) != 0;
            }
    }
    const uint64_t bits = __ballot(any);
    const uint64_t w = lb >> 6;
    if ((threadIdx.x & 63) == 0 && w < (nblocks + 63) / 64) bmap[w] = bits;
}

// One axis of a ray's walk.
struct RAxis {
    double o, d, inv, e, s, tn;
    int32_t c, n;
    bool up;
};

__device__ __forceinline__ double rb(const RAxis &a, int32_t k) { return a.e + (double)k * a.s; }

__device__ __forceinline__ double rnext(const RAxis &a)
{
    return a.d != 0.0 ? (rb(a, a.c + (a.up ? 1 : 0)) - a.o) * a.inv : __builtin_inf();
}

// Item 3 for one axis: slab parameters (or the miss test of a parallel axis).
__device__ __forceinline__ void rslab(const RAxis &a, double &near, double &far, bool &miss)
{
    if (a.d != 0.0) {
        const double ta = (rb(a, 0) - a.o) * a.inv, tb = (rb(a, a.n) - a.o) * a.inv;
        near = ta < tb ? ta : tb;
        far = ta < tb ? tb : ta;
    } else {
        near = -__builtin_inf();
        far = __builtin_inf();
        if (a.o < rb(a, 0) || a.o >= rb(a, a.n)) miss = true;
    }
}

__device__ __forceinline__ int32_t rcell(const RAxis &a, double t_in)
{
    const double f = floor(((a.o + t_in * a.d) - a.e) / a.s);
    return f >= 0.0 ? (f <= (double)(a.n - 1) ? (int32_t)f : a.n - 1) : 0;
}

// An empty block's exit event on axis a: the block boundary in the direction of travel (boundary index kb, parameter tb).
__device__ __forceinline__ void rexit(const RAxis &a, int32_t &kb, double &tb)
{
    const int32_t lo = (a.c >> kRenderShift) << kRenderShift;
    kb = a.up ? min(lo + (int32_t)kRenderB, a.n) : lo;
    tb = a.d != 0.0 ? (rb(a, kb) - a.o) * a.inv : __builtin_inf();
}

// Axis `ax` (not the exit axis xa) past each of its own events that comes before the exit event (xt, xa) in (t, axis) order.
__device__ __forceinline__ void radvance(RAxis &a, int ax, double xt, int xa)
{
    for (uint32_t k = 0; k < kRenderB && ax != xa && (a.tn < xt || (a.tn == xt && ax < xa)); ++k) {
        a.c += a.up ? 1 : -1;
        a.tn = rnext(a);
    }
}

__device__ __forceinline__ bool rinside(const RAxis &a) { return a.c >= 0 && a.c < a.n; }

// Item 2: origin and direction of the ray of pixel (u, v) of a view.
__device__ __forceinline__ void rpixel(const RenderView &vw, uint32_t u, uint32_t v, double &o0, double &o1, double &o2,
                                       double &d0, double &d1, double &d2)
{
    const double fx = vw.K[0], fy = vw.K[1], cx = vw.K[2], cy = vw.K[3];
    const double k1 = vw.dist[0], k2 = vw.dist[1], p1 = vw.dist[2], p2 = vw.dist[3], k3 = vw.dist[4];
    const double xd = (((double)u + 0.5) - cx) / fx, yd = (((double)v + 0.5) - cy) / fy;
    double x = xd, y = yd;
    for (int it = 0; it < 8; ++it) {
        const double r2 = x * x + y * y;
        const double cd = ((1.0 + k1 * r2) + (k2 * r2) * r2) + ((k3 * r2) * r2) * r2;
        const double dx = ((2.0 * p1) * x) * y + p2 * (r2 + (2.0 * x) * x);
        const double dy = p1 * (r2 + (2.0 * y) * y) + ((2.0 * p2) * x) * y;
        x = (xd - dx) / cd;
        y = (yd - dy) / cd;
    }
    const double *R = vw.R, *t = vw.t;
    d0 = (x * R[0] + y * R[3]) + R[6];
    d1 = (x * R[1] + y * R[4]) + R[7];
    d2 = (x * R[2] + y * R[5]) + R[8];
    o0 = -((R[0] * t[0] + R[3] * t[1]) + R[6] * t[2]);
    o1 = -((R[1] * t[0] + R[4] * t[1]) + R[7] * t[2]);
    o2 = -((R[2] * t[0] + R[5] * t[1]) + R[8] * t[2]);
}

// The rest of an axis once o and d are set: the grid's boundaries (item 1) and the direction's inverse and sign.
__device__ __forceinline__ void raxis(RAxis &a, double e, double s, uint32_t n)
{
    a.e = e; a.s = s; a.n = (int32_t)n;
    a.inv = a.d != 0.0 ? 1.0 / a.d : 0.0;
    a.up = a.d > 0.0;
}

// Item 3: the slab entry of a ray whose axes hold o, d, inv, e, s, n, up.  True: the ray misses the grid.  Otherwise t_in, the
// axis of entry (-1: the ray starts inside), and every axis's cell and next boundary parameter.
__device__ __forceinline__ bool rentry(RAxis &A0, RAxis &A1, RAxis &A2, double &t_in, int &ax)
{
    bool miss = false;
    double n0, f0, n1, f1, n2, f2;
    rslab(A0, n0, f0, miss);
    rslab(A1, n1, f1, miss);
    rslab(A2, n2, f2, miss);
    double t_out = __builtin_inf();
    t_in = 0.0;
    if (n0 > t_in) t_in = n0;
    if (n1 > t_in) t_in = n1;
    if (n2 > t_in) t_in = n2;
    if (f0 < t_out) t_out = f0;
    if (f1 < t_out) t_out = f1;
    if (f2 < t_out) t_out = f2;
    if (t_in >= t_out) miss = true;
    ax = -1;
    if (miss) return true;
    if (t_in > 0.0) ax = n0 == t_in ? 0 : (n1 == t_in ? 1 : (n2 == t_in ? 2 : -1));
    A0.c = ax == 0 ? (A0.up ? 0 : A0.n - 1) : rcell(A0, t_in);
    A1.c = ax == 1 ? (A1.up ? 0 : A1.n - 1) : rcell(A1, t_in);
    A2.c = ax == 2 ? (A2.up ? 0 : A2.n - 1) : rcell(A2, t_in);
    A0.tn = rnext(A0); A1.tn = rnext(A1); A2.tn = rnext(A2);
    return false;
}

// Item 4: the walk from the cells the axes hold (inside the grid, tn set).  True on a hit: oidx its linear index, tt the
// parameter and ax the axis of the step that entered it (both left as given when the first cell is the hit).  skip: empty
// blocks of 8^3 voxels are left in one step (bmap; the same results).  cells, skips: cells looked at, blocks skipped (added).
// t_stop: the walk gives up (no hit) once a step has taken its parameter to t_stop or beyond.  From the first step on tt never
// decreases (each axis's events are non-decreasing and every step takes the least), so a caller that only asks for hits with
// t < t_stop loses none; the starting cell is looked at whatever tt it is given.  +inf walks to the end -- unless a step takes
// tt itself to +inf, which needs all three tn at +inf: no direction of a validated view or light gets there.
__device__ __forceinline__ bool rwalk(const uint64_t *__restrict__ words, const uint64_t *__restrict__ bmap, uint32_t skip,
                                      const uint32_t (&n)[3], const uint32_t (&nb)[3], RAxis &A0, RAxis &A1, RAxis &A2,
                                      double &tt, int &ax, uint32_t &oidx, uint32_t &cells, uint32_t &skips, double t_stop)
{
    const uint64_t nx = n[0], ny = n[1], nbx = nb[0], nby = nb[1];
    uint64_t cw = ~0ull, cword = 0, cbw = ~0ull, cbword = 0;   // the occupancy / map word in hand
    bool hit = false;
    // every iteration moves an axis one way for good: at most nx + ny + nz of them
    const uint32_t limit = n[0] + n[1] + n[2] + 1;
    for (uint32_t guard = 0; guard < limit; ++guard) {
        bool full = true;
        if (skip) {
            const uint64_t lb = ((uint64_t)(A2.c >> kRenderShift) * nbx + (uint64_t)(A0.c >> kRenderShift)) * nby +
                                (uint64_t)(A1.c >> kRenderShift);
            if ((lb >> 6) != cbw) { cbw = lb >> 6; cbword = bmap[cbw]; }
            full = (cbword >> (lb & 63)) & 1ull;
        }
        if (full) {
            ++cells;
            const uint64_t lin = ((uint64_t)A2.c * nx + (uint64_t)A0.c) * ny + (uint64_t)A1.c;
            if ((lin >> 6) != cw) { cw = lin >> 6; cword = words[cw]; }
            if ((cword >> (lin & 63)) & 1ull) {
                hit = true;
                oidx = (uint32_t)lin;
                break;
            }
            int best = 0;
            double bt = A0.tn;
            if (A1.tn < bt) { best = 1; bt = A1.tn; }
            if (A2.tn < bt) { best = 2; bt = A2.tn; }
            tt = bt;
            ax = best;
            if (best == 0) { A0.c += A0.up ? 1 : -1; A0.tn = rnext(A0); }
            else if (best == 1) { A1.c += A1.up ? 1 : -1; A1.tn = rnext(A1); }
            else { A2.c += A2.up ? 1 : -1; A2.tn = rnext(A2); }
        } else {
            ++skips;
            int32_t k0, k1b, k2b;
            double b0, b1, b2;
            rexit(A0, k0, b0);
            rexit(A1, k1b, b1);
            rexit(A2, k2b, b2);
            int xa = 0;
            double xt = b0;
            if (b1 < xt) { xa = 1; xt = b1; }
            if (b2 < xt) { xa = 2; xt = b2; }
            radvance(A0, 0, xt, xa);
            radvance(A1, 1, xt, xa);
            radvance(A2, 2, xt, xa);
            if (xa == 0) { A0.c = A0.up ? k0 : k0 - 1; A0.tn = rnext(A0); }
            else if (xa == 1) { A1.c = A1.up ? k1b : k1b - 1; A1.tn = rnext(A1); }
            else { A2.c = A2.up ? k2b : k2b - 1; A2.tn = rnext(A2); }
            tt = xt;
            ax = xa;
        }
        if (!rinside(A0) || !rinside(A1) || !rinside(A2) || tt >= t_stop) break;
    }
    return hit;
}

__global__ __launch_bounds__(kRenderBlock) void k_render(const RenderParams p)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t tile = blockIdx.x * (kRenderBlock / 64) + (threadIdx.x >> 6);
    uint32_t hits = 0, cells = 0, skips = 0;
    if (tile < p.n_tiles) {
        const uint32_t view = tile / p.tiles_per_view, tr = tile % p.tiles_per_view;
        const uint32_t u = (tr % p.tiles_x) * 8 + (lane & 7), v = (tr / p.tiles_x) * 8 + (lane >> 3);
        if (u < p.W && v < p.H) {
            // 2 the pixel ray
            RAxis A0, A1, A2;
            rpixel(p.views[view], u, v, A0.o, A1.o, A2.o, A0.d, A1.d, A2.d);
            raxis(A0, p.e[0], p.s[0], p.n[0]);
            raxis(A1, p.e[1], p.s[1], p.n[1]);
            raxis(A2, p.e[2], p.s[2], p.n[2]);
            // 3 entry, 4 the walk
            uint32_t oidx = kRenderMiss, orgbf = p.bg | (255u << 24);
            float odepth = __builtin_inff();
            double tt = 0.0;
            int ax = -1;                                                 // axis of entry / of the last step; -1: started inside
            if (!rentry(A0, A1, A2, tt, ax)) {
                const bool hit = rwalk(p.words, p.bmap, p.skip, p.n, p.nb, A0, A1, A2, tt, ax, oidx, cells, skips, __builtin_inf());
                if (hit) {
                    hits = 1;
                    const bool pos = ax == 0 ? A0.up : (ax == 1 ? A1.up : A2.up);
                    const uint32_t face = ax < 0 ? 6u : 2u * (uint32_t)ax + (pos ? 0u : 1u);
                    odepth = (float)tt;
                    uint64_t lo = 0, hi = p.S;                            // the first record with index >= oidx
                    while (lo < hi) {
                        const uint64_t mid = (lo + hi) >> 1;
                        if ((uint32_t)p.records[mid] < oidx) lo = mid + 1; else hi = mid;
                    }
                    const uint64_t rec = lo < p.S ? p.records[lo] : 0ull;
                    const uint32_t sh = p.shade[face];
                    const uint32_t r = (((uint32_t)(rec >> 32) & 255u) * sh + 127u) / 255u;
                    const uint32_t g = (((uint32_t)(rec >> 40) & 255u) * sh + 127u) / 255u;
                    const uint32_t b = (((uint32_t)(rec >> 48) & 255u) * sh + 127u) / 255u;
                    orgbf = r | (g << 8) | (b << 16) | (face << 24);
                } else {
                    oidx = kRenderMiss;
                }
            }
            const uint64_t o = ((uint64_t)view * p.H + v) * p.W + u;
            p.idx[o] = oidx;
            p.depth[o] = odepth;
            p.rgbf[o] = orgbf;
        }
    }
    // every lane of the wave is here (the branches above have joined): wave sums, one atomic each from lane 0
    const uint32_t wh = wave_sum_u32(hits), wc = wave_sum_u32(cells), ws = wave_sum_u32(skips);
    if (lane == 0 && (wh | wc | ws)) {
        atomicAdd(p.ctr + 0, (unsigned long long)wh);
        atomicAdd(p.ctr + 1, (unsigned long long)wc);
        atomicAdd(p.ctr + 2, (unsigned long long)ws);
    }
}

}  // namespace vc
