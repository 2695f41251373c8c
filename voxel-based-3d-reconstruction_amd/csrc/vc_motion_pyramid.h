// gfx950 kernels of the coarse-to-fine block motion (vc_hull_motion_pyramid; contract in include/voxcarve.h and DESIGN.md section 8
// item 24).  Level 0 is the grid of vc_motion.h; level l has ceil(n / 2) cells per axis of level l - 1, a cell the OR of its up to
// eight children, in the same linear order and word layout.  The coarsest level is matched by k_motion_match; every finer level by
// k_motion_refine, which tries only the displacements around twice the vector of the parent block and of its listed face neighbours.
// Integers and bits only; restated in tests/motion_pyramid_np.py.
//
//   k_motion_halve   lane = word of the coarser level: per y-segment of at most 32 cells inside the word, the two source rows of
//                    the four (x, z) source lines ORed, neighbouring bits ORed, the even bits compressed
//   k_motion_refine  workgroup = listed block: the block's centres into LDS (lane 0, each distinct centre once), A's window into
//                    LDS once, per centre the (W + 2r)^2 rows of B's region around it; lanes own displacements (dy fastest); a
//                    displacement counts for the first centre whose cube holds it; argmin over a 64-bit key, ties and the number
//                    of displacements tried by LDS atomics
// Every word index is checked against its level's nwords (motion_row does), every block against its level's nblocks.
#pragma once
#include "vc_motion.h"

namespace vc {

constexpr uint32_t kPyramidMaxLevels = 3;
constexpr uint32_t kPyramidCentres = 7;                      // the parent and its six face neighbours
// the counters of a refined level, behind the five of kMotionCounters in the same array of 8
constexpr uint32_t kPyramidOrphans = 5, kPyramidEvaluated = 6, kPyramidBorrowed = 7;
constexpr uint32_t kMotionBorrowed = 2;                      // flags bit 1 of a row

struct MotionHalveParams {
    const uint64_t *src;        // the words of level l - 1
    uint64_t *dst;              // [g.nwords] the words of level l
    MotionGrid gs, g;           // the grids of level l - 1 and of level l (nx, ny, nz, n, nwords)
};

__global__ __launch_bounds__(kMotionBlock) void k_motion_halve(const MotionHalveParams p)
{
    const uint64_t w = (uint64_t)blockIdx.x * kMotionBlock + threadIdx.x;
    if (w >= p.g.nwords) return;
    const uint64_t lo = w << 6, hi = min(lo + 64u, p.g.n);
    uint64_t out = 0, pos = lo;
    while (pos < hi) {
        uint32_t ix, iy, iz;
        decompose((uint32_t)pos, p.g.nx, p.g.ny, ix, iy, iz);
        // the rest of the line, of the word, and of what two source rows of 64 bits give
        const uint32_t len = (uint32_t)min(min((uint64_t)(p.g.ny - iy), hi - pos), (uint64_t)32u);
        uint64_t v = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)                          // (lines off the source grid are empty: motion_row)
            v |= motion_row(p.src, p.gs, (int32_t)(2u * ix + (j & 1u)), (int32_t)(2u * iy), (int32_t)(2u * iz + (j >> 1)), 2u * len);
        v = (v | (v >> 1)) & 0x5555555555555555ull;              // bit 2j = cells 2j and 2j + 1
        v = (v | (v >> 1)) & 0x3333333333333333ull;
        v = (v | (v >> 2)) & 0x0f0f0f0f0f0f0f0full;
        v = (v | (v >> 4)) & 0x00ff00ff00ff00ffull;
        v = (v | (v >> 8)) & 0x0000ffff0000ffffull;
        v = (v | (v >> 16)) & 0x00000000ffffffffull;
        out |= v << (uint32_t)(pos - lo);                        // pos - lo + len <= 64
        pos += len;
    }
    p.dst[w] = out;
}

struct MotionRefineParams {
    const uint64_t *a, *b;      // the words of this level
    MotionGrid g;               // this level's grid and blocks (g.s is the coarsest level's search range, not used here)
    uint32_t r;                 // the refine radius
    MotionRow *rows;            // [listed]: block, count_a and count_b are there
    uint64_t listed;
    uint32_t *vec;              // [g.nblocks], zeroed: the vector of each listed block (kMotionListed)
    const uint32_t *pvec;       // [pnblocks]: the vectors of the next coarser level
    uint32_t pnbx, pnby, pnbz, pnblocks;
    unsigned long long *ctr;    // [8], zeroed: kMotionCounters, then orphans, evaluated, borrowed
};

// key of a displacement: the smallest wins.  cost < 2^17 (48^3 cells), |d - c|^2 <= 3 * 240^2 < 2^18, the components of d
// (|d| <= 120) biased by 128 in the order (dz, dx, dy)
__device__ __forceinline__ unsigned long long refine_key(uint32_t cost, uint32_t d2, int32_t dx, int32_t dy, int32_t dz)
{
    return ((unsigned long long)cost << 42) | ((unsigned long long)d2 << 24) | ((unsigned long long)(uint32_t)(dz + 128) << 16) |
           ((unsigned long long)(uint32_t)(dx + 128) << 8) | (unsigned long long)(uint32_t)(dy + 128);
}

__device__ __forceinline__ bool refine_in_cube(int32_t dx, int32_t dy, int32_t dz, int32_t ex, int32_t ey, int32_t ez, int32_t r)
{
    return abs(dx - ex) <= r && abs(dy - ey) <= r && abs(dz - ez) <= r;
}

// dynamic LDS: R^2 rows of B's region around one centre, then W^2 rows of A's window (R = b + 2a + 2r <= 64, W = b + 2a <= 48)
__global__ __launch_bounds__(kMotionBlock) void k_motion_refine(const MotionRefineParams p)
{
    extern __shared__ uint64_t s_rows[];
    __shared__ unsigned long long s_best;
    __shared__ uint32_t s_ties, s_cost0, s_eval, s_nc, s_orphan;
    __shared__ int32_t s_c[kPyramidCentres][3];
    const uint64_t rk = blockIdx.x;
    if (rk >= p.listed) return;                                  // (the whole workgroup)
    const uint32_t k = p.rows[rk].block;
    if (k >= p.g.nblocks) return;
    const uint32_t b = p.g.b, a = p.g.a;
    const int32_t r = (int32_t)p.r;
    const uint32_t W = b + 2u * a, R = W + 2u * p.r, side = 2u * p.r + 1u, nd = side * side * side;
    const uint32_t by = k % p.g.nby, t = k / p.g.nby, bx = t % p.g.nbx, bz = t / p.g.nbx;
    const int32_t ox = (int32_t)(bx * b) - (int32_t)a, oy = (int32_t)(by * b) - (int32_t)a, oz = (int32_t)(bz * b) - (int32_t)a;
    uint64_t *s_b = s_rows, *s_a = s_rows + R * R;
    if (threadIdx.x == 0) {
        s_best = ~0ull; s_ties = 0; s_cost0 = 0; s_eval = 0;
        // the centres: twice the vector of the parent and of its listed face neighbours, each distinct one once, the prediction first
        const int32_t px = (int32_t)(bx >> 1), py = (int32_t)(by >> 1), pz = (int32_t)(bz >> 1);
        uint32_t nc = 0, orphan = 0;
        for (uint32_t j = 0; j < kPyramidCentres; ++j) {
            const int32_t ax = (int32_t)((j + 1u) >> 1) - 1;      // 0: the parent; 1, 2: +x, -x; 3, 4: +y, -y; 5, 6: +z, -z
            const int32_t sg = j == 0 ? 0 : ((j & 1u) ? 1 : -1);
            const int32_t qx = px + (ax == 0 ? sg : 0), qy = py + (ax == 1 ? sg : 0), qz = pz + (ax == 2 ? sg : 0);
            uint32_t v = 0;
            if (qx >= 0 && qy >= 0 && qz >= 0 && qx < (int32_t)p.pnbx && qy < (int32_t)p.pnby && qz < (int32_t)p.pnbz) {
                const uint32_t pk = ((uint32_t)qz * p.pnbx + (uint32_t)qx) * p.pnby + (uint32_t)qy;
                if (pk < p.pnblocks) v = p.pvec[pk];
            }
            if (j == 0 && !(v & kMotionListed)) { orphan = 1; v = kMotionListed; }    // cannot be (contract item 4): counted, d = 0
            if (!(v & kMotionListed)) continue;
            const int32_t ex = 2 * motion_byte(v, 0), ey = 2 * motion_byte(v, 1), ez = 2 * motion_byte(v, 2);
            bool seen = false;
            for (uint32_t i = 0; i < nc; ++i) seen |= s_c[i][0] == ex && s_c[i][1] == ey && s_c[i][2] == ez;
            if (seen) continue;
            s_c[nc][0] = ex; s_c[nc][1] = ey; s_c[nc][2] = ez;   // nc < kPyramidCentres: at most one per j
            ++nc;
        }
        for (uint32_t i = nc; i < kPyramidCentres; ++i) s_c[i][0] = s_c[i][1] = s_c[i][2] = 0;
        s_nc = nc; s_orphan = orphan;
    }
    for (uint32_t i = threadIdx.x; i < W * W; i += kMotionBlock) {
        const uint32_t wz = i / W, wx = i - wz * W;
        s_a[i] = motion_row(p.a, p.g, ox + (int32_t)wx, oy, oz + (int32_t)wz, W);
    }
    __syncthreads();
    const uint32_t nc = s_nc;                                    // 1..7
    int32_t ex[kPyramidCentres], ey[kPyramidCentres], ez[kPyramidCentres];
    bool zero_in = false;
#pragma unroll
    for (uint32_t j = 0; j < kPyramidCentres; ++j) {
        ex[j] = s_c[j][0]; ey[j] = s_c[j][1]; ez[j] = s_c[j][2];
        zero_in |= j < nc && refine_in_cube(0, 0, 0, ex[j], ey[j], ez[j], r);
    }
    const uint64_t wmask = cc_below(W);                          // W <= 48
    const uint32_t npass = nc + (zero_in ? 0u : 1u);             // d = 0 has a pass of its own when no cube holds it (cost0)
    // a small cube leaves most lanes without a displacement (r = 1: 27 of 256): then `parts` lanes share one, each a part of the
    // window's z layers -- the largest power of two with parts * nd <= kMotionBlock, at most 64 and at most W
    uint32_t parts = 1;
    while (parts < 64u && 2u * parts * nd <= kMotionBlock && 2u * parts <= W) parts *= 2u;
    const uint32_t per = kMotionBlock / parts;                   // displacements per round (>= nd when parts > 1)
    unsigned long long best = ~0ull;
    uint32_t mincost = 0xffffffffu, mincnt = 0, neval = 0;
    for (uint32_t i = 0; i < npass; ++i) {                       // (workgroup-uniform)
        const bool extra = i >= nc;
        const int32_t qx = extra ? 0 : s_c[i][0], qy = extra ? 0 : s_c[i][1], qz = extra ? 0 : s_c[i][2];
        if (i) __syncthreads();                                  // the last pass is done with B's region
        for (uint32_t j = threadIdx.x; j < R * R; j += kMotionBlock) {
            const uint32_t rz = j / R, rx = j - rz * R;
            s_b[j] = motion_row(p.b, p.g, ox - qx - r + (int32_t)rx, oy - qy - r, oz - qz - r + (int32_t)rz, R);
        }
        __syncthreads();
        for (uint32_t base = 0; base < nd; base += per) {        // (workgroup-uniform: one round when a displacement has several lanes)
            const uint32_t o = base + threadIdx.x / parts, part = threadIdx.x & (parts - 1u);
            const uint32_t uy = o % side, q = o / side, ux = q % side, uz = q / side;     // u = d - centre + r
            const int32_t dx = qx + (int32_t)ux - r, dy = qy + (int32_t)uy - r, dz = qz + (int32_t)uz - r;
            bool dup = false;                                    // an earlier centre's cube holds it: counted there
#pragma unroll
            for (uint32_t j = 0; j + 1 < kPyramidCentres; ++j) dup |= j < i && refine_in_cube(dx, dy, dz, ex[j], ey[j], ez[j], r);
            const bool mine = o < nd && (extra ? !(dx | dy | dz) : !dup);
            uint32_t cost = 0;
            if (mine) {
                // the cell (wx, wy, wz) of the window looks at (wx + 2r - ux, ..) of the region; this lane's share of the z layers
                const uint32_t shx = 2u * p.r - ux, shy = 2u * p.r - uy, shz = 2u * p.r - uz;  // 0 .. 2r
                for (uint32_t wz = part; wz < W; wz += parts) {
                    const uint64_t *rb = s_b + (wz + shz) * R + shx;
                    const uint64_t *ra = s_a + wz * W;
                    for (uint32_t wx = 0; wx < W; ++wx) cost += (uint32_t)__popcll((ra[wx] ^ (rb[wx] >> shy)) & wmask);
                }
            }
            // the lanes of a displacement are neighbours in a wave (parts is a power of two, at most 64): their shares add up in each
            for (uint32_t m = parts >> 1; m; m >>= 1) cost += (uint32_t)__shfl_xor((int)cost, (int)m);
            if (!mine || part) continue;
            if (!(dx | dy | dz)) s_cost0 = cost;                 // (one lane of one pass)
            if (extra) continue;
            ++neval;
            const int32_t fx = dx - ex[0], fy = dy - ey[0], fz = dz - ez[0];
            const unsigned long long key = refine_key(cost, (uint32_t)(fx * fx + fy * fy + fz * fz), dx, dy, dz);
            best = key < best ? key : best;
            if (cost < mincost) { mincost = cost; mincnt = 1; }
            else if (cost == mincost) ++mincnt;
        }
    }
    if (best != ~0ull) atomicMin(&s_best, best);
    if (neval) atomicAdd(&s_eval, neval);
    __syncthreads();
    const unsigned long long win = s_best;
    const uint32_t wcost = (uint32_t)(win >> 42);
    if (mincnt && mincost == wcost) atomicAdd(&s_ties, mincnt);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int32_t dx = (int32_t)((win >> 8) & 0xffu) - 128, dy = (int32_t)(win & 0xffu) - 128, dz = (int32_t)((win >> 16) & 0xffu) - 128;
    // bit 0: a face neighbour of the winner was not tried; bit 1: the winner lies outside the prediction's own cube
    bool clipped = false;
#pragma unroll
    for (uint32_t f = 0; f < 6; ++f) {
        const int32_t sg = (f & 1u) ? -1 : 1;
        const int32_t nx = dx + (f < 2 ? sg : 0), ny = dy + (f >= 2 && f < 4 ? sg : 0), nz = dz + (f >= 4 ? sg : 0);
        bool in = false;
#pragma unroll
        for (uint32_t j = 0; j < kPyramidCentres; ++j) in |= j < nc && refine_in_cube(nx, ny, nz, ex[j], ey[j], ez[j], r);
        clipped |= !in;
    }
    const bool borrowed = !refine_in_cube(dx, dy, dz, ex[0], ey[0], ez[0], r);
    const uint32_t ties = s_ties;                                // <= 7 * 17^3 < 2^16
    MotionRow row = p.rows[rk];
    row.d[0] = (int8_t)dx; row.d[1] = (int8_t)dy; row.d[2] = (int8_t)dz;
    row.flags = (uint8_t)((clipped ? 1u : 0u) | (borrowed ? kMotionBorrowed : 0u));
    row.cost = wcost; row.cost0 = s_cost0;
    row.ties = (uint16_t)ties;
    p.rows[rk] = row;
    p.vec[k] = ((uint32_t)dx & 0xffu) | (((uint32_t)dy & 0xffu) << 8) | (((uint32_t)dz & 0xffu) << 16) | kMotionListed;
    if (dx | dy | dz) atomicAdd(p.ctr + 0, 1ull);
    if (ties == 1u) atomicAdd(p.ctr + 1, 1ull);
    if (clipped) atomicAdd(p.ctr + 2, 1ull);
    if (s_cost0) atomicAdd(p.ctr + 3, (unsigned long long)s_cost0);
    if (wcost) atomicAdd(p.ctr + 4, (unsigned long long)wcost);
    if (s_orphan) atomicAdd(p.ctr + kPyramidOrphans, 1ull);
    atomicAdd(p.ctr + kPyramidEvaluated, (unsigned long long)s_eval);
    if (borrowed) atomicAdd(p.ctr + kPyramidBorrowed, 1ull);
}

}  // namespace vc
