// gfx950 kernels of the block motion between two hulls (vc_hull_motion, vc_hull_warp, vc_paint_motion; contract in
// include/voxcarve.h and DESIGN.md section 8 item 24).  A is the current result's occupancy, B a kept hull's: the linear bit arrays of
// vc_fetch_occupancy, 64 voxels per word along y.  The grid is cut into cubes of b^3 voxels, block k = (bz NBx + bx) NBy + by.
// Integers and bits only; restated in tests/motion_np.py.
//
//   k_motion_list    lane = block: the voxels of A and of B in its b^3 cells (rows of b bits, clipped to the grid); a wave's ballot
//                    of the blocks that hold any is the group's mask, its popcount the group's count (scan_counts ranks them)
//   k_motion_rank    lane = block: a listed block's row at its rank (block, count_a, count_b), ascending k
//   k_motion_match   workgroup = listed block: the (b + 2a + 2s)^2 rows of B's search region and the (b + 2a)^2 rows of A's window
//                    into LDS, one 64-bit word each; lanes own displacements (dy fastest, so neighbours read the same row of B); a
//                    y displacement is a shift of the row, x and z displacements pick other rows; the argmin over the key
//                    (cost, |d|^2, order) and the count of the displacements at the smallest cost by LDS atomics
//   k_motion_warp    lane = word of the prediction: per y-segment of a block inside the word, B's bits moved by the block's vector
//   k_motion_paint   lane = record: RGB from its block's vector
// Every word index is checked against nwords before it is used, every block against nblocks, every rank against the list.
#pragma once
#include "vc_setops.h"           // kSetopBlock, setop_sums, tp_pop (vc_temporal.h), cc_below (vc_components.h), decompose

namespace vc {

constexpr uint32_t kMotionBlock = 256;
constexpr uint32_t kMotionCounters = 5;                      // moved, unique, clipped, cost0_sum, cost_sum
constexpr uint32_t kWarpCounters = 2;                        // |P|, |P & A|
constexpr uint32_t kMotionListed = 0x01000000u;              // vec[k]: dx | dy << 8 | dz << 16 (two's complement bytes) | listed

struct MotionGrid {
    uint32_t nx, ny, nz;
    uint32_t nbx, nby, nbz, nblocks;
    uint32_t b, a, s;
    uint64_t nwords, n;
};

// `len` (1..64) bits of the y line (ix, iz) from y0 on, bit j = the voxel (ix, y0 + j, iz); cells off the grid are empty.  The line
// starts at bit (iz nx + ix) ny of the array: anywhere in a word, and the row may straddle two.
__device__ __forceinline__ uint64_t motion_row(const uint64_t *__restrict__ words, const MotionGrid &g, int32_t ix, int32_t y0, int32_t iz,
                                               uint32_t len)
{
    if (ix < 0 || iz < 0 || ix >= (int32_t)g.nx || iz >= (int32_t)g.nz) return 0ull;
    const int32_t ylo = y0 < 0 ? 0 : y0, yhi = min(y0 + (int32_t)len, (int32_t)g.ny);
    if (ylo >= yhi) return 0ull;
    const uint32_t cnt = (uint32_t)(yhi - ylo);                  // 1..64
    const uint64_t off = ((uint64_t)iz * g.nx + (uint32_t)ix) * g.ny + (uint32_t)ylo;    // < n
    const uint64_t w = off >> 6;
    const uint32_t sh = (uint32_t)(off & 63u);
    if (w >= g.nwords) return 0ull;
    uint64_t v = words[w] >> sh;
    if (sh && w + 1 < g.nwords) v |= words[w + 1] << (64u - sh); // (sh = 0: the row lies in one word, and a shift by 64 is none)
    if (cnt < 64u) v &= cc_below(cnt);
    return v << (uint32_t)(ylo - y0);                            // ylo - y0 <= len - cnt <= 63
}

struct MotionListParams {
    const uint64_t *a, *b;
    MotionGrid g;
    uint32_t ngroups;
    uint32_t *counts;           // [nblocks] count_a | count_b << 16
    uint64_t *mask;             // [ngroups] the listed blocks of 64 k .. 64 k + 63
    uint32_t *cnt;              // [ngroups] their number
};

__global__ __launch_bounds__(kMotionBlock) void k_motion_list(const MotionListParams p)
{
    const uint32_t grp = blockIdx.x * (kMotionBlock / 64) + (threadIdx.x >> 6);
    if (grp >= p.ngroups) return;                                // (whole waves)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = grp * 64u + lane;
    uint32_t ca = 0, cb = 0;
    if (k < p.g.nblocks) {
        const uint32_t by = k % p.g.nby, t = k / p.g.nby, bx = t % p.g.nbx, bz = t / p.g.nbx;
        const int32_t y0 = (int32_t)(by * p.g.b);
        for (uint32_t jz = 0; jz < p.g.b; ++jz)
            for (uint32_t jx = 0; jx < p.g.b; ++jx) {
                const int32_t ix = (int32_t)(bx * p.g.b + jx), iz = (int32_t)(bz * p.g.b + jz);
                ca += (uint32_t)__popcll(motion_row(p.a, p.g, ix, y0, iz, p.g.b));
                cb += (uint32_t)__popcll(motion_row(p.b, p.g, ix, y0, iz, p.g.b));
            }
        p.counts[k] = ca | (cb << 16);                           // (b <= 16: at most 4096 each)
    }
    const uint64_t m = __ballot((ca | cb) != 0u);
    if (lane == 0) { p.mask[grp] = m; p.cnt[grp] = (uint32_t)__popcll(m); }
}

// one row of vc_motion_t (24 bytes) as the kernels write it
struct MotionRow {
    uint32_t block;
    int8_t d[3];
    uint8_t flags;
    uint32_t cost, cost0;
    uint16_t count_a, count_b, ties, reserved;
};
static_assert(sizeof(MotionRow) == 24, "vc_motion_t");

__global__ __launch_bounds__(kMotionBlock) void k_motion_rank(const MotionGrid g, uint32_t ngroups, const uint32_t *__restrict__ counts,
                                                               const uint64_t *__restrict__ mask, const uint32_t *__restrict__ off,
                                                               const uint64_t *__restrict__ boff, MotionRow *__restrict__ rows, uint64_t listed)
{
    const uint32_t k = blockIdx.x * kMotionBlock + threadIdx.x;
    const uint32_t grp = k >> 6, lane = k & 63u;
    if (k >= g.nblocks || grp >= ngroups) return;
    const uint64_t m = mask[grp];
    if (!((m >> lane) & 1ull)) return;
    const uint64_t r = boff[grp / kScanBlock] + off[grp] + (uint32_t)__popcll(m & cc_below(lane));
    if (r >= listed) return;
    const uint32_t c = counts[k];
    MotionRow row;
    row.block = k;
    row.d[0] = row.d[1] = row.d[2] = 0;
    row.flags = 0;
    row.cost = row.cost0 = 0;
    row.count_a = (uint16_t)(c & 0xffffu); row.count_b = (uint16_t)(c >> 16);
    row.ties = 0; row.reserved = 0;
    rows[r] = row;
}

struct MotionMatchParams {
    const uint64_t *a, *b;
    MotionGrid g;
    MotionRow *rows;            // [listed]: block, count_a and count_b are there
    uint64_t listed;
    uint32_t *vec;              // [nblocks], zeroed: the vector of each listed block (kMotionListed)
    unsigned long long *ctr;    // [kMotionCounters], zeroed
};

// key of a displacement: the smallest wins.  cost < 2^17 (48^3 cells), |d|^2 <= 192, order < 17^3
__device__ __forceinline__ unsigned long long motion_key(uint32_t cost, uint32_t d2, uint32_t order)
{
    return ((unsigned long long)cost << 21) | ((unsigned long long)d2 << 13) | order;
}

// dynamic LDS: R^2 rows of B's region, then W^2 rows of A's window (R = b + 2a + 2s <= 64, W = b + 2a <= 48)
__global__ __launch_bounds__(kMotionBlock) void k_motion_match(const MotionMatchParams p)
{
    extern __shared__ uint64_t s_rows[];
    __shared__ unsigned long long s_best;
    __shared__ uint32_t s_ties, s_cost0;
    const uint64_t r = blockIdx.x;
    if (r >= p.listed) return;                                   // (the whole workgroup)
    const uint32_t k = p.rows[r].block;
    if (k >= p.g.nblocks) return;
    const uint32_t b = p.g.b, a = p.g.a, s = p.g.s;
    const uint32_t W = b + 2u * a, R = W + 2u * s, side = 2u * s + 1u, nd = side * side * side;
    const uint32_t by = k % p.g.nby, t = k / p.g.nby, bx = t % p.g.nbx, bz = t / p.g.nbx;
    const int32_t ox = (int32_t)(bx * b) - (int32_t)a, oy = (int32_t)(by * b) - (int32_t)a, oz = (int32_t)(bz * b) - (int32_t)a;
    uint64_t *s_b = s_rows, *s_a = s_rows + R * R;
    if (threadIdx.x == 0) { s_best = ~0ull; s_ties = 0; s_cost0 = 0; }
    // stage; B's region is uniform when every row is empty or every row is full
    const uint64_t full = R >= 64u ? ~0ull : cc_below(R);
    bool any = false, all = true;
    for (uint32_t i = threadIdx.x; i < R * R; i += kMotionBlock) {
        const uint32_t rz = i / R, rx = i - rz * R;
        const uint64_t v = motion_row(p.b, p.g, ox - (int32_t)s + (int32_t)rx, oy - (int32_t)s, oz - (int32_t)s + (int32_t)rz, R);
        s_b[i] = v;
        any |= v != 0ull;
        all &= v == full;
    }
    for (uint32_t i = threadIdx.x; i < W * W; i += kMotionBlock) {
        const uint32_t wz = i / W, wx = i - wz * W;
        s_a[i] = motion_row(p.a, p.g, ox + (int32_t)wx, oy, oz + (int32_t)wz, W);
    }
    const int some = __syncthreads_or(any ? 1 : 0);              // (also the barrier behind the staging)
    const int solid = __syncthreads_and(all ? 1 : 0);
    const uint64_t wmask = cc_below(W);                          // W <= 48
    const uint32_t centre = (s * side + s) * side + s;           // order of d = 0
    // a uniform region of B gives every displacement the cost of d = 0: one evaluation stands for all (workgroup-uniform branch)
    const bool uniform = !some || solid;
    unsigned long long best = ~0ull;
    uint32_t mincost = 0xffffffffu, mincnt = 0;
    for (uint32_t o = threadIdx.x; o < nd; o += kMotionBlock) {
        if (uniform && o != centre) continue;
        const uint32_t ey = o % side, q = o / side, ex = q % side, ez = q / side;     // e = d + s
        const int32_t dx = (int32_t)ex - (int32_t)s, dy = (int32_t)ey - (int32_t)s, dz = (int32_t)ez - (int32_t)s;
        // the cell (wx, wy, wz) of the window looks at (wx + s - dx, wy + s - dy, wz + s - dz) of the region
        const uint32_t shx = 2u * s - ex, shy = 2u * s - ey, shz = 2u * s - ez;      // 0 .. 2s
        uint32_t cost = 0;
        for (uint32_t wz = 0; wz < W; ++wz) {
            const uint64_t *rb = s_b + (wz + shz) * R + shx;
            const uint64_t *ra = s_a + wz * W;
            for (uint32_t wx = 0; wx < W; ++wx) cost += (uint32_t)__popcll((ra[wx] ^ (rb[wx] >> shy)) & wmask);
        }
        const unsigned long long key = motion_key(cost, (uint32_t)(dx * dx + dy * dy + dz * dz), o);
        best = key < best ? key : best;
        if (cost < mincost) { mincost = cost; mincnt = 1; }
        else if (cost == mincost) ++mincnt;
        if (o == centre) s_cost0 = cost;
    }
    if (best != ~0ull) atomicMin(&s_best, best);
    __syncthreads();
    const unsigned long long win = s_best;
    const uint32_t wcost = (uint32_t)(win >> 21);
    if (mincnt && mincost == wcost) atomicAdd(&s_ties, mincnt);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t o = (uint32_t)(win & 0x1fffu);
    const uint32_t ey = o % side, q = o / side, ex = q % side, ez = q / side;
    const int32_t dx = (int32_t)ex - (int32_t)s, dy = (int32_t)ey - (int32_t)s, dz = (int32_t)ez - (int32_t)s;
    const uint32_t ties = uniform ? nd : s_ties;
    const bool clipped = (uint32_t)abs(dx) == s || (uint32_t)abs(dy) == s || (uint32_t)abs(dz) == s;
    MotionRow row = p.rows[r];
    row.d[0] = (int8_t)dx; row.d[1] = (int8_t)dy; row.d[2] = (int8_t)dz;
    row.flags = clipped ? 1u : 0u;
    row.cost = wcost; row.cost0 = s_cost0;
    row.ties = (uint16_t)ties;
    p.rows[r] = row;
    p.vec[k] = ((uint32_t)dx & 0xffu) | (((uint32_t)dy & 0xffu) << 8) | (((uint32_t)dz & 0xffu) << 16) | kMotionListed;
    if (dx | dy | dz) atomicAdd(p.ctr + 0, 1ull);
    if (ties == 1u) atomicAdd(p.ctr + 1, 1ull);
    if (clipped) atomicAdd(p.ctr + 2, 1ull);
    if (s_cost0) atomicAdd(p.ctr + 3, (unsigned long long)s_cost0);
    if (wcost) atomicAdd(p.ctr + 4, (unsigned long long)wcost);
}

__device__ __forceinline__ int32_t motion_byte(uint32_t v, uint32_t axis) { return (int32_t)(int8_t)((v >> (8u * axis)) & 0xffu); }

struct MotionWarpParams {
    const uint64_t *a, *b;
    MotionGrid g;
    const uint32_t *vec;        // [nblocks]
    uint64_t *out;              // [npad]: P, zero from nwords on
    uint64_t npad;
    unsigned long long *ctr;    // [kWarpCounters], zeroed
};

__global__ __launch_bounds__(kSetopBlock) void k_motion_warp(const MotionWarpParams p)
{
    __shared__ uint32_t s_cnt[kSetopBlock / 64][kWarpCounters];
    const uint64_t w = (uint64_t)blockIdx.x * kSetopBlock + threadIdx.x;
    uint32_t c[kWarpCounters] = {0, 0};
    if (w < p.npad) {
        uint64_t out = 0;
        if (w < p.g.nwords) {
            const uint64_t lo = w << 6, hi = min(lo + 64u, p.g.n);
            uint64_t pos = lo;
            while (pos < hi) {
                uint32_t ix, iy, iz;
                decompose((uint32_t)pos, p.g.nx, p.g.ny, ix, iy, iz);
                const uint32_t by = iy / p.g.b;
                const uint32_t yend = min((by + 1u) * p.g.b, p.g.ny);                 // the block's end on this line
                const uint32_t len = (uint32_t)min((uint64_t)(yend - iy), hi - pos);  // 1..16
                const uint32_t k = ((iz / p.g.b) * p.g.nbx + ix / p.g.b) * p.g.nby + by;
                const uint32_t v = k < p.g.nblocks ? p.vec[k] : 0u;
                if (v & kMotionListed) {
                    const uint64_t bits = motion_row(p.b, p.g, (int32_t)ix - motion_byte(v, 0), (int32_t)iy - motion_byte(v, 1),
                                                     (int32_t)iz - motion_byte(v, 2), len);
                    out |= bits << (uint32_t)(pos - lo);
                }
                pos += len;
            }
            c[0] = tp_pop(out);
            c[1] = tp_pop(out & p.a[w]);
        }
        p.out[w] = out;
    }
    setop_sums(c, s_cnt, p.ctr);
}

__global__ __launch_bounds__(kMotionBlock) void k_motion_paint(uint64_t *__restrict__ records, uint64_t S, const MotionGrid g,
                                                                const uint32_t *__restrict__ vec)
{
    const uint64_t r = (uint64_t)blockIdx.x * kMotionBlock + threadIdx.x;
    if (r >= S) return;
    const uint64_t rec = records[r];
    const uint32_t i = (uint32_t)rec;
    if (i >= g.n) return;
    uint32_t ix, iy, iz;
    decompose(i, g.nx, g.ny, ix, iy, iz);
    const uint32_t k = ((iz / g.b) * g.nbx + ix / g.b) * g.nby + iy / g.b;
    if (k >= g.nblocks) return;
    const uint32_t v = vec[k];
    uint64_t rgb = 0;
#pragma unroll
    for (uint32_t axis = 0; axis < 3; ++axis) {
        const int32_t ch = 128 + (127 * motion_byte(v, axis)) / (int32_t)g.s;        // C division: towards zero
        rgb |= (uint64_t)(uint32_t)(ch & 0xff) << (8u * axis);
    }
    records[r] = (rec & 0xff000000ffffffffull) | (rgb << 32);
}

}  // namespace vc
