// gfx950 kernels of the exact Euclidean distance transform of the hull (vc_hull_distance, vc_hull_morphology; contract in
// include/voxcarve.h and DESIGN.md section 8 item 12): squared distances in um^2 as unsigned 64-bit integers, a minimum over a
// set of sites, so any correct evaluation gives the same bits.  Restated in tests/distance_np.py.
//
// A transform runs over a BOX of cells (the hull's index box grown by one cell per side for the inside field and the
// morphology, the whole grid for the outside field), laid out like the grid: cell (lx, ly, lz) at (lz bx + lx) by + ly, y
// fastest.  The box's origin is signed: with VC_DIST_BORDER_OFF it may start at -1 and end at n, and a cell outside the grid is
// a site (the edge and corner cells of that layer are never nearer than a face cell, so counting them changes no minimum).
//
//   k_dist_box      lane = 16 records: the inclusive index box of the survivors, by wave reductions and guarded integer atomics
//   k_dist_y<MODE>  wave = one y line of the box, 64 cells per step: the site bits of a step are one ballot, the nearest site on
//                   either side of a lane is a count of leading / trailing zeros on that word or the carry from the words before
//                   / after it.  MODE says what a site is: an unset occupancy bit (or a cell outside the grid), a set bit, or a
//                   cell of the field above r2 (the eroded set, thresholded in place: a line is read whole before it is written)
//   k_dist_env      lane = one line along x or z, adjacent lanes on adjacent iy (every step of the walk is a coalesced load): the
//                   exact lower envelope of the parabolas g(i) + w (x - i)^2, Meijster's two scans in integers with w = q_a^2.
//                   The stack (site | first cell << 16, one u32 per entry) lives in a scratch plane laid out like the field; the
//                   pass reads one field and writes another, because a site's g is read again after cells beyond it are final
//   k_dist_records  lane = 16 records: their values from the box field, the maximum and the count above r2
//   k_compact_count<DistKept>, k_compact_scatter<DistKept>   (vc_compact.h) the kept records, stably
#pragma once
#include "vc_compact.h"          // k_compact_count, k_compact_scatter (vc_kernels.h: decompose, wave_*)

namespace vc {

constexpr uint32_t kDistBlock = 256;
constexpr uint32_t kDistPer = 16;                            // records per lane of k_dist_box and k_dist_records
constexpr uint32_t kDistGroup = kDistBlock * kDistPer;
constexpr uint32_t kDistMaxChunks = 66;                      // 64-cell steps of a y line: lines of up to 4096 + 2 cells
constexpr uint32_t kDistMaxLine = 4098;                      // cells of a line: a stack entry holds two of them in 16 bits each
constexpr uint64_t kDistInf = 0xffffffffffffffffull;

enum { kDistSiteOff = 0, kDistSiteOn = 1, kDistSiteAbove = 2 };

struct DistBox {
    int32_t o[3];               // grid index of the box's cell 0 per axis x, y, z (-1 possible with the border layer)
    uint32_t b[3];              // cells per axis
    uint32_t nx, ny, nz;
};

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint64_t dist_load(const unsigned long long *a)
{
    return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// box[0..2] = min ix, iy, iz (preset to 0xffffffff), box[3..5] = max (preset to 0).  Lane t of workgroup g takes records
// g kDistGroup + r kDistBlock + t, r < kDistPer; a wave makes an atomic only when it would change the stored value (lo only
// falls, hi only rises: a stale read costs an atomic too many, never a wrong skip) -- unguarded, every wave's six atomics hit the
// same six addresses and the kernel is nothing but that queue
__global__ __launch_bounds__(kDistBlock) void k_dist_box(const uint64_t *__restrict__ records, uint64_t S, uint32_t nx, uint32_t ny,
                                                          uint32_t *__restrict__ box)
{
    const uint64_t base = (uint64_t)blockIdx.x * kDistGroup + threadIdx.x;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0, 0, 0};
#pragma unroll 4
    for (uint32_t r = 0; r < kDistPer; ++r) {
        const uint64_t s = base + (uint64_t)r * kDistBlock;
        if (s >= S) break;
        uint32_t c[3];
        decompose((uint32_t)records[s], nx, ny, c[0], c[1], c[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const uint32_t l = wave_min_u32(lo[a]), h = wave_max_u32(hi[a]);
        if ((threadIdx.x & 63u) == 0 && l != 0xffffffffu) {
            if (l < __hip_atomic_load(box + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(box + a, l);
            if (h > __hip_atomic_load(box + 3 + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(box + 3 + a, h);
        }
    }
}

// Is cell (lx, ly, lz) of the box a site?  (kDistSiteAbove reads the field instead: k_dist_y)
template <int MODE>
__device__ __forceinline__ bool dist_site(const DistBox &bx, const uint64_t *__restrict__ words, uint32_t lx, uint32_t ly, uint32_t lz)
{
    const int32_t gx = bx.o[0] + (int32_t)lx, gy = bx.o[1] + (int32_t)ly, gz = bx.o[2] + (int32_t)lz;
    if (gx < 0 || gy < 0 || gz < 0 || gx >= (int32_t)bx.nx || gy >= (int32_t)bx.ny || gz >= (int32_t)bx.nz) return MODE == kDistSiteOff;
    const uint64_t i = ((uint64_t)gz * bx.nx + (uint32_t)gx) * bx.ny + (uint32_t)gy;
    const bool on = (words[i >> 6] >> (i & 63u)) & 1ull;
    return MODE == kDistSiteOff ? !on : on;
}

// f[cell] = (q_y * cells to the nearest site of the cell's y line)^2, kDistInf on a line without sites
template <int MODE>
__global__ __launch_bounds__(kDistBlock) void k_dist_y(const DistBox bx, const uint64_t *__restrict__ words, uint64_t *__restrict__ f,
                                                        uint64_t r2, uint64_t qy)
{
    __shared__ uint64_t s_mask[kDistBlock / 64][kDistMaxChunks];
    __shared__ int32_t s_left[kDistBlock / 64][kDistMaxChunks];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t nlines = (uint64_t)bx.b[0] * bx.b[2];
    const uint64_t line = (uint64_t)blockIdx.x * (kDistBlock / 64) + wave;
    const bool live = line < nlines;                             // (whole waves; every wave meets the barrier)
    const uint32_t by = bx.b[1], nchunks = (by + 63u) / 64u;
    const uint32_t lz = live ? (uint32_t)(line / bx.b[0]) : 0u, lx = live ? (uint32_t)(line % bx.b[0]) : 0u;
    uint64_t *row = f + line * by;
    if (live) {
        int32_t carry = -1;                                      // the last site before this step
        for (uint32_t c = 0; c < nchunks; ++c) {
            const uint32_t ly = c * 64u + lane;
            bool site = false;
            if (ly < by) site = MODE == kDistSiteAbove ? row[ly] > r2 : dist_site<MODE>(bx, words, lx, ly, lz);
            const uint64_t m = __ballot(site);
            if (lane == 0) { s_mask[wave][c] = m; s_left[wave][c] = carry; }
            if (m) carry = (int32_t)(c * 64u + 63u - (uint32_t)__clzll((long long)m));
        }
    }
    __syncthreads();
    if (!live) return;
    int32_t carry = -1;                                          // the first site after this step
    for (uint32_t c = nchunks; c-- > 0;) {
        const uint64_t m = s_mask[wave][c];
        const uint64_t ml = m & (~0ull >> (63u - lane)), mr = m & (~0ull << lane);     // bits at or below / at or above the lane
        const int32_t left = ml ? (int32_t)(c * 64u + 63u - (uint32_t)__clzll((long long)ml)) : s_left[wave][c];
        const int32_t right = mr ? (int32_t)(c * 64u + (uint32_t)__ffsll((unsigned long long)mr) - 1u) : carry;
        const int32_t ly = (int32_t)(c * 64u + lane);
        uint32_t d = 0xffffffffu;
        if (left >= 0) d = (uint32_t)(ly - left);
        if (right >= 0 && (uint32_t)(right - ly) < d) d = (uint32_t)(right - ly);
        if ((uint32_t)ly < by) {
            const uint64_t e = (uint64_t)d * qy;
            row[ly] = d == 0xffffffffu ? kDistInf : e * e;
        }
        if (m) carry = (int32_t)(c * 64u + (uint32_t)__ffsll((unsigned long long)m) - 1u);
    }
}

// out(x) = min over cells i of the line with g(i) != kDistInf of g(i) + w (x - i)^2; kDistInf on a line without such a cell.
// Line L: cells at ((L / inner) * outer + L % inner) + k * stride, k < m.  g < 2^62 and w m^2 <= 2^60 (vc_hull_distance checks
// the metric), so every sum below fits 63 bits.
__global__ __launch_bounds__(kDistBlock) void k_dist_env(const uint64_t *__restrict__ g, uint64_t *__restrict__ out, uint32_t *__restrict__ st,
                                                          uint64_t nlines, uint64_t inner, uint64_t outer, uint64_t stride, uint32_t m, uint64_t w)
{
    const uint64_t L = (uint64_t)blockIdx.x * kDistBlock + threadIdx.x;
    if (L >= nlines) return;
    const uint64_t base = (L / inner) * outer + L % inner;
    int32_t q = -1;                                              // top of the stack; its entry is kept in registers too
    uint32_t sq = 0, tq = 0;                                     // the top's site and the first cell it owns
    uint64_t gq = 0;                                             // g(sq)
    for (uint32_t u = 0; u < m; ++u) {
        const uint64_t gu = g[base + u * stride];
        if (gu == kDistInf) continue;
        while (q >= 0) {                                         // the top loses its first cell to u: it owns nothing
            const int64_t a = (int64_t)tq - (int64_t)sq, b = (int64_t)u - (int64_t)tq;
            if (gq + w * (uint64_t)(a * a) <= gu + w * (uint64_t)(b * b)) break;
            if (--q >= 0) {
                const uint32_t e = st[base + (uint64_t)q * stride];
                sq = e & 0xffffu; tq = e >> 16;
                gq = g[base + sq * stride];
            }
        }
        if (q < 0) {
            q = 0; sq = u; tq = 0; gq = gu;
            st[base] = u;
        } else {
            // the last cell where the top's parabola is not above u's: floor((F(u) - F(sq)) / (2 w (u - sq))), F(i) = g(i) + w i^2.
            // The top holds its first cell tq >= 0 against u (the loop above), so that cell is >= tq and the numerator is not
            // negative: the truncating division is the floor
            const uint64_t num = (gu + w * (uint64_t)u * u) - (gq + w * (uint64_t)sq * sq);
            const uint64_t sep = num / (2 * w * (uint64_t)(u - sq));
            if (sep + 1 < (uint64_t)m) {
                ++q; sq = u; tq = (uint32_t)(sep + 1); gq = gu;
                st[base + (uint64_t)q * stride] = sq | (tq << 16);
            }
        }
    }
    if (q < 0) {
        for (uint32_t u = 0; u < m; ++u) out[base + u * stride] = kDistInf;
        return;
    }
    for (uint32_t u = m; u-- > 0;) {
        const int64_t d = (int64_t)u - (int64_t)sq;
        out[base + u * stride] = gq + w * (uint64_t)(d * d);
        if (u == tq && q > 0) {
            --q;
            const uint32_t e = st[base + (uint64_t)q * stride];
            sq = e & 0xffffu; tq = e >> 16;
            gq = g[base + sq * stride];
        }
    }
}

// val[s] = the box field at record s; acc[0] = max over the records, acc[1] += records with a value above r2.  Records per lane
// as in k_dist_box; the maximum's atomic is guarded in the same way, the count takes one add per wave of kDistPer x 64 records
__global__ __launch_bounds__(kDistBlock) void k_dist_records(const DistBox bx, const uint64_t *__restrict__ records, uint64_t S,
                                                              const uint64_t *__restrict__ f, uint64_t r2, uint64_t *__restrict__ val,
                                                              unsigned long long *__restrict__ acc)
{
    const uint64_t base = (uint64_t)blockIdx.x * kDistGroup + threadIdx.x;
    uint64_t mx = 0;
    uint32_t above = 0;
#pragma unroll 4
    for (uint32_t r = 0; r < kDistPer; ++r) {
        const uint64_t s = base + (uint64_t)r * kDistBlock;
        if (s >= S) break;
        uint32_t ix, iy, iz;
        decompose((uint32_t)records[s], bx.nx, bx.ny, ix, iy, iz);
        const uint32_t lx = (uint32_t)((int32_t)ix - bx.o[0]), ly = (uint32_t)((int32_t)iy - bx.o[1]), lz = (uint32_t)((int32_t)iz - bx.o[2]);
        const uint64_t v = f[((uint64_t)lz * bx.b[0] + lx) * bx.b[1] + ly];
        val[s] = v;
        mx = v > mx ? v : mx;
        above += v > r2 ? 1u : 0u;
    }
    mx = wave_max_u64(mx);
    above = wave_sum_u32(above);
    if ((threadIdx.x & 63u) == 0) {
        if (mx > dist_load(acc + 0)) atomicMax(acc + 0, (unsigned long long)mx);
        if (above) atomicAdd(acc + 1, (unsigned long long)above);
    }
}

// Selector of the morphology's compaction (vc_compact.h).  Erosion keeps the records whose inside distance is above r2; the
// opening those within r2 of the eroded set (kDistInf: there is none).  A dropped record leaves its occupancy word.
struct DistKept {
    const uint64_t *val;
    uint64_t r2;
    uint32_t open;
    const uint64_t *records;
    uint64_t *words;
    uint64_t *out;
    __device__ bool pick(uint64_t s) const
    {
        const uint64_t v = val[s];
        return open ? (v != kDistInf && v <= r2) : v > r2;
    }
    __device__ void drop(uint64_t s) const
    {
        const uint32_t i = (uint32_t)records[s];
        atomicAnd((unsigned long long *)(words + (i >> 6)), ~(1ull << (i & 63u)));
    }
    __device__ void put(uint64_t s, uint64_t d) const { out[d] = records[s]; }
};

}  // namespace vc
