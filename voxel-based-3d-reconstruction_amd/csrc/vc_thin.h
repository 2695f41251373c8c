// gfx950 kernels of the homotopic thinning of the hull to a curve skeleton (vc_hull_thin; contract in include/voxcarve.h, DESIGN.md
// section 8 item 19).  Restated in tests/thin_np.py.  Integers and bits only.  A sub-step removes voxels of one subfield, no two of
// which are 26-neighbours, and the predicate reads the 3 x 3 x 3 neighbourhood alone: no lane reads a bit that another lane of its
// launch clears, so the lanes clear their bits in place (an atomic AND on the word) and no order of evaluation shows.
//
//   k_thin_anchor  lane = anchor voxel of the host's list: its bit into the anchor words; the first list position that is no
//                  survivor (atomicMin) for the refusal
//   k_thin_pinned  lane = record: the bit of every record whose geodesic key holds distance 0 into the anchor words
//   k_thin_count   lane = anchor word: the distinct anchors
//   k_thin_border  lane = record: the border list {voxel, record} before the first pass -- the voxels with a face neighbour in the
//                  background, the only ones a direction step can mark; their bits in the listed words
//   k_thin_mark    lane = entry of the border list (grid-stride over the count on the device): still in H, no anchor, p + d
//                  background -> appended to the step's candidates by one atomic per wave
//   k_thin_sub     lane = candidate (grid-stride over the count on the device): of subfield s, simple, in "curve" mode no end
//                  point -> bit cleared, peel written, one atomic per wave on the pass's count; its face neighbours in H that
//                  are not listed yet join the border list (their record from the words' record offsets, as vc_components.h
//                  ranks a voxel).  The background only grows, so a listed voxel stays a border voxel until it is removed.
//   k_thin_table   thread = 32 codes: the predicate of all 2^26 codes as bits (route 2 looks it up, route 1 evaluates it)
//   k_thin_rows    lane = kept voxel: its row {voxel, record, degree} and the degree counts
// The 27 cells of a voxel's cube are gathered from nine rows of the working words (ix +- 1, iz +- 1), three consecutive iy bits
// each; a row's window may straddle two words.  Rows outside the grid and cells beyond iy = 0 or ny - 1 are background.  Every word
// index is below the word count by construction (a window starts at a voxel of the grid) and the second word is read only when it
// exists.
#pragma once
#include "vc_measure.h"          // MsDiv, ms_div

namespace vc {

constexpr uint32_t kThBlock = 256;
constexpr uint32_t kThMaxBlocks = 2048;                          // of the grid-stride launches
constexpr uint32_t kThTableWords = 1u << 21;                     // u32 words of the table: 2^26 bits
// counters (u32): the candidates of the six direction steps of a pass, the voxels the pass removed, the direction steps that had
// a candidate, the distinct anchors, the first bad anchor's list position, kept voxels of degree 0 / 1 / >= 3, the entries of the
// border list (behind the removed count: the pass's one read-back takes both)
enum { kThCntCand = 0, kThCntRemoved = 6, kThCntBorder = 7, kThCntAnchors = 8, kThCntBad = 9, kThCntIsolated = 10, kThCntEnds = 11,
       kThCntJunctions = 12, kThCntSteps = 13, kThCnt = 16 };

struct ThParams {
    unsigned long long *work;          // [nwords] the working copy of the occupancy
    const unsigned long long *anchor;  // [nwords]
    const uint32_t *table;             // [kThTableWords], route 2
    uint32_t *cnt;                     // [kThCnt]
    unsigned long long *cand;          // [border] {voxel, record << 32}
    unsigned long long *border;        // [S] the border list, entries as cand's
    unsigned long long *listed;        // [nwords] the voxels that are or were in the border list
    const unsigned long long *orig;    // [nwords] the result's own occupancy: with woff, a voxel's record
    const uint32_t *woff;              // [nwords] survivors in the words before each word
    uint16_t *peel;                    // [S]
    uint64_t nwords;
    uint32_t nx, ny, nz, ncol;
    MsDiv by_ncol, by_ny;
};

struct ThCell { uint32_t ix, iy, iz; };

__device__ __forceinline__ ThCell th_cell(const ThParams &p, uint32_t i)
{
    ThCell c;
    c.iz = ms_div(i, p.by_ncol);
    const uint32_t col = i - c.iz * p.ncol;
    c.ix = ms_div(col, p.by_ny);
    c.iy = col - c.ix * p.ny;
    return c;
}

__device__ __forceinline__ uint32_t th_bit(const unsigned long long *w, uint32_t i) { return (uint32_t)(w[i >> 6] >> (i & 63u)) & 1u; }

// Bits c - 1, c, c + 1 of the words as bits 0, 1, 2; lo / hi: whether c - 1 / c + 1 lie in c's row.
__device__ __forceinline__ uint32_t th_row3(const unsigned long long *w, uint64_t nwords, uint32_t c, bool lo, bool hi)
{
    const uint32_t start = lo ? c - 1u : c, k = start >> 6, sh = start & 63u;
    unsigned long long v = w[k] >> sh;
    if (sh > 61u && (uint64_t)k + 1 < nwords) v |= w[k + 1] << (64u - sh);
    uint32_t r = (uint32_t)v & 7u;
    if (!lo) r = (r << 1) & 7u;
    if (!hi) r &= 3u;
    return r;
}

// The 27 cells of voxel i's cube, cell (dz + 1) 9 + (dx + 1) 3 + (dy + 1); the centre as it is in the words.
__device__ __forceinline__ uint32_t th_cube(const ThParams &p, uint32_t i, const ThCell &c)
{
    const bool lo = c.iy > 0, hi = c.iy + 1 < p.ny;
    uint32_t m = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz) {
        if ((dz < 0 && c.iz == 0) || (dz > 0 && c.iz + 1 >= p.nz)) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            if ((dx < 0 && c.ix == 0) || (dx > 0 && c.ix + 1 >= p.nx)) continue;
            const uint32_t at = (uint32_t)((int64_t)i + (int64_t)dz * (int64_t)p.ncol + (int64_t)dx * (int64_t)p.ny);
            m |= th_row3(p.work, p.nwords, at, lo, hi) << (uint32_t)((dz + 1) * 9 + (dx + 1) * 3);
        }
    }
    return m;
}

constexpr uint32_t kThAll = (1u << 27) - 1u, kThCentre = 1u << 13;
constexpr uint32_t kThY0 = 0x1249249u, kThY2 = 0x4924924u;      // the cells of dy = -1 / +1: bits 0, 3, 6, .. / 2, 5, 8, ..
constexpr uint32_t kThX0 = 0x01c0e07u, kThX2 = 0x70381c0u;      // of dx = -1 / +1: bits 0..2, 9..11, 18..20 / 6..8, 15..17, 24..26
constexpr uint32_t kThFaces = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22);
constexpr uint32_t kThCorners = (1u << 0) | (1u << 2) | (1u << 6) | (1u << 8) | (1u << 18) | (1u << 20) | (1u << 24) | (1u << 26);
constexpr uint32_t kThN18 = kThAll & ~kThCorners & ~kThCentre;

// (a shift up leaves bits above the cube, which a later shift down would bring back: every result is cut to the 27 cells)
__device__ __forceinline__ uint32_t th_grow_y(uint32_t g) { return g | ((g << 1) & kThAll & ~kThY0) | ((g >> 1) & ~kThY2); }
__device__ __forceinline__ uint32_t th_grow_x(uint32_t g) { return g | ((g << 3) & kThAll & ~kThX0) | ((g >> 3) & ~kThX2); }
__device__ __forceinline__ uint32_t th_grow_z(uint32_t g) { return g | ((g << 9) & kThAll) | (g >> 9); }

__device__ __forceinline__ uint32_t th_code(uint32_t cube) { return (cube & 0x1fffu) | ((cube >> 14) << 13); }
__device__ __forceinline__ uint32_t th_cube_of(uint32_t code) { return (code & 0x1fffu) | ((code >> 13) << 14); }

// The predicate: m = the cube's object cells without the centre.  Simple when the object cells are one 26-component and the
// background cells of N18 that are 6-connected, inside N18, to one face neighbour hold every background face neighbour.  Both are
// floods by shifts of the whole cube: a 26-step is a step along y, then x, then z; a 6-step the union of the three.
__device__ __forceinline__ bool th_simple(uint32_t m)
{
    if (m == 0) return false;
    uint32_t g = m & (0u - m);
    for (int it = 0; it < 26; ++it) {
        const uint32_t n = th_grow_z(th_grow_x(th_grow_y(g))) & m;
        if (n == g) break;
        g = n;
    }
    if (g != m) return false;
    const uint32_t b = ~m & kThN18, faces = b & kThFaces;
    if (faces == 0) return false;
    g = faces & (0u - faces);
    for (int it = 0; it < 18; ++it) {
        const uint32_t n = (th_grow_y(g) | th_grow_x(g) | th_grow_z(g)) & b;
        if (n == g) break;
        g = n;
    }
    return (faces & ~g) == 0;
}

__global__ __launch_bounds__(kThBlock) void k_thin_table(uint32_t *__restrict__ table)
{
    const uint32_t t = blockIdx.x * kThBlock + threadIdx.x;
    if (t >= kThTableWords) return;
    uint32_t bits = 0;
    for (uint32_t k = 0; k < 32; ++k) bits |= (th_simple(th_cube_of(t * 32u + k)) ? 1u : 0u) << k;
    table[t] = bits;
}

__global__ __launch_bounds__(kThBlock) void k_thin_anchor(const uint32_t *__restrict__ list, uint32_t n_list, uint64_t n_voxels,
                                                         const unsigned long long *__restrict__ words, unsigned long long *__restrict__ anchor,
                                                         uint32_t *__restrict__ cnt)
{
    const uint32_t t = blockIdx.x * kThBlock + threadIdx.x;
    if (t >= n_list) return;
    const uint32_t v = list[t];
    if (v >= n_voxels || !th_bit(words, v)) { atomicMin(cnt + kThCntBad, t); return; }
    atomicOr(anchor + (v >> 6), 1ull << (v & 63u));
}

__global__ __launch_bounds__(kThBlock) void k_thin_pinned(const uint64_t *__restrict__ records, const unsigned long long *__restrict__ key,
                                                         uint64_t S, unsigned long long *__restrict__ anchor)
{
    const uint64_t s = (uint64_t)blockIdx.x * kThBlock + threadIdx.x;
    if (s >= S || (key[s] >> 8) != 0) return;
    const uint32_t v = (uint32_t)records[s];
    atomicOr(anchor + (v >> 6), 1ull << (v & 63u));
}

__global__ __launch_bounds__(kThBlock) void k_thin_count(const unsigned long long *__restrict__ anchor, uint64_t nwords, uint32_t *__restrict__ cnt)
{
    const uint64_t w = (uint64_t)blockIdx.x * kThBlock + threadIdx.x;
    const uint32_t n = wave_sum_u32(w < nwords ? (uint32_t)__popcll(anchor[w]) : 0u);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(cnt + kThCntAnchors, n);
}

// One slot per lane that has something to append, by one atomic of the wave's first such lane.
__device__ __forceinline__ uint32_t th_append(uint32_t *counter, bool mine)
{
    const unsigned long long m = __ballot(mine);
    if (m == 0) return 0;
    const uint32_t lane = threadIdx.x & 63u, first = (uint32_t)__ffsll((long long)m) - 1u;
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)first);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// Whether voxel i, in cell c, has the neighbour towards d0 .. d5 = -z, +z, -y, +y, -x, +x inside the grid, and that neighbour's index.
__device__ __forceinline__ bool th_toward(const ThParams &p, uint32_t i, const ThCell &c, uint32_t d, uint32_t &at)
{
    if (d == 0) { at = i - p.ncol; return c.iz > 0; }
    if (d == 1) { at = i + p.ncol; return c.iz + 1 < p.nz; }
    if (d == 2) { at = i - 1u; return c.iy > 0; }
    if (d == 3) { at = i + 1u; return c.iy + 1 < p.ny; }
    if (d == 4) { at = i - p.ny; return c.ix > 0; }
    at = i + p.ny;
    return c.ix + 1 < p.nx;
}

__global__ __launch_bounds__(kThBlock) void k_thin_border(const ThParams p, const uint64_t *__restrict__ records, uint64_t S)
{
    const uint64_t s = (uint64_t)blockIdx.x * kThBlock + threadIdx.x;                              // (whole waves: th_append)
    bool mine = false;
    uint32_t i = 0;
    if (s < S) {
        i = (uint32_t)records[s];
        const ThCell c = th_cell(p, i);
#pragma unroll
        for (uint32_t d = 0; d < 6; ++d) {
            uint32_t at;
            if (!th_toward(p, i, c, d, at) || !th_bit(p.orig, at)) mine = true;
        }
    }
    const uint32_t slot = th_append(p.cnt + kThCntBorder, mine);
    if (mine) {
        p.border[slot] = (unsigned long long)i | (s << 32);
        atomicOr(p.listed + (i >> 6), 1ull << (i & 63u));
    }
}

__global__ __launch_bounds__(kThBlock) void k_thin_mark(const ThParams p, uint32_t d)
{
    const uint32_t n = p.cnt[kThCntBorder];
    for (uint32_t base = blockIdx.x * kThBlock; base < n; base += gridDim.x * kThBlock) {          // (whole waves: th_append)
        const uint32_t j = base + threadIdx.x;
        bool mine = false;
        unsigned long long e = 0;
        if (j < n) {
            e = p.border[j];
            const uint32_t i = (uint32_t)e;
            if (th_bit(p.work, i) && !th_bit(p.anchor, i)) {
                uint32_t at;
                mine = !th_toward(p, i, th_cell(p, i), d, at) || !th_bit(p.work, at);
            }
        }
        const uint32_t slot = th_append(p.cnt + kThCntCand + d, mine);
        if (mine) p.cand[slot] = e;
    }
}

template <bool TABLE>
__global__ __launch_bounds__(kThBlock) void k_thin_sub(const ThParams p, uint32_t d, uint32_t s, uint32_t curve, uint32_t code)
{
    const uint32_t n = p.cnt[kThCntCand + d];
    if (s == 0 && blockIdx.x == 0 && threadIdx.x == 0 && n) atomicAdd(p.cnt + kThCntSteps, 1u);
    for (uint32_t base = blockIdx.x * kThBlock; base < n; base += gridDim.x * kThBlock) {
        const uint32_t j = base + threadIdx.x;
        bool go = false;
        if (j < n) {
            const unsigned long long e = p.cand[j];
            const uint32_t i = (uint32_t)e;
            const ThCell c = th_cell(p, i);
            if (((c.ix & 1u) | (c.iy & 1u) << 1 | (c.iz & 1u) << 2) == s) {
                const uint32_t m = th_cube(p, i, c) & ~kThCentre;
                if (TABLE) { const uint32_t k = th_code(m); go = (p.table[k >> 5] >> (k & 31u)) & 1u; }
                else go = th_simple(m);
                if (curve && (m & (m - 1u)) == 0) go = false;    // (one neighbour: an end point)
                if (go) {
                    atomicAnd(p.work + (i >> 6), ~(1ull << (i & 63u)));
                    p.peel[e >> 32] = (uint16_t)code;
                    // its face neighbours in H are border voxels from now on (no voxel of this launch: another subfield)
#pragma unroll
                    for (uint32_t f = 0; f < 6; ++f) {
                        uint32_t at;
                        if (!th_toward(p, i, c, f, at) || !th_bit(p.work, at) || th_bit(p.listed, at)) continue;
                        const unsigned long long bit = 1ull << (at & 63u);
                        if (atomicOr(p.listed + (at >> 6), bit) & bit) continue;                 // (another lane listed it)
                        const uint32_t rec = p.woff[at >> 6] + (uint32_t)__popcll(p.orig[at >> 6] & (bit - 1ull));
                        p.border[atomicAdd(p.cnt + kThCntBorder, 1u)] = (unsigned long long)at | ((unsigned long long)rec << 32);
                    }
                }
            }
        }
        const uint32_t k = (uint32_t)__popcll(__ballot(go));
        if ((threadIdx.x & 63u) == 0 && k) atomicAdd(p.cnt + kThCntRemoved, k);
    }
}

// The border list's compaction (vc_compact.h): the entries whose voxel is still in H.
struct ThSelLive {
    const unsigned long long *live, *work;
    unsigned long long *out;
    __device__ bool pick(uint64_t s) const { return th_bit(work, (uint32_t)live[s]); }
    __device__ void drop(uint64_t) const {}
    __device__ void put(uint64_t s, uint64_t d) const { out[d] = live[s]; }
};

// The kept voxels after the last pass, in record order: the output list {voxel, record}.
struct ThSelKept {
    const uint64_t *records;
    const unsigned long long *work;
    unsigned long long *out;
    __device__ bool pick(uint64_t s) const { return th_bit(work, (uint32_t)records[s]); }
    __device__ void drop(uint64_t) const {}
    __device__ void put(uint64_t s, uint64_t d) const { out[d] = (records[s] & 0xffffffffull) | (s << 32); }
};

struct ThRow { uint32_t voxel, record, degree; };                // vc_skeleton_voxel_t: the degree in the low byte of the third word

__global__ __launch_bounds__(kThBlock) void k_thin_rows(const ThParams p, const unsigned long long *__restrict__ live, uint32_t n_live,
                                                       ThRow *__restrict__ rows)
{
    const uint32_t j = blockIdx.x * kThBlock + threadIdx.x;
    uint32_t deg = 0xffffffffu;
    if (j < n_live) {
        const unsigned long long e = live[j];
        const uint32_t i = (uint32_t)e;
        deg = (uint32_t)__popc(th_cube(p, i, th_cell(p, i)) & ~kThCentre);
        rows[j] = ThRow{i, (uint32_t)(e >> 32), deg};
    }
    const uint32_t n0 = (uint32_t)__popcll(__ballot(deg == 0)), n1 = (uint32_t)__popcll(__ballot(deg == 1)),
                   n3 = (uint32_t)__popcll(__ballot(deg >= 3 && deg != 0xffffffffu));
    if ((threadIdx.x & 63u) == 0) {
        if (n0) atomicAdd(p.cnt + kThCntIsolated, n0);
        if (n1) atomicAdd(p.cnt + kThCntEnds, n1);
        if (n3) atomicAdd(p.cnt + kThCntJunctions, n3);
    }
}

}  // namespace vc
