// gfx950 kernels of the connected components of the hull (vc_hull_components; contract in include/voxcarve.h and DESIGN.md
// section 8 item 8): union-find over the survivors' RECORD indices (memory and work proportional to the survivors, not to the
// grid), sizes and boxes per component, the keep rule, and a stable compaction of the kept records.  Restated in
// tests/components_np.py.
//
//   k_cc_wcount      wave = 64 occupancy words: their popcounts summed (then scan_counts over the word groups)
//   k_cc_woff        lane = word: woff[w] = survivors in words before w -- the record index of voxel j is
//                    woff[j >> 6] + popc(word & below(j & 63))
//   k_cc_init        lane = record: parent = the first record of its run of set bits in one iy column inside one word (the
//                    local unions need no atomics: a run is consecutive records)
//   k_cc_union<N>    lane = record: atomic-min unions with the occupied neighbours of the negative half-neighbourhood (3, 9 or
//                    13 for N = 6, 18, 26; every undirected edge once).  A record inside a run skips a neighbour whose own
//                    predecessor in its column is occupied in the same word: the record before it in the run has made that
//                    union already
//   k_cc_compress    lane = record: parent[s] = root, label[s] = the root's linear index (the smallest of the component)
//   k_compact_count<CcRoots>, k_compact_scatter<CcRoots>   (vc_compact.h) the root list (ascending label) and cid[root]
//   k_cc_clear       lane = component: size 0, empty box
//   k_cc_stats       workgroup = kCompactGroup records: size and box of each component by integer atomics, reduced over a lane's
//                    records, then a wave, then the workgroup while they lie in one component (the body holds nearly every
//                    voxel: unreduced atomics would all hit one address)
//   k_cc_select      one workgroup: radix select of the keep_largest-th key, key = size << 32 | ~k (size descending, then
//                    label ascending; unique)
//   k_cc_mark        lane = component: the keep rule, the vc_component_t entry, the kept count and the largest size
//   k_compact_count<CcKept>, k_compact_scatter<CcKept>     the kept records, stably (the dropped ones leave their word)
// Parents only ever decrease (parent[s] <= s, inside s's set), so every root is its component's first record whatever order
// the unions run in: labels, lists and boxes are exact and bit-reproducible.
#pragma once
#include "vc_compact.h"          // kCompactGroup, k_compact_count, k_compact_scatter (vc_kernels.h: decompose, uf_*, wave_*)

namespace vc {

constexpr uint32_t kCcBlock = 256;
static_assert(kCcBlock * kCompactPer == kCompactGroup, "k_cc_stats takes the compaction's groups");
constexpr uint32_t kCcSelectBlock = 1024;
constexpr uint32_t kCcCompWords = 10;                        // u32 per vc_component_t

struct CcParams {
    const uint64_t *records;    // [S] ascending linear index in the low 32 bits
    uint64_t *words;            // occupancy words of the whole grid
    const uint32_t *woff;       // [nwords] survivors before each word
    uint32_t *parent;           // [S] union-find forest over record indices, then the root of each record
    uint32_t *label;            // [S] linear index of each record's root
    uint32_t *cid;              // [S] component number of a root (written at roots only)
    const uint32_t *roots;      // [K] root record of each component, ascending
    uint32_t *size;             // [K]
    uint32_t *box;              // [K][6] lo x, y, z, hi x, y, z
    const uint8_t *kept;        // [K]
    uint64_t S;
    uint32_t nx, ny, nz;
};

__device__ __forceinline__ uint32_t cc_load(const uint32_t *a, uint32_t s)
{
    return __hip_atomic_load(a + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t cc_below(uint32_t b) { return (1ull << b) - 1ull; }    // b < 64

// wave g of the grid: words 64 g .. 64 g + 63, one per lane
__global__ __launch_bounds__(kCcBlock) void k_cc_wcount(const uint64_t *__restrict__ words, uint64_t nwords, uint32_t ngroups,
                                                         uint32_t *__restrict__ cnt)
{
    const uint32_t g = blockIdx.x * (kCcBlock / 64) + (threadIdx.x >> 6);
    if (g >= ngroups) return;                                    // (whole waves)
    const uint64_t w = (uint64_t)g * 64 + (threadIdx.x & 63u);
    const uint32_t c = wave_sum_u32(w < nwords ? (uint32_t)__popcll(words[w]) : 0u);
    if ((threadIdx.x & 63u) == 0) cnt[g] = c;
}

__global__ __launch_bounds__(kCcBlock) void k_cc_woff(const uint64_t *__restrict__ words, uint64_t nwords, uint32_t ngroups,
                                                       const uint32_t *__restrict__ off, const uint64_t *__restrict__ boff,
                                                       uint32_t *__restrict__ woff)
{
    const uint32_t g = blockIdx.x * (kCcBlock / 64) + (threadIdx.x >> 6);
    if (g >= ngroups) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)g * 64 + lane;
    const uint32_t c = w < nwords ? (uint32_t)__popcll(words[w]) : 0u;
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= (uint32_t)d) incl += o;
    }
    if (w < nwords) woff[w] = (uint32_t)(boff[g / kScanBlock] + off[g]) + incl - c;
}

__global__ __launch_bounds__(kCcBlock) void k_cc_init(const CcParams p)
{
    const uint64_t s = (uint64_t)blockIdx.x * kCcBlock + threadIdx.x;
    if (s >= p.S) return;
    const uint32_t i = (uint32_t)p.records[s];
    const uint32_t b = i & 63u, iy = i % p.ny;
    const uint64_t zeros = ~p.words[i >> 6] & cc_below(b);       // unset bits below b
    const uint32_t r0 = zeros ? 64u - (uint32_t)__clzll((long long)zeros) : 0u;
    const uint32_t c0 = iy >= b ? 0u : b - iy;                   // the column's first bit in this word
    p.parent[s] = (uint32_t)s - (b - max(r0, c0));
}

template <int CONN>
__global__ __launch_bounds__(kCcBlock) void k_cc_union(const CcParams p)
{
    constexpr int kMaxL1 = CONN == 6 ? 1 : CONN == 18 ? 2 : 3;
    const uint64_t s = (uint64_t)blockIdx.x * kCcBlock + threadIdx.x;
    if (s >= p.S) return;
    const uint32_t i = (uint32_t)p.records[s];
    uint32_t ix, iy, iz;
    decompose(i, p.nx, p.ny, ix, iy, iz);
    const uint64_t wi = p.words[i >> 6];
    const bool inrun = (i & 63u) != 0 && iy != 0 && ((wi >> ((i & 63u) - 1)) & 1ull);   // record s - 1 is voxel i - 1, same run
#pragma unroll
    for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const bool neg = dz < 0 || (dz == 0 && (dx < 0 || (dx == 0 && dy < 0)));
                const int l1 = (dx != 0) + (dy != 0) + (dz != 0);
                if (!neg || l1 > kMaxL1) continue;
                if (dz == 0 && dx == 0) {                        // (0, -1, 0): voxel i - 1
                    if (inrun || iy == 0) continue;
                } else {
                    if ((dz < 0 && iz == 0) || (dx < 0 && ix == 0) || (dx > 0 && ix + 1 >= p.nx)) continue;
                    if ((dy < 0 && iy == 0) || (dy > 0 && iy + 1 >= p.ny)) continue;
                }
                const uint32_t jy = iy + dy, jx = ix + dx, jz = iz + dz;
                const uint32_t j = (jz * p.nx + jx) * p.ny + jy;
                const uint64_t wj = p.words[j >> 6];
                const uint32_t bj = j & 63u;
                if (!((wj >> bj) & 1ull)) continue;
                // the record before s in its run has neighbour j - 1 at the same offset; when j - 1 is in j's run that union is made
                if (inrun && (dz != 0 || dx != 0) && bj != 0 && jy != 0 && ((wj >> (bj - 1)) & 1ull)) continue;
                uf_union(p.parent, (uint32_t)s, p.woff[j >> 6] + (uint32_t)__popcll(wj & cc_below(bj)));
            }
}

__global__ __launch_bounds__(kCcBlock) void k_cc_compress(const CcParams p)
{
    const uint64_t s = (uint64_t)blockIdx.x * kCcBlock + threadIdx.x;
    if (s >= p.S) return;
    const uint32_t r = uf_find(p.parent, (uint32_t)s);
    p.parent[s] = r;                                             // (a valid ancestor for every concurrent find)
    p.label[s] = (uint32_t)p.records[r];
}

// Selectors of the compactions (vc_compact.h).  The roots, stably: roots[k] = s and cid[s] = k for the k-th root s.
struct CcRoots {
    const uint32_t *parent;
    uint32_t *roots, *cid;
    __device__ bool pick(uint64_t s) const { return parent[s] == (uint32_t)s; }
    __device__ void drop(uint64_t) const {}
    __device__ void put(uint64_t s, uint64_t d) const { roots[d] = (uint32_t)s; cid[s] = (uint32_t)d; }
};

// The records of the kept components, copied to out; a dropped record leaves its occupancy word (64-bit atomicAnd: neighbours
// share words).
struct CcKept {
    const uint32_t *parent, *cid;
    const uint8_t *kept;
    const uint64_t *records;
    uint64_t *words;
    uint64_t *out;
    __device__ bool pick(uint64_t s) const { return kept[cid[parent[s]]] != 0; }
    __device__ void drop(uint64_t s) const
    {
        const uint32_t i = (uint32_t)records[s];
        atomicAnd((unsigned long long *)(words + (i >> 6)), ~(1ull << (i & 63u)));
    }
    __device__ void put(uint64_t s, uint64_t d) const { out[d] = records[s]; }
};

__global__ __launch_bounds__(kCcBlock) void k_cc_clear(const CcParams p, uint32_t K)
{
    const uint32_t k = blockIdx.x * kCcBlock + threadIdx.x;
    if (k >= K) return;
    p.size[k] = 0;
    uint32_t *bx = p.box + (size_t)k * 6;
    bx[0] = bx[1] = bx[2] = 0xffffffffu;
    bx[3] = bx[4] = bx[5] = 0;
}

// One component's partial size and box into the totals.  A box atomic is made only when it would change the stored value
// (lo only falls, hi only rises: a stale read costs an atomic too many, never a wrong skip) -- the body's box is settled
// after a few workgroups, and its size takes one atomic per workgroup.
__device__ __forceinline__ void cc_flush(const CcParams &p, uint32_t k, uint32_t n, const uint32_t lo[3], const uint32_t hi[3])
{
    if (!n) return;
    atomicAdd(p.size + k, n);
    uint32_t *bx = p.box + (size_t)k * 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (lo[a] < cc_load(bx, a)) atomicMin(bx + a, lo[a]);
        if (hi[a] > cc_load(bx, 3 + a)) atomicMax(bx + 3 + a, hi[a]);
    }
}

// Component sizes and boxes (size zeroed, box lo at 0xffffffff, hi at 0 beforehand).  Workgroup g takes records
// g kCompactGroup + r kCcBlock + t, r = 0 .. kCompactPer - 1; a lane sums while its records stay in one component, a wave whose lanes
// all hold the same one reduces, and the workgroup's waves that agree merge in LDS: the body, which holds nearly every
// voxel, takes one set of atomics per workgroup (unreduced, every record's atomics would hit one address).
__global__ __launch_bounds__(kCcBlock) void k_cc_stats(const CcParams p)
{
    __shared__ uint32_t s_k[kCcBlock / 64], s_v[kCcBlock / 64][7];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kCompactGroup;
    uint32_t kc = 0xffffffffu, n = 0, lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0, 0, 0};
    for (uint32_t r = 0; r < kCompactPer; ++r) {
        const uint64_t s = base + (uint64_t)r * kCcBlock + t;
        if (s >= p.S) break;
        const uint32_t k = p.cid[p.parent[s]];
        uint32_t c[3];
        decompose((uint32_t)p.records[s], p.nx, p.ny, c[0], c[1], c[2]);
        if (k != kc) {
            if (n) cc_flush(p, kc, n, lo, hi);
            kc = k; n = 0;
            lo[0] = lo[1] = lo[2] = 0xffffffffu; hi[0] = hi[1] = hi[2] = 0;
        }
        n += 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], c[a]); hi[a] = max(hi[a], c[a]); }
    }
    // lanes without records hold n = 0 and neutral values: they agree with any component
    const uint32_t k0 = wave_min_u32(n ? kc : 0xffffffffu);
    const bool uniform = __ballot(n != 0 && kc != k0) == 0;
    if (!uniform) {
        cc_flush(p, kc, n, lo, hi);
        if (lane == 0) s_k[wave] = 0xffffffffu;
    } else {
        const uint32_t wn = wave_sum_u32(n);
        uint32_t wl[3], wh[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { wl[a] = wave_min_u32(lo[a]); wh[a] = wave_max_u32(hi[a]); }
        if (lane == 0) {
            s_k[wave] = wn ? k0 : 0xffffffffu;
            s_v[wave][0] = wn;
            for (int a = 0; a < 3; ++a) { s_v[wave][1 + a] = wl[a]; s_v[wave][4 + a] = wh[a]; }
        }
    }
    __syncthreads();
    if (t == 0) {                                                // consecutive waves of one component merged, then flushed
        uint32_t k = 0xffffffffu, m = 0, l[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, h[3] = {0, 0, 0};
        for (uint32_t w = 0; w < kCcBlock / 64; ++w) {
            if (s_k[w] == 0xffffffffu) continue;
            if (s_k[w] != k) {
                if (m) cc_flush(p, k, m, l, h);
                k = s_k[w]; m = 0;
                l[0] = l[1] = l[2] = 0xffffffffu; h[0] = h[1] = h[2] = 0;
            }
            m += s_v[w][0];
            for (int a = 0; a < 3; ++a) { l[a] = min(l[a], s_v[w][1 + a]); h[a] = max(h[a], s_v[w][4 + a]); }
        }
        if (m) cc_flush(p, k, m, l, h);
    }
}

__device__ __forceinline__ uint64_t cc_key(const uint32_t *size, uint32_t k)
{
    return ((uint64_t)size[k] << 32) | (uint64_t)(0xffffffffu - k);
}

// thr[0] = the `want`-th largest key (1-based, want <= K), by eight passes of 8-bit digits from the top; the keys are unique,
// so exactly `want` components have a key >= thr[0].  want == 0: thr[0] = 0 (no rank limit).
__global__ __launch_bounds__(kCcSelectBlock) void k_cc_select(const uint32_t *__restrict__ size, uint32_t K, uint32_t want,
                                                               uint64_t *__restrict__ thr)
{
    __shared__ uint32_t hist[256];
    __shared__ uint64_t s_prefix, s_mask;
    __shared__ uint32_t s_rem;
    const uint32_t t = threadIdx.x;
    if (want == 0) {
        if (t == 0) thr[0] = 0;
        return;
    }
    if (t == 0) { s_prefix = 0; s_mask = 0; s_rem = want; }
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (t < 256) hist[t] = 0;
        __syncthreads();
        const uint64_t prefix = s_prefix, mask = s_mask;
        for (uint32_t k = t; k < K; k += kCcSelectBlock) {
            const uint64_t key = cc_key(size, k);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (t == 0) {
            uint32_t rem = s_rem;
            int d = 255;
            for (; d > 0; --d) {
                if (rem <= hist[d]) break;
                rem -= hist[d];
            }
            s_rem = rem;
            s_prefix = prefix | ((uint64_t)d << shift);
            s_mask = mask | (255ull << shift);
        }
        __syncthreads();
    }
    if (t == 0) thr[0] = s_prefix;
}

// misc[0] += kept components, misc[1] = max size
__global__ __launch_bounds__(kCcBlock) void k_cc_mark(const CcParams p, uint32_t K, uint64_t min_voxels, const uint64_t *__restrict__ thr,
                                                       uint8_t *__restrict__ kept, uint32_t *__restrict__ comp, uint32_t *__restrict__ misc)
{
    const uint32_t k = blockIdx.x * kCcBlock + threadIdx.x;
    bool keep = false;
    uint32_t sz = 0;
    if (k < K) {
        sz = p.size[k];
        keep = (uint64_t)sz >= min_voxels && cc_key(p.size, k) >= thr[0];
        kept[k] = keep ? 1 : 0;
        uint32_t *c = comp + (size_t)k * kCcCompWords;
        const uint32_t *bx = p.box + (size_t)k * 6;
        c[0] = (uint32_t)p.records[p.roots[k]];
        c[1] = sz;
        for (int a = 0; a < 6; ++a) c[2 + a] = bx[a];
        c[8] = keep ? 1u : 0u;
        c[9] = 0u;
    }
    const uint32_t n = (uint32_t)__popcll(__ballot(keep));
    const uint32_t m = wave_max_u32(sz);
    if ((threadIdx.x & 63u) == 0) {
        if (n) atomicAdd(misc + 0, n);
        if (m) atomicMax(misc + 1, m);
    }
}

}  // namespace vc
