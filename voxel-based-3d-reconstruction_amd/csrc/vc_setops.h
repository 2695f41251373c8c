// gfx950 kernels of the set algebra on hulls (vc_hull_keep / vc_hull_upload, vc_hull_combine, vc_hull_compare; contract in
// include/voxcarve.h and DESIGN.md section 8 item 21).  A is the current result's occupancy, B a kept hull's: words of the same
// layout in a buffer of an even word count with a zeroed pad, so that two words load as 16 bytes.  Restated in tests/setops_np.py.
//
//   k_kept_bits        lane = word of an uploaded occupancy: its popcount, and an error for a set bit at or beyond n
//   k_kept_records     lane = uploaded record: an error unless its index is below n and above its predecessor's; its bit into the
//                      words by a 64-bit atomic
//   k_setop_words      lane = two adjacent words of A and B (16-byte loads); the launch-uniform op (its branches are scalar), the
//                      valid-bit mask, R to the staging buffer; |R|, |A & B|, |R \ A|, |A \ R| are popcounts, summed over the wave
//                      and the workgroup: one atomic per counter per workgroup.  The result's words are only read
//   k_setop_commit     lane = two adjacent words: R into the result's words, A into the staging buffer (the kernels below ask
//                      which voxels are new)
//   k_cc_wcount, scan_counts, k_cc_woff   (vc_components.h) survivors before each word of R
//   k_merge_old        (vc_merge.h) every record of A whose bit is in R to its new rank
//   k_merge_from       lane = record of B: to its new rank when its bit is in R and the voxel is new or the op is COPY; the
//                      `added` byte of a new voxel
//   k_setop_fresh      lane = word of R & ~A: a fresh record (merge_fresh, vc_merge.h) for each bit at its rank
//   k_compare_words    lane = two adjacent words of A and B: |A & B|, |A \ B|, |B \ A| as above, and the index boxes of A ^ B and
//                      A | B by y-line segments of each word (a segment's lowest and highest bit), reduced over the wave
//   k_compare_max / k_compare_arg   lane = word of the one-sided difference: the maximum of the box field over its voxels, then the
//                      smallest index among the voxels that attain it
// Every word index is checked against nwords before it is used, every rank against S1, every cell against the box.
#pragma once
#include "vc_temporal.h"         // Word2, tp_pop, tp_valid (vc_merge.h: MergeParams, merge_fresh, kMergeBlock)
#include "vc_distance.h"         // DistBox

namespace vc {

constexpr uint32_t kSetopBlock = 256;
constexpr uint32_t kSetopCounters = 4;                       // |R|, |A & B|, |R \ A|, |A \ R|
constexpr uint32_t kCompareCounters = 3;                     // |A & B|, |A \ B|, |B \ A|

enum { kSetopCopy = 0, kSetopAnd = 1, kSetopOr = 2, kSetopAndNot = 3, kSetopXor = 4 };

__global__ __launch_bounds__(kSetopBlock) void k_kept_bits(const uint64_t *__restrict__ words, uint64_t nwords, uint64_t n,
                                                            unsigned long long *__restrict__ ctr /* [0] count, [1] errors */)
{
    __shared__ uint32_t s_cnt[kSetopBlock / 64][2];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * kSetopBlock + threadIdx.x;
    uint32_t c = 0, bad = 0;
    if (w < nwords) {
        const uint64_t v = words[w], valid = tp_valid(w, n);
        c = tp_pop(v & valid);
        bad = (v & ~valid) ? 1u : 0u;
    }
    c = wave_sum_u32(c); bad = wave_sum_u32(bad);
    if (lane == 0) { s_cnt[wave][0] = c; s_cnt[wave][1] = bad; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kSetopBlock / 64; ++v) sum += s_cnt[v][threadIdx.x];
        if (sum) atomicAdd(ctr + threadIdx.x, (unsigned long long)sum);
    }
}

// words: zeroed beforehand
__global__ __launch_bounds__(kSetopBlock) void k_kept_records(const uint64_t *__restrict__ records, uint64_t S, uint64_t nwords, uint64_t n,
                                                               unsigned long long *__restrict__ words, unsigned long long *__restrict__ ctr)
{
    const uint64_t s = (uint64_t)blockIdx.x * kSetopBlock + threadIdx.x;
    if (s >= S) return;
    const uint32_t i = (uint32_t)records[s];
    const bool ordered = s == 0 || (uint32_t)records[s - 1] < i;
    const uint64_t w = i >> 6;
    if (!ordered || i >= n || w >= nwords) { atomicAdd(ctr + 1, 1ull); return; }
    atomicOr(words + w, 1ull << (i & 63u));
}

struct SetopParams {
    const uint64_t *a, *b;      // the result's words (at least npad of them), the register's [npad]
    uint64_t *stage;            // [npad] R
    unsigned long long *ctr;    // [kSetopCounters], zeroed
    uint64_t nwords, n;
    uint32_t op;
};

__device__ __forceinline__ Word2 setop_apply(uint32_t op, Word2 a, Word2 b)
{
    switch (op) {                                                // (launch-uniform)
    case kSetopCopy: return b;
    case kSetopAnd: return a & b;
    case kSetopOr: return a | b;
    case kSetopAndNot: return a & ~b;
    default: return a ^ b;
    }
}

__device__ __forceinline__ Word2 setop_valid(uint64_t w, uint64_t nwords, uint64_t n)    // w even
{
    return {tp_valid(w, n), w + 1 < nwords ? tp_valid(w + 1, n) : 0ull};
}

template <uint32_t N>
__device__ __forceinline__ void setop_sums(uint32_t (&c)[N], uint32_t (*s_cnt)[N], unsigned long long *ctr)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
        const uint32_t s = wave_sum_u32(c[k]);
        if (lane == 0) s_cnt[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kSetopBlock / 64; ++v) sum += s_cnt[v][threadIdx.x];
        if (sum) atomicAdd(ctr + threadIdx.x, (unsigned long long)sum);
    }
}

__global__ __launch_bounds__(kSetopBlock) void k_setop_words(const SetopParams p)
{
    __shared__ uint32_t s_cnt[kSetopBlock / 64][kSetopCounters];
    const uint64_t w = ((uint64_t)blockIdx.x * kSetopBlock + threadIdx.x) * 2u;
    uint32_t c[kSetopCounters] = {0, 0, 0, 0};
    if (w < p.nwords) {                                          // (w is even: w + 1 < npad)
        const Word2 valid = setop_valid(w, p.nwords, p.n);
        const Word2 a = *reinterpret_cast<const Word2 *>(p.a + w) & valid;
        const Word2 b = *reinterpret_cast<const Word2 *>(p.b + w) & valid;
        const Word2 r = setop_apply(p.op, a, b) & valid;
        *reinterpret_cast<Word2 *>(p.stage + w) = r;
        c[0] = tp_pop(r);
        c[1] = tp_pop(a & b);
        c[2] = tp_pop(r & ~a);
        c[3] = tp_pop(a & ~r);
    }
    setop_sums(c, s_cnt, p.ctr);
}

// words <- stage (R), stage <- the words' valid bits (A)
__global__ __launch_bounds__(kSetopBlock) void k_setop_commit(uint64_t *__restrict__ words, uint64_t *__restrict__ stage, uint64_t nwords, uint64_t n)
{
    const uint64_t w = ((uint64_t)blockIdx.x * kSetopBlock + threadIdx.x) * 2u;
    if (w >= nwords) return;
    const Word2 a = *reinterpret_cast<const Word2 *>(words + w) & setop_valid(w, nwords, n);
    const Word2 r = *reinterpret_cast<const Word2 *>(stage + w);
    if (w + 1 < nwords) *reinterpret_cast<Word2 *>(words + w) = r;
    else words[w] = r.x;                                         // (the word behind the last belongs to the result's own padding)
    *reinterpret_cast<Word2 *>(stage + w) = a;
}

// p.words = R; a = A's words, or null when no voxel is new
__global__ __launch_bounds__(kMergeBlock) void k_merge_from(const MergeParams p, const uint64_t *__restrict__ records, uint64_t SB, uint64_t nwords,
                                                             const uint64_t *__restrict__ a, int copy)
{
    const uint64_t s = (uint64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (s >= SB) return;
    const uint64_t rec = records[s];
    const uint32_t i = (uint32_t)rec, w = i >> 6, b = i & 63u;
    if (w >= nwords) return;
    const uint64_t o = p.words[w];
    if (!((o >> b) & 1ull)) return;
    const bool fresh = a ? !((a[w] >> b) & 1ull) : false;
    if (!fresh && !copy) return;
    const uint64_t r = (uint64_t)p.woff[w] + (uint32_t)__popcll(o & cc_below(b));
    if (r >= p.S1) return;
    p.out[r] = rec;
    if (fresh) p.added[r] = 1;
}

__global__ __launch_bounds__(kMergeBlock) void k_setop_fresh(const MergeParams p, const uint64_t *__restrict__ a, uint64_t nwords, uint64_t n)
{
    const uint64_t w = (uint64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (w >= nwords) return;
    const uint64_t o = p.words[w] & tp_valid(w, n);
    uint64_t f = o & ~a[w];
    if (!f) return;
    const uint64_t rank0 = p.woff[w];
    while (f) {
        const uint32_t b = (uint32_t)__ffsll((unsigned long long)f) - 1u;
        f &= f - 1;
        const uint64_t r = rank0 + (uint32_t)__popcll(o & cc_below(b));
        if (r < p.S1) merge_fresh(p, (w << 6) + b, r);
    }
}

struct CompareParams {
    const uint64_t *a, *b;
    unsigned long long *ctr;    // [kCompareCounters], zeroed
    uint32_t *box;              // [12]: lo[3], hi[3] of A ^ B, then of A | B; lo = UINT32_MAX, hi = 0 beforehand
    uint64_t nwords, n;
    uint32_t nx, ny, nz;
};

// the index box of the set bits of word w: its y-line segments one after the other, each by its lowest and highest bit
__device__ __forceinline__ void compare_box(uint64_t m, uint64_t w, uint32_t nx, uint32_t ny, uint32_t *lo, uint32_t *hi)
{
    while (m) {
        const uint32_t b = (uint32_t)__ffsll((unsigned long long)m) - 1u;
        uint32_t ix, iy, iz;
        decompose((uint32_t)((w << 6) + b), nx, ny, ix, iy, iz);
        const uint32_t len = min(ny - iy, 64u - b);              // the rest of the y line inside the word
        const uint64_t seg = (len >= 64u ? ~0ull : cc_below(len)) << b;
        const uint64_t s = m & seg;
        const uint32_t top = iy + (63u - (uint32_t)__clzll((long long)s)) - b;
        lo[0] = min(lo[0], ix); lo[1] = min(lo[1], iy); lo[2] = min(lo[2], iz);
        hi[0] = max(hi[0], ix); hi[1] = max(hi[1], top); hi[2] = max(hi[2], iz);
        m &= ~seg;
    }
}

__global__ __launch_bounds__(kSetopBlock) void k_compare_words(const CompareParams p)
{
    __shared__ uint32_t s_cnt[kSetopBlock / 64][kCompareCounters];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = ((uint64_t)blockIdx.x * kSetopBlock + threadIdx.x) * 2u;
    uint32_t c[kCompareCounters] = {0, 0, 0};
    uint32_t lo[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[6] = {0, 0, 0, 0, 0, 0};
    if (w < p.nwords) {
        const Word2 valid = setop_valid(w, p.nwords, p.n);
        const Word2 a = *reinterpret_cast<const Word2 *>(p.a + w) & valid;
        const Word2 b = *reinterpret_cast<const Word2 *>(p.b + w) & valid;
        c[0] = tp_pop(a & b);
        c[1] = tp_pop(a & ~b);
        c[2] = tp_pop(b & ~a);
        const Word2 d = a ^ b, u = a | b;
        compare_box(d.x, w, p.nx, p.ny, lo, hi);
        compare_box(d.y, w + 1, p.nx, p.ny, lo, hi);
        compare_box(u.x, w, p.nx, p.ny, lo + 3, hi + 3);
        compare_box(u.y, w + 1, p.nx, p.ny, lo + 3, hi + 3);
    }
    // a wave makes an atomic only when it would change the stored value (lo only falls, hi only rises)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t l = wave_min_u32(lo[k]), h = wave_max_u32(hi[k]);
        const uint32_t at = (uint32_t)(k < 3 ? k : k + 3);
        if (lane == 0 && l != 0xffffffffu) {
            if (l < p.box[at]) atomicMin(p.box + at, l);
            if (h > p.box[at + 3]) atomicMax(p.box + at + 3, h);
        }
    }
    setop_sums(c, s_cnt, p.ctr);
}

// cell of voxel i in the box field, or false when the voxel lies off the box
__device__ __forceinline__ bool compare_cell(const DistBox &bx, uint32_t i, uint64_t &cell)
{
    uint32_t ix, iy, iz;
    decompose(i, bx.nx, bx.ny, ix, iy, iz);
    const int64_t lx = (int64_t)ix - bx.o[0], ly = (int64_t)iy - bx.o[1], lz = (int64_t)iz - bx.o[2];
    if (lx < 0 || ly < 0 || lz < 0 || lx >= (int64_t)bx.b[0] || ly >= (int64_t)bx.b[1] || lz >= (int64_t)bx.b[2]) return false;
    cell = ((uint64_t)lz * bx.b[0] + (uint64_t)lx) * bx.b[1] + (uint64_t)ly;
    return true;
}

// acc[0] = max over the voxels of x & ~y of f (ARG = false); acc[1] = the smallest index among those with f == acc[0] (ARG = true)
template <bool ARG>
__global__ __launch_bounds__(kSetopBlock) void k_compare_far(const DistBox bx, const uint64_t *__restrict__ f, const uint64_t *__restrict__ x,
                                                              const uint64_t *__restrict__ y, uint64_t nwords, uint64_t n,
                                                              unsigned long long *__restrict__ acc)
{
    const uint64_t w = (uint64_t)blockIdx.x * kSetopBlock + threadIdx.x;
    if (w >= nwords) return;
    uint64_t d = x[w] & ~y[w] & tp_valid(w, n);
    if (!d) return;
    const uint64_t want = ARG ? acc[0] : 0ull;
    uint64_t mx = 0;
    uint32_t arg = 0xffffffffu;
    bool any = false;
    while (d) {
        const uint32_t b = (uint32_t)__ffsll((unsigned long long)d) - 1u;
        d &= d - 1;
        const uint32_t i = (uint32_t)((w << 6) + b);
        uint64_t cell;
        if (!compare_cell(bx, i, cell)) continue;
        const uint64_t v = f[cell];
        any = true;
        if (ARG) { if (v == want && i < arg) arg = i; }          // (ascending bits: the first match is the smallest)
        else mx = v > mx ? v : mx;
    }
    if (ARG) { if (arg != 0xffffffffu && arg < acc[1]) atomicMin(acc + 1, (unsigned long long)arg); }
    else if (any && mx > acc[0]) atomicMax(acc, (unsigned long long)mx);
}

}  // namespace vc
