// gfx950 kernels of the temporal vote over the last hulls (vc_hull_temporal; contract in include/voxcarve.h and DESIGN.md section 8
// item 17).  The pass keeps a ring of `window` occupancy snapshots and its previous output P on the device; a voxel's count over
// the ring is never formed per voxel: the snapshots' words are summed in four bit planes, 64 voxels per word operation.
// Restated in tests/temporal_np.py.
//
//   k_temporal_vote    lane = two adjacent occupancy words (16-byte loads; every buffer of the pass holds an even number of words
//                      with a zeroed pad, the result's own words are longer than that by their padding to kLutPad voxels): the
//                      current words, the m - 1 older snapshots and P; the count planes by carry-save adders; the planes against
//                      the launch-uniform thresholds `on` and `off`, bit-sliced; O = (c >= on) | (P & (c >= off)) to the staging
//                      buffer.  |O|, added, removed, raw_changed and out_changed are popcounts, summed over the wave and the
//                      workgroup: one atomic per counter per workgroup.  The result's words are only read
//   k_cc_wcount, scan_counts, k_cc_woff   (vc_components.h) survivors before each word of O
//   k_merge_old        (vc_merge.h) every old record whose bit is in O to its new rank
//   k_temporal_new     lane = word of O: the planes again from the ring (which now holds the newest snapshot), the vote byte of each
//                      set bit at its rank; RECORDS: a fresh record (merge_fresh, vc_merge.h) for each bit of O & ~H_t
// Every word index is checked against nwords before it is used, every rank against S1.
#pragma once
#include "vc_merge.h"            // MergeParams, merge_fresh, kMergeBlock (vc_components.h: cc_below; vc_kernels.h: wave_sum_u32)

namespace vc {

constexpr uint32_t kTemporalBlock = 256;
constexpr uint32_t kTemporalCounters = 5;                    // |O|, added, removed, raw_changed, out_changed

struct TemporalParams {
    const uint64_t *ring;       // [window][npad] snapshots; slot `head` is the newest
    const uint64_t *cur;        // k_temporal_vote: the result's words, H_t (not yet in the ring)
    const uint64_t *prev;       // P, [npad] (null: empty)
    uint64_t *stage;            // [npad] O
    unsigned long long *ctr;    // [kTemporalCounters], zeroed
    uint64_t nwords, npad, n;   // occupancy words, the even word count of the pass's buffers, voxels
    uint32_t window, head;
    uint32_t count;             // snapshots to read from `head` backwards: m - 1 (vote), m (new)
    uint32_t on, off;
};

// two adjacent words, loaded and stored as one 16-byte access
struct alignas(16) Word2 { uint64_t x, y; };
__device__ __forceinline__ Word2 operator&(Word2 a, Word2 b) { return {a.x & b.x, a.y & b.y}; }
__device__ __forceinline__ Word2 operator|(Word2 a, Word2 b) { return {a.x | b.x, a.y | b.y}; }
__device__ __forceinline__ Word2 operator^(Word2 a, Word2 b) { return {a.x ^ b.x, a.y ^ b.y}; }
__device__ __forceinline__ Word2 operator~(Word2 a) { return {~a.x, ~a.y}; }
__device__ __forceinline__ uint32_t tp_pop(uint64_t a) { return (uint32_t)__popcll(a); }
__device__ __forceinline__ uint32_t tp_pop(Word2 a) { return (uint32_t)__popcll(a.x) + (uint32_t)__popcll(a.y); }

// the bits of word w that are voxels of a grid of n
__device__ __forceinline__ uint64_t tp_valid(uint64_t w, uint64_t n)
{
    const uint64_t lo = w << 6;
    return lo + 64u <= n ? ~0ull : (lo < n ? cc_below((uint32_t)(n - lo)) : 0ull);
}

// the count of each of a word's 64 voxels in four bit planes (b0 = ones .. b3 = eights); counts stay below 16
template <typename T>
struct Planes { T b0, b1, b2, b3; };

template <typename T>
__device__ __forceinline__ void tp_add1(Planes<T> &p, T x)
{
    const T c1 = p.b0 & x;
    p.b0 = p.b0 ^ x;
    const T c2 = p.b1 & c1;
    p.b1 = p.b1 ^ c1;
    const T c4 = p.b2 & c2;
    p.b2 = p.b2 ^ c2;
    p.b3 = p.b3 ^ c4;
}

// two words at once: one carry-save adder (ones, x, y) -> (carry of weight 2, ones), then the carry ripples up
template <typename T>
__device__ __forceinline__ void tp_add2(Planes<T> &p, T x, T y)
{
    const T u = x ^ y;
    const T c2 = (x & y) | (u & p.b0);
    p.b0 = u ^ p.b0;
    const T c4 = p.b1 & c2;
    p.b1 = p.b1 ^ c2;
    const T c8 = p.b2 & c4;
    p.b2 = p.b2 ^ c4;
    p.b3 = p.b3 ^ c8;
}

// the voxels whose count is >= t, 1 <= t <= 15 (launch-uniform: the branches are scalar)
template <typename T>
__device__ __forceinline__ T tp_ge(const Planes<T> &p, uint32_t t)
{
    const T b[4] = {p.b0, p.b1, p.b2, p.b3};
    T gt = T{}, eq = ~T{};
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        if ((t >> k) & 1u) eq = eq & b[k];
        else { gt = gt | (eq & b[k]); eq = eq & ~b[k]; }
    }
    return gt | eq;
}

// snapshots `from` .. count - 1 (0 = slot head, then backwards round the ring) of the words at `w` into the planes, two per step
template <typename T>
__device__ __forceinline__ void tp_count(const TemporalParams &p, uint64_t w, uint32_t from, Planes<T> &pl)
{
    uint32_t a = from;
    for (; a + 1 < p.count; a += 2) {
        const uint32_t s0 = (p.head + p.window - a) % p.window, s1 = (p.head + p.window - a - 1) % p.window;
        const T x = *reinterpret_cast<const T *>(p.ring + (uint64_t)s0 * p.npad + w);
        const T y = *reinterpret_cast<const T *>(p.ring + (uint64_t)s1 * p.npad + w);
        tp_add2(pl, x, y);
    }
    if (a < p.count) {
        const uint32_t s0 = (p.head + p.window - a) % p.window;
        tp_add1(pl, *reinterpret_cast<const T *>(p.ring + (uint64_t)s0 * p.npad + w));
    }
}

__global__ __launch_bounds__(kTemporalBlock) void k_temporal_vote(const TemporalParams p)
{
    __shared__ uint32_t s_cnt[kTemporalBlock / 64][kTemporalCounters];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t w = ((uint64_t)blockIdx.x * kTemporalBlock + threadIdx.x) * 2u;
    uint32_t c[kTemporalCounters] = {0, 0, 0, 0, 0};
    if (w < p.nwords) {                                          // (w is even: w + 1 < npad)
        const Word2 valid = {tp_valid(w, p.n), w + 1 < p.nwords ? tp_valid(w + 1, p.n) : 0ull};
        const Word2 h = *reinterpret_cast<const Word2 *>(p.cur + w) & valid;
        Planes<Word2> pl = {h, Word2{}, Word2{}, Word2{}};
        Word2 h1 = Word2{};
        if (p.count) {                                           // H_{t-1}, kept for raw_changed
            h1 = *reinterpret_cast<const Word2 *>(p.ring + (uint64_t)p.head * p.npad + w) & valid;
            tp_add1(pl, h1);
        }
        tp_count(p, w, 1u, pl);
        const Word2 prev = p.prev ? *reinterpret_cast<const Word2 *>(p.prev + w) & valid : Word2{};
        const Word2 o = (tp_ge(pl, p.on) | (prev & tp_ge(pl, p.off))) & valid;
        *reinterpret_cast<Word2 *>(p.stage + w) = o;
        c[0] = tp_pop(o);
        c[1] = tp_pop(o & ~h);
        c[2] = tp_pop(h & ~o);
        c[3] = p.count ? tp_pop(h ^ h1) : 0u;
        c[4] = tp_pop(o ^ prev);
    }
#pragma unroll
    for (uint32_t k = 0; k < kTemporalCounters; ++k) {
        const uint32_t s = wave_sum_u32(c[k]);
        if (lane == 0) s_cnt[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kTemporalCounters) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t v = 0; v < kTemporalBlock / 64; ++v) sum += s_cnt[v][threadIdx.x];
        if (sum) atomicAdd(p.ctr + threadIdx.x, (unsigned long long)sum);
    }
}

template <bool RECORDS>
__global__ __launch_bounds__(kMergeBlock) void k_temporal_new(const MergeParams g, const TemporalParams p, uint8_t *__restrict__ votes)
{
    const uint64_t w = (uint64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (w >= p.nwords) return;
    const uint64_t o = g.words[w] & tp_valid(w, p.n);
    if (!o) return;
    Planes<uint64_t> pl = {0, 0, 0, 0};
    tp_count(p, w, 0u, pl);
    const uint64_t fresh = RECORDS ? o & ~p.ring[(uint64_t)p.head * p.npad + w] : 0ull;
    const uint64_t rank0 = g.woff[w];
    uint64_t a = o;
    while (a) {
        const uint32_t b = (uint32_t)__ffsll((unsigned long long)a) - 1u;
        a &= a - 1;
        const uint64_t r = rank0 + (uint32_t)__popcll(o & cc_below(b));
        if (r >= g.S1) continue;
        votes[r] = (uint8_t)(((pl.b0 >> b) & 1ull) | (((pl.b1 >> b) & 1ull) << 1) | (((pl.b2 >> b) & 1ull) << 2) | (((pl.b3 >> b) & 1ull) << 3));
        if (RECORDS && ((fresh >> b) & 1ull)) merge_fresh(g, (w << 6) + b, r);
    }
}

}  // namespace vc
