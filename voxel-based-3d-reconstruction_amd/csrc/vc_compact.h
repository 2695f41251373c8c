// gfx950 stable compaction of records [0, S) by a selector: the passes over the current carve result (vc_photo.h,
// vc_components.h) keep or list a subset of the records in record order.
//
//   k_compact_count<Sel>    workgroup = kCompactGroup records: how many sel.pick(s); sel.drop(s) for every other record
//   k_compact_scatter<Sel>  the same records, sel.put(s, d) for the picked ones with d their scanned position (stable)
//
// Between the two, scan_counts (voxcarve.hip) turns the counts into offsets.  A selector is a small struct passed by value:
//   bool pick(uint64_t s) const      record s is kept; the same answer in both kernels
//   void drop(uint64_t s) const      (count only) a record that is not picked; empty where nothing is to be done
//   void put(uint64_t s, uint64_t d) const   (scatter only) record s is the d-th picked one
#pragma once
#include "vc_kernels.h"          // kScanBlock, wave_sum_u32

namespace vc {

constexpr uint32_t kCompactBlock = 256;
constexpr uint32_t kCompactPer = 16;                             // records per lane
constexpr uint32_t kCompactGroup = kCompactBlock * kCompactPer;  // records per group (<= 4096: the scan's u32 block sums hold)

// lane t of workgroup g looks at records g kCompactGroup + r kCompactBlock + t, r = 0 .. kCompactPer - 1 (coalesced)
template <class Sel>
__global__ __launch_bounds__(kCompactBlock) void k_compact_count(uint64_t S, uint32_t *__restrict__ cnt, const Sel sel)
{
    __shared__ uint32_t s_wave[kCompactBlock / 64];
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kCompactGroup;
    uint32_t n = 0;
#pragma unroll 4
    for (uint32_t r = 0; r < kCompactPer; ++r) {
        const uint64_t s = base + (uint64_t)r * kCompactBlock + t;
        if (s >= S) continue;
        if (sel.pick(s)) n += 1;
        else sel.drop(s);
    }
    const uint32_t w = wave_sum_u32(n);
    if ((t & 63u) == 0) s_wave[t >> 6] = w;
    __syncthreads();
    if (t == 0) {
        uint32_t total = 0;
        for (uint32_t k = 0; k < kCompactBlock / 64; ++k) total += s_wave[k];
        cnt[blockIdx.x] = total;
    }
}

// The picked records of workgroup g go to boff[g / kScanBlock] + off[g] + (picked records of the group before them): order is
// r-major, then wave, then lane, which is ascending s -- the compaction is stable.
template <class Sel>
__global__ __launch_bounds__(kCompactBlock) void k_compact_scatter(uint64_t S, const uint32_t *__restrict__ off,
                                                                   const uint64_t *__restrict__ boff, const Sel sel)
{
    __shared__ uint32_t s_pos[kCompactPer][kCompactBlock / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kCompactGroup;
    uint32_t pick = 0;
#pragma unroll
    for (uint32_t r = 0; r < kCompactPer; ++r) {
        const uint64_t s = base + (uint64_t)r * kCompactBlock + t;
        const bool k = s < S && sel.pick(s);
        pick |= (uint32_t)k << r;
        const uint64_t b = __ballot(k);
        if (lane == 0) s_pos[r][wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (t == 0) {                                                // exclusive scan over (r, wave), r-major
        uint32_t run = 0;
        for (uint32_t r = 0; r < kCompactPer; ++r)
            for (uint32_t w = 0; w < kCompactBlock / 64; ++w) { const uint32_t v = s_pos[r][w]; s_pos[r][w] = run; run += v; }
    }
    __syncthreads();
    const uint64_t o = boff[blockIdx.x / kScanBlock] + off[blockIdx.x];
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t r = 0; r < kCompactPer; ++r) {
        const bool k = (pick >> r) & 1u;
        const uint64_t b = __ballot(k);
        if (k) sel.put(base + (uint64_t)r * kCompactBlock + t, o + s_pos[r][wave] + (uint32_t)__popcll(b & below));
    }
}

}  // namespace vc
