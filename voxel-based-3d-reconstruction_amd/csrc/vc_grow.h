// gfx950 kernels of the growing half of the hull's morphology (vc_hull_grow: dilation and closing by a ball in um; contract in
// include/voxcarve.h and DESIGN.md section 8 item 13).  The fields come from the transforms of vc_distance.h, unchanged; what is
// new here turns a thresholded box field into an ordered result that is LARGER than its input.  Restated in tests/closing_np.py.
//
//   k_grow_mark<MODE>  wave = kGrowLines y lines of the box, 64 cells per step: the cells of the new set are one ballot (f <= r2 for
//                      the dilation, f > r2 or "no site" for the closing).  A box line starts anywhere inside an occupancy word, so
//                      a step's bits fall into two words: lane 0 takes the low one, lane 1 the high one; the bits the hull does not
//                      have yet are OR-ed into the ADDED words (a zeroed copy of the word range the box spans) with 64-bit atomics,
//                      and only where there are such bits.  The hull's own words are not written: the count is read back and every
//                      buffer of the hand-over sized before the result changes.  Counts are summed over the workgroup's lines and
//                      make one atomic per workgroup.  MODE = kGrowCount only counts the cells with f <= r2 (|Dl| of a closing)
//   k_grow_apply       lane = word of the range: the added bits into the occupancy words
//   k_cc_wcount, scan_counts, k_cc_woff   (vc_components.h) survivors before each word of the new occupancy
//   k_merge_old        (vc_merge.h) every old record to its new rank
//   k_grow_new         lane = word of the range: a fresh record (merge_fresh, vc_merge.h) for each added bit at its rank
// Every index formed from the box is checked against the grid before it is used.
#pragma once
#include "vc_merge.h"            // MergeParams, merge_fresh (vc_components.h: cc_below; vc_kernels.h: wave_sum_u32)
#include "vc_distance.h"         // DistBox, kDistBlock, kDistInf

namespace vc {

constexpr uint32_t kGrowLines = 8;                           // y lines per wave of k_grow_mark
constexpr uint32_t kGrowBlock = 256;

enum { kGrowDilate = 0, kGrowClose = 1, kGrowCount = 2 };

template <int MODE>
__global__ __launch_bounds__(kDistBlock) void k_grow_mark(const DistBox bx, const uint64_t *__restrict__ f, uint64_t r2,
                                                           const uint64_t *__restrict__ words, uint64_t nwords,
                                                           unsigned long long *__restrict__ addw, uint64_t w0, uint64_t nrange,
                                                           unsigned long long *__restrict__ ctr)
{
    __shared__ uint32_t s_cnt[kDistBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t nlines = (uint64_t)bx.b[0] * bx.b[2];
    const uint64_t first = ((uint64_t)blockIdx.x * (kDistBlock / 64) + wave) * kGrowLines;
    const uint32_t by = bx.b[1], nchunks = (by + 63u) / 64u;
    uint32_t cnt = 0;                                            // kGrowCount: the same in every lane; else lanes 0 and 1 hold theirs
    for (uint32_t k = 0; k < kGrowLines; ++k) {
        const uint64_t line = first + k;
        if (line >= nlines) break;                               // (whole waves)
        const uint32_t lz = (uint32_t)(line / bx.b[0]), lx = (uint32_t)(line % bx.b[0]);
        const int32_t gx = bx.o[0] + (int32_t)lx, gy = bx.o[1], gz = bx.o[2] + (int32_t)lz;
        // the box is clipped to the grid: a line that is not inside it whole marks nothing
        if (gx < 0 || gy < 0 || gz < 0 || gx >= (int32_t)bx.nx || gz >= (int32_t)bx.nz || (uint64_t)gy + by > bx.ny) continue;
        const uint64_t base = ((uint64_t)gz * bx.nx + (uint32_t)gx) * bx.ny + (uint32_t)gy;
        const uint64_t *row = f + line * by;
        for (uint32_t c = 0; c < nchunks; ++c) {
            const uint32_t ly = c * 64u + lane;
            bool in = false;
            if (ly < by) {
                const uint64_t v = row[ly];
                in = MODE == kGrowClose ? (v > r2 || v == kDistInf) : v <= r2;
            }
            const uint64_t m = __ballot(in);
            if (MODE == kGrowCount) cnt += (uint32_t)__popcll(m);
            else if (m && lane < 2) {
                const uint64_t i0 = base + (uint64_t)c * 64u;
                const uint32_t sh = (uint32_t)(i0 & 63u);
                const uint64_t part = lane == 0 ? m << sh : (sh ? m >> (64u - sh) : 0ull);
                const uint64_t w = (i0 >> 6) + lane;
                if (part && w < nwords && w >= w0 && w - w0 < nrange) {
                    const uint64_t fresh = part & ~words[w];
                    if (fresh) {
                        atomicOr(addw + (w - w0), (unsigned long long)fresh);
                        cnt += (uint32_t)__popcll(fresh);
                    }
                }
            }
        }
    }
    if (MODE != kGrowCount) cnt = wave_sum_u32(lane < 2 ? cnt : 0u);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < kDistBlock / 64; ++w) sum += s_cnt[w];
        if (sum) atomicAdd(ctr, (unsigned long long)sum);
    }
}

__global__ __launch_bounds__(kGrowBlock) void k_grow_apply(uint64_t *__restrict__ words, uint64_t nwords,
                                                            const unsigned long long *__restrict__ addw, uint64_t w0, uint64_t nrange)
{
    const uint64_t k = (uint64_t)blockIdx.x * kGrowBlock + threadIdx.x;
    if (k >= nrange || w0 + k >= nwords) return;
    const uint64_t a = addw[k];
    if (a) words[w0 + k] |= a;
}

// addw: [nrange] added bits of words w0 ..
__global__ __launch_bounds__(kGrowBlock) void k_grow_new(const MergeParams p, const unsigned long long *__restrict__ addw, uint64_t w0,
                                                          uint64_t nrange, uint64_t nwords)
{
    const uint64_t k = (uint64_t)blockIdx.x * kGrowBlock + threadIdx.x;
    if (k >= nrange || w0 + k >= nwords) return;
    uint64_t a = addw[k];
    if (!a) return;
    const uint64_t w = w0 + k, nw = p.words[w];
    const uint64_t rank0 = p.woff[w];
    while (a) {
        const uint32_t b = (uint32_t)__ffsll((unsigned long long)a) - 1u;
        a &= a - 1;
        const uint64_t r = rank0 + (uint32_t)__popcll(nw & cc_below(b));
        if (r < p.S1) merge_fresh(p, (w << 6) + b, r);
    }
}

}  // namespace vc
