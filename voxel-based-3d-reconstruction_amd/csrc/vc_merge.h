// gfx950 kernels that make the records follow an occupancy which gained (and possibly lost) voxels: what vc_hull_grow and
// vc_hull_temporal share (host side: the merge route in voxcarve.hip).  Each walks the words with a kernel of its own.
//
//   k_merge_old        lane = old record: to its new rank woff[w] + popc(word & below), its 8 bytes unchanged, when its bit is set
//   merge_fresh        the fresh record of one voxel at its rank, coloured as the footprint carve colours (one float64 projection
//                      of the centre, the in-image test, one load from the colour camera's image in record layout; the mask is
//                      not consulted), and the record's `added` byte
#pragma once
#include "vc_components.h"       // cc_below (vc_kernels.h: decompose, kSeenFlag; vc_device.h: project_point, pixel_offset)

namespace vc {

constexpr uint32_t kMergeBlock = 256;

struct MergeParams {
    const double *xs, *ys, *zs;
    const uint32_t *frame;      // the colour camera's image, one dword per pixel in record layout (or null)
    const uint64_t *words;      // the NEW occupancy
    const uint32_t *woff;       // [nwords] survivors before each word of it
    uint64_t *out;              // [S1] the merged records
    uint8_t *added;             // [S1] 1 = created by this call (zeroed beforehand)
    uint64_t S1;
    uint32_t nx, ny, nz, H, W;
    int has_cam;
    CamDev cam;
};

__global__ __launch_bounds__(kMergeBlock) void k_merge_old(const MergeParams p, const uint64_t *__restrict__ records, uint64_t S0, uint64_t nwords)
{
    const uint64_t s = (uint64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (s >= S0) return;
    const uint64_t rec = records[s];
    const uint32_t i = (uint32_t)rec, w = i >> 6, b = i & 63u;
    if (w >= nwords) return;
    const uint64_t o = p.words[w];                               // (word and offset in one round trip: neither load waits for the test)
    const uint64_t r = (uint64_t)p.woff[w] + (uint32_t)__popcll(o & cc_below(b));
    if (((o >> b) & 1ull) && r < p.S1) p.out[r] = rec;           // a cleared bit: no longer in the hull
}

// r < p.S1 is the caller's to check; a voxel past the grid's last layer gets no record
__device__ __forceinline__ void merge_fresh(const MergeParams &p, uint64_t i, uint64_t r)
{
    uint32_t ix, iy, iz;
    decompose((uint32_t)i, p.nx, p.ny, ix, iy, iz);
    if (iz >= p.nz) return;
    uint64_t rec = (uint32_t)i;
    if (p.has_cam) {
        double u, v;
        project_point(p.cam, p.xs[ix], p.ys[iy], p.zs[iz], u, v);
        const int32_t off = pixel_offset(u, v, p.H, p.W);
        if (off >= 0) rec |= (p.frame ? (uint64_t)p.frame[off] : (uint64_t)kSeenFlag) << 32;   // R | G<<8 | B<<16 | seen<<24
    }
    p.out[r] = rec;
    p.added[r] = 1;
}

}  // namespace vc
