// gfx950 kernels of photo-consistency carving (vc_photo_carve; contract in include/voxcarve.h and DESIGN.md section 8 item 7):
// rounds of the visibility pass of vc_visible.h over the records that are still survivors; a surface voxel whose visible cameras
// disagree on its colour leaves the occupancy words, which exposes the voxels behind it to the next round.  Restated in
// tests/photo_np.py.
//
//   k_vis_fill, k_vis_surface<true>, k_vis_splat, k_vis_splat_big   (vc_visible.h) maps and surface list of round r's survivors;
//                   k_vis_surface<true> skips the records earlier rounds removed
//   k_photo_test    lane = surface survivor: the visibility test of k_vis_color, integer sums and sums of squares of the visible
//                   cameras' RGB, the variance test; a removed voxel gets rounds[s] = r and its bit leaves its word (64-bit
//                   atomicAnd: face neighbours share words); one atomic per workgroup on the round's removal counter
//   k_compact_count<PhotoKept>, k_compact_scatter<PhotoKept>   (vc_compact.h) the kept records (rounds[s] == 0) to their
//                   scanned positions in record order (stable compaction)
// Jacobi: the words are read only by k_vis_surface, which runs before the round's tests; the removals of round r are first seen
// by the surface test of round r + 1.  The maps, the list and the tests never depend on the order in which lanes run.
#pragma once
#include "vc_compact.h"          // k_compact_count, k_compact_scatter
#include "vc_visible.h"          // VisParams, kVisBlock

#pragma clang fp contract(off)

namespace vc {

constexpr uint32_t kPhotoMaxRounds = 255;                    // rounds[] is u8

struct PhotoParams {
    uint8_t *rounds;            // [S] 0 = kept so far, else the round that removed the record
    uint64_t *words;            // the occupancy words VisParams::words points at (bits are cleared here)
    uint32_t *removed;          // this round's removal counter
    uint64_t thr;               // var_threshold T, squared 8-bit levels
    uint32_t min_views;         // m
    uint32_t round;             // r, 1-based
};

__global__ __launch_bounds__(kVisBlock) void k_photo_test(const VisParams p, const PhotoParams q)
{
    __shared__ uint32_t s_wave[kVisBlock / 64];
    const uint32_t n = __hip_atomic_load(p.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const size_t HW = (size_t)p.H * p.W;
    uint32_t gone = 0;
    for (uint32_t k = blockIdx.x * kVisBlock + threadIdx.x; k < n; k += gridDim.x * kVisBlock) {
        const uint32_t s = p.list[k];
        const uint32_t i = (uint32_t)p.records[s];
        uint32_t ix, iy, iz;
        decompose(i, p.nx, p.ny, ix, iy, iz);
        const double X = p.xs[ix], Y = p.ys[iy], Z = p.zs[iz];
        uint32_t cnt = 0, sr = 0, sg = 0, sb = 0, qr = 0, qg = 0, qb = 0;
        for (uint32_t c = 0; c < p.C; ++c) {                     // (k_vis_color's visibility test, operation for operation)
            const CamDev &cam = p.cam[c];
            const double x = cam.r[0] * X + cam.r[1] * Y + cam.r[2] * Z + cam.t[0];
            const double y = cam.r[3] * X + cam.r[4] * Y + cam.r[5] * Z + cam.t[1];
            const double d = cam.r[6] * X + cam.r[7] * Y + cam.r[8] * Z + cam.t[2];
            double u, v;
            distort_and_project(cam, x, y, d, u, v);
            const int32_t off = pixel_offset(u, v, p.H, p.W);
            if (!(d > 0.0) || off < 0) continue;
            const float zm = __uint_as_float(p.zmap[c * HW + (uint32_t)off]);
            if (!((float)d <= zm + p.tol)) continue;
            const uint32_t px = p.frames[c * HW + (uint32_t)off];
            const uint32_t r = px & 0xffu, g = (px >> 8) & 0xffu, b = (px >> 16) & 0xffu;
            cnt += 1;
            sr += r; sg += g; sb += b;
            qr += r * r; qg += g * g; qb += b * b;               // <= 16 * 255^2: u32
        }
        if (cnt < q.min_views) continue;
        // D = sum_k (n q_k - s_k^2) = n^2 x (sum of the per-channel population variances); each term >= 0 (Cauchy-Schwarz)
        const uint64_t N = cnt;
        const uint64_t D = (N * qr - (uint64_t)sr * sr) + (N * qg - (uint64_t)sg * sg) + (N * qb - (uint64_t)sb * sb);
        if (D > q.thr * N * N) {
            q.rounds[s] = (uint8_t)q.round;
            atomicAnd((unsigned long long *)(q.words + (i >> 6)), ~(1ull << (i & 63u)));
            gone += 1;
        }
    }
    const uint32_t t = threadIdx.x;
    const uint32_t w = wave_sum_u32(gone);
    if ((t & 63u) == 0) s_wave[t >> 6] = w;
    __syncthreads();
    if (t == 0) {
        uint32_t total = 0;
        for (uint32_t k = 0; k < kVisBlock / 64; ++k) total += s_wave[k];
        if (total) atomicAdd(q.removed, total);
    }
}

// Selector of the compaction after the rounds: the records no round removed, copied to out
struct PhotoKept {
    const uint8_t *rounds;
    const uint64_t *records;
    uint64_t *out;
    __device__ bool pick(uint64_t s) const { return rounds[s] == 0; }
    __device__ void drop(uint64_t) const {}
    __device__ void put(uint64_t s, uint64_t d) const { out[d] = records[s]; }
};

}  // namespace vc
