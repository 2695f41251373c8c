// gfx950 kernels of the footprint carve (vc_carve_footprint; contract in include/voxcarve.h and DESIGN.md section 8 item 11,
// restated in tests/footprint_np.py): a camera passes a voxel by the foreground count of the pixel box that the voxel's whole
// cell projects to (8 lattice corners + the centre), not by the one pixel under its centre.
//
//   k_foot_rows     wave = one row of one camera's prepared bit mask: row-wise inclusive counts into the (H+1) x (W+1) table
//   k_foot_cols     lane = one table column: running sum down the rows; table[y][x] = foreground pixels in rows < y, columns < x
//   k_carve_foot    wave = 64 consecutive linear indices = one occupancy word.  Per camera a lane projects its centre and the
//                   four lattice points of its cell at L[iy]; the four at L[iy + 1] are the next lane's (their min / max come
//                   over by a lane shift) where that lane holds iy + 1 of the same column.  The lanes without such a
//                   neighbour (lane 63, the last iy of a column, the slab's last voxel) get theirs in a fix-up pass: their 4
//                   points each are dealt one per lane over the wave (16 such voxels per pass; a word of ny >= 64 needs one
//                   pass of one projection), reduced over quads and handed back.  That is 5 projections per voxel-view and
//                   one more per wave instead of 9.  Then the box, four table loads, the rule, __ballot into the word.
// Exact early-outs only: the union of the lanes' boxes is counted once per camera (zero: the camera fails all 64 voxels under
// every rule), and a word stops visiting cameras when no lane can reach min_views any more (not with view masks).
// Every table index is formed from a box clamped to [-1, W] x [-1, H] and intersected with the image: no camera can make one
// that is out of range.
#pragma once
#include "vc_kernels.h"

#pragma clang fp contract(off)

namespace vc {

constexpr uint32_t kFootAny = 1, kFootCover = 2;             // VC_FOOT_ANY, VC_FOOT_COVER

struct FootParams {
    const double *lx, *ly, *lz;     // cell lattices, nx + 1 | ny + 1 | nz + 1 values (whole grid; a slab starts at lz[z0])
    const uint32_t *sat;            // [C][(H + 1) (W + 1)]
    uint32_t rule, q;               // kFootAny | kFootCover, q in 1..256
};

// row y of camera c: table[c][y + 1][x + 1] = foreground pixels of the row in columns <= x; table[c][y + 1][0] = 0; row 0 = 0
__global__ __launch_bounds__(kBlock) void k_foot_rows(const uint32_t *__restrict__ bits, uint32_t *__restrict__ sat, uint32_t C, uint32_t H,
                                                      uint32_t W, uint32_t mwords)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = (blockIdx.x * kBlock + threadIdx.x) >> 6;  // wave-uniform: camera c, row y
    if (r >= C * H) return;
    const uint32_t c = r / H, y = r - c * H;
    const uint32_t *mb = bits + (size_t)c * mwords;
    uint32_t *row = sat + ((size_t)c * (H + 1) + (y + 1)) * (W + 1);
    if (lane == 0) row[0] = 0;
    if (y == 0) for (uint32_t x = lane; x <= W; x += 64) (row - (W + 1))[x] = 0;
    uint32_t run = 0;
    for (uint32_t x0 = 0; x0 < W; x0 += 64) {                    // wave-uniform
        const uint32_t x = x0 + lane;
        const uint32_t b = (x < W && mask_bit(mb, (int32_t)(y * W + x))) ? 1u : 0u;
        const uint32_t incl = wave_inclusive_scan(b, lane);
        if (x < W) row[x + 1] = run + incl;
        run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
}

__global__ __launch_bounds__(kBlock) void k_foot_cols(uint32_t *__restrict__ sat, uint32_t C, uint32_t H, uint32_t W)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= C * (W + 1)) return;
    const uint32_t c = t / (W + 1), x = t - c * (W + 1);
    uint32_t *col = sat + (size_t)c * (H + 1) * (W + 1) + x;
    uint32_t run = 0;
#pragma unroll 8
    for (uint32_t y = 1; y <= H; ++y) {
        run += col[(size_t)y * (W + 1)];
        col[(size_t)y * (W + 1)] = run;
    }
}

// floor, then clamp to [-1, hi] in float64, then convert (NaN, which only lanes whose centre the camera does not see can hold,
// lands on -1: fmax ignores it)
__device__ __forceinline__ int32_t foot_clamp(double x, uint32_t hi)
{
    return (int32_t)fmin(fmax(floor(x), -1.0), (double)hi);
}

// foreground pixels inside [x0, x1] x [y0, y1] (a box clamped to [-1, W] x [-1, H]) intersected with the image
__device__ __forceinline__ uint32_t foot_count(const uint32_t *__restrict__ t, int32_t x0, int32_t x1, int32_t y0, int32_t y1, uint32_t H,
                                               uint32_t W)
{
    const int32_t a = x0 < 0 ? 0 : x0, b = x1 > (int32_t)W - 1 ? (int32_t)W - 1 : x1;
    const int32_t c = y0 < 0 ? 0 : y0, d = y1 > (int32_t)H - 1 ? (int32_t)H - 1 : y1;
    if (a > b || c > d) return 0;                                // a in [0, W], b in [-1, W - 1]: below, 0 <= a <= b + 1 <= W
    const size_t s = (size_t)W + 1;
    return t[(size_t)(d + 1) * s + (uint32_t)(b + 1)] - t[(size_t)c * s + (uint32_t)(b + 1)] - t[(size_t)(d + 1) * s + (uint32_t)a] +
           t[(size_t)c * s + (uint32_t)a];
}

template <bool VM>
__global__ __launch_bounds__(kBlock) void k_carve_foot(const CarveParams p, const FootParams f)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;   // wave-uniform: the occupancy word
    if (w >= ((p.n + 63) >> 6)) return;
    const uint64_t j = (w << 6) + lane;
    const bool valid = j < p.n;
    uint32_t ix, iy, izl;
    decompose((uint32_t)(valid ? j : p.n - 1), p.nx, p.ny, ix, iy, izl);
    const double X = p.xs[ix], Y = p.ys[iy], Z = p.zs[p.z0 + izl];
    const double x0 = f.lx[ix], x1 = f.lx[ix + 1], y0 = f.ly[iy], z0 = f.lz[p.z0 + izl], z1 = f.lz[p.z0 + izl + 1];
    // lanes whose upper plane (L[iy + 1]) is not the next lane's lower plane
    const uint64_t need = __ballot(valid && (lane == 63u || iy + 1 == p.ny || j + 1 >= p.n));
    const bool mine = (need >> lane) & 1ull;
    const uint32_t nfix = (uint32_t)__popcll(need);
    const uint32_t myfix = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
    const uint32_t nvalid = (uint32_t)__popcll(__ballot(valid));
    const size_t tstride = ((size_t)p.H + 1) * ((size_t)p.W + 1);
    uint32_t vm = 0, cnt = 0;
    uint64_t nproj = 0, nskip = 0;                               // wave-uniform work counters
    for (uint32_t c = 0; c < p.C; ++c) {                         // wave-uniform
        // no voxel of the word can still reach min_views: the word is decided (result unchanged)
        if (!VM && __ballot(valid && cnt + (p.C - c) >= p.min_views) == 0ull) break;
        const CamDev &cam = p.cam[c];
        double uc, vc, u, v;
        project_point(cam, X, Y, Z, uc, vc);
        project_point(cam, x0, y0, z0, u, v);
        double ulo = u, uhi = u, vlo = v, vhi = v;               // lower plane: NaN-ignoring min / max of its 4 points
        project_point(cam, x1, y0, z0, u, v);
        ulo = fmin(ulo, u); uhi = fmax(uhi, u); vlo = fmin(vlo, v); vhi = fmax(vhi, v);
        project_point(cam, x0, y0, z1, u, v);
        ulo = fmin(ulo, u); uhi = fmax(uhi, u); vlo = fmin(vlo, v); vhi = fmax(vhi, v);
        project_point(cam, x1, y0, z1, u, v);
        ulo = fmin(ulo, u); uhi = fmax(uhi, u); vlo = fmin(vlo, v); vhi = fmax(vhi, v);
        // upper plane: the next lane's lower plane ...
        double nulo = __shfl_down(ulo, 1), nuhi = __shfl_down(uhi, 1), nvlo = __shfl_down(vlo, 1), nvhi = __shfl_down(vhi, 1);
        nproj += 5ull * nvalid;
        // ... or, for the lanes in `need`, 4 points dealt over the wave: lane l of a pass projects point l & 3 of the (l >> 2)-th
        for (uint32_t t0 = 0; t0 < nfix; t0 += 16) {             // wave-uniform
            const uint32_t t = t0 + (lane >> 2);
            const bool on = t < nfix;
            const uint32_t src = on ? select_bit(need, t) : 0u;
            const uint32_t six = (uint32_t)__shfl((int)ix, (int)src), siy = (uint32_t)__shfl((int)iy, (int)src);
            const uint32_t siz = (uint32_t)__shfl((int)izl, (int)src);
            double fu, fv;
            project_point(cam, f.lx[six + (lane & 1u)], f.ly[siy + 1], f.lz[p.z0 + siz + ((lane >> 1) & 1u)], fu, fv);
            double a = fu, b = fu, cc = fv, d = fv;
            a = fmin(a, __shfl_xor(a, 1)); b = fmax(b, __shfl_xor(b, 1)); cc = fmin(cc, __shfl_xor(cc, 1)); d = fmax(d, __shfl_xor(d, 1));
            a = fmin(a, __shfl_xor(a, 2)); b = fmax(b, __shfl_xor(b, 2)); cc = fmin(cc, __shfl_xor(cc, 2)); d = fmax(d, __shfl_xor(d, 2));
            const int from = (int)((myfix & 15u) << 2);
            const double ga = __shfl(a, from), gb = __shfl(b, from), gc = __shfl(cc, from), gd = __shfl(d, from);
            if (mine && (myfix & ~15u) == t0) { nulo = ga; nuhi = gb; nvlo = gc; nvhi = gd; }
            nproj += (nfix - t0 < 16u ? nfix - t0 : 16u) * 4ull;
        }
        const bool sees = valid && !(uc != uc) && !(vc != vc);   // a NaN centre: the camera does not see the voxel
        ulo = fmin(fmin(ulo, nulo), uc); uhi = fmax(fmax(uhi, nuhi), uc);
        vlo = fmin(fmin(vlo, nvlo), vc); vhi = fmax(fmax(vhi, nvhi), vc);
        const int32_t bx0 = foot_clamp(ulo, p.W), bx1 = foot_clamp(uhi, p.W), by0 = foot_clamp(vlo, p.H), by1 = foot_clamp(vhi, p.H);
        // union of the lanes' boxes (coordinates + 1: 0 .. W + 1), counted once
        const uint32_t ux0 = wave_min_u32(sees ? (uint32_t)(bx0 + 1) : 0xffffffffu), ux1 = wave_max_u32(sees ? (uint32_t)(bx1 + 1) : 0u);
        const uint32_t uy0 = wave_min_u32(sees ? (uint32_t)(by0 + 1) : 0xffffffffu), uy1 = wave_max_u32(sees ? (uint32_t)(by1 + 1) : 0u);
        const uint32_t *tab = f.sat + (size_t)c * tstride;
        if (ux0 == 0xffffffffu || foot_count(tab, (int32_t)ux0 - 1, (int32_t)ux1 - 1, (int32_t)uy0 - 1, (int32_t)uy1 - 1, p.H, p.W) == 0) {
            nskip += 1;
            continue;                                            // no foreground under the whole word: fails under every rule
        }
        bool pass = false;
        if (sees) {
            const uint64_t k = foot_count(tab, bx0, bx1, by0, by1, p.H, p.W);
            const uint64_t area = (uint64_t)(uint32_t)(bx1 - bx0 + 1) * (uint64_t)(uint32_t)(by1 - by0 + 1);
            pass = f.rule == kFootAny ? k > 0 : k * 256ull >= (uint64_t)f.q * area;
        }
        if (pass) { vm |= 1u << c; cnt += 1; }
    }
    if (VM && valid) p.viewmask[j] = (uint16_t)vm;
    const uint64_t ballot = __ballot(valid && cnt >= p.min_views);
    if (lane == 0) p.words[w] = ballot;
    stat_add(p.stats, 5 /* VC_WORK_FOOT_PROJECTIONS */, (uint32_t)w, lane, nproj);
    stat_add(p.stats, 6 /* VC_WORK_FOOT_UNION_SKIPS */, (uint32_t)w, lane, nskip);
    stat_add(p.stats, 7 /* VC_WORK_FOOT_WORDS */, (uint32_t)w, lane, 1);
}

}  // namespace vc
