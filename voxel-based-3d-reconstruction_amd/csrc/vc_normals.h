// gfx950 kernels of the hull's surface normals and their consumers (vc_hull_normals, vc_shade_render, vc_surface_normals;
// contract in include/voxcarve.h).  Restated in tests/normals_np.py.
//
//   k_cc_wcount, scan_counts, k_cc_woff   (vc_components.h) survivors before each occupancy word: the record of voxel j is
//                    woff[j >> 6] + popc(word & below(j & 63))
//   k_normals        wave = kNrmWords consecutive occupancy words, one after the other; lane = voxel of the word in hand.  A zero
//                    word costs its load.  The six face neighbours of the word's 64 voxels are six 64-bit strings at fixed bit
//                    distances (-+1, -+ny, -+nx ny), each funnel-shifted out of two lane-uniform loads; a word without a surface
//                    voxel ends there.  Then one round per row (dx, dz) of the ball: voxel j's window of 2 ky + 1 cells starts at
//                    bit j + (dz nx + dx) ny - ky of the occupancy, a distance that is the same for every lane, so the 64 windows
//                    lie in three consecutive words (lane-uniform loads) and each lane funnel-shifts its own out of them.  What
//                    depends on the lane is the validity only: the row has to lie in the grid (ix + dx, iz + dz) and the window is
//                    cut to the lane's own y line (a word straddles lines whenever ny % 64 != 0).  A row adds popc . dx, popc . dz
//                    and sum(dy) = sum(bit positions) - ky popc, the positions' sum from five masked popcounts.  A round whose
//                    three words are zero is skipped.  Counters: summed over the workgroup, one atomic each and none for a zero.
//   k_shade          lane = pixel of the last render: the hit's record by the render's own binary search, float64 Lambert term in
//                    the contract's operation order (this file is built without contraction)
//   k_surf_normals   lane = vertex of the last surface mesh: the stored quadruple of the ON element's record
// Every index formed from a neighbour distance is checked against the grid, and every word index against the word count, before
// it is used.
#pragma once
#include "vc_components.h"       // cc_below, k_cc_wcount, k_cc_woff (vc_kernels.h: decompose, wave_sum_u32)
#include "vc_render.h"           // kRenderMiss

#pragma clang fp contract(off)

namespace vc {

constexpr uint32_t kNrmBlock = 256;
constexpr uint32_t kNrmWords = 8;                            // occupancy words per wave of k_normals
constexpr uint32_t kNrmMaxExt = 15;                          // a y window of 2 ext + 1 <= 31 cells
constexpr uint32_t kNrmMaxRows = (2 * kNrmMaxExt + 1) * (2 * kNrmMaxExt + 1);

struct NrmParams {
    const uint64_t *words;      // occupancy of the current result (dense)
    const uint32_t *woff;       // [nwords] survivors before each word
    const uint32_t *rows;       // [nrows] (dx & 255) | (dz & 255) << 8 | ky << 16: the rows of the ball
    short4 *out;                // [S] stored quadruples, zeroed beforehand
    unsigned long long *ctr;    // [2] surface records, surface records with n = 0
    uint64_t nwords, n, S;
    long long q[3];             // um
    uint32_t nrows, nx, ny, nz;
};

// word w of the occupancy, 0 outside it
__device__ __forceinline__ uint64_t nrm_word(const uint64_t *__restrict__ words, long long w, uint64_t nwords)
{
    return (w >= 0 && (uint64_t)w < nwords) ? words[w] : 0ull;
}

// bits [pos, pos + 64) of the occupancy (pos may lie before or behind it: zeros there)
__device__ __forceinline__ uint64_t nrm_bits64(const uint64_t *__restrict__ words, long long pos, uint64_t nwords)
{
    const long long w = pos >> 6;                            // floor
    const uint32_t sh = (uint32_t)(pos & 63);
    const uint64_t lo = nrm_word(words, w, nwords);
    return sh ? (lo >> sh) | (nrm_word(words, w + 1, nwords) << (64u - sh)) : lo;
}

__global__ __launch_bounds__(kNrmBlock) void k_normals(const NrmParams p)
{
    __shared__ uint32_t s_cnt[kNrmBlock / 64][2];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t first = ((uint64_t)blockIdx.x * (kNrmBlock / 64) + wave) * kNrmWords;
    const long long ny = p.ny, plane = (long long)p.nx * p.ny;
    uint32_t n_surf = 0, n_zero = 0;                         // the same in every lane
    for (uint32_t k = 0; k < kNrmWords; ++k) {
        const uint64_t w = first + k;
        if (w >= p.nwords) break;                            // (whole waves)
        const uint64_t W = p.words[w];
        if (!W) continue;
        const long long base = (long long)(w << 6);
        const uint64_t lin = (w << 6) + lane;
        uint32_t ix = 0, iy = 0, iz = 0;
        const bool on = lin < p.n && ((W >> lane) & 1ull);
        if (lin < p.n) decompose((uint32_t)lin, p.nx, p.ny, ix, iy, iz);
        // the six face neighbours: a neighbour outside the grid counts as OFF
        const uint64_t ym = nrm_bits64(p.words, base - 1, p.nwords), yp = nrm_bits64(p.words, base + 1, p.nwords);
        const uint64_t xm = nrm_bits64(p.words, base - ny, p.nwords), xp = nrm_bits64(p.words, base + ny, p.nwords);
        const uint64_t zm = nrm_bits64(p.words, base - plane, p.nwords), zp = nrm_bits64(p.words, base + plane, p.nwords);
        const bool inner = (iy > 0 && ((ym >> lane) & 1ull)) && (iy + 1 < p.ny && ((yp >> lane) & 1ull)) &&
                           (ix > 0 && ((xm >> lane) & 1ull)) && (ix + 1 < p.nx && ((xp >> lane) & 1ull)) &&
                           (iz > 0 && ((zm >> lane) & 1ull)) && (iz + 1 < p.nz && ((zp >> lane) & 1ull));
        const bool surf = on && !inner;
        const uint64_t smask = __ballot(surf);
        if (!smask) continue;
        int32_t cx = 0, cy = 0, cz = 0;                      // sums of dx, dy, dz over the ON cells of the ball
        for (uint32_t r = 0; r < p.nrows; ++r) {
            const uint32_t row = p.rows[r];
            const int32_t dx = (int32_t)(int8_t)(row & 255u), dz = (int32_t)(int8_t)((row >> 8) & 255u);
            const uint32_t ky = (row >> 16) & 15u;
            // lane j's window: bits [start + j, start + j + 2 ky] of the occupancy
            const long long start = base + ((long long)dz * p.nx + dx) * ny - (long long)ky;
            const long long w0 = start >> 6;                 // floor
            const uint32_t o = (uint32_t)(start & 63);
            const uint64_t A = nrm_word(p.words, w0, p.nwords), B = nrm_word(p.words, w0 + 1, p.nwords),
                           C = nrm_word(p.words, w0 + 2, p.nwords);
            if (!(A | B | C)) continue;
            const uint32_t at = o + lane, sh = at & 63u;     // at <= 126
            const uint64_t lo = at < 64u ? A : B, hi = at < 64u ? B : C;
            uint32_t win = (uint32_t)(sh ? (lo >> sh) | (hi << (64u - sh)) : lo);
            // bit b of the window is dy = b - ky: inside the lane's y line for b in [ky - iy, ky + ny - 1 - iy]
            const uint32_t blo = ky > iy ? ky - iy : 0u;
            const uint32_t room = p.ny - 1u - iy;
            const uint32_t bhi = room < ky ? ky + room : 2u * ky;       // <= 30
            uint32_t m = ((2u << bhi) - 1u) & ~((1u << blo) - 1u);
            if (dx == 0 && dz == 0) m &= ~(1u << ky);        // the voxel itself is no offset of the ball
            const bool row_in = (uint32_t)((int32_t)ix + dx) < p.nx && (uint32_t)((int32_t)iz + dz) < p.nz;
            win = row_in ? win & m : 0u;
            const int32_t c = __popc(win);
            const int32_t sb = __popc(win & 0xAAAAAAAAu) + 2 * __popc(win & 0xCCCCCCCCu) + 4 * __popc(win & 0xF0F0F0F0u) +
                               8 * __popc(win & 0xFF00FF00u) + 16 * __popc(win & 0xFFFF0000u);
            cx += dx * c;
            cz += dz * c;
            cy += sb - (int32_t)ky * c;
        }
        bool zero = false;
        if (surf) {
            const long long n0 = -(p.q[0] * cx), n1 = -(p.q[1] * cy), n2 = -(p.q[2] * cz);
            const long long a0 = n0 < 0 ? -n0 : n0, a1 = n1 < 0 ? -n1 : n1, a2 = n2 < 0 ? -n2 : n2;
            const long long m = a0 > a1 ? (a0 > a2 ? a0 : a2) : (a1 > a2 ? a1 : a2);
            short4 v = make_short4(0, 0, 0, 1);
            if (m) { v.x = (short)(n0 * 32767 / m); v.y = (short)(n1 * 32767 / m); v.z = (short)(n2 * 32767 / m); }
            zero = m == 0;
            const uint64_t s = (uint64_t)p.woff[w] + (uint32_t)__popcll(W & cc_below(lane));
            if (s < p.S) p.out[s] = v;
        }
        n_surf += (uint32_t)__popcll(smask);
        n_zero += (uint32_t)__popcll(__ballot(zero));
    }
    if (lane == 0) { s_cnt[wave][0] = n_surf; s_cnt[wave][1] = n_zero; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
#pragma unroll
        for (uint32_t i = 0; i < kNrmBlock / 64; ++i) { a += s_cnt[i][0]; b += s_cnt[i][1]; }
        if (a) atomicAdd(p.ctr + 0, (unsigned long long)a);
        if (b) atomicAdd(p.ctr + 1, (unsigned long long)b);
    }
}

struct ShadeParams {
    const uint32_t *idx;        // [V H W] of the render
    const uint32_t *rgbf;       // [V H W] of the render: R | G << 8 | B << 16 | face << 24
    const uint64_t *records;    // [S] ascending index
    const short4 *normals;      // [S]
    const double *light;        // [V][3]
    uint32_t *out;              // [V H W] R | G << 8 | B << 16
    uint64_t S, npix, view_pix;
    uint32_t ambient;
};

__global__ __launch_bounds__(kNrmBlock) void k_shade(const ShadeParams p)
{
    const uint64_t o = (uint64_t)blockIdx.x * kNrmBlock + threadIdx.x;
    if (o >= p.npix) return;
    const uint32_t idx = p.idx[o];
    uint32_t px = p.rgbf[o] & 0xFFFFFFu;                     // a miss keeps the background, a hit without a normal its own colour
    if (idx != kRenderMiss) {
        uint64_t lo = 0, hi = p.S;                           // the first record with index >= idx
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((uint32_t)p.records[mid] < idx) lo = mid + 1; else hi = mid;
        }
        if (lo < p.S) {
            const short4 n = p.normals[lo];
            const int32_t n0 = n.x, n1 = n.y, n2 = n.z;
            if (n.w != 0 && (n0 | n1 | n2) != 0) {
                const double *L = p.light + 3 * (o / p.view_pix);
                const double L0 = L[0], L1 = L[1], L2 = L[2];
                const double dot = ((double)n0 * L0 + (double)n1 * L1) + (double)n2 * L2;
                const double nn = (double)((long long)n0 * n0 + (long long)n1 * n1 + (long long)n2 * n2);
                const double ll = (L0 * L0 + L1 * L1) + L2 * L2;
                double c = 0.0;
                if (dot > 0.0) {
                    c = dot / sqrt(nn * ll);
                    c = c < 1.0 ? c : 1.0;
                }
                const uint32_t s = p.ambient + (uint32_t)floor((double)(255u - p.ambient) * c + 0.5);
                const uint64_t rec = p.records[lo];
                const uint32_t r = (((uint32_t)(rec >> 32) & 255u) * s + 127u) / 255u;
                const uint32_t g = (((uint32_t)(rec >> 40) & 255u) * s + 127u) / 255u;
                const uint32_t b = (((uint32_t)(rec >> 48) & 255u) * s + 127u) / 255u;
                px = r | (g << 8) | (b << 16);
            }
        }
    }
    p.out[o] = px;
}

// edges: the entries of k_surf_edges (vc_surface.h): element | axis << 32 | (the lower element is ON) << 34
__global__ __launch_bounds__(kNrmBlock) void k_surf_normals(const uint64_t *__restrict__ edges, uint64_t V,
                                                             const uint64_t *__restrict__ records, uint64_t S,
                                                             const short4 *__restrict__ normals, uint32_t nx, uint32_t ny,
                                                             short4 *__restrict__ out)
{
    const uint64_t v = (uint64_t)blockIdx.x * kNrmBlock + threadIdx.x;
    if (v >= V) return;
    const uint64_t ent = edges[v];
    const uint32_t e = (uint32_t)ent, axis = (uint32_t)(ent >> 32) & 3u;
    const bool on_low = (ent >> 34) & 1ull;
    const uint32_t ion = on_low ? e : e + (axis == 0 ? nx * ny : (axis == 1 ? ny : 1u));
    uint64_t lo = 0, hi = S;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint32_t)records[mid] < ion) lo = mid + 1; else hi = mid;
    }
    out[v] = (lo < S && (uint32_t)records[lo] == ion) ? normals[lo] : make_short4(0, 0, 0, 0);
}

}  // namespace vc
