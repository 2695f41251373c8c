// gfx950 kernels of the lit pass (vc_light_render; contract in include/voxcarve.h): cast shadows,
// ambient occlusion and a chequered floor for the images of the last vc_render.  Restated in tests/light_np.py.
//
//   k_light_classify   lane = pixel of the last render: 0 background, 1 hull, 2 floor (item 6: the pixel ray against the floor
//                      plane, in front of the render's hit), and the five outputs of a pixel that casts no secondary ray
//                      (background, face 6).  Hull and floor pixels: wave sums, one atomic each.
//   LightSel           the selector of the project's stable compaction (vc_compact.h): the pixels that cast rays, in pixel order.
//   k_light            16 lanes = one listed pixel, four pixels to a wave.  Lane k walks occlusion ray k (k_render's walk, block
//                      skipping included, from the start cell of item 2 or, on the floor, from the slab entry); the group's
//                      first lane walks the shadow ray as well.  The sixteen `open` bits of a group are a quarter of one wave
//                      ballot; the first lane shades and stores.  No LDS, no atomics on the images.  At most kLightMaxBlocks
//                      blocks stride over the list, their counts in registers: five atomics per wave, not per four pixels.
//
// Every lane of a wave reaches the ballot and the wave sums: a lane without a pixel or without a ray sits the walks out.
#pragma once
#include "vc_kernels.h"          // wave_sum_u32
#include "vc_render.h"           // RenderView, RAxis, rpixel, raxis, rentry, rwalk, kRenderMiss

#pragma clang fp contract(off)

namespace vc {

constexpr uint32_t kLightBlock = 256;        // 4 waves: 16 listed pixels, 16 lanes each
constexpr uint32_t kLightRays = 16;
constexpr uint32_t kLightMaxBlocks = 1024;   // of k_light: four waves to a SIMD of 256 CUs; more blocks only add counter atomics

struct LightParams {
    const uint64_t *words;                   // occupancy of the current result (dense)
    const uint64_t *bmap;                    // the render's block map, bit per 8^3 block
    const uint64_t *records;                 // [S] ascending index
    const short4 *normals;                   // [S] of vc_hull_normals (smooth = 1)
    uint64_t S;
    const RenderView *views;                 // [V] of the last render
    const uint32_t *idx;                     // [V H W] the render's indices (kRenderMiss: a miss)
    const float *depth;                      // [V H W] the render's depths
    const uint32_t *rgbf;                    // [V H W] the render's R | G << 8 | B << 16 | face << 24
    const uint32_t *jobs;                    // [njobs] the pixels that cast rays, ascending
    uint32_t *rgb;                           // [V H W] R | G << 8 | B << 16
    float *odepth;                           // [V H W]
    uint8_t *kind, *shadow, *ao;             // [V H W]
    unsigned long long *ctr;                 // [7] hull, floor, shadowed, facing away, rays, cells looked at, blocks skipped
    double e[3], s[3];                       // b(k) = e + (double)k s
    uint32_t n[3], nb[3];
    uint32_t H, W, npix, njobs;
    uint32_t skip;                           // 1: skip empty blocks (same results)
    double pos[4];
    uint32_t ambient, smooth, floor;
    double ao_reach, floor_z, rect[4], cell;
    uint32_t floor_rgb[2];                   // R | G << 8 | B << 16
};

__global__ __launch_bounds__(kLightBlock) void k_light_classify(const LightParams p)
{
    const uint32_t o = blockIdx.x * kLightBlock + threadIdx.x;
    uint32_t hull = 0, flr = 0;
    if (o < p.npix) {
        const uint32_t idx = p.idx[o], q = p.rgbf[o];
        const float dep = p.depth[o];
        uint32_t kind = idx != kRenderMiss ? 1u : 0u;
        if (p.floor) {                                                   // 6 the floor
            const uint32_t view = o / (p.H * p.W), r = o % (p.H * p.W);
            double o0, o1, o2, d0, d1, d2;
            rpixel(p.views[view], r % p.W, r / p.W, o0, o1, o2, d0, d1, d2);
            if (d2 != 0.0) {
                const double tf = (p.floor_z - o2) / d2;
                if (tf > 0.0 && (idx == kRenderMiss || tf < (double)dep)) {
                    const double qx = o0 + tf * d0, qy = o1 + tf * d1;
                    if (qx >= p.rect[0] && qx <= p.rect[1] && qy >= p.rect[2] && qy <= p.rect[3]) kind = 2u;
                }
            }
        }
        hull = kind == 1u;
        flr = kind == 2u;
        p.kind[o] = (uint8_t)kind;
        if (kind == 0u || (kind == 1u && (q >> 24) == 6u)) {             // no secondary rays: the render's pixel
            p.rgb[o] = q & 0xFFFFFFu;
            p.odepth[o] = dep;
            p.shadow[o] = 0;
            p.ao[o] = (uint8_t)kLightRays;
        }
    }
    const uint32_t wh = wave_sum_u32(hull), wf = wave_sum_u32(flr);
    if ((threadIdx.x & 63u) == 0 && (wh | wf)) {
        atomicAdd(p.ctr + 0, (unsigned long long)wh);
        atomicAdd(p.ctr + 1, (unsigned long long)wf);
    }
}

// The pixels k_light works on, into `jobs` in pixel order.
struct LightSel {
    const uint8_t *kind;
    const uint32_t *rgbf;
    uint32_t *jobs;
    __device__ bool pick(uint64_t s) const { return kind[s] == 2 || (kind[s] == 1 && (rgbf[s] >> 24) != 6u); }
    __device__ void drop(uint64_t) const {}
    __device__ void put(uint64_t s, uint64_t d) const { jobs[d] = (uint32_t)s; }
};

// One secondary ray from Q along (e0, e1, e2).  from_cell: item 3 of the lit pass, the walk starts at cell (c0, c1, c2) with
// t = 0, and a start cell outside the grid is an open ray; otherwise the entry of vc_render's item 3, then the walk.
// True on a hit, t its parameter; the walk ends without one once a step has taken it to t_stop (items 4 and 5 ask for hits
// with t below a bound only, and the caller still compares).
__device__ __forceinline__ bool light_ray(const LightParams &p, double q0, double q1, double q2, double e0, double e1, double e2,
                                          bool from_cell, int32_t c0, int32_t c1, int32_t c2, double t_stop, double &t,
                                          uint32_t &cells, uint32_t &skips)
{
    RAxis A0, A1, A2;
    A0.o = q0; A1.o = q1; A2.o = q2;
    A0.d = e0; A1.d = e1; A2.d = e2;
    raxis(A0, p.e[0], p.s[0], p.n[0]);
    raxis(A1, p.e[1], p.s[1], p.n[1]);
    raxis(A2, p.e[2], p.s[2], p.n[2]);
    int ax = -1;
    t = 0.0;
    if (from_cell) {
        A0.c = c0; A1.c = c1; A2.c = c2;
        if (!rinside(A0) || !rinside(A1) || !rinside(A2)) return false;
        A0.tn = rnext(A0); A1.tn = rnext(A1); A2.tn = rnext(A2);
    } else if (rentry(A0, A1, A2, t, ax)) {
        return false;
    }
    uint32_t hit_idx = kRenderMiss;
    return rwalk(p.words, p.bmap, p.skip, p.n, p.nb, A0, A1, A2, t, ax, hit_idx, cells, skips, t_stop);
}

// component `a` of a vector whose components along u = (a + 1) % 3, v = (a + 2) % 3 and a are (cu, cv, ca)
__device__ __forceinline__ double light_comp(uint32_t b, uint32_t a, double cu, double cv, double ca)
{
    return b == a ? ca : (b == (a + 1u) % 3u ? cu : cv);
}

__global__ __launch_bounds__(kLightBlock) void k_light(const LightParams p)
{
    const uint32_t lane = threadIdx.x & 63u, sub = threadIdx.x & 15u;
    const uint32_t per = kLightBlock / kLightRays;
    uint32_t rays = 0, nshadow = 0, naway = 0;
    uint64_t tcells = 0, tskips = 0;
    // a block takes 16 listed pixels at a time and keeps its counts in registers until the list is done: the counters are five
    // addresses, and one atomic per wave and group of pixels was most of this kernel's time.  `base` is the block's alone, so
    // the waves of a block, and the lanes of a wave, go round the same number of times.
    for (uint32_t base = blockIdx.x * per; base < p.njobs; base += gridDim.x * per) {
        const uint32_t job = base + (threadIdx.x >> 4);
        const bool live = job < p.njobs;
        uint32_t cells = 0, skips = 0;
        // 1, 2, 6 the pixel's point, face frame and start cell (the same in the sixteen lanes of a group)
        uint32_t o = 0, kind = 0, axis = 2, idx = 0;
        int32_t c0 = 0, c1 = 0, c2 = 0;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, sigma = 1.0, tf = 0.0;
        if (live) {
            o = p.jobs[job];
            kind = p.kind[o];
            const uint32_t view = o / (p.H * p.W), r = o % (p.H * p.W);
            double o0, o1, o2, d0, d1, d2;
            rpixel(p.views[view], r % p.W, r / p.W, o0, o1, o2, d0, d1, d2);
            if (kind == 1u) {
                const double t1 = (double)p.depth[o];
                q0 = o0 + t1 * d0; q1 = o1 + t1 * d1; q2 = o2 + t1 * d2;
                idx = p.idx[o];
                const uint32_t face = p.rgbf[o] >> 24;                       // 0..5: the list holds no face 6
                axis = face >> 1;
                const int32_t back = (face & 1u) ? 1 : -1;
                sigma = (double)back;
                c1 = (int32_t)(idx % p.n[1]);
                c0 = (int32_t)((idx / p.n[1]) % p.n[0]);
                c2 = (int32_t)(idx / (p.n[1] * p.n[0]));
                if (axis == 0) c0 += back; else if (axis == 1) c1 += back; else c2 += back;
            } else {
                tf = (p.floor_z - o2) / d2;
                q0 = o0 + tf * d0; q1 = o1 + tf * d1; q2 = o2 + tf * d2;
                sigma = o2 < p.floor_z ? -1.0 : 1.0;
            }
        }
        const bool from_cell = kind == 1u;
        // 5 the occlusion ray of this lane
        bool open = true;
        if (live && p.ao_reach > 0.0) {
            const uint32_t ring = sub >> 2, j = sub & 3u;
            int32_t iu, iv;
            if (ring & 1u) { iu = (j & 2u) ? -1 : 1; iv = (j & 1u) ? -1 : 1; }
            else { iu = j < 2u ? ((j & 1u) ? -1 : 1) : 0; iv = j < 2u ? 0 : ((j & 1u) ? -1 : 1); }
            const int32_t in = ring < 2u ? 2 : 1;
            const uint32_t ua = (axis + 1u) % 3u, va = (axis + 2u) % 3u;
            const double su = ua == 0 ? p.s[0] : (ua == 1 ? p.s[1] : p.s[2]);
            const double sv = va == 0 ? p.s[0] : (va == 1 ? p.s[1] : p.s[2]);
            const double sa = axis == 0 ? p.s[0] : (axis == 1 ? p.s[1] : p.s[2]);
            const double cu = (double)iu * su, cv = (double)iv * sv, ca = (double)(sigma < 0.0 ? -in : in) * sa;
            const double reach = p.ao_reach / sqrt((double)(iu * iu + iv * iv + in * in));
            double t;
            const bool hit = light_ray(p, q0, q1, q2, light_comp(0, axis, cu, cv, ca), light_comp(1, axis, cu, cv, ca),
                                       light_comp(2, axis, cu, cv, ca), from_cell, c0, c1, c2, reach, t, cells, skips);
            open = !(hit && t < reach);
            rays += 1;
        }
        const uint64_t bits = __ballot(live && open);
        // 4 the shadow ray, 7 the shade, 8 the outputs: the group's first lane
        if (live && sub == 0) {
            const uint32_t ao = (uint32_t)__popcll((bits >> (lane & 48u)) & 0xFFFFull);
            const bool point = p.pos[3] != 0.0;
            const double e0 = point ? p.pos[0] - q0 : p.pos[0], e1 = point ? p.pos[1] - q1 : p.pos[1], e2 = point ? p.pos[2] - q2 : p.pos[2];
            const double ea = axis == 0 ? e0 : (axis == 1 ? e1 : e2);
            uint32_t shadow = 0;
            if (sigma * ea <= 0.0) {
                shadow = 2;
                naway += 1;
            } else {
                double t;
                const bool hit = light_ray(p, q0, q1, q2, e0, e1, e2, from_cell, c0, c1, c2, point ? 1.0 : __builtin_inf(), t, cells, skips);
                shadow = (hit && (!point || t < 1.0)) ? 1u : 0u;
                nshadow += shadow;
                rays += 1;
            }
            int32_t n0 = axis == 0 ? (int32_t)sigma : 0, n1 = axis == 1 ? (int32_t)sigma : 0, n2 = axis == 2 ? (int32_t)sigma : 0;
            uint32_t base = p.floor_rgb[0];
            if (kind == 1u) {
                uint64_t lo = 0, hi = p.S;                                   // the first record with index >= idx
                while (lo < hi) {
                    const uint64_t mid = (lo + hi) >> 1;
                    if ((uint32_t)p.records[mid] < idx) lo = mid + 1; else hi = mid;
                }
                base = lo < p.S ? (uint32_t)(p.records[lo] >> 32) & 0xFFFFFFu : 0u;
                if (p.smooth && lo < p.S) {
                    const short4 nq = p.normals[lo];
                    if (nq.w != 0 && ((int32_t)nq.x | (int32_t)nq.y | (int32_t)nq.z) != 0) { n0 = nq.x; n1 = nq.y; n2 = nq.z; }
                }
            } else {
                const long long kx = (long long)floor(q0 / p.cell), ky = (long long)floor(q1 / p.cell);
                base = p.floor_rgb[(uint32_t)(kx + ky) & 1u];
            }
            uint32_t s = (p.ambient * ao * 2u + 16u) / 32u;
            if (shadow == 0) {
                const double dot = ((double)n0 * e0 + (double)n1 * e1) + (double)n2 * e2;
                const double nn = (double)((long long)n0 * n0 + (long long)n1 * n1 + (long long)n2 * n2);
                const double ll = (e0 * e0 + e1 * e1) + e2 * e2;
                double c = 0.0;
                if (dot > 0.0) {
                    c = dot / sqrt(nn * ll);
                    c = c < 1.0 ? c : 1.0;
                }
                s += (uint32_t)floor((double)(255u - p.ambient) * c + 0.5);
            }
            const uint32_t r = ((base & 255u) * s + 127u) / 255u;
            const uint32_t g = (((base >> 8) & 255u) * s + 127u) / 255u;
            const uint32_t b = (((base >> 16) & 255u) * s + 127u) / 255u;
            p.rgb[o] = r | (g << 8) | (b << 16);
            p.odepth[o] = kind == 1u ? p.depth[o] : (float)tf;
            p.shadow[o] = (uint8_t)shadow;
            p.ao[o] = (uint8_t)ao;
        }
        tcells += cells;
        tskips += skips;
    }
    // every lane of the wave is here (the branches above have joined): wave sums, one atomic each from lane 0
    const uint32_t ws = wave_sum_u32(nshadow), wa = wave_sum_u32(naway), wr = wave_sum_u32(rays);
    // (a lane's walks of a whole list can pass 2^32 / 64 cells: the sums in two parts of 20 and up to 32 bits)
    const uint64_t wc = ((uint64_t)wave_sum_u32((uint32_t)(tcells >> 20)) << 20) + wave_sum_u32((uint32_t)tcells & 0xFFFFFu);
    const uint64_t wk = ((uint64_t)wave_sum_u32((uint32_t)(tskips >> 20)) << 20) + wave_sum_u32((uint32_t)tskips & 0xFFFFFu);
    if (lane == 0 && (ws | wa | wr | wc | wk)) {
        if (ws) atomicAdd(p.ctr + 2, (unsigned long long)ws);
        if (wa) atomicAdd(p.ctr + 3, (unsigned long long)wa);
        atomicAdd(p.ctr + 4, (unsigned long long)wr);
        atomicAdd(p.ctr + 5, (unsigned long long)wc);
        atomicAdd(p.ctr + 6, (unsigned long long)wk);
    }
}

}  // namespace vc
