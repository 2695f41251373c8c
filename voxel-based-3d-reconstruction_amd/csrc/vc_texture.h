// gfx950 kernel of the free-viewpoint texturing pass (vc_texture_render; contract in include/voxcarve.h, DESIGN.md section 8
// item 22): every hit of the last vc_render is refined along its own ray against the silhouettes, then coloured from the camera
// frames that see the refined point, weighted by how close each camera looks to the viewing direction.  Restated in
// tests/texture_np.py.
//
//   k_texture   wave = 8 x 8 pixel tile of a view (k_render's tiling: neighbouring rays sample neighbouring frame pixels),
//               lane = pixel.  The pixel ray as k_render makes it, the bracket test at both ends, `steps` bisection rounds (each a
//               float64 projection + mask bit per camera until the count is decided), then two passes over the cameras:
//                 pass 1  candidate test (in image, in front, not hidden behind vc_color_visible's depth map) and the 16-bit
//                         weight, packed four to a 64-bit register: 16 cameras are four registers, addressed with selects on the
//                         wave-uniform camera index, never an array the compiler would put in scratch;
//                 pass 2  a camera's rank among the weights ((weight, -index) order); the `best` first are projected again
//                         (the same operations, the same pixel), sampled and blended.
//               The sums stay below 2^32 (16 weights of 65535 times 255, plus half the weight sum), so the contract's 64-bit
//               integers are computed in 32 bits.  Hits, refined, textured, fallback, camera tests: wave sums, one atomic each.
//
// Every loop runs the same number of rounds in every lane (a lane that has decided sits the round out), so the camera index
// and the camera's parameters stay in scalar registers.  Every index is formed from a value that passed pixel_offset or was
// clamped into the image.
#pragma once
#include "vc_device.h"
#include "vc_kernels.h"          // kMaxCameras, wave_sum_u32
#include "vc_render.h"           // RenderView, rpixel, kRenderMiss

#pragma clang fp contract(off)

namespace vc {

constexpr uint32_t kTexBlock = 256;          // 4 waves, an 8 x 8 pixel tile each
constexpr uint32_t kTexMaxSteps = 24;
constexpr uint32_t kTexMaxSharpen = 6;

struct TexParams {
    const RenderView *views;                 // [V] of the last render
    const uint32_t *idx;                     // [V H W] the render's indices (kRenderMiss: a miss)
    const float *depth;                      // [V H W] the render's depths
    const uint32_t *rgbf;                    // [V H W] the render's R | G << 8 | B << 16 | face << 24
    const uint32_t *zmap;                    // [C][CH CW] float32 bits, the current vc_color_visible maps
    const uint32_t *frames;                  // [C][CH CW] R | G << 8 | B << 16 | seen << 24 of the slot
    const uint32_t *bits;                    // [C][mwords] the carve's post-filtered masks
    uint32_t *rgbc;                          // [V H W] R | G << 8 | B << 16 | count << 24
    float *odepth;                           // [V H W]
    uint8_t *best, *refined;                 // [V H W]
    unsigned long long *ctr;                 // [5] hits, refined, textured, fallback, camera tests
    uint32_t H, W, tiles_x, tiles_per_view, n_tiles;
    uint32_t C, CH, CW, mwords, m, steps, keep, sharpen, filter;
    float tol;
    double reach;
    double centre[kMaxCameras][3];           // the cameras' centres, made on the host as the render makes a view's origin
    CamDev cam[kMaxCameras];
};

// Sixteen 16-bit weights in four registers; c is the same in every lane.
struct TexWeights { uint64_t q0, q1, q2, q3; };

__device__ __forceinline__ uint32_t tex_weight(const TexWeights &w, uint32_t c)
{
    const uint32_t s = c >> 2;
    const uint64_t q = s == 0 ? w.q0 : (s == 1 ? w.q1 : (s == 2 ? w.q2 : w.q3));
    return (uint32_t)(q >> ((c & 3u) * 16u)) & 0xffffu;
}

__device__ __forceinline__ void tex_put(TexWeights &w, uint32_t c, uint32_t v)
{
    const uint32_t s = c >> 2;
    const uint64_t x = (uint64_t)v << ((c & 3u) * 16u);
    w.q0 |= s == 0 ? x : 0ull;
    w.q1 |= s == 1 ? x : 0ull;
    w.q2 |= s == 2 ? x : 0ull;
    w.q3 |= s == 3 ? x : 0ull;
}

// T(X, Y, Z) >= m for the lanes with `active`, decided as early as the count allows; `tests` counts the cameras tried.
// (surf_inside of vc_surface.h without its camera ordering and its reject masks: the bisection round stays one short loop.)
__device__ __forceinline__ bool tex_inside(const TexParams &p, double X, double Y, double Z, bool active, uint32_t &tests)
{
    if (p.m > p.C) return false;
    const uint32_t max_fail = p.C - p.m;
    uint32_t pass = 0, fail = 0;
    bool done = !active, inside = false;
    for (uint32_t c = 0; c < p.C; ++c) {
        if (done) continue;
        double u, v;
        project_point(p.cam[c], X, Y, Z, u, v);
        const int32_t off = pixel_offset(u, v, p.CH, p.CW);
        const bool ok = off >= 0 && mask_bit(p.bits + (size_t)c * p.mwords, off);
        ++tests;
        if (ok) {
            if (++pass >= p.m) { inside = true; done = true; }
        } else if (++fail > max_fail) done = true;
    }
    return inside;
}

__device__ __forceinline__ uint32_t tex_clamp(int32_t v, uint32_t n)
{
    return v < 0 ? 0u : ((uint32_t)v < n ? (uint32_t)v : n - 1u);
}

// item 6 of the contract, filter = 1: the four pixels around (u - 0.5, v - 0.5), 8-bit fractions, integer blend per channel
__device__ __forceinline__ uint32_t tex_bilinear(const uint32_t *__restrict__ f, double u, double v, uint32_t H, uint32_t W)
{
    const double fu = u - 0.5, fv = v - 0.5;
    const double x0 = floor(fu), y0 = floor(fv);
    const uint32_t ax = (uint32_t)(int32_t)floor((fu - x0) * 256.0), ay = (uint32_t)(int32_t)floor((fv - y0) * 256.0);
    const uint32_t xa = tex_clamp((int32_t)x0, W), xb = tex_clamp((int32_t)x0 + 1, W);
    const uint32_t ya = tex_clamp((int32_t)y0, H), yb = tex_clamp((int32_t)y0 + 1, H);
    const uint32_t p00 = f[(size_t)ya * W + xa], p10 = f[(size_t)ya * W + xb];
    const uint32_t p01 = f[(size_t)yb * W + xa], p11 = f[(size_t)yb * W + xb];
    uint32_t out = 0;
#pragma unroll
    for (uint32_t sh = 0; sh < 24; sh += 8) {
        const uint32_t a = (p00 >> sh) & 255u, b = (p10 >> sh) & 255u, c = (p01 >> sh) & 255u, d = (p11 >> sh) & 255u;
        const uint32_t ch = ((a * (256u - ax) + b * ax) * (256u - ay) + (c * (256u - ax) + d * ax) * ay + 32768u) >> 16;
        out |= ch << sh;
    }
    return out;
}

__global__ __launch_bounds__(kTexBlock) void k_texture(const TexParams p)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t tile = blockIdx.x * (kTexBlock / 64) + (threadIdx.x >> 6);
    uint32_t hits = 0, nref = 0, ntex = 0, nfall = 0, tests = 0;
    if (tile < p.n_tiles) {
        const uint32_t view = tile / p.tiles_per_view, tr = tile % p.tiles_per_view;
        const uint32_t pu = (tr % p.tiles_x) * 8 + (lane & 7), pv = (tr / p.tiles_x) * 8 + (lane >> 3);
        if (pu < p.W && pv < p.H) {
            const uint64_t o = ((uint64_t)view * p.H + pv) * p.W + pu;
            uint32_t orgbc = p.rgbf[o] & 0xFFFFFFu;                      // a miss and a pixel no camera colours keep the render's
            uint32_t obest = 255u, oref = 0u;
            float odepth = __builtin_inff();
            if (p.idx[o] != kRenderMiss) {
                hits = 1;
                // 1 the pixel ray, as k_render makes it
                double o0, o1, o2, d0, d1, d2;
                rpixel(p.views[view], pu, pv, o0, o1, o2, d0, d1, d2);
                const double t0 = (double)p.depth[o];
                // 3 the bracket and the bisection
                double tt = t0;
                if (p.steps) {
                    const bool in0 = tex_inside(p, o0 + t0 * d0, o1 + t0 * d1, o2 + t0 * d2, true, tests);
                    const double back = t0 - p.reach;
                    double lo = in0 ? (back > 0.0 ? back : 0.0) : t0;
                    double hi = in0 ? t0 : t0 + p.reach;
                    // (the end at t0 has been tested: the other end decides)
                    const double te = in0 ? lo : hi;
                    const bool ine = tex_inside(p, o0 + te * d0, o1 + te * d1, o2 + te * d2, true, tests);
                    const bool ref = in0 ? !ine : ine;
                    for (uint32_t k = 0; k < p.steps; ++k) {
                        const double mid = (lo + hi) * 0.5;
                        const bool in = tex_inside(p, o0 + mid * d0, o1 + mid * d1, o2 + mid * d2, ref, tests);
                        if (ref) { if (in) hi = mid; else lo = mid; }
                    }
                    if (ref) { tt = (lo + hi) * 0.5; oref = 1u; nref = 1; }
                }
                odepth = (float)tt;
                const double X = o0 + tt * d0, Y = o1 + tt * d1, Z = o2 + tt * d2;
                // 4, 5 the candidates and their weights
                const size_t HW = (size_t)p.CH * p.CW;
                TexWeights wq = {0ull, 0ull, 0ull, 0ull};
                const double b0 = o0 - X, b1 = o1 - Y, b2 = o2 - Z;
                const double bb = (b0 * b0 + b1 * b1) + b2 * b2;
                for (uint32_t c = 0; c < p.C; ++c) {
                    const CamDev &cam = p.cam[c];
                    const double qx = cam.r[0] * X + cam.r[1] * Y + cam.r[2] * Z + cam.t[0];
                    const double qy = cam.r[3] * X + cam.r[4] * Y + cam.r[5] * Z + cam.t[1];
                    const double qz = cam.r[6] * X + cam.r[7] * Y + cam.r[8] * Z + cam.t[2];
                    double u, v;
                    distort_and_project(cam, qx, qy, qz, u, v);
                    const int32_t off = pixel_offset(u, v, p.CH, p.CW);
                    uint32_t w = 0;
                    if (qz > 0.0 && off >= 0) {
                        const float zm = __uint_as_float(p.zmap[c * HW + (uint32_t)off]);
                        if ((float)qz <= zm + p.tol) {
                            const double a0 = p.centre[c][0] - X, a1 = p.centre[c][1] - Y, a2 = p.centre[c][2] - Z;
                            const double dot = (a0 * b0 + a1 * b1) + a2 * b2;
                            const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
                            const double nn = aa * bb;
                            double cw = 0.0;
                            // (a finite normal number: at least the smallest normal, below +inf; NaN fails both)
                            if (dot > 0.0 && nn >= 2.2250738585072014e-308 && nn < __builtin_inf()) {
                                cw = dot / sqrt(nn);
                                cw = cw < 1.0 ? cw : 1.0;
                            }
                            for (uint32_t s = 0; s < p.sharpen; ++s) cw = cw * cw;
                            w = (uint32_t)floor(cw * 65535.0 + 0.5);
                        }
                    }
                    tex_put(wq, c, w);
                }
                // 5, 6, 7 the `keep` heaviest, their samples, the blend
                uint32_t ws = 0, sr = 0, sg = 0, sb = 0, cnt = 0;
                for (uint32_t c = 0; c < p.C; ++c) {
                    const uint32_t w = tex_weight(wq, c);
                    uint32_t rank = 0;
                    for (uint32_t e = 0; e < p.C; ++e) {
                        const uint32_t we = tex_weight(wq, e);
                        rank += (we > w || (we == w && e < c)) ? 1u : 0u;
                    }
                    if (w != 0 && rank < p.keep) {
                        const CamDev &cam = p.cam[c];
                        double u, v;
                        project_point(cam, X, Y, Z, u, v);
                        // (a candidate: (u, v) passed pixel_offset in pass 1, and these are the same operations)
                        const int32_t off = pixel_offset(u, v, p.CH, p.CW);
                        const uint32_t *f = p.frames + c * HW;
                        uint32_t px = 0;
                        if (off >= 0) px = p.filter ? tex_bilinear(f, u, v, p.CH, p.CW) : f[(uint32_t)off];
                        ws += w;
                        sr += w * (px & 255u); sg += w * ((px >> 8) & 255u); sb += w * ((px >> 16) & 255u);
                        cnt += 1;
                        if (rank == 0) obest = c;
                    }
                }
                if (ws) {
                    const uint32_t h = ws / 2;
                    orgbc = ((sr + h) / ws) | (((sg + h) / ws) << 8) | (((sb + h) / ws) << 16) | (cnt << 24);
                    ntex = 1;
                } else {
                    nfall = 1;
                }
            }
            p.rgbc[o] = orgbc;
            p.odepth[o] = odepth;
            p.best[o] = (uint8_t)obest;
            p.refined[o] = (uint8_t)oref;
        }
    }
    // every lane of the wave is here (the branches above have joined): wave sums, one atomic each from lane 0
    const uint32_t wh = wave_sum_u32(hits), wr = wave_sum_u32(nref), wt = wave_sum_u32(ntex), wf = wave_sum_u32(nfall);
    const uint32_t wp = wave_sum_u32(tests);
    if (lane == 0 && wh) {
        atomicAdd(p.ctr + 0, (unsigned long long)wh);
        atomicAdd(p.ctr + 1, (unsigned long long)wr);
        atomicAdd(p.ctr + 2, (unsigned long long)wt);
        atomicAdd(p.ctr + 3, (unsigned long long)wf);
        atomicAdd(p.ctr + 4, (unsigned long long)wp);
    }
}

}  // namespace vc
