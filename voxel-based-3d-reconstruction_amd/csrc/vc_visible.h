// gfx950 kernels of occlusion-aware colouring (vc_color_visible; contract in include/voxcarve.h and DESIGN.md section 8):
// each SURFACE survivor (a face neighbour is no survivor or lies outside the grid) splats its voxel box into a per-camera depth
// map, then takes the rounded mean colour of the cameras whose map it is not hidden behind.  Restated in tests/visible_np.py.
//
//   k_vis_fill      maps := +inf bits; counters := 0
//   k_vis_surface   lane = 16 survivor records: the surface test on the occupancy words, the surface survivors compacted into
//                   a list (one atomic per workgroup, order irrelevant), every survivor's camera mask := 0
//                   (<true>: records a photo-consistency round has removed are skipped -- vc_photo.h)
//   k_vis_splat     lane = surface survivor, grid y = camera: camera z of the centre and the 8 corners, the corners' pixel
//                   rectangle; small rectangles pixel by pixel, large ones queued
//   k_vis_splat_big a workgroup per queued rectangle
//   k_vis_color     lane = surface survivor, every camera: in-image and depth test at the centre's pixel, mean colour into
//                   the record's RGB bytes, the camera mask
// The maps hold float32 bits: positive floats order like their u32 bits, so atomicMin on the bits is a min on the depths and
// the maps come out the same whatever order the splats land in.  No host synchronisation: the counts never leave the device.
#pragma once
#include "vc_kernels.h"          // CamDev, decompose, kMaxCameras

#pragma clang fp contract(off)

namespace vc {

constexpr uint32_t kVisBlock = 256;
constexpr uint32_t kVisInf = 0x7f800000u;         // bits of +inf
constexpr uint32_t kVisQueue = 1u << 20;          // queue entries (16 B each); a full queue leaves the lane to do its own
constexpr uint32_t kVisSurfPer = 16;              // records per lane of k_vis_surface

struct VisParams {
    const double *xs, *ys, *zs;
    const uint64_t *words;      // occupancy of the grid (slab = whole grid), dead groups zeroed
    uint64_t *records;          // {u32 idx, r, g, b, seen}, S of them
    uint64_t S;
    uint32_t nx, ny, nz, C, H, W;
    double hx, hy, hz;          // half extents of a voxel box
    float tol;                  // depth tolerance
    uint32_t *zmap;             // [C][H W] float32 bits
    const uint32_t *frames;     // [C][H W] R | G << 8 | B << 16 | seen << 24
    uint16_t *vis;              // [S] camera mask
    uint32_t *list;             // [S] record positions of the surface survivors (ctr[0] of them)
    uint32_t *ctr;              // [0] surface survivors, [1] queued rectangles
    uint4 *queue;               // {camera, key, x0 | y0 << 16, x1 | y1 << 16}
    uint32_t big;               // rectangles of more pixels than this are queued for a workgroup each (option visible_big_rect)
    CamDev cam[kMaxCameras];
    const uint8_t *rounds;      // [S] round that removed the record, 0 = kept (k_vis_surface<true> only; vc_photo.h)
};

__device__ __forceinline__ bool vis_alive(const uint64_t *__restrict__ words, uint64_t j)
{
    return (words[j >> 6] >> (j & 63u)) & 1ull;
}

// camera-space z, the third row of project_point's rigid transform (same operations, same order)
__device__ __forceinline__ double vis_cam_z(const CamDev &c, double X, double Y, double Z)
{
    return c.r[6] * X + c.r[7] * Y + c.r[8] * Z + c.t[2];
}

// CHECK: a plain look first -- the stored value only ever falls, so one at or below the key makes the atomic a no-op (one round
// trip per pixel instead of an atomic that is issued and not waited for: option visible_check)
template <bool CHECK>
__device__ __forceinline__ void vis_min(uint32_t *__restrict__ z, uint32_t key)
{
    if (!CHECK || key < __hip_atomic_load(z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(z, key);
}

__global__ __launch_bounds__(kVisBlock) void k_vis_fill(uint32_t *__restrict__ zmap, uint64_t n, uint32_t *__restrict__ ctr)
{
    const uint64_t i = (uint64_t)blockIdx.x * kVisBlock + threadIdx.x;
    if (i == 0) { ctr[0] = 0u; ctr[1] = 0u; }
    const uint64_t q = i * 4u;
    if (q + 4u <= n) reinterpret_cast<uint4 *>(zmap)[i] = make_uint4(kVisInf, kVisInf, kVisInf, kVisInf);
    else for (uint64_t k = q; k < n; ++k) zmap[k] = kVisInf;
}

__device__ __forceinline__ bool vis_surface(const VisParams &p, uint32_t i)
{
    uint32_t ix, iy, iz;
    decompose(i, p.nx, p.ny, ix, iy, iz);
    const uint64_t j = i, nxy = (uint64_t)p.nx * p.ny;
    // (a neighbour's word is read only when the neighbour lies inside the grid)
    return iy + 1 >= p.ny || iy == 0 || ix + 1 >= p.nx || ix == 0 || iz + 1 >= p.nz || iz == 0 ||
           !vis_alive(p.words, j + 1) || !vis_alive(p.words, j - 1) || !vis_alive(p.words, j + p.ny) ||
           !vis_alive(p.words, j - p.ny) || !vis_alive(p.words, j + nxy) || !vis_alive(p.words, j - nxy);
}

// A workgroup takes kVisBlock x kVisSurfPer consecutive records (lane t: records base + r kVisBlock + t, coalesced) and appends
// its surface survivors to the list with ONE atomic: one per wave of 64 records put 470 000 atomics on a single address at
// 1024^3 (2.3 ms, measured), one per 4096 records puts 7 300.
// SKIP: records with rounds[s] != 0 are no survivors any more (their bits have left the words) and never join the list.
template <bool SKIP>
__global__ __launch_bounds__(kVisBlock) void k_vis_surface(const VisParams p)
{
    __shared__ uint32_t s_wave[kVisBlock / 64], s_base;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kVisBlock * kVisSurfPer;
    uint32_t bits = 0;
#pragma unroll 4
    for (uint32_t r = 0; r < kVisSurfPer; ++r) {
        const uint64_t s = base + (uint64_t)r * kVisBlock + t;
        if (s < p.S) {
            if ((!SKIP || p.rounds[s] == 0) && vis_surface(p, (uint32_t)p.records[s])) bits |= 1u << r;
            p.vis[s] = 0;
        }
    }
    const uint32_t cnt = (uint32_t)__popc(bits);
    uint32_t x = cnt;                                            // inclusive scan over the wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    if (t == 0) {
        uint32_t total = 0;
        for (uint32_t w = 0; w < kVisBlock / 64; ++w) { const uint32_t v = s_wave[w]; s_wave[w] = total; total += v; }
        s_base = total ? atomicAdd(p.ctr, total) : 0u;
    }
    __syncthreads();
    uint32_t pos = s_base + s_wave[wave] + x - cnt;
    while (bits) {
        const uint32_t r = (uint32_t)__ffs(bits) - 1u;
        bits &= bits - 1u;
        p.list[pos++] = (uint32_t)(base + (uint64_t)r * kVisBlock + t);
    }
}

// grid y = camera (wave-uniform: the camera's parameters stay in scalar registers)
template <bool CHECK>
__global__ __launch_bounds__(kVisBlock) void k_vis_splat(const VisParams p)
{
    const uint32_t c = blockIdx.y;
    const CamDev &cam = p.cam[c];
    const uint32_t n = __hip_atomic_load(p.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t *__restrict__ zc = p.zmap + (size_t)c * p.H * p.W;
    for (uint32_t k = blockIdx.x * kVisBlock + threadIdx.x; k < n; k += gridDim.x * kVisBlock) {
        const uint32_t i = (uint32_t)p.records[p.list[k]];
        uint32_t ix, iy, iz;
        decompose(i, p.nx, p.ny, ix, iy, iz);
        const double X = p.xs[ix], Y = p.ys[iy], Z = p.zs[iz];
        const double d = vis_cam_z(cam, X, Y, Z);
        if (!(d > 0.0)) continue;
        double umin = 0, umax = 0, vmin = 0, vmax = 0;
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double cx = (q & 2) ? X + p.hx : X - p.hx;
            const double cy = (q & 1) ? Y + p.hy : Y - p.hy;
            const double cz = (q & 4) ? Z + p.hz : Z - p.hz;
            const double x = cam.r[0] * cx + cam.r[1] * cy + cam.r[2] * cz + cam.t[0];
            const double y = cam.r[3] * cx + cam.r[4] * cy + cam.r[5] * cz + cam.t[1];
            const double z = cam.r[6] * cx + cam.r[7] * cy + cam.r[8] * cz + cam.t[2];
            ok = ok && z > 0.0;
            double u, v;
            distort_and_project(cam, x, y, z, u, v);
            ok = ok && __builtin_isfinite(u) && __builtin_isfinite(v);
            umin = q ? fmin(umin, u) : u; umax = q ? fmax(umax, u) : u;
            vmin = q ? fmin(vmin, v) : v; vmax = q ? fmax(vmax, v) : v;
        }
        if (!ok) continue;
        // (every value is finite here, so fmin / fmax are the plain min / max)
        const double fx0 = fmax(floor(umin), 0.0), fx1 = fmin(floor(umax), (double)(p.W - 1));
        const double fy0 = fmax(floor(vmin), 0.0), fy1 = fmin(floor(vmax), (double)(p.H - 1));
        if (!(fx0 <= fx1 && fy0 <= fy1)) continue;
        const uint32_t x0 = (uint32_t)fx0, x1 = (uint32_t)fx1, y0 = (uint32_t)fy0, y1 = (uint32_t)fy1;
        const uint32_t key = __float_as_uint((float)d);
        const uint64_t area = (uint64_t)(x1 - x0 + 1) * (y1 - y0 + 1);
        if (area > p.big) {
            const uint32_t e = atomicAdd(p.ctr + 1, 1u);
            if (e < kVisQueue) {
                p.queue[e] = make_uint4(c, key, x0 | (y0 << 16), x1 | (y1 << 16));
                continue;
            }
        }
        for (uint32_t y = y0; y <= y1; ++y)
            for (uint32_t x = x0; x <= x1; ++x) vis_min<CHECK>(zc + (size_t)y * p.W + x, key);
    }
}

template <bool CHECK>
__global__ __launch_bounds__(kVisBlock) void k_vis_splat_big(const VisParams p)
{
    uint32_t n = __hip_atomic_load(p.ctr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n > kVisQueue) n = kVisQueue;
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
        const uint4 r = p.queue[e];
        const uint32_t x0 = r.z & 0xffffu, y0 = r.z >> 16, x1 = r.w & 0xffffu, y1 = r.w >> 16;
        const uint32_t w = x1 - x0 + 1, area = w * (y1 - y0 + 1);
        uint32_t *__restrict__ zc = p.zmap + (size_t)r.x * p.H * p.W;
        for (uint32_t t = threadIdx.x; t < area; t += kVisBlock) {
            const uint32_t y = y0 + t / w, x = x0 + t % w;
            vis_min<CHECK>(zc + (size_t)y * p.W + x, r.y);
        }
    }
}

__global__ __launch_bounds__(kVisBlock) void k_vis_color(const VisParams p)
{
    const uint32_t n = __hip_atomic_load(p.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const size_t HW = (size_t)p.H * p.W;
    for (uint32_t k = blockIdx.x * kVisBlock + threadIdx.x; k < n; k += gridDim.x * kVisBlock) {
        const uint32_t s = p.list[k];
        const uint64_t rec = p.records[s];
        uint32_t ix, iy, iz;
        decompose((uint32_t)rec, p.nx, p.ny, ix, iy, iz);
        const double X = p.xs[ix], Y = p.ys[iy], Z = p.zs[iz];
        uint32_t mask = 0, cnt = 0, sr = 0, sg = 0, sb = 0;
        for (uint32_t c = 0; c < p.C; ++c) {
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
            mask |= 1u << c;
            cnt += 1;
            sr += px & 0xffu; sg += (px >> 8) & 0xffu; sb += (px >> 16) & 0xffu;
        }
        p.vis[s] = (uint16_t)mask;
        if (cnt) {
            const uint32_t h = cnt / 2;
            const uint64_t rgb = (uint64_t)((sr + h) / cnt) | ((uint64_t)((sg + h) / cnt) << 8) | ((uint64_t)((sb + h) / cnt) << 16);
            p.records[s] = (rec & 0xff000000ffffffffull) | (rgb << 32);
        }
    }
}

}  // namespace vc
