// gfx950 kernels for the contour stage of the reference's extract_foreground_mask, background_subtraction.py:171-193:
// findContours(RETR_TREE, CHAIN_APPROX_SIMPLE), every contour of area >= figure_threshold filled, each of its children whose
// oriented area is >= figure_inner_threshold cleared again with its outline kept.  Border following is sequential; what the
// stage outputs is not.  Restated over connected components of the mask padded with a ring of zeros (OpenCV pads the same way):
//   * foreground components 8-connected, background components 4-connected; the padding's background component is the
//     FRAME.  A component is named by its raster-first padded pixel (label = minimum padded linear index; the frame is 0).
//   * parent of a component = the component of its raster-first pixel's left neighbour (Suzuki-Abe's start condition): the
//     background around a foreground component, the foreground around a hole.  The frame has none.
//   * contourArea of a component's border = area of the (H+1) x (W+1) cells between pixel centres attributed to the
//     component and all its descendants; a cell's area goes to its corners' components by the number of foreground corners
//     (half units: 4 -> 2 to the fg component; 3 -> 1 fg, 1 the bg corner's; 2 edge-adjacent -> 2 bg; 2 diagonal -> 1 to each
//     bg corner's; 0 or 1 -> 2 bg).  Outer borders are traced counter-clockwise (negative oriented area), holes clockwise.
//   * output of pixel p in component X: F = deepest component on the path X -> frame whose |area| >= T (none: 0); F == X: 255;
//     else Z = F's child on the path: Z's oriented area >= t -> 0, except p in Z, Z foreground and p 4-adjacent to F (Z's
//     outline, redrawn): 255; otherwise 255.
// tests/contour_literal.py restates the published border following, fill and loop; tests/test_contour_stage.py holds this
// formulation (tests/contour_components.py) to it and tests/test_gpu_contour.py these kernels.
//
// Per camera (grid z) four u32 planes of the padded size Np = (H + 2) (W + 2): lab (union-find parents, then labels), own
// (area attributed to a root, half units), tot (subtree sum of own; then the root's output code), par (parent of a root).
// Everything runs on one stream without host synchronisation; counts of components never leave the device.
#pragma once
#include "vc_kernels.h"          // uf_find, uf_union

namespace vc {

constexpr uint32_t kFillBlock = 256;
constexpr uint32_t kFillWave = 64;
static_assert(kFillBlock % kFillWave == 0, "the area reduction works on whole 64-lane waves");
constexpr uint32_t kFillMaxCameras = 16;
constexpr uint32_t kCodeZero = 0xffffffffu, kCodeOne = 0xfffffffeu;   // output codes of a root; anything else: outline test

struct FillParams {
    const uint8_t *mask;     // [cams][H W], foreground where != 0
    uint8_t *out;            // [cams][H W], {0, 255}
    uint32_t *lab, *own, *tot, *par;   // [cams][Np]
    uint32_t H, W, Wp, Np;
    uint32_t max_depth;      // bound of every walk up the tree (nesting needs a ring of pixels per level)
    double T[kFillMaxCameras], t[kFillMaxCameras];
};

__device__ __forceinline__ bool fill_fg(const uint8_t *m, const FillParams &p, uint32_t q)   // q: padded index
{
    const uint32_t y = q / p.Wp, x = q - y * p.Wp;
    if (y == 0 || x == 0 || y > p.H || x > p.W) return false;
    return m[(size_t)(y - 1) * p.W + (x - 1)] != 0;
}

// Every padded pixel its own set; the area planes cleared.
__global__ __launch_bounds__(kFillBlock) void k_fill_init(const FillParams p)
{
    const uint32_t q = blockIdx.x * kFillBlock + threadIdx.x;
    if (q >= p.Np) return;
    const size_t o = (size_t)blockIdx.z * p.Np + q;
    p.lab[o] = q;
    p.own[o] = 0u;
    p.tot[o] = 0u;
}

// Labelling runs in two passes over tiles of kTile x kTile padded pixels (one workgroup, one lane per pixel).  k_fill_local
// unites the pixels of a tile in LDS and leaves each pointing at its tile-local root: local index ly * kTile + lx orders the
// tile's pixels as the padded linear index does, so that root is the component's minimum global index within the tile, and the
// global array is a valid forest (every pointer <= its index, inside its set).  k_fill_merge then unites only across tile
// edges, where the global atomics are: about 4 / kTile of the pixels instead of all of them.
constexpr uint32_t kTile = 16;
static_assert(kTile * kTile == kFillBlock, "one lane per pixel of a tile");

__device__ __forceinline__ bool fill_same(const uint8_t *m, const FillParams &p, uint32_t gy, uint32_t gx, bool f)
{
    return fill_fg(m, p, gy * p.Wp + gx) == f;
}

// Grid (ceil(Wp / kTile), ceil(Hp / kTile), cams), kFillBlock lanes.
__global__ __launch_bounds__(kFillBlock) void k_fill_local(const FillParams p)
{
    __shared__ uint32_t S[kFillBlock];
    const uint32_t t = threadIdx.x, ly = t / kTile, lx = t - ly * kTile;
    const uint32_t gy = blockIdx.y * kTile + ly, gx = blockIdx.x * kTile + lx;
    const bool valid = gy < p.H + 2 && gx < p.Wp;
    const uint8_t *m = p.mask + (size_t)blockIdx.z * p.H * p.W;
    S[t] = t;
    __syncthreads();
    if (valid) {
        const bool f = fill_fg(m, p, gy * p.Wp + gx);
        if (lx > 0 && fill_same(m, p, gy, gx - 1, f)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(S, t, t - 1);
        if (ly > 0) {
            if (fill_same(m, p, gy - 1, gx, f)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(S, t, t - kTile);
            if (f) {
                if (lx > 0 && fill_fg(m, p, (gy - 1) * p.Wp + gx - 1)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(S, t, t - kTile - 1);
                if (lx + 1 < kTile && gx + 1 < p.Wp && fill_fg(m, p, (gy - 1) * p.Wp + gx + 1)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(S, t, t - kTile + 1);
            }
        }
    }
    __syncthreads();
    if (!valid) return;
    const uint32_t r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(S, t), ry = r / kTile, rx = r - ry * kTile;
    p.lab[(size_t)blockIdx.z * p.Np + gy * p.Wp + gx] = (blockIdx.y * kTile + ry) * p.Wp + blockIdx.x * kTile + rx;
}

// Union with the raster-earlier neighbours of the same class that lie in another tile: left and up (both classes), up-left and
// up-right (foreground).  Same grid as k_fill_local.
__global__ __launch_bounds__(kFillBlock) void k_fill_merge(const FillParams p)
{
    const uint32_t t = threadIdx.x, ly = t / kTile, lx = t - ly * kTile;
    if (ly != 0 && lx != 0 && lx != kTile - 1) return;            // interior of the tile: k_fill_local united it
    const uint32_t y = blockIdx.y * kTile + ly, x = blockIdx.x * kTile + lx;
    if (y >= p.H + 2 || x >= p.Wp) return;
    const uint32_t q = y * p.Wp + x;
    const uint8_t *m = p.mask + (size_t)blockIdx.z * p.H * p.W;
    uint32_t *L = p.lab + (size_t)blockIdx.z * p.Np;
    const bool f = fill_fg(m, p, q);
    if (lx == 0 && x > 0 && fill_fg(m, p, q - 1) == f) uf_union(L, q, q - 1);
    if (y > 0) {
        if (ly == 0 && fill_fg(m, p, q - p.Wp) == f) uf_union(L, q, q - p.Wp);
        if (f) {
            if ((ly == 0 || lx == 0) && x > 0 && fill_fg(m, p, q - p.Wp - 1)) uf_union(L, q, q - p.Wp - 1);
            if ((ly == 0 || lx == kTile - 1) && x + 1 < p.Wp && fill_fg(m, p, q - p.Wp + 1)) uf_union(L, q, q - p.Wp + 1);
        }
    }
}

// Every pixel points at its root: label = minimum padded index of the component.
__global__ __launch_bounds__(kFillBlock) void k_fill_compress(const FillParams p)
{
    const uint32_t q = blockIdx.x * kFillBlock + threadIdx.x;
    if (q >= p.Np) return;
    uint32_t *L = p.lab + (size_t)blockIdx.z * p.Np;
    const uint32_t r = uf_find(L, q);
    __hip_atomic_store(&L[q], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A wave adds (key, v) pairs into own[]: one atomic per distinct key of the wave.  Every lane of the wave calls it
// (key kCodeZero = nothing to add).
__device__ __forceinline__ void fill_wave_add(uint32_t *own, uint32_t key, uint32_t v)
{
    const uint32_t lane = threadIdx.x & (kFillWave - 1);
    for (;;) {
        const unsigned long long pending = __ballot(key != kCodeZero);
        if (!pending) return;
        const int leader = __ffsll((long long)pending) - 1;
        const uint32_t lk = __shfl(key, leader);
        uint32_t s = key == lk ? v : 0u;
#pragma unroll
        for (uint32_t off = kFillWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, (int)off);
        if (lane == (uint32_t)leader) atomicAdd(&own[lk], s);
        if (key == lk) key = kCodeZero;
    }
}

// One lane per cell (cy, cx), cy <= H, cx <= W, between padded pixel centres (cy, cx) .. (cy + 1, cx + 1): its area goes to
// the components at its corners (the frame's share is dropped: the frame has no border).  The same lane also records the
// parent of the component whose root is padded pixel (cy, cx) -- every image pixel is such a corner.
__global__ __launch_bounds__(kFillBlock) void k_fill_area(const FillParams p)
{
    const uint32_t i = blockIdx.x * kFillBlock + threadIdx.x;
    const uint32_t ncells = (p.H + 1) * (p.W + 1);
    const uint8_t *m = p.mask + (size_t)blockIdx.z * p.H * p.W;
    const uint32_t *L = p.lab + (size_t)blockIdx.z * p.Np;
    uint32_t ka = kCodeZero, kb = kCodeZero, va = 0, vb = 0;
    if (i < ncells) {
        const uint32_t cy = i / (p.W + 1), cx = i - cy * (p.W + 1);
        const uint32_t q0 = cy * p.Wp + cx, q[4] = {q0, q0 + 1, q0 + p.Wp, q0 + p.Wp + 1};   // TL, TR, BL, BR
        bool f[4];
        uint32_t l[4];
        int nf = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { f[j] = fill_fg(m, p, q[j]); l[j] = L[q[j]]; nf += f[j]; }
        int jf = 0, jb = 0;                                       // first fg / first bg corner
#pragma unroll
        for (int j = 3; j >= 0; --j) { if (f[j]) jf = j; else jb = j; }
        if (nf == 4) { ka = l[0]; va = 2; }
        else if (nf == 3) { ka = l[jf]; va = 1; kb = l[jb]; vb = 1; }
        else if (nf == 2 && f[0] == f[3]) {                       // diagonal pair: one half unit to each bg corner's component
            ka = f[0] ? l[1] : l[0]; va = 1;
            kb = f[0] ? l[2] : l[3]; vb = 1;
        } else { ka = l[jb]; va = 2; }
        if (ka == 0) ka = kCodeZero;
        if (kb == 0) kb = kCodeZero;
        if (q0 != 0 && L[q0] == q0) p.par[(size_t)blockIdx.z * p.Np + q0] = L[q0 - 1];
    }
    uint32_t *own = p.own + (size_t)blockIdx.z * p.Np;
    fill_wave_add(own, ka, va);
    fill_wave_add(own, kb, vb);
}

// tot[X] = own of X and of all its descendants: each root adds its own area to itself and its ancestors below the frame.
__global__ __launch_bounds__(kFillBlock) void k_fill_subtree(const FillParams p)
{
    const uint32_t q = blockIdx.x * kFillBlock + threadIdx.x;
    if (q == 0 || q >= p.Np) return;
    const size_t b = (size_t)blockIdx.z * p.Np;
    if (p.lab[b + q] != q) return;
    const uint32_t v = p.own[b + q];
    if (v == 0) return;
    uint32_t node = q;
    for (uint32_t d = 0; d < p.max_depth && node != 0; ++d) {
        atomicAdd(&p.tot[b + node], v);
        node = p.par[b + node];
    }
}

// Output code of each root X (written to own[X], which nothing reads any more): the walk to the deepest figure F.
__global__ __launch_bounds__(kFillBlock) void k_fill_resolve(const FillParams p)
{
    const uint32_t q = blockIdx.x * kFillBlock + threadIdx.x;
    if (q >= p.Np) return;
    const size_t b = (size_t)blockIdx.z * p.Np;
    if (p.lab[b + q] != q) return;
    const uint8_t *m = p.mask + (size_t)blockIdx.z * p.H * p.W;
    const double T = p.T[blockIdx.z], t = p.t[blockIdx.z];
    uint32_t code = kCodeZero;
    uint32_t node = q, prev = 0;
    bool found = false;
    for (uint32_t d = 0; d < p.max_depth && node != 0; ++d) {
        if ((double)p.tot[b + node] * 0.5 >= T) { found = true; break; }
        prev = node;
        node = p.par[b + node];
    }
    if (found) {
        if (node == q) code = kCodeOne;
        else {
            const bool zf = fill_fg(m, p, prev);
            const double a = (double)p.tot[b + prev] * 0.5;
            if ((zf ? -a : a) >= t) code = (zf && prev == q) ? node : kCodeZero;   // cleared; Z's own outline (4-adjacent to F) redrawn
            else code = kCodeOne;
        }
    }
    p.own[b + q] = code;
}

// One lane per image pixel: its component's code.
__global__ __launch_bounds__(kFillBlock) void k_fill_output(const FillParams p)
{
    const uint32_t i = blockIdx.x * kFillBlock + threadIdx.x;
    if (i >= p.H * p.W) return;
    const size_t b = (size_t)blockIdx.z * p.Np;
    const uint32_t y = i / p.W, x = i - y * p.W;
    const uint32_t q = (y + 1) * p.Wp + x + 1;
    const uint32_t code = p.own[b + p.lab[b + q]];
    uint8_t v = 0;
    if (code == kCodeOne) v = 255;
    else if (code != kCodeZero) {
        const uint32_t *L = p.lab + b;
        v = (L[q - 1] == code || L[q + 1] == code || L[q - p.Wp] == code || L[q + p.Wp] == code) ? 255 : 0;
    }
    p.out[(size_t)blockIdx.z * p.H * p.W + i] = v;
}

}  // namespace vc
