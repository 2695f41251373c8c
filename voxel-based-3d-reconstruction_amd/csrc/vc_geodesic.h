// gfx950 kernels of the geodesic distances through the hull (vc_hull_geodesic, vc_geodesic_path, vc_paint_geodesic; contract in
// include/voxcarve.h and DESIGN.md section 8 item 16).  Integers only, wave64.  A key is d << 8 | label in one u64 per RECORD,
// kGeoNone = 2^64 - 1 where unreached; inside the relaxations an unreached key reads as kGeoInf = 2^62, so that key + (w << 8)
// never wraps and never wins.  Restated in tests/geodesic_np.py.
//
//   k_geo_seed_list    lane = seed: its record through woff + popcount; key 0; its tile and the neighbour tiles whose halo holds it
//                      listed (nobody lowered a source's key, so nobody else tells them); the first seed that is no survivor
//   k_geo_seed_layers  lane = record: key 0 and the same tiles listed when its iz lies in the layers
//   k_geo_tiles<N>     workgroup = one listed tile of 4 x 64 x 4 cells (x, y, z; y runs along the occupancy words): keys and a
//                      one-cell halo into LDS (66 x 6 x 6 x 8 B = 19 008 B), min-plus rounds in LDS until the tile is stable, the
//                      lowered cells written back, every neighbour tile whose halo holds a lowered cell listed for the next launch.
//                      A workgroup writes its own cells only and waits for nobody: a halo read that misses a concurrent store is a
//                      valid upper bound, and the storing tile lists this one again
//   k_geo_sweep<N>     lane = record: pulls from its neighbours' keys over the whole hull, in place; flag[0] = something fell
//   k_geo_best         the largest d among the reached records (atomicMax) and how many are reached
//   k_geo_pick         the lowest record that holds it (records ascend in the linear index)
//   k_geo_source       one lane: the picked record becomes source `label` when its d > 0; the same tiles listed; the extremum's entry
//   k_geo_path<<<1,64>>>  one wave, lanes = neighbour offsets: next(v) by a wave minimum per step
//   k_geo_paint        lane = record: RGB by region from the palette (LDS) or the grey ramp 255 d div max_d
#pragma once
#include "vc_components.h"       // cc_below (vc_kernels.h: decompose, wave_min_u32, wave_sum_u32); vc_distance.h: wave_max_u64

namespace vc {

constexpr uint32_t kGeoBlock = 256;
constexpr uint32_t kGeoTX = 4, kGeoTY = 64, kGeoTZ = 4;                          // cells per tile
constexpr uint32_t kGeoHX = kGeoTX + 2, kGeoHY = kGeoTY + 2, kGeoHZ = kGeoTZ + 2;  // with the halo
constexpr uint32_t kGeoHalo = kGeoHX * kGeoHY * kGeoHZ;
static_assert(kGeoBlock == kGeoTY * kGeoTZ, "a lane owns the cells (0 .. kGeoTX - 1, ly, lz)");
constexpr uint32_t kGeoMaxK = 32;
constexpr unsigned long long kGeoNone = 0xffffffffffffffffull, kGeoInf = 1ull << 62;
constexpr uint32_t kGeoNoRec = 0xffffffffu;

struct GeoParams {
    const uint64_t *records;         // [S]
    const uint64_t *words;           // occupancy words of the whole grid (dense)
    const uint32_t *woff;            // [nwords] survivors before each word
    unsigned long long *key;         // [S]
    uint64_t S;
    uint32_t nx, ny, nz;
    uint32_t lo[3];                  // the low corner of the survivors' index box: tile (0, 0, 0) starts there
    uint32_t nt[3];                  // tiles per axis
    uint32_t tiles;                  // their product: the capacity of a list
    unsigned long long w8[8];        // edge length << 8 by |dx| | |dy| << 1 | |dz| << 2 (entry 0 unused)
    uint32_t *flag[2];               // [tiles] 1: listed in list[parity]
    uint32_t *list[2];               // [tiles]
    uint32_t *count;                 // [2] entries of list[parity]
};

__device__ __forceinline__ unsigned long long geo_load(const unsigned long long *a)
{
    return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void geo_store(unsigned long long *a, unsigned long long v)
{
    __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the record of voxel i, kGeoNoRec when it is no survivor
__device__ __forceinline__ uint32_t geo_record(const GeoParams &p, uint32_t i)
{
    const uint64_t w = p.words[i >> 6];
    const uint32_t b = i & 63u;
    if (!((w >> b) & 1ull)) return kGeoNoRec;
    return p.woff[i >> 6] + (uint32_t)__popcll(w & cc_below(b));
}

// Lists `tile` in list[par] unless it is there already.
__device__ __forceinline__ void geo_list(const GeoParams &p, uint32_t par, uint32_t tile)
{
    if (atomicExch(p.flag[par] + tile, 1u) != 0u) return;
    const uint32_t at = atomicAdd(p.count + par, 1u);
    if (at < p.tiles) p.list[par][at] = tile;                     // (a flag per tile: the count cannot pass the capacity; the host checks it)
}

// A new source at (ix, iy, iz): its tile is listed in list[0], and so is every neighbour tile whose halo holds the cell -- the
// source's key was set from outside, so no tile has lowered it and told them.
__device__ __forceinline__ void geo_list_source(const GeoParams &p, uint32_t ix, uint32_t iy, uint32_t iz)
{
    const uint32_t c[3] = {ix - p.lo[0], iy - p.lo[1], iz - p.lo[2]}, td[3] = {kGeoTX, kGeoTY, kGeoTZ};
    int lo[3], hi[3];
    uint32_t t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        t[a] = c[a] / td[a];
        const uint32_t l = c[a] % td[a];
        lo[a] = (l == 0 && t[a] > 0) ? -1 : 0;
        hi[a] = (l == td[a] - 1 && t[a] + 1 < p.nt[a]) ? 1 : 0;
    }
    for (int dz = lo[2]; dz <= hi[2]; ++dz)
        for (int dx = lo[0]; dx <= hi[0]; ++dx)
            for (int dy = lo[1]; dy <= hi[1]; ++dy)
                geo_list(p, 0, ((uint32_t)((int)t[2] + dz) * p.nt[0] + (uint32_t)((int)t[0] + dx)) * p.nt[1] + (uint32_t)((int)t[1] + dy));
}

// acc[0] += seeds that were no source yet, acc[1] = min position of a seed that is no survivor (preset to 2^64 - 1)
__global__ __launch_bounds__(kGeoBlock) void k_geo_seed_list(const GeoParams p, const uint32_t *__restrict__ seeds, uint64_t n_seeds,
                                                             uint64_t n_voxels, unsigned long long *__restrict__ acc)
{
    const uint64_t k = (uint64_t)blockIdx.x * kGeoBlock + threadIdx.x;
    if (k >= n_seeds) return;
    const uint32_t i = seeds[k];
    const uint32_t s = (uint64_t)i < n_voxels ? geo_record(p, i) : kGeoNoRec;
    if (s == kGeoNoRec) {
        atomicMin(acc + 1, (unsigned long long)k);
        return;
    }
    if (atomicExch(p.key + s, 0ull) != 0ull) atomicAdd(acc + 0, 1ull);
    uint32_t ix, iy, iz;
    decompose(i, p.nx, p.ny, ix, iy, iz);
    geo_list_source(p, ix, iy, iz);
}

__global__ __launch_bounds__(kGeoBlock) void k_geo_seed_layers(const GeoParams p, uint32_t z0, uint32_t z1, unsigned long long *__restrict__ acc)
{
    const uint64_t s = (uint64_t)blockIdx.x * kGeoBlock + threadIdx.x;
    bool mine = false;
    if (s < p.S) {
        uint32_t ix, iy, iz;
        decompose((uint32_t)p.records[s], p.nx, p.ny, ix, iy, iz);
        mine = iz >= z0 && iz <= z1;
        if (mine) {
            p.key[s] = 0ull;
            geo_list_source(p, ix, iy, iz);
        }
    }
    const uint32_t n = (uint32_t)__popcll(__ballot(mine));
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(acc + 0, (unsigned long long)n);
}

template <int CONN>
__device__ __forceinline__ constexpr bool geo_edge(int dx, int dy, int dz)
{
    const int l1 = (dx != 0) + (dy != 0) + (dz != 0);
    return l1 >= 1 && l1 <= (CONN == 6 ? 1 : CONN == 18 ? 2 : 3);
}

// Round `par`: workgroup b takes tile list[par][b]; lists for round par ^ 1.
template <int CONN>
__global__ __launch_bounds__(kGeoBlock) void k_geo_tiles(const GeoParams p, uint32_t par)
{
    __shared__ unsigned long long s_key[kGeoHalo];
    __shared__ uint32_t s_dirs;
    const uint32_t t = threadIdx.x;
    const uint32_t tile = p.list[par][blockIdx.x];
    const uint32_t ty = tile % p.nt[1], tx = (tile / p.nt[1]) % p.nt[0], tz = tile / (p.nt[1] * p.nt[0]);
    // grid coordinates of the halo's cell 0 (may be -1)
    const int32_t ox = (int32_t)(p.lo[0] + tx * kGeoTX) - 1, oy = (int32_t)(p.lo[1] + ty * kGeoTY) - 1, oz = (int32_t)(p.lo[2] + tz * kGeoTZ) - 1;
    if (t == 0) {
        s_dirs = 0;
        p.flag[par][tile] = 0;                                    // (nobody sets this parity's flags during this round)
    }
    for (uint32_t c = t; c < kGeoHalo; c += kGeoBlock) {
        const uint32_t hy = c % kGeoHY, hx = (c / kGeoHY) % kGeoHX, hz = c / (kGeoHY * kGeoHX);
        const int32_t gx = ox + (int32_t)hx, gy = oy + (int32_t)hy, gz = oz + (int32_t)hz;
        unsigned long long k = kGeoInf;
        if (gx >= 0 && gy >= 0 && gz >= 0 && gx < (int32_t)p.nx && gy < (int32_t)p.ny && gz < (int32_t)p.nz) {
            const uint32_t s = geo_record(p, ((uint32_t)gz * p.nx + (uint32_t)gx) * p.ny + (uint32_t)gy);
            if (s != kGeoNoRec) {
                k = geo_load(p.key + s);
                k = k < kGeoInf ? k : kGeoInf;
            }
        }
        s_key[c] = k;
    }
    // this lane's cells: (lx, ly, lz), lx = 0 .. kGeoTX - 1
    const uint32_t ly = t % kGeoTY, lz = t / kGeoTY;
    uint32_t rec[kGeoTX];
    uint32_t at[kGeoTX];
#pragma unroll
    for (uint32_t lx = 0; lx < kGeoTX; ++lx) {
        at[lx] = ((lz + 1) * kGeoHX + lx + 1) * kGeoHY + ly + 1;
        const int32_t gx = ox + 1 + (int32_t)lx, gy = oy + 1 + (int32_t)ly, gz = oz + 1 + (int32_t)lz;
        rec[lx] = kGeoNoRec;
        if (gx < (int32_t)p.nx && gy < (int32_t)p.ny && gz < (int32_t)p.nz)
            rec[lx] = geo_record(p, ((uint32_t)gz * p.nx + (uint32_t)gx) * p.ny + (uint32_t)gy);
    }
    __syncthreads();
    unsigned long long first[kGeoTX];
#pragma unroll
    for (uint32_t lx = 0; lx < kGeoTX; ++lx) first[lx] = s_key[at[lx]];
    for (;;) {
        unsigned long long nv[kGeoTX];
#pragma unroll
        for (uint32_t lx = 0; lx < kGeoTX; ++lx) {
            unsigned long long best = kGeoNone;
            if (rec[lx] != kGeoNoRec) {
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
                        for (int dy = -1; dy <= 1; ++dy) {
                            if (!geo_edge<CONN>(dx, dy, dz)) continue;
                            const unsigned long long c = s_key[(int)at[lx] + (dz * (int)kGeoHX + dx) * (int)kGeoHY + dy] +
                                                         p.w8[(dx != 0) | (dy != 0) << 1 | (dz != 0) << 2];
                            best = c < best ? c : best;
                        }
            }
            nv[lx] = best;
        }
        __syncthreads();
        int fell = 0;
#pragma unroll
        for (uint32_t lx = 0; lx < kGeoTX; ++lx)
            if (nv[lx] < s_key[at[lx]]) {                         // (cells that are no survivors hold kGeoInf and nv = kGeoNone)
                s_key[at[lx]] = nv[lx];
                fell = 1;
            }
        if (!__syncthreads_or(fell)) break;
    }
    // write back what fell, and collect the directions of the neighbour tiles whose halo holds such a cell
    uint32_t dirs = 0;
#pragma unroll
    for (uint32_t lx = 0; lx < kGeoTX; ++lx) {
        const unsigned long long k = s_key[at[lx]];
        if (rec[lx] == kGeoNoRec || k >= first[lx]) continue;
        geo_store(p.key + rec[lx], k);
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
                    if (!geo_edge<CONN>(dx, dy, dz)) continue;
                    const bool onx = dx == 0 || (dx < 0 ? lx == 0 : lx == kGeoTX - 1);
                    const bool ony = dy == 0 || (dy < 0 ? ly == 0 : ly == kGeoTY - 1);
                    const bool onz = dz == 0 || (dz < 0 ? lz == 0 : lz == kGeoTZ - 1);
                    if (onx && ony && onz) dirs |= 1u << ((dz + 1) * 9 + (dx + 1) * 3 + (dy + 1));
                }
    }
    if (dirs) atomicOr(&s_dirs, dirs);
    __syncthreads();                                              // (the stores above are in flight before any flag is set; the next
    if (t < 27 && ((s_dirs >> t) & 1u)) {                         //  launch reads them, whatever order they land in)
        const int dz = (int)(t / 9) - 1, dx = (int)((t / 3) % 3) - 1, dy = (int)(t % 3) - 1;
        const int nx_ = (int)tx + dx, ny_ = (int)ty + dy, nz_ = (int)tz + dz;
        if (nx_ >= 0 && ny_ >= 0 && nz_ >= 0 && nx_ < (int)p.nt[0] && ny_ < (int)p.nt[1] && nz_ < (int)p.nt[2])
            geo_list(p, par ^ 1u, ((uint32_t)nz_ * p.nt[0] + (uint32_t)nx_) * p.nt[1] + (uint32_t)ny_);
    }
}

template <int CONN>
__global__ __launch_bounds__(kGeoBlock) void k_geo_sweep(const GeoParams p, uint32_t *__restrict__ flag)
{
    const uint64_t s = (uint64_t)blockIdx.x * kGeoBlock + threadIdx.x;
    if (s >= p.S) return;
    uint32_t ix, iy, iz;
    decompose((uint32_t)p.records[s], p.nx, p.ny, ix, iy, iz);
    unsigned long long mine = geo_load(p.key + s);
    mine = mine < kGeoInf ? mine : kGeoInf;
    unsigned long long best = mine;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                if (!geo_edge<CONN>(dx, dy, dz)) continue;
                if ((dz < 0 && iz == 0) || (dz > 0 && iz + 1 >= p.nz) || (dx < 0 && ix == 0) || (dx > 0 && ix + 1 >= p.nx)) continue;
                if ((dy < 0 && iy == 0) || (dy > 0 && iy + 1 >= p.ny)) continue;
                const uint32_t r = geo_record(p, ((iz + dz) * p.nx + (ix + dx)) * p.ny + (iy + dy));
                if (r == kGeoNoRec) continue;
                unsigned long long k = geo_load(p.key + r);
                k = (k < kGeoInf ? k : kGeoInf) + p.w8[(dx != 0) | (dy != 0) << 1 | (dz != 0) << 2];
                best = k < best ? k : best;
            }
    if (best < mine) {
        geo_store(p.key + s, best);
        if (!__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// acc[0] = max d over the reached records (preset to 0), acc[1] += reached
__global__ __launch_bounds__(kGeoBlock) void k_geo_best(const unsigned long long *__restrict__ key, uint64_t S, unsigned long long *__restrict__ acc)
{
    unsigned long long d = 0;
    uint32_t n = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * kGeoBlock + threadIdx.x; s < S; s += (uint64_t)gridDim.x * kGeoBlock) {
        const unsigned long long k = key[s];
        if (k == kGeoNone) continue;
        n += 1;
        d = (k >> 8) > d ? (k >> 8) : d;
    }
    d = wave_max_u64(d);
    n = wave_sum_u32(n);
    if ((threadIdx.x & 63u) == 0) {
        if (d > geo_load(acc + 0)) atomicMax(acc + 0, d);
        if (n) atomicAdd(acc + 1, (unsigned long long)n);
    }
}

// pick[0] = the lowest record whose d is acc[0] (preset to 0xffffffff)
__global__ __launch_bounds__(kGeoBlock) void k_geo_pick(const unsigned long long *__restrict__ key, uint64_t S, const unsigned long long *__restrict__ acc,
                                                        uint32_t *__restrict__ pick)
{
    const unsigned long long want = acc[0];
    uint32_t r = 0xffffffffu;
    for (uint64_t s = (uint64_t)blockIdx.x * kGeoBlock + threadIdx.x; s < S; s += (uint64_t)gridDim.x * kGeoBlock) {
        const unsigned long long k = key[s];
        if (k != kGeoNone && (k >> 8) == want) r = min(r, (uint32_t)s);
    }
    r = wave_min_u32(r);
    if ((threadIdx.x & 63u) == 0 && r != 0xffffffffu) atomicMin(pick, r);
}

// out[0] = d, out[1] = record | voxel << 32 (record 0xffffffff: no reached record at all).  With d > 0 the record becomes the source
// of `label` and its tile is listed in list[0].
__global__ void k_geo_source(const GeoParams p, const unsigned long long *__restrict__ acc, const uint32_t *__restrict__ pick, uint32_t label,
                             unsigned long long *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t s = pick[0];
    out[0] = acc[0];
    out[1] = 0xffffffffull;
    if (s == 0xffffffffu || (uint64_t)s >= p.S) return;
    const uint32_t i = (uint32_t)p.records[s];
    out[1] = (unsigned long long)s | ((unsigned long long)i << 32);
    if (acc[0] == 0) return;
    p.key[s] = (unsigned long long)label;
    uint32_t ix, iy, iz;
    decompose(i, p.nx, p.ny, ix, iy, iz);
    geo_list_source(p, ix, iy, iz);
}

constexpr uint32_t kGeoPathOk = 0, kGeoPathNoSurvivor = 1, kGeoPathUnreached = 2, kGeoPathBroken = 3;

// One wave.  out[0 .. min(n, capacity)) = the path from `voxel`, res[0] = n (its whole length), res[1] = kGeoPath*.  At most
// max_steps voxels are visited (d falls strictly along a path, so S bounds it).
__global__ __launch_bounds__(64) void k_geo_path(const GeoParams p, uint32_t connectivity, uint32_t voxel, uint32_t *__restrict__ out,
                                                 uint32_t capacity, uint64_t max_steps, uint32_t *__restrict__ res)
{
    const uint32_t lane = threadIdx.x;
    const int dz = (int)(lane / 9) - 1, dx = (int)((lane / 3) % 3) - 1, dy = (int)(lane % 3) - 1;
    const int l1 = (dx != 0) + (dy != 0) + (dz != 0);
    const bool edge = lane < 27 && l1 >= 1 && l1 <= (connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3);
    const unsigned long long w8 = p.w8[(dx != 0) | (dy != 0) << 1 | (dz != 0) << 2];
    uint32_t v = voxel, n = 0, status = kGeoPathOk;
    const uint32_t s0 = geo_record(p, v);
    if (s0 == kGeoNoRec) status = kGeoPathNoSurvivor;
    unsigned long long kv = status == kGeoPathOk ? p.key[s0] : 0ull;
    if (status == kGeoPathOk && kv == kGeoNone) status = kGeoPathUnreached;
    while (status == kGeoPathOk) {
        if (n < capacity && lane == 0) out[n] = v;
        n += 1;
        if ((kv >> 8) == 0) break;
        if ((uint64_t)n > max_steps) { status = kGeoPathBroken; break; }
        uint32_t ix, iy, iz;
        decompose(v, p.nx, p.ny, ix, iy, iz);
        uint32_t cand = 0xffffffffu;
        unsigned long long ck = 0;
        const int jx = (int)ix + dx, jy = (int)iy + dy, jz = (int)iz + dz;
        if (edge && jx >= 0 && jy >= 0 && jz >= 0 && jx < (int)p.nx && jy < (int)p.ny && jz < (int)p.nz) {
            const uint32_t j = ((uint32_t)jz * p.nx + (uint32_t)jx) * p.ny + (uint32_t)jy;
            const uint32_t r = geo_record(p, j);
            if (r != kGeoNoRec) {
                ck = p.key[r];
                if (ck != kGeoNone && ck + w8 == kv) cand = j;
            }
        }
        const uint32_t nxt = wave_min_u32(cand);
        if (nxt == 0xffffffffu) { status = kGeoPathBroken; break; }
        // the key of the chosen neighbour, from the lane that holds it
        const uint32_t src = (uint32_t)__ffsll((long long)__ballot(cand == nxt)) - 1u;
        kv = ((unsigned long long)__shfl((uint32_t)(ck >> 32), (int)src) << 32) | (unsigned long long)__shfl((uint32_t)ck, (int)src);
        v = nxt;
    }
    if (lane == 0) { res[0] = n; res[1] = status; }
}

struct GeoPalette { uint32_t rgb[kGeoMaxK + 1]; };                // r | g << 8 | b << 16 per label 0 .. K

// mode 0: the label's palette entry; mode 1: grey 255 d div max_d (0 when max_d = 0); unreached records take `none`
__global__ __launch_bounds__(kGeoBlock) void k_geo_paint(uint64_t *__restrict__ records, uint64_t S, const unsigned long long *__restrict__ key,
                                                        uint32_t mode, unsigned long long max_d, uint32_t none, const GeoPalette pal)
{
    __shared__ uint32_t s_pal[kGeoMaxK + 1];
    if (threadIdx.x <= kGeoMaxK) s_pal[threadIdx.x] = pal.rgb[threadIdx.x] & 0xffffffu;
    __syncthreads();
    const uint64_t s = (uint64_t)blockIdx.x * kGeoBlock + threadIdx.x;
    if (s >= S) return;
    const unsigned long long k = key[s];
    uint32_t rgb = none & 0xffffffu;
    if (k != kGeoNone) {
        if (mode == 0) {
            const uint32_t label = (uint32_t)(k & 255ull);
            rgb = s_pal[label <= kGeoMaxK ? label : 0];
        } else {
            const uint32_t g = max_d ? (uint32_t)(((k >> 8) * 255ull) / max_d) : 0u;
            rgb = g | g << 8 | g << 16;
        }
    }
    records[s] = (records[s] & 0xff000000ffffffffull) | ((uint64_t)rgb << 32);
}

}  // namespace vc
