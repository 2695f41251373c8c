// gfx950 kernels of the split of the hull into K figures on the floor plane (vc_hull_clusters, vc_paint_clusters; contract in
// include/voxcarve.h).  Restated in tests/clusters_np.py.  Integer atomics only: every sum is a sum
// over a set, every minimum and maximum exact, so the order of arrival does not show in any output.
//
//   k_cl_floor_records  the floor map by one u32 atomic per record, onto the record's column: the default, because it measured
//                    faster than the walk over the words below at 1024^3 and level with it elsewhere
//   k_cl_floor       the floor map from the occupancy words (vc_set_option "cluster_floor_records" = 0), no record touched:
//                    wave = 64 consecutive columns x kClLayers z layers; lane = column.  Layer iz of the 64 columns is the 64-bit
//                    string at bit iz nx ny + 64 g of the occupancy, a position that is the same for every lane: two lane-uniform
//                    loads (one when nx ny % 64 == 0), a funnel shift, and the lane takes its own bit.  The counts stay in a
//                    register; one u32 atomic per lane and wave, 256 contiguous bytes per wave, none for a zero.
//   k_cl_moments     lane = column: Wtot, sum w Px, sum w Py and the number of columns with a survivor, reduced per workgroup
//   k_cl_seed_best   lane = column: the largest key of seed j among the weighted columns, key = 2^63 - 1 - d2(P, M) for j = 0 (the
//                    nearest to M) and 1 + min_{i<j} d2(P, c_i) after that (the farthest from the seeds so far); the distance
//                    may need 62 bits, so the column cannot ride in the same atomic:
//   k_cl_seed_pick   the lowest column among those that hold the largest key
//   k_cl_round       lane = column: its label, and {W_k, sum w Px, sum w Py, columns} per label present in the wave, summed in LDS,
//                    one 64-bit atomic per non-zero entry per workgroup
//   k_cl_columns     lane = column, after the last round: voxels and the (ix, iy) box per label -- a label's records are the
//                    survivors of its columns, so neither needs the records
//   k_cl_records     lane = record: the label of its column, the colour histogram of the workgroup in LDS (K x 512 u32, at most
//                    32 KB; only non-zero bins are flushed), iz ranges per label reduced over the wave first
//   k_cl_paint       lane = record: RGB from the palette (LDS), one 8-byte store
// Every column index is checked against nx ny, every word index against the word count, every label against K before it indexes.
#pragma once
#include "vc_components.h"       // (vc_kernels.h: wave_min_u32, wave_max_u32)

namespace vc {

constexpr uint32_t kClBlock = 256;
constexpr uint32_t kClMaxK = 16;
constexpr uint32_t kClLayers = 32;                           // z layers per wave of k_cl_floor
constexpr uint32_t kClBins = 512;
constexpr uint32_t kClAcc = 4;                               // u64 per cluster and round: W, sum w Px, sum w Py, columns
constexpr uint32_t kClMaxBlocks = 2048;                      // of the kernels that stride
constexpr uint32_t kClNoLabel = 255;

struct ClCentres { long long c[kClMaxK][2]; };
struct ClPalette { uint32_t rgb[kClMaxK]; };                 // R | G << 8 | B << 16

struct ClCols {
    const uint32_t *fmap;       // [ncol] survivors per column
    uint32_t ncol, ny, min_column;
    long long qx, qy;           // um
};

__device__ __forceinline__ unsigned long long cl_wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long cl_wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}

__device__ __forceinline__ long long cl_d2(long long px, long long py, long long cx, long long cy)
{
    const long long dx = px - cx, dy = py - cy;
    return dx * dx + dy * dy;
}

// bits [pos, pos + 64) of the occupancy, zeros behind its last word
__device__ __forceinline__ uint64_t cl_bits64(const uint64_t *__restrict__ words, uint64_t pos, uint64_t nwords)
{
    const uint64_t w = pos >> 6;
    const uint32_t sh = (uint32_t)(pos & 63u);
    const uint64_t lo = w < nwords ? words[w] : 0ull;
    if (!sh) return lo;
    const uint64_t hi = w + 1 < nwords ? words[w + 1] : 0ull;
    return (lo >> sh) | (hi << (64u - sh));
}

__global__ __launch_bounds__(kClBlock) void k_cl_floor(const uint64_t *__restrict__ words, uint64_t nwords, uint32_t ncol, uint32_t nz,
                                                      uint32_t ngroups, uint32_t nchunks, uint32_t *__restrict__ fmap)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t wv = (uint64_t)blockIdx.x * (kClBlock / 64) + wave;
    if (wv >= (uint64_t)ngroups * nchunks) return;           // (whole waves)
    const uint32_t chunk = (uint32_t)(wv / ngroups), g = (uint32_t)(wv - (uint64_t)chunk * ngroups);
    const uint32_t z0 = chunk * kClLayers, z1 = min(z0 + kClLayers, nz);
    const uint64_t first = (uint64_t)g * 64u;
    uint32_t cnt = 0;
#pragma unroll 4
    for (uint32_t z = z0; z < z1; ++z)
        cnt += (uint32_t)(cl_bits64(words, (uint64_t)z * ncol + first, nwords) >> lane) & 1u;
    // the last group of a layer reads into the next layer when ncol % 64 != 0: those lanes own no column
    const uint64_t col = first + lane;
    if (col < ncol && cnt) atomicAdd(fmap + col, cnt);
}

__global__ __launch_bounds__(kClBlock) void k_cl_floor_records(const uint64_t *__restrict__ records, uint64_t S, uint32_t ncol,
                                                              uint32_t *__restrict__ fmap)
{
    const uint64_t s = (uint64_t)blockIdx.x * kClBlock + threadIdx.x;
    if (s >= S) return;
    atomicAdd(fmap + (uint32_t)records[s] % ncol, 1u);
}

// Column col of this lane in the stride loop's pass `base` (uniform over the workgroup): its count, weight and position.
__device__ __forceinline__ bool cl_column(const ClCols &p, uint64_t base, uint32_t &col, uint32_t &n, uint32_t &w, long long &px, long long &py)
{
    const uint64_t c = base + threadIdx.x;
    const bool valid = c < p.ncol;
    col = valid ? (uint32_t)c : 0u;
    n = valid ? p.fmap[col] : 0u;
    w = n >= p.min_column ? n : 0u;
    const uint32_t ix = col / p.ny;
    px = p.qx * (long long)ix;
    py = p.qy * (long long)(col - ix * p.ny);
    return valid;
}

__global__ __launch_bounds__(kClBlock) void k_cl_moments(const ClCols p, unsigned long long *__restrict__ acc /* [4] */)
{
    __shared__ unsigned long long s_v[kClBlock / 64][4];
    unsigned long long v[4] = {0, 0, 0, 0};
    for (uint64_t base = (uint64_t)blockIdx.x * kClBlock; base < p.ncol; base += (uint64_t)gridDim.x * kClBlock) {
        uint32_t col, n, w;
        long long px, py;
        cl_column(p, base, col, n, w, px, py);
        v[0] += w; v[1] += (unsigned long long)w * (unsigned long long)px; v[2] += (unsigned long long)w * (unsigned long long)py;
        v[3] += n ? 1u : 0u;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        v[a] = cl_wave_sum_u64(v[a]);
        if (lane == 0) s_v[wave][a] = v[a];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long t = 0;
        for (uint32_t k = 0; k < kClBlock / 64; ++k) t += s_v[k][threadIdx.x];
        if (t) atomicAdd(acc + threadIdx.x, t);
    }
}

struct ClSeed {
    const uint32_t *seedcol;    // [kClMaxK] the columns of the seeds so far
    unsigned long long *best;   // [kClMaxK] the largest key per seed, zeroed beforehand
    uint32_t *pick;             // == seedcol, 0xffffffff beforehand
    long long mx, my;           // M
    uint32_t j;
};

// The seeds so far as positions, into LDS; then the key of a weighted column (0: none).
__device__ __forceinline__ void cl_seed_centres(const ClCols &p, const ClSeed &q, long long (*s_c)[2])
{
    if (threadIdx.x < q.j && threadIdx.x < kClMaxK) {
        const uint32_t c = min(q.seedcol[threadIdx.x], p.ncol - 1u), ix = c / p.ny;
        s_c[threadIdx.x][0] = p.qx * (long long)ix;
        s_c[threadIdx.x][1] = p.qy * (long long)(c - ix * p.ny);
    }
    __syncthreads();
}
__device__ __forceinline__ unsigned long long cl_seed_key(const ClSeed &q, const long long (*s_c)[2], uint32_t w, long long px, long long py)
{
    if (!w) return 0ull;
    if (q.j == 0) return 0x7fffffffffffffffull - (unsigned long long)cl_d2(px, py, q.mx, q.my);
    long long m = cl_d2(px, py, s_c[0][0], s_c[0][1]);
    for (uint32_t i = 1; i < q.j; ++i) m = min(m, cl_d2(px, py, s_c[i][0], s_c[i][1]));
    return 1ull + (unsigned long long)m;
}

__global__ __launch_bounds__(kClBlock) void k_cl_seed_best(const ClCols p, const ClSeed q)
{
    __shared__ long long s_c[kClMaxK][2];
    cl_seed_centres(p, q, s_c);
    unsigned long long v = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * kClBlock; base < p.ncol; base += (uint64_t)gridDim.x * kClBlock) {
        uint32_t col, n, w;
        long long px, py;
        cl_column(p, base, col, n, w, px, py);
        const unsigned long long k = cl_seed_key(q, s_c, w, px, py);
        v = k > v ? k : v;
    }
    v = cl_wave_max_u64(v);
    // (the stored key only rises: a stale read costs an atomic too many, never a wrong skip)
    if ((threadIdx.x & 63u) == 0 && v > __hip_atomic_load(q.best + q.j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(q.best + q.j, v);
}

__global__ __launch_bounds__(kClBlock) void k_cl_seed_pick(const ClCols p, const ClSeed q)
{
    __shared__ long long s_c[kClMaxK][2];
    cl_seed_centres(p, q, s_c);
    const unsigned long long want = q.best[q.j];
    uint32_t c = 0xffffffffu;
    for (uint64_t base = (uint64_t)blockIdx.x * kClBlock; base < p.ncol; base += (uint64_t)gridDim.x * kClBlock) {
        uint32_t col, n, w;
        long long px, py;
        cl_column(p, base, col, n, w, px, py);
        if (w && cl_seed_key(q, s_c, w, px, py) == want) c = min(c, col);
    }
    c = wave_min_u32(c);
    if ((threadIdx.x & 63u) == 0 && c != 0xffffffffu) atomicMin(q.pick + q.j, c);
}

__global__ __launch_bounds__(kClBlock) void k_cl_round(const ClCols p, uint32_t K, const ClCentres ctr, uint8_t *__restrict__ flab,
                                                      unsigned long long *__restrict__ acc /* [K][kClAcc], zeroed */)
{
    __shared__ unsigned long long s_acc[kClMaxK][kClAcc];
    __shared__ long long s_c[kClMaxK][2];
    if (threadIdx.x < kClMaxK * kClAcc) (&s_acc[0][0])[threadIdx.x] = 0;
    if (threadIdx.x < K) { s_c[threadIdx.x][0] = ctr.c[threadIdx.x][0]; s_c[threadIdx.x][1] = ctr.c[threadIdx.x][1]; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * kClBlock; base < p.ncol; base += (uint64_t)gridDim.x * kClBlock) {
        uint32_t col, n, w;
        long long px, py;
        const bool valid = cl_column(p, base, col, n, w, px, py);
        uint32_t label = kClNoLabel;
        if (n) {
            long long dmin = cl_d2(px, py, s_c[0][0], s_c[0][1]);
            label = 0;
            for (uint32_t k = 1; k < K; ++k) {
                const long long d = cl_d2(px, py, s_c[k][0], s_c[k][1]);
                if (d < dmin) { dmin = d; label = k; }           // (a tie keeps the lower k)
            }
        }
        if (valid) flab[col] = (uint8_t)label;
        for (uint32_t k = 0; k < K; ++k) {
            const bool mine = label == k;
            const unsigned long long m = __ballot(mine);
            if (!m) continue;                                    // (uniform over the wave)
            const unsigned long long wk = mine ? w : 0u;
            const unsigned long long sw = cl_wave_sum_u64(wk);
            const unsigned long long sx = cl_wave_sum_u64(wk * (unsigned long long)px), sy = cl_wave_sum_u64(wk * (unsigned long long)py);
            if (lane == 0) {
                if (sw) { atomicAdd(&s_acc[k][0], sw); atomicAdd(&s_acc[k][1], sx); atomicAdd(&s_acc[k][2], sy); }
                atomicAdd(&s_acc[k][3], (unsigned long long)__popcll(m));
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < K * kClAcc) {
        const unsigned long long v = (&s_acc[0][0])[threadIdx.x];
        if (v) atomicAdd(acc + threadIdx.x, v);
    }
}

// voxels [K] (zeroed) and the boxes blo, bhi [K][3] in (ix, iy, iz) (lo at 0xffffffff, hi at 0 beforehand; iz by k_cl_records)
__global__ __launch_bounds__(kClBlock) void k_cl_columns(const ClCols p, uint32_t K, const uint8_t *__restrict__ flab,
                                                        unsigned long long *__restrict__ voxels, uint32_t *__restrict__ blo,
                                                        uint32_t *__restrict__ bhi)
{
    __shared__ unsigned long long s_n[kClMaxK];
    __shared__ uint32_t s_b[kClMaxK][4];
    if (threadIdx.x < kClMaxK) {
        s_n[threadIdx.x] = 0;
        s_b[threadIdx.x][0] = s_b[threadIdx.x][1] = 0xffffffffu;
        s_b[threadIdx.x][2] = s_b[threadIdx.x][3] = 0;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * kClBlock; base < p.ncol; base += (uint64_t)gridDim.x * kClBlock) {
        uint32_t col, n, w;
        long long px, py;
        cl_column(p, base, col, n, w, px, py);
        const uint32_t label = n ? flab[col] : kClNoLabel;
        const uint32_t ix = col / p.ny, iy = col - ix * p.ny;
        for (uint32_t k = 0; k < K; ++k) {
            const bool mine = label == k;
            if (!__ballot(mine)) continue;
            const unsigned long long sn = cl_wave_sum_u64(mine ? n : 0u);
            const uint32_t x0 = wave_min_u32(mine ? ix : 0xffffffffu), y0 = wave_min_u32(mine ? iy : 0xffffffffu);
            const uint32_t x1 = wave_max_u32(mine ? ix : 0u), y1 = wave_max_u32(mine ? iy : 0u);
            if (lane == 0) {
                atomicAdd(&s_n[k], sn);
                atomicMin(&s_b[k][0], x0); atomicMin(&s_b[k][1], y0);
                atomicMax(&s_b[k][2], x1); atomicMax(&s_b[k][3], y1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < K && s_n[threadIdx.x]) {
        const uint32_t k = threadIdx.x;
        atomicAdd(voxels + k, s_n[k]);
        atomicMin(blo + 3 * k + 0, s_b[k][0]); atomicMin(blo + 3 * k + 1, s_b[k][1]);
        atomicMax(bhi + 3 * k + 0, s_b[k][2]); atomicMax(bhi + 3 * k + 1, s_b[k][3]);
    }
}

struct ClRecords {
    const uint64_t *records;    // [S]
    const uint8_t *flab;        // [ncol]
    uint8_t *lab;               // [S]
    uint32_t *hist;             // [K][kClBins], zeroed
    uint32_t *blo, *bhi;        // [K][3] each: this kernel reduces entry 2 (iz)
    uint64_t S, per;            // records per workgroup, a multiple of kClBlock
    uint32_t ncol, K, zlo, zhi;
};

__global__ __launch_bounds__(kClBlock) void k_cl_records(const ClRecords p)
{
    __shared__ uint32_t s_hist[kClMaxK * kClBins];
    __shared__ uint32_t s_z[kClMaxK][2];
    for (uint32_t b = threadIdx.x; b < p.K * kClBins; b += kClBlock) s_hist[b] = 0;
    if (threadIdx.x < kClMaxK) { s_z[threadIdx.x][0] = 0xffffffffu; s_z[threadIdx.x][1] = 0; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t begin = (uint64_t)blockIdx.x * p.per, end = min(begin + p.per, p.S);
    for (uint64_t base = begin; base < end; base += kClBlock) {
        const uint64_t s = base + threadIdx.x;
        const bool valid = s < end;
        const uint64_t rec = valid ? p.records[s] : 0ull;
        const uint32_t idx = (uint32_t)rec, iz = idx / p.ncol, col = idx - iz * p.ncol;
        uint32_t label = valid ? p.flab[col] : kClNoLabel;
        if (valid) p.lab[s] = (uint8_t)label;
        if (label >= p.K) label = kClNoLabel;                    // (a record in a column without a count: nothing to index)
        if (label != kClNoLabel && ((rec >> 56) & 1ull) && iz >= p.zlo && iz <= p.zhi) {
            const uint32_t r = (uint32_t)(rec >> 32) & 255u, g = (uint32_t)(rec >> 40) & 255u, b = (uint32_t)(rec >> 48) & 255u;
            atomicAdd(&s_hist[label * kClBins + (((r >> 5) << 6) | ((g >> 5) << 3) | (b >> 5))], 1u);
        }
        for (uint32_t k = 0; k < p.K; ++k) {
            const bool mine = label == k;
            if (!__ballot(mine)) continue;
            const uint32_t z0 = wave_min_u32(mine ? iz : 0xffffffffu), z1 = wave_max_u32(mine ? iz : 0u);
            if (lane == 0) { atomicMin(&s_z[k][0], z0); atomicMax(&s_z[k][1], z1); }
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < p.K * kClBins; b += kClBlock)
        if (s_hist[b]) atomicAdd(p.hist + b, s_hist[b]);
    if (threadIdx.x < p.K && s_z[threadIdx.x][0] != 0xffffffffu) {
        atomicMin(p.blo + 3 * threadIdx.x + 2, s_z[threadIdx.x][0]);
        atomicMax(p.bhi + 3 * threadIdx.x + 2, s_z[threadIdx.x][1]);
    }
}

__global__ __launch_bounds__(kClBlock) void k_cl_paint(uint64_t *__restrict__ records, uint64_t S, const uint8_t *__restrict__ lab,
                                                      const ClPalette pal)
{
    __shared__ uint32_t s_pal[kClMaxK];
    if (threadIdx.x < kClMaxK) s_pal[threadIdx.x] = pal.rgb[threadIdx.x] & 0xffffffu;
    __syncthreads();
    const uint64_t s = (uint64_t)blockIdx.x * kClBlock + threadIdx.x;
    if (s >= S) return;
    const uint32_t label = lab[s];
    if (label >= kClMaxK) return;
    records[s] = (records[s] & 0xff000000ffffffffull) | ((uint64_t)s_pal[label] << 32);
}

}  // namespace vc
