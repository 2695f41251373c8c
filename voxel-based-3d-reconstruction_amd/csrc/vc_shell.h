// gfx950 kernels of the hull's shell (vc_hull_shell; contract in include/voxcarve.h).  Restated in
// tests/shell_np.py.  The shell is the list of the ON cells with an exposed face, in ascending cell index, at level 0 (the
// voxels) or on a grid 2^L times coarser.  Integers only; the order of the list is the order of the cells, the colour sums are
// integer atomics, so neither the evaluation order nor the order of arrival shows in any output.
//
//   level 0   k_compact_count<ShSel0<true>>   (vc_compact.h) the face byte of every record from the occupancy words, kept per
//                                             record; pick = "the byte is not 0"
//             scan_counts, the count read back, the shell buffers sized
//             k_compact_scatter<ShSel0<false>>  record and face byte of the picked ones, stably
//   level L   k_sh_mark     lane = record: its level-0 face byte, kept per record (it says which records add their colour), and
//                           its coarse cell's bit into the coarse occupancy.  The records are in index order, so a wave's 64
//                           cells mostly share one or two u32 of it: per u32 present in the wave (readfirstlane of the lowest
//                           pending lane's, ballot of its equals) the lanes' bits are ORed over the wave and one lane adds them
//                           with one integer atomicOr that returns nothing.  (One atomic per record and cell took 0.88 ms at
//                           1024^3, as much as everything else of the pass)
//             k_sh_cshell   lane = coarse word: the bits whose face byte is not 0 (the shell word); the ON cells counted
//             k_cc_wcount, scan_counts, k_cc_woff (vc_components.h) over the shell words: the cells of the list before each word
//             k_sh_emit     lane = shell word: {j, 0, 0, 0, 0} and the face byte of each of its bits, in ascending bit
//             k_sh_accum    lane = record of the level-0 shell with seen & 1: r, g, b, 1 into the accumulator of its cell's rank
//                           in the list (woff[j >> 6] + popc(shell word below j & 63)), four integer atomicAdd
//             k_sh_final    lane = shell cell: the rounded means and seen = 1 where the count is not 0
//   both      k_sh_fcount   the shell cells per face bit: per lane, wave, workgroup, then six atomics per workgroup
//   viewer    k_sh_viewer   lane = shell cell: three floats from the per-axis tables, three from the colour table (host-made in
//                           float64, so that the floats are the contract's bit for bit)
// A face byte comes from six bits of an occupancy read as u32 at j +- 1, j +- ny, j +- nx ny; a row's ends, a layer's and the
// grid's are exposed without a read, so nothing wraps and no index leaves the words.  Every word index is checked against the
// word count, every list position against the list's length before it indexes.
#pragma once
#include "vc_measure.h"          // MsDiv, ms_div (vc_components.h: k_cc_wcount, k_cc_woff; vc_compact.h)

namespace vc {

constexpr uint32_t kShBlock = 256;
constexpr uint32_t kShCountBlocks = 512;                     // workgroups of k_sh_fcount at most
constexpr uint32_t kShCounters = 7;                          // u64: six face counts, then the ON cells of the coarse grid

// A grid of bits: the fine occupancy or the coarse one.
struct ShGrid {
    const uint32_t *words32;    // the occupancy as nw32 u32
    uint64_t nw32;
    uint32_t nx, ny, nz, ncol;  // ncol = nx ny
    MsDiv by_ncol, by_ny;
};

__device__ __forceinline__ uint32_t sh_bit(const ShGrid &g, uint32_t j)
{
    const uint32_t w = j >> 5;
    return w < g.nw32 ? (g.words32[w] >> (j & 31u)) & 1u : 0u;
}

__device__ __forceinline__ void sh_cell(const ShGrid &g, uint32_t j, uint32_t &ix, uint32_t &iy, uint32_t &iz)
{
    iz = ms_div(j, g.by_ncol);
    const uint32_t col = j - iz * g.ncol;
    ix = ms_div(col, g.by_ny);
    iy = col - ix * g.ny;
}

// bit f: the neighbour towards -x, +x, -y, +y, -z, +z is OFF or outside the grid
__device__ __forceinline__ uint32_t sh_faces_at(const ShGrid &g, uint32_t j, uint32_t ix, uint32_t iy, uint32_t iz)
{
    uint32_t f = 0;
    if (ix == 0 || !sh_bit(g, j - g.ny)) f |= 1u;
    if (ix + 1 >= g.nx || !sh_bit(g, j + g.ny)) f |= 2u;
    if (iy == 0 || !sh_bit(g, j - 1u)) f |= 4u;
    if (iy + 1 >= g.ny || !sh_bit(g, j + 1u)) f |= 8u;
    if (iz == 0 || !sh_bit(g, j - g.ncol)) f |= 16u;
    if (iz + 1 >= g.nz || !sh_bit(g, j + g.ncol)) f |= 32u;
    return f;
}

__device__ __forceinline__ uint32_t sh_faces(const ShGrid &g, uint32_t j)
{
    uint32_t ix, iy, iz;
    sh_cell(g, j, ix, iy, iz);
    return sh_faces_at(g, j, ix, iy, iz);
}

// The coarse grid of a level: its dimensions and the shift.
struct ShLevel { uint32_t L, nx, ny; };

__device__ __forceinline__ uint32_t sh_coarse(const ShGrid &fine, const ShLevel &c, uint32_t i)
{
    uint32_t ix, iy, iz;
    sh_cell(fine, i, ix, iy, iz);
    return ((iz >> c.L) * c.nx + (ix >> c.L)) * c.ny + (iy >> c.L);
}

// Selector of the level-0 shell (vc_compact.h).  FIRST: the count kernel computes the face bytes and leaves them in fb[S]; the
// scatter kernel reads them there.
template <bool FIRST>
struct ShSel0 {
    ShGrid g;
    const uint64_t *records;    // [S]
    uint8_t *fb;                // [S]
    uint64_t *out;              // [T] (scatter)
    uint8_t *faces;             // [T] (scatter)
    uint64_t T;
    __device__ bool pick(uint64_t s) const
    {
        if (!FIRST) return fb[s] != 0;
        const uint32_t f = sh_faces(g, (uint32_t)records[s]);
        fb[s] = (uint8_t)f;
        return f != 0;
    }
    __device__ void drop(uint64_t) const {}
    __device__ void put(uint64_t s, uint64_t d) const
    {
        if (d >= T) return;
        out[d] = records[s];
        faces[d] = fb[s];
    }
};

__global__ __launch_bounds__(kShBlock) void k_sh_mark(const uint64_t *__restrict__ records, uint64_t S, const ShGrid fine, const ShLevel c,
                                                      uint8_t *__restrict__ fb, uint32_t *__restrict__ cwords32, uint64_t cnw32)
{
    const uint64_t s = (uint64_t)blockIdx.x * kShBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t w = 0xffffffffu, bit = 0;
    if (s < S) {
        const uint32_t i = (uint32_t)records[s];
        uint32_t ix, iy, iz;
        sh_cell(fine, i, ix, iy, iz);
        fb[s] = (uint8_t)sh_faces_at(fine, i, ix, iy, iz);
        const uint32_t j = ((iz >> c.L) * c.nx + (ix >> c.L)) * c.ny + (iy >> c.L);
        if ((j >> 5) < cnw32) { w = j >> 5; bit = 1u << (j & 31u); }
    }
    // per coarse word present in the wave, one atomic of the lanes' bits ORed together (whole waves: every lane takes part in
    // the moves)
    unsigned long long pending = __ballot(w != 0xffffffffu);
    while (pending) {                                            // (uniform over the wave)
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(__ffsll((long long)pending) - 1));
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)first);
        const bool mine = w == k;
        pending &= ~__ballot(mine);
        uint32_t bits = mine ? bit : 0u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, d);
        if (lane == first) atomicOr(cwords32 + k, bits);
    }
}

__global__ __launch_bounds__(kShBlock) void k_sh_cshell(const ShGrid cg, const uint64_t *__restrict__ cwords, uint64_t nwc,
                                                        uint64_t *__restrict__ shw, unsigned long long *__restrict__ on)
{
    __shared__ uint32_t s_on;
    if (threadIdx.x == 0) s_on = 0;
    __syncthreads();
    const uint64_t w = (uint64_t)blockIdx.x * kShBlock + threadIdx.x;
    const uint64_t bits = w < nwc ? cwords[w] : 0ull;
    uint64_t shell = 0;
    for (uint64_t m = bits; m; m &= m - 1ull) {
        const uint32_t b = (uint32_t)__ffsll((long long)m) - 1u;
        if (sh_faces(cg, (uint32_t)(w * 64 + b))) shell |= 1ull << b;
    }
    if (w < nwc) shw[w] = shell;
    const uint32_t n = wave_sum_u32((uint32_t)__popcll(bits));
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&s_on, n);
    __syncthreads();
    if (threadIdx.x == 0 && s_on) atomicAdd(on, (unsigned long long)s_on);
}

__global__ __launch_bounds__(kShBlock) void k_sh_emit(const ShGrid cg, const uint64_t *__restrict__ shw, uint64_t nwc,
                                                      const uint32_t *__restrict__ woff, uint64_t *__restrict__ out,
                                                      uint8_t *__restrict__ faces, uint64_t T)
{
    const uint64_t w = (uint64_t)blockIdx.x * kShBlock + threadIdx.x;
    if (w >= nwc) return;
    uint64_t m = shw[w];
    if (!m) return;
    for (uint64_t d = woff[w]; m && d < T; m &= m - 1ull, ++d) {
        const uint32_t j = (uint32_t)(w * 64 + ((uint32_t)__ffsll((long long)m) - 1u));
        out[d] = (uint64_t)j;
        faces[d] = (uint8_t)sh_faces(cg, j);
    }
}

__global__ __launch_bounds__(kShBlock) void k_sh_accum(const uint64_t *__restrict__ records, const uint8_t *__restrict__ fb, uint64_t S,
                                                       const ShGrid fine, const ShLevel c, const uint64_t *__restrict__ shw, uint64_t nwc,
                                                       const uint32_t *__restrict__ woff, uint32_t *__restrict__ acc, uint64_t T)
{
    const uint64_t s = (uint64_t)blockIdx.x * kShBlock + threadIdx.x;
    if (s >= S || !fb[s]) return;
    const uint64_t rec = records[s];
    if (!((rec >> 56) & 1ull)) return;
    const uint32_t j = sh_coarse(fine, c, (uint32_t)rec);
    const uint64_t w = j >> 6;
    if (w >= nwc) return;
    const uint64_t word = shw[w], bit = 1ull << (j & 63u);
    if (!(word & bit)) return;                                   // (a coarse cell with no exposed face)
    const uint64_t d = (uint64_t)woff[w] + (uint32_t)__popcll(word & (bit - 1ull));
    if (d >= T) return;
    uint32_t *a = acc + 4 * d;
    atomicAdd(a + 0, (uint32_t)(rec >> 32) & 255u);
    atomicAdd(a + 1, (uint32_t)(rec >> 40) & 255u);
    atomicAdd(a + 2, (uint32_t)(rec >> 48) & 255u);
    atomicAdd(a + 3, 1u);
}

__global__ __launch_bounds__(kShBlock) void k_sh_final(const uint32_t *__restrict__ acc, uint64_t *__restrict__ out, uint64_t T)
{
    const uint64_t d = (uint64_t)blockIdx.x * kShBlock + threadIdx.x;
    if (d >= T) return;
    const uint32_t n = acc[4 * d + 3];
    if (!n) return;
    const uint64_t r = (acc[4 * d + 0] + n / 2) / n, g = (acc[4 * d + 1] + n / 2) / n, b = (acc[4 * d + 2] + n / 2) / n;
    out[d] = (out[d] & 0xffffffffull) | r << 32 | g << 40 | b << 48 | 1ull << 56;
}

__global__ __launch_bounds__(kShBlock) void k_sh_fcount(const uint8_t *__restrict__ faces, uint64_t T, unsigned long long *__restrict__ out)
{
    __shared__ uint32_t s_n[6];
    if (threadIdx.x < 6) s_n[threadIdx.x] = 0;
    __syncthreads();
    uint32_t n[6] = {0, 0, 0, 0, 0, 0};
    for (uint64_t d = (uint64_t)blockIdx.x * kShBlock + threadIdx.x; d < T; d += (uint64_t)gridDim.x * kShBlock) {
        const uint32_t f = faces[d];
#pragma unroll
        for (int k = 0; k < 6; ++k) n[k] += (f >> k) & 1u;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t v = wave_sum_u32(n[k]);                   // (a workgroup's share of T stays far below 2^32)
        if ((threadIdx.x & 63u) == 0 && v) atomicAdd(s_n + k, v);
    }
    __syncthreads();
    if (threadIdx.x < 6 && s_n[threadIdx.x]) atomicAdd(out + threadIdx.x, (unsigned long long)s_n[threadIdx.x]);
}

// tab: x[nx] | y[ny] | z[nz] | colour[256]; positions {x, z, y} (the z table holds the negated values), colours {r, g, b}
__global__ __launch_bounds__(kShBlock) void k_sh_viewer(const uint64_t *__restrict__ rec, uint64_t T, const ShGrid cg,
                                                        const float *__restrict__ tab, float *__restrict__ pos, float *__restrict__ col)
{
    const uint64_t d = (uint64_t)blockIdx.x * kShBlock + threadIdx.x;
    if (d >= T) return;
    const uint64_t r = rec[d];
    uint32_t cx, cy, cz;
    sh_cell(cg, (uint32_t)r, cx, cy, cz);
    if (cx >= cg.nx || cy >= cg.ny || cz >= cg.nz) return;       // (no such cell: nothing to index)
    const float *ty = tab + cg.nx, *tz = ty + cg.ny, *tc = tz + cg.nz;
    pos[3 * d + 0] = tab[cx]; pos[3 * d + 1] = tz[cz]; pos[3 * d + 2] = ty[cy];
    col[3 * d + 0] = tc[(r >> 32) & 255u]; col[3 * d + 1] = tc[(r >> 40) & 255u]; col[3 * d + 2] = tc[(r >> 48) & 255u];
}

}  // namespace vc
