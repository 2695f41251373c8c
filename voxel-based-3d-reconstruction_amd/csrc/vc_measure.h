// gfx950 kernels of the hull's figures measured per group of records (vc_hull_measure; contract in include/voxcarve.h, DESIGN.md
// section 8 item 18).  Restated in tests/measure_np.py.  Integer atomics only: every value is a sum, a minimum or a maximum over a
// set, so neither the evaluation order nor the order of arrival shows in any output.
//
//   k_ms_init     the G output structs: zeros, lo = 0xffffffff
//   k_ms_all      source VC_MEASURE_ALL: lane = record over the workgroup's stretch of the list, 21 sums and the box in
//                 registers, reduced over the wave and the workgroup once at the end
//   k_ms_groups   lane = record with its label: per label present in the wave (readfirstlane of the lowest pending lane's label,
//                 ballot of its equals) the nine counts are popcounts of ballots, the twelve sums seventeen wave sums of u32 by
//                 data-parallel-primitive moves (the products in 16-bit halves), the box six wave minima / maxima; the wave's
//                 leader adds them to the workgroup's table in LDS
//                 (the first `tab` labels) or, beyond it, straight to the outputs.  A label that fewer than kMsDense lanes of the
//                 wave hold is not worth 23 wave reductions: those lanes add their own record.
//   k_ms_fold     both of them store their table with plain stores, one slot per workgroup; this adds the slots up into the
//                 outputs (with 2 048 workgroups each flushing 27 atomics onto the same two cache lines the call took 0.183 ms
//                 at 512^3 with one group, 0.094 ms this way)
//   k_ms_profile  lane = record: {n, sum ix, sum iy} per (group, layer) present in the wave, held by the wave while the key
//                 stays -- the records are iz-major, so it mostly does -- and added with global atomics when it changes
// (ix, iy, iz) come from the index by two host-made reciprocal multipliers (MsDiv).  The six neighbour bits come from the occupancy
// words (whole: the dead groups of a hierarchical carve are zeroed before the launch) read as u32 at i +- 1, i +- ny, i +- nx ny;
// a wave's 64 records mostly share them.  Every word index is checked against the word count, every label against G before it
// indexes, every layer against nz.
#pragma once
#include "vc_components.h"       // (vc_kernels.h: wave_min_u32, wave_max_u32)

namespace vc {

constexpr uint32_t kMsBlock = 256;
constexpr uint32_t kMsMaxBlocks = 2048;
constexpr uint32_t kMsStride = 24;                           // u64 per vc_measure_t: 21 sums, then lo[3] hi[3] as six u32
constexpr uint32_t kMsSums = 21;
constexpr uint32_t kMsTable = 320;                           // labels of the LDS table: 60 KB of the 64 KB a launch gets without opting in
constexpr uint32_t kMsDense = 8;                             // lanes of a wave that share a label before the wave reduces for it
constexpr uint64_t kMsPartBytes = 32ull << 20;               // of the workgroups' tables (host: fewer workgroups when a table is large)
constexpr uint32_t kMsFoldSlices = 16;                       // threads of k_ms_fold per cell of the table
constexpr uint32_t kMsNone = 0xffffffffu;
enum { kMsVoxels = 0, kMsSurface = 1, kMsSeen = 2, kMsS1 = 3, kMsS2 = 6, kMsFaces = 12, kMsRgb = 18 };
static_assert(kMsTable * kMsStride * 8 + 1024 <= 65536, "the table and the rest of the workgroup's LDS fit 64 KB");

// n / d for every u32 n by one 64 x 32 multiplication: m = floor((2^64 - 1) / d) + 1, n / d = (m n) >> 64 (exact for d >= 2;
// d = 1 wraps m to 0, which stands for it)
struct MsDiv { unsigned long long m; uint32_t d; };
__device__ __forceinline__ uint32_t ms_div(uint32_t n, const MsDiv &q) { return q.m ? (uint32_t)__umul64hi(q.m, (unsigned long long)n) : n; }

struct MsParams {
    const uint64_t *records;    // [S]
    const uint32_t *words32;    // the occupancy as 2 nwords u32
    const void *labels;         // u8 [S] (clusters), u64 [S] with the label in the low byte (geodesic keys), u32 [S] (host)
    unsigned long long *out;    // [G][kMsStride], made by k_ms_init
    unsigned long long *part;   // [workgroups][tab][kMsStride]: each workgroup's table as it ends (k_ms_fold adds them up)
    unsigned long long *prof;   // [G][nz][3], zeroed (k_ms_profile)
    uint64_t S, per, nw32;      // records, records per workgroup (a multiple of kMsBlock), u32 words of the occupancy
    uint32_t nx, ny, nz, ncol, G, tab;
    MsDiv by_ncol, by_ny;
};

enum { kMsLabelsNone = 0, kMsLabelsU8 = 1, kMsLabelsKey = 2, kMsLabelsU32 = 3 };

template <int KIND>
__device__ __forceinline__ uint32_t ms_label(const MsParams &p, uint64_t s)
{
    uint32_t v = 0;
    if (KIND == kMsLabelsU8) v = static_cast<const uint8_t *>(p.labels)[s];
    if (KIND == kMsLabelsKey) v = (uint32_t)static_cast<const uint64_t *>(p.labels)[s] & 255u;     // (255: unreached)
    if (KIND == kMsLabelsU32) v = static_cast<const uint32_t *>(p.labels)[s];
    return v < p.G ? v : kMsNone;
}

// What a record adds: its cell, its colour if seen, its exposed faces (bit f: -x, +x, -y, +y, -z, +z).
struct MsRec { uint32_t ix, iy, iz, r, g, b, seen, faces; };

__device__ __forceinline__ uint32_t ms_bit(const MsParams &p, uint32_t j)
{
    const uint32_t w = j >> 5;
    return w < p.nw32 ? (p.words32[w] >> (j & 31u)) & 1u : 0u;
}

__device__ __forceinline__ MsRec ms_record(const MsParams &p, uint64_t rec)
{
    MsRec o;
    const uint32_t i = (uint32_t)rec;
    o.iz = ms_div(i, p.by_ncol);
    const uint32_t col = i - o.iz * p.ncol;
    o.ix = ms_div(col, p.by_ny);
    o.iy = col - o.ix * p.ny;
    o.seen = (uint32_t)(rec >> 56) & 1u;
    o.r = o.seen ? (uint32_t)(rec >> 32) & 255u : 0u;
    o.g = o.seen ? (uint32_t)(rec >> 40) & 255u : 0u;
    o.b = o.seen ? (uint32_t)(rec >> 48) & 255u : 0u;
    uint32_t f = 0;
    if (o.ix == 0 || !ms_bit(p, i - p.ny)) f |= 1u;
    if (o.ix + 1 >= p.nx || !ms_bit(p, i + p.ny)) f |= 2u;
    if (o.iy == 0 || !ms_bit(p, i - 1u)) f |= 4u;
    if (o.iy + 1 >= p.ny || !ms_bit(p, i + 1u)) f |= 8u;
    if (o.iz == 0 || !ms_bit(p, i - p.ncol)) f |= 16u;
    if (o.iz + 1 >= p.nz || !ms_bit(p, i + p.ncol)) f |= 32u;
    o.faces = f;
    return o;
}

__device__ __forceinline__ unsigned long long ms_wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// The six products of s2, in the contract's order.
__device__ __forceinline__ void ms_products(const MsRec &o, unsigned long long *q)
{
    const unsigned long long x = o.ix, y = o.iy, z = o.iz;
    q[0] = x * x; q[1] = y * y; q[2] = z * z; q[3] = x * y; q[4] = x * z; q[5] = y * z;
}

__device__ __forceinline__ void ms_add(unsigned long long *d, unsigned long long v) { if (v) atomicAdd(d, v); }
__device__ __forceinline__ void ms_box(unsigned long long *entry, const uint32_t *lo, const uint32_t *hi)
{
    uint32_t *b = reinterpret_cast<uint32_t *>(entry + kMsSums);
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(b + a, lo[a]); atomicMax(b + 3 + a, hi[a]); }
}

// One record of its own lane into an entry (of the LDS table or of the outputs).
__device__ __forceinline__ void ms_add_record(unsigned long long *entry, const MsRec &o)
{
    atomicAdd(entry + kMsVoxels, 1ull);
    if (o.faces) atomicAdd(entry + kMsSurface, 1ull);
    if (o.seen) atomicAdd(entry + kMsSeen, 1ull);
    ms_add(entry + kMsS1 + 0, o.ix); ms_add(entry + kMsS1 + 1, o.iy); ms_add(entry + kMsS1 + 2, o.iz);
    unsigned long long q[6];
    ms_products(o, q);
#pragma unroll
    for (int a = 0; a < 6; ++a) ms_add(entry + kMsS2 + a, q[a]);
#pragma unroll
    for (int f = 0; f < 6; ++f)
        if ((o.faces >> f) & 1u) atomicAdd(entry + kMsFaces + f, 1ull);
    ms_add(entry + kMsRgb + 0, o.r); ms_add(entry + kMsRgb + 1, o.g); ms_add(entry + kMsRgb + 2, o.b);
    const uint32_t c[3] = {o.ix, o.iy, o.iz};
    ms_box(entry, c, c);
}

// A wave's partials of one label into an entry.
__device__ __forceinline__ void ms_add_wave(unsigned long long *entry, const unsigned long long *v, const uint32_t *lo, const uint32_t *hi)
{
#pragma unroll
    for (uint32_t a = 0; a < kMsSums; ++a) ms_add(entry + a, v[a]);
    ms_box(entry, lo, hi);
}

__global__ __launch_bounds__(kMsBlock) void k_ms_init(unsigned long long *__restrict__ out, uint32_t G)
{
    const uint32_t t = blockIdx.x * kMsBlock + threadIdx.x;
    if (t >= G * kMsStride) return;
    const uint32_t f = t % kMsStride;
    // lo[0] lo[1] | lo[2] hi[0] | hi[1] hi[2]
    out[t] = f < kMsSums ? 0ull : f == kMsSums ? 0xffffffffffffffffull : f == kMsSums + 1 ? 0x00000000ffffffffull : 0ull;
}

__global__ __launch_bounds__(kMsBlock) void k_ms_all(const MsParams p)
{
    __shared__ unsigned long long s_acc[kMsStride];
    if (threadIdx.x < kMsStride)
        s_acc[threadIdx.x] = threadIdx.x == kMsSums ? 0xffffffffffffffffull : threadIdx.x == kMsSums + 1 ? 0x00000000ffffffffull : 0ull;
    __syncthreads();
    unsigned long long v[kMsSums];
#pragma unroll
    for (uint32_t a = 0; a < kMsSums; ++a) v[a] = 0;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0, 0, 0};
    const uint64_t begin = (uint64_t)blockIdx.x * p.per, end = min(begin + p.per, p.S);
    for (uint64_t s = begin + threadIdx.x; s < end; s += kMsBlock) {
        const MsRec o = ms_record(p, p.records[s]);
        v[kMsVoxels] += 1; v[kMsSurface] += o.faces ? 1u : 0u; v[kMsSeen] += o.seen;
        v[kMsS1] += o.ix; v[kMsS1 + 1] += o.iy; v[kMsS1 + 2] += o.iz;
        unsigned long long q[6];
        ms_products(o, q);
#pragma unroll
        for (int a = 0; a < 6; ++a) v[kMsS2 + a] += q[a];
#pragma unroll
        for (int f = 0; f < 6; ++f) v[kMsFaces + f] += (o.faces >> f) & 1u;
        v[kMsRgb] += o.r; v[kMsRgb + 1] += o.g; v[kMsRgb + 2] += o.b;
        lo[0] = min(lo[0], o.ix); lo[1] = min(lo[1], o.iy); lo[2] = min(lo[2], o.iz);
        hi[0] = max(hi[0], o.ix); hi[1] = max(hi[1], o.iy); hi[2] = max(hi[2], o.iz);
    }
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t a = 0; a < kMsSums; ++a) {
        v[a] = ms_wave_sum_u64(v[a]);
        if (lane == 0) ms_add(s_acc + a, v[a]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min_u32(lo[a]); hi[a] = wave_max_u32(hi[a]); }
    if (lane == 0 && v[kMsVoxels]) ms_box(s_acc, lo, hi);
    __syncthreads();
    if (threadIdx.x < kMsStride) p.part[(size_t)blockIdx.x * kMsStride + threadIdx.x] = s_acc[threadIdx.x];
}

template <int KIND>
__global__ __launch_bounds__(kMsBlock) void k_ms_groups(const MsParams p)
{
    extern __shared__ unsigned long long s_tab[];           // [tab][kMsStride]
    const uint32_t cells = p.tab * kMsStride;
    for (uint32_t t = threadIdx.x; t < cells; t += kMsBlock) {
        const uint32_t f = t % kMsStride;
        s_tab[t] = f < kMsSums ? 0ull : f == kMsSums ? 0xffffffffffffffffull : f == kMsSums + 1 ? 0x00000000ffffffffull : 0ull;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t begin = (uint64_t)blockIdx.x * p.per, end = min(begin + p.per, p.S);
    for (uint64_t base = begin; base < end; base += kMsBlock) {   // (whole workgroups: every lane is active in the wave sums)
        const uint64_t s = base + threadIdx.x;
        const bool valid = s < end;
        const uint32_t label = valid ? ms_label<KIND>(p, s) : kMsNone;
        MsRec o = {0, 0, 0, 0, 0, 0, 0, 0};
        if (label != kMsNone) o = ms_record(p, p.records[s]);
        unsigned long long pending = __ballot(label != kMsNone);
        bool alone = false;
        while (pending) {                                        // (uniform over the wave)
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(__ffsll((long long)pending) - 1));
            const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)label, (int)first);
            const bool mine = label == k;
            const unsigned long long m = __ballot(mine);
            pending &= ~m;
            if ((uint32_t)__popcll(m) < kMsDense) { alone = alone || mine; continue; }
            unsigned long long v[kMsSums];
            v[kMsVoxels] = (unsigned long long)__popcll(m);
            v[kMsSurface] = (unsigned long long)__popcll(__ballot(mine && o.faces));
            v[kMsSeen] = (unsigned long long)__popcll(__ballot(mine && o.seen));
#pragma unroll
            for (int f = 0; f < 6; ++f) v[kMsFaces + f] = (unsigned long long)__popcll(__ballot(mine && ((o.faces >> f) & 1u)));
            // Sums of u32 by data-parallel-primitive moves (wave_sum_u32: no LDS, the result in a scalar register).  A wave's
            // sums of ix, iy, iz stay below 2^22, those of r, g, b below 2^14 (r and g share a sum); a product is below 2^32, so
            // its two 16-bit halves sum below 2^22 each.
            v[kMsS1] = wave_sum_u32(mine ? o.ix : 0u); v[kMsS1 + 1] = wave_sum_u32(mine ? o.iy : 0u); v[kMsS1 + 2] = wave_sum_u32(mine ? o.iz : 0u);
            const uint32_t rg = wave_sum_u32(mine ? o.r | (o.g << 16) : 0u);
            v[kMsRgb] = rg & 0xffffu; v[kMsRgb + 1] = rg >> 16; v[kMsRgb + 2] = wave_sum_u32(mine ? o.b : 0u);
            unsigned long long q[6];
            ms_products(o, q);
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const uint32_t ql = wave_sum_u32(mine ? (uint32_t)q[a] & 0xffffu : 0u), qh = wave_sum_u32(mine ? (uint32_t)(q[a] >> 16) : 0u);
                v[kMsS2 + a] = (unsigned long long)ql + ((unsigned long long)qh << 16);
            }
            uint32_t lo[3], hi[3];
            lo[0] = wave_min_u32(mine ? o.ix : 0xffffffffu); lo[1] = wave_min_u32(mine ? o.iy : 0xffffffffu); lo[2] = wave_min_u32(mine ? o.iz : 0xffffffffu);
            hi[0] = wave_max_u32(mine ? o.ix : 0u); hi[1] = wave_max_u32(mine ? o.iy : 0u); hi[2] = wave_max_u32(mine ? o.iz : 0u);
            if (lane == first) {                                 // (two calls: each knows its address space)
                if (k < p.tab) ms_add_wave(s_tab + (size_t)k * kMsStride, v, lo, hi);
                else ms_add_wave(p.out + (size_t)k * kMsStride, v, lo, hi);
            }
        }
        if (alone) {
            if (label < p.tab) ms_add_record(s_tab + (size_t)label * kMsStride, o);
            else ms_add_record(p.out + (size_t)label * kMsStride, o);
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < cells; t += kMsBlock) p.part[(size_t)blockIdx.x * cells + t] = s_tab[t];
}

// The workgroups' tables added up into the outputs: thread = one u64 cell of the table and one of kMsFoldSlices slices of the
// workgroups, so that a wave reads 512 contiguous bytes per workgroup; one atomic per thread at the end (kMsFoldSlices on an
// address, where thousands of workgroups flushing their tables themselves queued on the same few cache lines).  An empty entry
// holds zeros and lo = 0xffffffff > hi = 0, which change nothing.
__global__ __launch_bounds__(kMsBlock) void k_ms_fold(const unsigned long long *__restrict__ part, uint32_t workgroups, uint32_t cells,
                                                     unsigned long long *__restrict__ out)
{
    const uint32_t id = blockIdx.x * kMsBlock + threadIdx.x;
    const uint32_t slice = id / cells, t = id - slice * cells;
    if (slice >= kMsFoldSlices) return;
    const uint32_t f = t % kMsStride;
    unsigned long long sum = 0;
    uint32_t a = f == kMsSums + 2 ? 0u : 0xffffffffu, b = f == kMsSums ? 0xffffffffu : 0u;     // the two u32 of a box cell
    for (uint32_t w = slice; w < workgroups; w += kMsFoldSlices) {
        const unsigned long long v = part[(size_t)w * cells + t];
        const uint32_t va = (uint32_t)v, vb = (uint32_t)(v >> 32);
        sum += v;
        a = f == kMsSums + 2 ? max(a, va) : min(a, va);          // lo[0] lo[1] | lo[2] hi[0] | hi[1] hi[2]
        b = f == kMsSums ? min(b, vb) : max(b, vb);
    }
    if (f < kMsSums) { ms_add(out + t, sum); return; }
    uint32_t *o = reinterpret_cast<uint32_t *>(out + t);
    if (f == kMsSums + 2) atomicMax(o, a); else atomicMin(o, a);
    if (f == kMsSums) atomicMin(o + 1, b); else atomicMax(o + 1, b);
}

__device__ __forceinline__ void ms_profile_flush(const MsParams &p, uint32_t key, unsigned long long n, unsigned long long sx, unsigned long long sy)
{
    if (key == kMsNone) return;
    unsigned long long *e = p.prof + (size_t)key * 3;
    ms_add(e, n); ms_add(e + 1, sx); ms_add(e + 2, sy);
}

template <int KIND>
__global__ __launch_bounds__(kMsBlock) void k_ms_profile(const MsParams p)
{
    const uint32_t lane = threadIdx.x & 63u;
    // the wave holds the sums of one (group, layer) over its iterations and adds them when another comes: the records are
    // iz-major, so the waves of a moment would otherwise all queue on the three addresses of one layer
    uint32_t held = kMsNone;
    unsigned long long hn = 0, hx = 0, hy = 0;
    const uint64_t begin = (uint64_t)blockIdx.x * p.per, end = min(begin + p.per, p.S);
    for (uint64_t base = begin; base < end; base += kMsBlock) {
        const uint64_t s = base + threadIdx.x;
        uint32_t label = s < end ? ms_label<KIND>(p, s) : kMsNone;
        uint32_t ix = 0, iy = 0, iz = 0;
        if (label != kMsNone) {
            const uint32_t i = (uint32_t)p.records[s];
            iz = ms_div(i, p.by_ncol);
            const uint32_t col = i - iz * p.ncol;
            ix = ms_div(col, p.by_ny);
            iy = col - ix * p.ny;
            if (iz >= p.nz) label = kMsNone;                     // (no such record: nothing to index)
        }
        const uint32_t key = label != kMsNone ? label * p.nz + iz : kMsNone;     // (G nz <= 2^20)
        unsigned long long pending = __ballot(key != kMsNone);
        while (pending) {
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(__ffsll((long long)pending) - 1));
            const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)first);
            const bool mine = key == k;
            const unsigned long long m = __ballot(mine);
            pending &= ~m;
            const unsigned long long xy = ms_wave_sum_u64(mine ? (unsigned long long)ix | ((unsigned long long)iy << 32) : 0ull);
            if (k != held) {                                     // (uniform over the wave)
                if (lane == 0) ms_profile_flush(p, held, hn, hx, hy);
                held = k; hn = hx = hy = 0;
            }
            hn += (unsigned long long)__popcll(m); hx += xy & 0xffffffffull; hy += xy >> 32;
        }
    }
    if (lane == 0) ms_profile_flush(p, held, hn, hx, hy);
}

}  // namespace vc
