// gfx950 kernel of the motion-compensated vote over the last hulls (vc_hull_temporal_motion; contract in include/voxcarve.h and
// DESIGN.md section 8 item 25).  The ring, P and the count planes are vc_temporal.h's, the field is vc_motion.h's (k_motion_list,
// k_motion_rank, k_motion_match between the current words and the ring's newest snapshot).  Integers and bits only; restated in
// tests/temporal_motion_np.py.
//
//   k_temporal_align_vote   lane = occupancy word of the output.  The word's y-segments are walked by block once: per segment one
//                           decomposition and one vec[k] (an unlisted block has d = 0: its content stays), then the same displaced
//                           row (motion_row) from each of the m - 1 kept snapshots and from P.  The aligned word of every snapshot
//                           goes to the same slot of the second ring, its bits into the count planes; the planes against `on` and
//                           `off` with the aligned P; O to the staging buffer; the six counters as k_temporal_vote sums its five.
//
// The snapshot count is a run-time value of up to 14, so the words being assembled cannot live in a register array indexed by
// it (that would be scratch).  Each lane assembles them in LDS slots of its own, s_acc[snapshot][lane]: 15 x 256 x 8 B = 30 KB,
// a lane reads and writes only its own column, so there is no barrier, and consecutive lanes hold consecutive 8-byte cells, so
// there is no bank conflict beyond the two banks a 64-bit access takes.  The alternative, finishing each snapshot's word by a
// read-modify-write of the lane's own word in the second ring, turns one store per snapshot word into a load and a store per
// segment (up to 16 for b = 4, more on short lines), all of them through L2: the LDS slot costs no memory traffic at all.
// The aligned P is consumed by the lane that gathers it and by nothing after the call (P becomes O), so it is never stored.
// Every word index is checked against nwords before it is used, every block against nblocks; pad words are written as zero.
#pragma once
#include "vc_motion.h"           // MotionGrid, motion_row, motion_byte, kMotionListed; setop_sums, decompose (vc_setops.h); Planes (vc_temporal.h)

namespace vc {

constexpr uint32_t kAlignCounters = 6;                       // |O|, added, removed, raw_changed, out_changed, aligned_changed
constexpr uint32_t kAlignSlots = 15;                         // window - 1 <= 14 snapshots and P

struct TemporalAlignParams {
    const uint64_t *ring;       // [window][npad] snapshots as the last call left them; slot `head` is the newest (raw H_{t-1})
    uint64_t *ring2;            // [window][npad] the aligned snapshots, same slots
    const uint64_t *cur;        // the result's words, H_t
    const uint64_t *prev;       // P, [npad] (null: empty)
    const uint32_t *vec;        // [nblocks] the field (null: no field, nothing is moved)
    uint64_t *stage;            // [npad] O
    unsigned long long *ctr;    // [kAlignCounters], zeroed
    MotionGrid g;
    uint64_t npad;
    uint32_t window, head;
    uint32_t count;             // snapshots to align from `head` backwards: m - 1 <= 14
    uint32_t on, off;
};

__global__ __launch_bounds__(kSetopBlock) void k_temporal_align_vote(const TemporalAlignParams p)
{
    __shared__ uint64_t s_acc[kAlignSlots][kSetopBlock];
    __shared__ uint32_t s_cnt[kSetopBlock / 64][kAlignCounters];
    const uint32_t tid = threadIdx.x;
    const uint64_t w = (uint64_t)blockIdx.x * kSetopBlock + tid;
    const uint32_t count = min(p.count, kAlignSlots - 1u);
    const uint32_t na = count + (p.prev ? 1u : 0u);              // the volumes to gather: slot `count` of s_acc is P's
    uint32_t c[kAlignCounters] = {0, 0, 0, 0, 0, 0};
    if (w < p.g.nwords) {
        const uint64_t valid = tp_valid(w, p.g.n);
        const uint64_t h = p.cur[w] & valid;
        for (uint32_t j = 0; j < na; ++j) s_acc[j][tid] = 0ull;
        if (na) {
            const uint64_t lo = w << 6, hi = min(lo + 64u, p.g.n);
            uint64_t pos = lo;
            while (pos < hi) {
                uint32_t ix, iy, iz;
                decompose((uint32_t)pos, p.g.nx, p.g.ny, ix, iy, iz);
                const uint32_t by = iy / p.g.b;
                const uint32_t yend = min((by + 1u) * p.g.b, p.g.ny);                 // the block's end on this line
                const uint32_t len = (uint32_t)min((uint64_t)(yend - iy), hi - pos);  // 1..16
                const uint32_t k = ((iz / p.g.b) * p.g.nbx + ix / p.g.b) * p.g.nby + by;
                uint32_t v = (p.vec && k < p.g.nblocks) ? p.vec[k] : 0u;
                if (!(v & kMotionListed)) v = 0u;                                     // an unlisted block stays where it is
                const int32_t sx = (int32_t)ix - motion_byte(v, 0), sy = (int32_t)iy - motion_byte(v, 1), sz = (int32_t)iz - motion_byte(v, 2);
                const uint32_t sh = (uint32_t)(pos - lo);
                uint32_t slot = p.head;
                for (uint32_t j = 0; j < count; ++j) {
                    s_acc[j][tid] |= motion_row(p.ring + (uint64_t)slot * p.npad, p.g, sx, sy, sz, len) << sh;
                    slot = slot ? slot - 1u : p.window - 1u;
                }
                if (p.prev) s_acc[count][tid] |= motion_row(p.prev, p.g, sx, sy, sz, len) << sh;
                pos += len;
            }
        }
        Planes<uint64_t> pl = {h, 0ull, 0ull, 0ull};
        uint64_t h1 = 0ull, h1a = 0ull;
        uint32_t slot = p.head;
        for (uint32_t j = 0; j < count; ++j) {
            const uint64_t x = s_acc[j][tid] & valid;
            p.ring2[(uint64_t)slot * p.npad + w] = x;
            tp_add1(pl, x);
            if (j == 0) { h1a = x; h1 = p.ring[(uint64_t)slot * p.npad + w] & valid; }
            slot = slot ? slot - 1u : p.window - 1u;
        }
        const uint64_t prev = p.prev ? s_acc[count][tid] & valid : 0ull;
        const uint64_t o = (tp_ge(pl, p.on) | (prev & tp_ge(pl, p.off))) & valid;
        p.stage[w] = o;
        c[0] = tp_pop(o);
        c[1] = tp_pop(o & ~h);
        c[2] = tp_pop(h & ~o);
        c[3] = count ? tp_pop(h ^ h1) : 0u;
        c[4] = tp_pop(o ^ prev);
        c[5] = count ? tp_pop(h ^ h1a) : 0u;
    } else if (w < p.npad) {                                     // the pad word of every buffer the kernel writes
        uint32_t slot = p.head;
        for (uint32_t j = 0; j < count; ++j) {
            p.ring2[(uint64_t)slot * p.npad + w] = 0ull;
            slot = slot ? slot - 1u : p.window - 1u;
        }
        p.stage[w] = 0ull;
    }
    setop_sums(c, s_cnt, p.ctr);
}

}  // namespace vc
