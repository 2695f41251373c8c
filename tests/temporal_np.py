"""The contract of vc_hull_temporal (include/voxcarve.h) restated in numpy: a ring of the last `window` hulls, the count of each voxel
over it, thresholds that scale with the ring while it fills, a vote with hysteresis against the previous output.  Integers only.

  Literal        the definition with Python loops over frames and voxels (small grids)
  Vote           the same state machine on whole boolean volumes
  records_after  the 8-byte records, vote bytes and `added` bytes the device leaves

A hull is a boolean volume of any shape; the device's order is the volume's C order (dn.volume / dn.indices: [nz, nx, ny])."""
import numpy as np

MAX_WINDOW = 15


def thresholds(window, keep_on, keep_off, m):
    """(on, off) of a call that sees m hulls: ceil(keep m / window) in integers."""
    if not 1 <= keep_off <= keep_on <= window <= MAX_WINDOW:
        raise ValueError("window %r, keep_on %r, keep_off %r: expected 1 <= keep_off <= keep_on <= window <= %d" % (window, keep_on, keep_off, MAX_WINDOW))
    assert 1 <= m <= window
    return (keep_on * m + window - 1) // window, (keep_off * m + window - 1) // window


class Literal:
    """The definition, voxel by voxel: hulls are kept as flat lists of bools, newest last."""

    def __init__(self, window):
        self.window = window
        self.hulls = []
        self.prev = None

    def push(self, hull, keep_on, keep_off):
        cells = [bool(v) for v in np.asarray(hull).reshape(-1)]
        self.hulls = (self.hulls + [cells])[-self.window:]
        m = len(self.hulls)
        on, off = thresholds(self.window, keep_on, keep_off, m)
        out, counts = [], []
        for v in range(len(cells)):
            c = 0
            for j in range(m):
                if self.hulls[m - 1 - j][v]:
                    c += 1
            was = self.prev is not None and self.prev[v]
            out.append(c >= on or (was and c >= off))
            counts.append(c)
        raw_changed = 0 if m == 1 else sum(1 for a, b in zip(self.hulls[-1], self.hulls[-2]) if a != b)
        out_changed = sum(1 for v in range(len(cells)) if out[v] != (self.prev is not None and self.prev[v]))
        self.prev = out
        shape = np.asarray(hull).shape
        return np.array(out, dtype=bool).reshape(shape), np.array(counts, dtype=np.uint8).reshape(shape), \
            {"frames": m, "on": on, "off": off, "raw_changed": raw_changed, "out_changed": out_changed}


class Vote:
    """The state the device keeps (ring, P, window) and one call of vc_hull_temporal on whole volumes."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.window = 0
        self.ring = []          # newest last, at most `window`
        self.prev = None

    def history(self, age):
        """The raw hull pushed `age` calls ago; IndexError for an age the ring does not hold."""
        if not 0 <= age < len(self.ring):
            raise IndexError(age)
        return self.ring[len(self.ring) - 1 - age]

    def push(self, hull, window, keep_on, keep_off):
        """-> (O_t, counts u8, stats); a `window` other than the ring's starts over."""
        hull = np.asarray(hull, dtype=bool)
        thresholds(window, keep_on, keep_off, 1)
        if window != self.window or (self.ring and self.ring[-1].shape != hull.shape):
            self.reset()
            self.window = window
        ring = (self.ring + [hull.copy()])[-window:]
        m = len(ring)
        on, off = thresholds(window, keep_on, keep_off, m)
        c = np.zeros(hull.shape, dtype=np.uint8)
        for h in ring:
            c += h
        prev = np.zeros(hull.shape, dtype=bool) if self.prev is None else self.prev
        out = (c >= on) | (prev & (c >= off))
        stats = {"window": window, "frames": m, "on": on, "off": off, "survivors_before": int(hull.sum()), "survivors_after": int(out.sum()),
                 "added": int((out & ~hull).sum()), "removed": int((hull & ~out).sum()),
                 "raw_changed": 0 if m == 1 else int((ring[-1] ^ ring[-2]).sum()), "out_changed": int((out ^ prev).sum())}
        self.ring, self.prev = ring, out
        return out, c, stats


def plain_vote(hulls, k):
    """{ v : v is in at least k of hulls }."""
    return np.sum(np.stack([np.asarray(h, dtype=bool) for h in hulls]).astype(np.int64), axis=0) >= k


def records_after(records, hull, out, counts, grid, bounds, cam=None, frame=None, H=None, W=None):
    """(records, votes, added) of O_t = out: the records of hull & out byte for byte, a fresh record for every voxel of out & ~hull
    as closing_np.records_after colours one, the records of hull & ~out dropped; votes = counts at each record."""
    import closing_np as cl
    records = np.asarray(records, dtype=np.uint64)
    flat_out = np.asarray(out, dtype=bool).reshape(-1)
    old_idx = (records & np.uint64(0xffffffff)).astype(np.int64)
    assert np.array_equal(old_idx, np.flatnonzero(np.asarray(hull).reshape(-1))), "the records are the hull's"
    kept = records[flat_out[old_idx]]
    got, added = cl.records_after(kept, out, grid, bounds, cam, frame, H, W)
    votes = np.asarray(counts, dtype=np.uint8).reshape(-1)[(got & np.uint64(0xffffffff)).astype(np.int64)]
    return got, votes, added


def noisy_masks(masks, t, p=0.02):
    """The masks of frame t with a share p of each mask's pixels flipped, seeded by the frame number: cameras in order from one
    generator."""
    rng = np.random.default_rng(7000 + t)
    return [np.where(rng.random(m.shape) < p, 255 - m, m).astype(np.uint8) for m in masks]
