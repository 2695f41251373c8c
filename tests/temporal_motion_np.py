"""The contract of vc_hull_temporal_motion (include/voxcarve.h) restated in numpy: the ring and P of
vc_hull_temporal, but before a call counts, every older snapshot and P are aligned to the current hull by the block motion field
between the ring's newest snapshot and the current hull.  The ring keeps the aligned snapshots.  Integers only.

  align        X'(v) = X(v - d_k) for v in listed block k, X'(v) = X(v) in an unlisted block; sources off the grid are empty
  AlignedVote  the state the device keeps (ring, P, window, the last field) and one call on whole volumes
  Literal      the same voxel by voxel and displacement by displacement (motion_np.match_literal), for the smallest grids

A hull is a boolean volume occ[iz, ix, iy] as in motion_np; grid = (nx, ny, nz).  Records go through temporal_np.records_after."""
import numpy as np

import motion_np as mo
import temporal_np as tn

MOTION_STATS = ("blocks", "listed", "moved", "unique", "clipped", "cost0_sum", "cost_sum")


def grid_of(hull):
    nz, nx, ny = np.asarray(hull).shape
    return (nx, ny, nz)


def no_rows(grid, b, s):
    """The rows of a call without a field (the first push after a reset)."""
    return mo._rows(grid, b, s, [], [], [], [], [], [], [])


def align(rows, vol, grid, b):
    """vol moved block by block: listed block k gathers from v - d_k (empty off the grid), every other block stays as it is."""
    vol = np.asarray(vol, dtype=bool)
    nx, ny, nz = grid
    out = vol.copy()
    for (bx, by, bz), (dx, dy, dz) in zip(np.asarray(rows["ijk"], dtype=np.int64).reshape(-1, 3), np.asarray(rows["d"], dtype=np.int64).reshape(-1, 3)):
        if not (dx or dy or dz):
            continue
        z, x, y = np.meshgrid(np.arange(bz * b, min(bz * b + b, nz)), np.arange(bx * b, min(bx * b + b, nx)),
                              np.arange(by * b, min(by * b + b, ny)), indexing="ij")
        sz, sx, sy = z - dz, x - dx, y - dy
        ok = (sz >= 0) & (sz < nz) & (sx >= 0) & (sx < nx) & (sy >= 0) & (sy < ny)
        blk = np.zeros(z.shape, dtype=bool)
        blk[ok] = vol[sz[ok], sx[ok], sy[ok]]
        out[z, x, y] = blk
    return out


def field_stats(rows, grid, b, have):
    nb = mo.block_dims(grid, b)
    if not have:
        return dict({k: 0 for k in MOTION_STATS}, blocks=int(nb[0] * nb[1] * nb[2]))
    st = mo.stats(rows, np.zeros(1), np.zeros(1), grid, b)
    return {k: st[k] for k in MOTION_STATS}


class AlignedVote:
    """Ring (aligned snapshots, newest last and raw), P and the rows of the last call."""

    match = staticmethod(mo.match)

    def __init__(self):
        self.reset()

    def reset(self):
        self.window = 0
        self.ring = []
        self.prev = None
        self.rows = None

    def history(self, age):
        if not 0 <= age < len(self.ring):
            raise IndexError(age)
        return self.ring[len(self.ring) - 1 - age]

    def push(self, hull, window, keep_on, keep_off, b, ap, s):
        """-> (O_t, counts u8, stats); a `window` or a grid other than the ring's starts over."""
        hull = np.asarray(hull, dtype=bool)
        tn.thresholds(window, keep_on, keep_off, 1)
        grid = grid_of(hull)
        if window != self.window or (self.ring and self.ring[-1].shape != hull.shape):
            self.reset()
            self.window = window
        have = len(self.ring)
        rows = self.match(hull, self.ring[-1], grid, b, ap, s) if have else no_rows(grid, b, s)
        keep = min(have, window - 1)
        aligned = [align(rows, h, grid, b) for h in self.ring[have - keep:]] if keep else []
        prev = np.zeros(hull.shape, dtype=bool) if self.prev is None else align(rows, self.prev, grid, b)
        ring = aligned + [hull.copy()]
        m = len(ring)
        on, off = tn.thresholds(window, keep_on, keep_off, m)
        c = np.zeros(hull.shape, dtype=np.uint8)
        for h in ring:
            c += h
        out = (c >= on) | (prev & (c >= off))
        stats = {"window": window, "frames": m, "on": on, "off": off, "block": b, "apron": ap, "search": s,
                 "survivors_before": int(hull.sum()), "survivors_after": int(out.sum()),
                 "added": int((out & ~hull).sum()), "removed": int((hull & ~out).sum()),
                 "raw_changed": 0 if m == 1 else int((hull ^ self.ring[-1]).sum()),
                 "aligned_changed": 0 if m == 1 else int((hull ^ ring[-2]).sum()), "out_changed": int((out ^ prev).sum())}
        stats.update(field_stats(rows, grid, b, have))
        self.ring, self.prev, self.rows = ring, out, rows
        return out, c, stats


class Literal:
    """The definition, voxel by voxel: volumes are kept as boolean arrays but every cell is visited by a Python loop."""

    def __init__(self, window):
        self.window = window
        self.ring = []
        self.prev = None

    @staticmethod
    def _aligned(rows, vol, grid, b):
        nx, ny, nz = grid
        nbx, nby, _ = mo.block_dims(grid, b)
        d_of = {int(k): tuple(int(v) for v in d) for k, d in zip(rows["block"], np.asarray(rows["d"]).reshape(-1, 3))}
        out = np.zeros_like(vol)
        for iz in range(nz):
            for ix in range(nx):
                for iy in range(ny):
                    dx, dy, dz = d_of.get(((iz // b) * nbx + ix // b) * nby + iy // b, (0, 0, 0))
                    sx, sy, sz = ix - dx, iy - dy, iz - dz
                    if 0 <= sx < nx and 0 <= sy < ny and 0 <= sz < nz:
                        out[iz, ix, iy] = vol[sz, sx, sy]
        return out

    def push(self, hull, keep_on, keep_off, b, ap, s):
        hull = np.asarray(hull, dtype=bool)
        grid = grid_of(hull)
        have = len(self.ring)
        rows = mo.match_literal(hull, self.ring[-1], grid, b, ap, s) if have else no_rows(grid, b, s)
        keep = min(have, self.window - 1)
        raw_prev = self.ring[-1] if have else None
        ring = [self._aligned(rows, h, grid, b) for h in self.ring[have - keep:]] + [hull.copy()]
        prev = np.zeros(hull.shape, dtype=bool) if self.prev is None else self._aligned(rows, self.prev, grid, b)
        m = len(ring)
        on, off = tn.thresholds(self.window, keep_on, keep_off, m)
        out, counts = np.zeros(hull.shape, dtype=bool), np.zeros(hull.shape, dtype=np.uint8)
        for v in np.ndindex(hull.shape):
            c = 0
            for h in ring:
                if h[v]:
                    c += 1
            counts[v] = c
            out[v] = c >= on or (bool(prev[v]) and c >= off)
        stats = {"frames": m, "on": on, "off": off,
                 "raw_changed": 0 if m == 1 else sum(1 for v in np.ndindex(hull.shape) if hull[v] != raw_prev[v]),
                 "aligned_changed": 0 if m == 1 else sum(1 for v in np.ndindex(hull.shape) if hull[v] != ring[-2][v]),
                 "out_changed": sum(1 for v in np.ndindex(hull.shape) if out[v] != prev[v])}
        stats.update(field_stats(rows, grid, b, have))
        self.ring, self.prev, self.rows = ring, out, rows
        return out, counts, stats


def moving_boxes(grid, seed, frames, s, bodies=1, flips=0.02):
    """`frames` hulls: `bodies` random boxes, each moved by its own constant vector within the search range per frame, with a
    share `flips` of all cells flipped in every frame."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = grid
    parts = []
    for _ in range(bodies):
        body = np.zeros((nz, nx, ny), dtype=bool)
        lo = [int(rng.integers(0, max(1, n // 3))) for n in (nz, nx, ny)]
        hi = [int(min(n, l + rng.integers(max(1, n // 3), max(2, n // 2 + 2)))) for n, l in zip((nz, nx, ny), lo)]
        body[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        parts.append((body, tuple(int(v) for v in rng.integers(-s, s + 1, 3))))
    out = []
    for t in range(frames):
        h = np.zeros((nz, nx, ny), dtype=bool)
        for body, step in parts:
            h |= mo.shifted(body, tuple(t * v for v in step))
        out.append(h ^ (rng.random(h.shape) < flips))
    return out


def ellipsoid_scene(t, centre, step, rng, grid=(40, 40, 40), semi=(7, 5, 9)):
    """(clean, noisy) hull of frame t: the ellipsoid at centre + t step; 10 % of its voxels dropped, 0.3 % of all cells set."""
    clean = mo.ellipsoid(grid, tuple(c + t * d for c, d in zip(centre, step)), semi)
    drop = rng.random(clean.shape) < 0.10
    speck = rng.random(clean.shape) < 0.003
    return clean, (clean & ~drop) | speck
