"""What goes with CarveEngine.thin_hull on the host (vc_hull_thin; contract in include/voxcarve.h): arithmetic over the few
thousand voxels of a skeleton -- their world positions, the edges between them, lengths in millimetres, the branches between end
points and junctions, and the limb's half thickness where the caller has a distance field.

An edge joins two skeleton voxels that are 26-neighbours; its length is the one vc_hull_geodesic gives the same step: with
q = the grid steps rounded to whole um, (isqrt(4 s) + 1) div 2 um for s = (q_x dx)^2 + (q_y dy)^2 + (q_z dz)^2.  A curve
skeleton is one voxel wide, but where three limbs meet the junction voxels are 26-neighbours of each other, so the edges form
small triangles there: length_mm sums every edge and overstates a tree's length by those; the branches do not."""
import math

import numpy as np

from .measure import grid_metric

# the 13 offsets (dx, dy, dz) whose opposite is not in the list
HALF = tuple((dx, dy, dz) for dz in (-1, 0, 1) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dz, dx, dy) > (0, 0, 0))


def steps_um(grid, bounds):
    """q = (q_x, q_y, q_z): the grid steps in whole um, as vc_hull_distance rounds them (0 on an axis of one cell)."""
    _, step = grid_metric(grid, bounds)
    return tuple(int(np.rint(s * 1000.0)) for s in step)


def edge_um(q, off):
    s = sum((int(a) * int(d)) ** 2 for a, d in zip(q, off))
    return (math.isqrt(4 * s) + 1) // 2


def _index(skeleton, grid):
    nx, ny, _ = grid
    if "index" in skeleton:
        return np.asarray(skeleton["index"], dtype=np.int64).reshape(-1, 3)
    i = np.asarray(skeleton["voxel"], dtype=np.int64)
    return np.stack([(i // ny) % nx, i % ny, i // (nx * ny)], axis=1)


def edges_of(skeleton, grid):
    """(edges int64 [E, 2] with a < b in rows of the skeleton, ascending; offsets int64 [E, 3] = index[b] - index[a])."""
    nx, ny, nz = grid
    voxel = np.asarray(skeleton["voxel"], dtype=np.int64)
    at = _index(skeleton, grid)
    pairs, offs = [], []
    for dx, dy, dz in HALF:
        x, y, z = at[:, 0] + dx, at[:, 1] + dy, at[:, 2] + dz
        ok = np.flatnonzero((x >= 0) & (x < nx) & (y >= 0) & (y < ny) & (z >= 0) & (z < nz))
        j = (z[ok] * nx + x[ok]) * ny + y[ok]
        t = np.minimum(np.searchsorted(voxel, j), max(voxel.size - 1, 0))
        hit = voxel[t] == j if voxel.size else np.zeros(0, dtype=bool)
        pairs.append(np.stack([ok[hit], t[hit]], axis=1))
        offs.append(np.tile(np.array([[dx, dy, dz]], dtype=np.int64), (int(hit.sum()), 1)))
    e = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    o = np.concatenate(offs) if offs else np.zeros((0, 3), np.int64)
    order = np.lexsort((e[:, 1], e[:, 0]))
    return e[order].astype(np.int64).reshape(-1, 2), o[order].reshape(-1, 3)


def describe(skeleton, grid, bounds, depth_mm=None):
    """skeleton: the dict of CarveEngine.fetch_skeleton (voxel, record, degree).  Returns a dict: positions_mm float64 [K, 3] (the
    cell centres), edges int64 [E, 2] (rows a < b of 26-adjacent skeleton voxels), edge_mm float64 [E], length_mm (their sum),
    endpoints / junctions (rows of degree 1 / >= 3) and, when depth_mm = CarveEngine.fetch_record_depth() of a current
    hull_distance() is given (float [S], per record of the hull), radius_mm float64 [K]: the depth at each skeleton voxel, the
    limb's half thickness there."""
    lo, step = grid_metric(grid, bounds)
    at = _index(skeleton, grid)
    degree = np.asarray(skeleton["degree"])
    e, off = edges_of(skeleton, grid)
    q = steps_um(grid, bounds)
    by_kind = {}
    mm = np.empty(e.shape[0], dtype=np.float64)
    for k, o in enumerate(np.abs(off).tolist()):
        o = tuple(o)
        if o not in by_kind:
            by_kind[o] = edge_um(q, o) / 1000.0
        mm[k] = by_kind[o]
    out = {"positions_mm": lo + at.astype(np.float64) * step, "edges": e, "edge_mm": mm, "length_mm": float(mm.sum()),
           "endpoints": np.flatnonzero(degree == 1), "junctions": np.flatnonzero(degree >= 3)}
    if depth_mm is not None:
        out["radius_mm"] = np.asarray(depth_mm, dtype=np.float64)[np.asarray(skeleton["record"], dtype=np.int64)]
    return out


def branches(skeleton, grid, bounds):
    """The maximal chains of degree-2 voxels between voxels of any other degree: a list of dicts {rows: int64 [n] (rows of the
    skeleton along the chain, its two ends -- voxels of another degree, where there are any -- included), length_mm}.  The
    chains come in the order of their lowest degree-2 row, each walked from that voxel's lower-row neighbour's side; a ring of
    degree-2 voxels alone starts at its lowest row and comes back to it.  Two voxels of other degrees that touch directly form no
    branch."""
    degree = np.asarray(skeleton["degree"]).astype(np.int64)
    d = describe(skeleton, grid, bounds)
    K = degree.size
    near = [[] for _ in range(K)]
    for (a, b), mm in zip(d["edges"].tolist(), d["edge_mm"].tolist()):
        near[a].append((b, mm))
        near[b].append((a, mm))
    for lst in near:
        lst.sort()
    seen = np.zeros(K, dtype=bool)
    out = []
    for start in np.flatnonzero(degree == 2).tolist():
        if seen[start]:
            continue
        seen[start] = True
        sides = []
        ring = False
        for first, mm in near[start]:                            # walk away from `start` through each of its two neighbours
            rows, length, prev, cur = [], 0.0, start, first
            length += mm
            while True:
                rows.append(cur)
                if cur == start:
                    ring = True
                    break
                if degree[cur] != 2:
                    break
                seen[cur] = True
                step = [(n, w) for n, w in near[cur] if n != prev]
                prev, (cur, w) = cur, step[0]
                length += w
            sides.append((rows, length))
            if ring:
                break
        if ring:
            rows, length = sides[0]
            out.append({"rows": np.array([start] + rows, dtype=np.int64), "length_mm": float(length)})
        else:
            (r0, l0), (r1, l1) = sides
            out.append({"rows": np.array(r0[::-1] + [start] + r1, dtype=np.int64), "length_mm": float(l0 + l1)})
    return out
