"""Restatement of vc_hull_components (include/voxcarve.h): the connected components of a survivor list,
their sizes and boxes, the keep rule and the filtered list.  Two forms:

  components(idx, grid, ...)          vectorised union-find over the record list: edges of the negative half-neighbourhood found
                                      by binary search in the sorted list, roots hooked onto the smaller root, pointer jumping.
                                      Memory is proportional to the survivors, never to the grid.
  components_literal(idx, grid, ...)  a breadth-first search from each unvisited survivor in ascending index order over a dense
                                      volume, neighbour by neighbour (small grids).

Both return a dict: labels u32 [S] (the smallest linear index of each record's component), and over the components in
ascending label: label u32 [K], size u32 [K], lo / hi u32 [K, 3] (inclusive, (ix, iy, iz)), kept bool [K]; keep bool [S] per
record, idx the kept records (ascending).  Linear index i = (iz nx + ix) ny + iy."""
import itertools
from collections import deque

import numpy as np

CONNECTIVITIES = (6, 18, 26)


def offsets(connectivity, half=False):
    """(dx, dy, dz) of the neighbourhood (scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3)); half: only those whose
    linear offset is negative (each undirected edge once)."""
    if connectivity not in CONNECTIVITIES:
        raise ValueError("connectivity %r, expected one of %s" % (connectivity, CONNECTIVITIES))
    l1 = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for dz, dx, dy in itertools.product((-1, 0, 1), repeat=3):
        n = abs(dx) + abs(dy) + abs(dz)
        if n == 0 or n > l1:
            continue
        if half and not (dz < 0 or (dz == 0 and (dx < 0 or (dx == 0 and dy < 0)))):
            continue
        out.append((dx, dy, dz))
    return out


def _coords(idx, grid):
    nx, ny, nz = grid
    i = np.asarray(idx, dtype=np.int64)
    iy = i % ny
    t = i // ny
    return t % nx, iy, t // nx


def keep_rule(size, label, min_voxels=0, keep_largest=0):
    """kept per component: size >= min_voxels and, when keep_largest > 0, rank < keep_largest (size descending, label ascending)."""
    size = np.asarray(size, dtype=np.int64)
    kept = size >= int(min_voxels)
    if keep_largest:
        order = np.lexsort((np.asarray(label, dtype=np.int64), -size))
        rank = np.empty(size.size, dtype=np.int64)
        rank[order] = np.arange(size.size)
        kept &= rank < int(keep_largest)
    return kept


def _finish(idx, grid, root, min_voxels, keep_largest):
    """root: record index of each record's component root (its first record)."""
    idx = np.asarray(idx, dtype=np.int64)
    S = idx.size
    roots = np.flatnonzero(root == np.arange(S))
    cid = np.zeros(S, dtype=np.int64)
    cid[roots] = np.arange(roots.size)
    k = cid[root]
    K = roots.size
    size = np.bincount(k, minlength=K)
    ix, iy, iz = _coords(idx, grid)
    lo = np.full((K, 3), np.iinfo(np.int64).max, dtype=np.int64)
    hi = np.zeros((K, 3), dtype=np.int64)
    for a, c in enumerate((ix, iy, iz)):
        np.minimum.at(lo[:, a], k, c)
        np.maximum.at(hi[:, a], k, c)
    label = idx[roots]
    kept = keep_rule(size, label, min_voxels, keep_largest)
    keep = kept[k] if S else np.zeros(0, dtype=bool)
    return {"labels": idx[root].astype(np.uint32), "label": label.astype(np.uint32), "size": size.astype(np.uint32),
            "lo": lo.astype(np.uint32), "hi": hi.astype(np.uint32), "kept": kept, "keep": keep,
            "idx": idx[keep].astype(np.uint32)}


def edges(idx, grid, off):
    """(s, t) record pairs for one neighbour offset (dx, dy, dz): t is the record of voxel s + offset when it survives."""
    nx, ny, nz = grid
    idx = np.asarray(idx, dtype=np.int64)
    dx, dy, dz = off
    ix, iy, iz = _coords(idx, grid)
    jx, jy, jz = ix + dx, iy + dy, iz + dz
    ok = (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny) & (jz >= 0) & (jz < nz)
    s = np.flatnonzero(ok)
    j = (jz[s] * nx + jx[s]) * ny + jy[s]
    t = np.searchsorted(idx, j)
    t = np.minimum(t, max(idx.size - 1, 0))
    hit = idx[t] == j if idx.size else np.zeros(0, dtype=bool)
    return s[hit], t[hit]


def _jump(parent):
    while True:
        pp = parent[parent]
        if np.array_equal(pp, parent):
            return parent
        parent = pp


def components(idx, grid, connectivity=26, min_voxels=0, keep_largest=0):
    """Vectorised form: hook the larger root of every edge onto the smaller, jump pointers, until no edge joins two roots."""
    idx = np.asarray(idx, dtype=np.int64)
    S = idx.size
    parent = np.arange(S, dtype=np.int64)
    pairs = [edges(idx, grid, off) for off in offsets(connectivity, half=True)]
    a = np.concatenate([p[0] for p in pairs]) if pairs else np.zeros(0, np.int64)
    b = np.concatenate([p[1] for p in pairs]) if pairs else np.zeros(0, np.int64)
    while a.size:
        ra, rb = parent[a], parent[b]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        live = lo != hi
        if not live.any():
            break
        a, b, lo, hi = a[live], b[live], lo[live], hi[live]
        np.minimum.at(parent, hi, lo)
        parent = _jump(parent)
    return _finish(idx, grid, parent, min_voxels, keep_largest)


def components_literal(idx, grid, connectivity=26, min_voxels=0, keep_largest=0):
    """Literal form: dense volume, breadth-first search from each unvisited survivor in ascending index order."""
    nx, ny, nz = grid
    idx = np.asarray(idx, dtype=np.int64)
    rank = {int(i): s for s, i in enumerate(idx)}
    nb = offsets(connectivity)
    root = np.full(idx.size, -1, dtype=np.int64)
    for s0, i0 in enumerate(idx):
        if root[s0] >= 0:
            continue
        root[s0] = s0
        todo = deque([int(i0)])
        while todo:
            i = todo.popleft()
            iy, t = i % ny, i // ny
            ix, iz = t % nx, t // nx
            for dx, dy, dz in nb:
                jx, jy, jz = ix + dx, iy + dy, iz + dz
                if not (0 <= jx < nx and 0 <= jy < ny and 0 <= jz < nz):
                    continue
                s = rank.get((jz * nx + jx) * ny + jy)
                if s is not None and root[s] < 0:
                    root[s] = s0
                    todo.append((jz * nx + jx) * ny + jy)
    return _finish(idx, grid, root, min_voxels, keep_largest)
