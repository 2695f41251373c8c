"""Restatement of vc_hull_geodesic, vc_geodesic_path and vc_paint_geodesic (include/voxcarve.h): geodesic
distances through the hull in whole micrometres, its extremities by repeated farthest-point selection, their regions and the
shortest paths back.  Integers only.  A hull is its ascending list of linear indices idx (i = (iz nx + ix) ny + iy), a voxel is
named by its record r (its position in idx); q = (q_x, q_y, q_z) are the steps in micrometres (distance_np.steps_um).

A key is d << 8 | label; NONE = 2^64 - 1 is the key of an unreached voxel ((d, label) = (2^64 - 1, 255)).  Two forms of the
relaxation, both started from any keys that are lengths of real paths:

  relax_dijkstra   the literal one: a heap of (key, record) in Python integers, one voxel settled at a time
  relax_bellman    vectorised min-plus rounds in numpy: every voxel lowered in a round pushes key + (w << 8) to its neighbours
                   (np.minimum.at), until a round lowers nothing

geodesic() runs the whole contract with either (and warm- or cold-started re-relaxations), path() follows `next`, paint() gives
the bytes of vc_paint_geodesic."""
import heapq
import math

import numpy as np

NONE = np.uint64(0xffffffffffffffff)
INF = np.uint64(1) << np.uint64(62)          # the stand-in for NONE inside the relaxations: INF + (w << 8) does not wrap
MAX_K = 32
UNREACHED_RGB = (255, 0, 255)
TILE = (4, 64, 4)                            # cells per tile of the device's tile route in x, y, z (VC_GEO_TILE_X / _Y / _Z)


def edge_lengths(q):
    """The 7 edge lengths in um, index m - 1 for m = |dx| | |dy| << 1 | |dz| << 2: (isqrt(4 s) + 1) div 2, the Euclidean length
    rounded to the nearest um."""
    out = []
    for m in range(1, 8):
        s = sum((int(q[a]) * ((m >> a) & 1)) ** 2 for a in range(3))
        out.append((math.isqrt(4 * s) + 1) // 2)
    return tuple(out)


def offsets(connectivity, q):
    """[(dx, dy, dz, w)] of the neighbourhood, in ascending order of the neighbour's linear index (dz, then dx, then dy)."""
    if connectivity not in (6, 18, 26):
        raise ValueError("connectivity %r, expected 6, 18 or 26" % (connectivity,))
    l1max = {6: 1, 18: 2, 26: 3}[connectivity]
    w = edge_lengths(q)
    out = []
    for dz in (-1, 0, 1):
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                l1 = abs(dx) + abs(dy) + abs(dz)
                if 1 <= l1 <= l1max:
                    out.append((dx, dy, dz, w[(abs(dx) | abs(dy) << 1 | abs(dz) << 2) - 1]))
    return out


def coords(idx, grid):
    nx, ny, _ = grid
    i = np.asarray(idx, dtype=np.int64)
    return (i // ny) % nx, i % ny, i // (nx * ny)


def neighbours(idx, grid, connectivity, q):
    """nbr int64 [S, n_off]: the record of each neighbour, -1 where there is none; w uint64 [n_off] already shifted by 8."""
    nx, ny, nz = grid
    idx = np.asarray(idx, dtype=np.int64)
    rec = np.full((nz + 2, nx + 2, ny + 2), -1, dtype=np.int64)
    ix, iy, iz = coords(idx, grid)
    rec[iz + 1, ix + 1, iy + 1] = np.arange(idx.size)
    offs = offsets(connectivity, q)
    nbr = np.empty((idx.size, len(offs)), dtype=np.int64)
    for o, (dx, dy, dz, _) in enumerate(offs):
        nbr[:, o] = rec[iz + 1 + dz, ix + 1 + dx, iy + 1 + dy]
    return nbr, np.array([w << 8 for _, _, _, w in offs], dtype=np.uint64)


def relax_dijkstra(keys, nbr, w8, sources):
    """keys (uint64 [S], INF where unreached) lowered in place to the fixpoint; sources = the records whose keys were just set."""
    k = [int(v) for v in keys]
    w = [int(v) for v in w8]
    heap = [(k[int(s)], int(s)) for s in sources]
    heapq.heapify(heap)
    rows = nbr.tolist()
    while heap:
        kv, v = heapq.heappop(heap)
        if kv > k[v]:
            continue
        for o, u in enumerate(rows[v]):
            if u >= 0 and kv + w[o] < k[u]:
                k[u] = kv + w[o]
                heapq.heappush(heap, (k[u], u))
    keys[:] = np.array(k, dtype=np.uint64)
    return keys


def relax_bellman(keys, nbr, w8, sources):
    """The same fixpoint by rounds; returns the number of rounds that lowered something."""
    front = np.unique(np.asarray(sources, dtype=np.int64))
    rounds = 0
    while front.size:
        before = keys.copy()
        for o in range(nbr.shape[1]):
            u = nbr[front, o]
            ok = u >= 0
            np.minimum.at(keys, u[ok], keys[front[ok]] + w8[o])
        front = np.flatnonzero(keys < before)
        rounds += bool(front.size)
    return rounds


RELAX = {"dijkstra": relax_dijkstra, "bellman": relax_bellman}


def seeds_by_layer(idx, grid, mode, layers):
    """The records of the `layers` layers iz_max - layers + 1 .. iz_max ("floor": world up is -z) or iz_min .. iz_min + layers - 1
    ("top") of the survivors' box."""
    _, _, iz = coords(idx, grid)
    if iz.size == 0:
        return np.zeros(0, dtype=np.int64)
    if layers < 1:
        raise ValueError("layers %r" % (layers,))
    if mode == "floor":
        return np.flatnonzero(iz > int(iz.max()) - layers)
    if mode == "top":
        return np.flatnonzero(iz < int(iz.min()) + layers)
    raise ValueError("seed mode %r" % (mode,))


def records_of(idx, voxels):
    """Records of a list of linear indices; ValueError naming the first that is no survivor."""
    idx = np.asarray(idx, dtype=np.int64)
    v = np.asarray(voxels, dtype=np.int64).reshape(-1)
    r = np.searchsorted(idx, v)
    bad = (r >= idx.size) | (idx[np.minimum(r, max(idx.size - 1, 0))] != v) if idx.size else np.ones(v.size, dtype=bool)
    if bad.any():
        raise ValueError("seed %d (voxel %d) is no survivor" % (int(np.flatnonzero(bad)[0]), int(v[np.flatnonzero(bad)[0]])))
    return r


def geodesic(idx, grid, q, connectivity, seed_records, K=0, method="bellman", warm=True, paths=False):
    """The contract, items 1 to 3.  Returns a dict: d uint64 [S] (NONE where unreached), labels uint8 [S] (255 there), keys (the
    packed words, NONE where unreached), extrema: a list of dicts (label, voxel, record, d, ix, iy, iz, and with paths=True path:
    the linear indices from E_k to the nearest source that existed when it was picked) and the stats survivors, seeds, reached,
    unreached, max_d, extremities, edge_um, q."""
    if not 0 <= K <= MAX_K:
        raise ValueError("K = %r not in [0, %d]" % (K, MAX_K))
    idx = np.asarray(idx, dtype=np.int64)
    nbr, w8 = neighbours(idx, grid, connectivity, q)
    relax = RELAX[method]
    keys = np.full(idx.size, INF, dtype=np.uint64)
    srcs = [(int(s), 0) for s in np.unique(np.asarray(seed_records, dtype=np.int64))]
    n_seeds = len(srcs)
    for s, lab in srcs:
        keys[s] = lab
    relax(keys, nbr, w8, [s for s, _ in srcs])
    ix, iy, iz = coords(idx, grid)
    extrema = []
    for k in range(1, K + 1):
        reached = keys < INF
        if not reached.any():
            break
        d = np.where(reached, keys >> np.uint64(8), np.uint64(0))
        r = int(np.argmax(d))                                     # (the first maximum: the lowest record = the lowest index)
        if int(d[r]) == 0:
            break
        extrema.append({"label": k, "voxel": int(idx[r]), "record": r, "d": int(d[r]), "ix": int(ix[r]), "iy": int(iy[r]),
                        "iz": int(iz[r])})
        if paths:                                                 # (before E_k becomes a source: back to the nearest earlier one)
            extrema[-1]["path"] = path(np.where(reached, keys, NONE), nbr, w8, idx, r)
        srcs.append((r, k))
        if warm:
            keys[r] = k
            relax(keys, nbr, w8, [r])
        else:
            keys[:] = INF
            for s, lab in srcs:
                keys[s] = min(int(keys[s]), lab)
            relax(keys, nbr, w8, [s for s, _ in srcs])
    reached = keys < INF
    out_keys = np.where(reached, keys, NONE)
    d = np.where(reached, keys >> np.uint64(8), NONE)
    return {"d": d, "labels": np.where(reached, keys & np.uint64(255), np.uint64(255)).astype(np.uint8), "keys": out_keys,
            "extrema": extrema, "survivors": int(idx.size), "seeds": n_seeds, "reached": int(reached.sum()),
            "unreached": int(idx.size - reached.sum()), "max_d": int(d[reached].max()) if reached.any() else 0,
            "extremities": len(extrema), "edge_um": edge_lengths(q), "q": tuple(int(v) for v in q), "nbr": nbr, "w8": w8}


def path(keys, nbr, w8, idx, record):
    """Item 4: the linear indices from `record` to a voxel with d = 0, following next(v) = the lowest-index neighbour u with
    key(u) + (w << 8) == key(v).  ValueError for an unreached voxel."""
    v = int(record)
    if keys[v] == NONE:
        raise ValueError("record %d is unreached" % v)
    out = [int(idx[v])]
    while int(keys[v]) >> 8:
        nxt = -1
        for o in range(nbr.shape[1]):                             # (offsets ascend in the neighbour's linear index)
            u = int(nbr[v, o])
            if u >= 0 and keys[u] != NONE and int(keys[u]) + int(w8[o]) == int(keys[v]):
                nxt = u
                break
        if nxt < 0:
            raise AssertionError("no next voxel at record %d: the keys are no fixpoint" % v)
        v = nxt
        out.append(int(idx[v]))
    return out


def paint(rgb, keys, mode, palette=None, max_d=0):
    """The bytes vc_paint_geodesic leaves: rgb uint8 [S, 3] by region (mode "labels", palette uint8 [>= regions, 3]) or by the
    grey ramp 255 d div max_d (mode "distance"; 0 when max_d = 0); unreached voxels take UNREACHED_RGB."""
    out = np.array(rgb, dtype=np.uint8, copy=True)
    reached = keys != NONE
    if mode == "labels":
        pal = np.asarray(palette, dtype=np.uint8)
        out[reached] = pal[(keys[reached] & np.uint64(255)).astype(np.int64)]
    elif mode == "distance":
        d = keys[reached] >> np.uint64(8)
        g = (d * np.uint64(255) // np.uint64(max_d)).astype(np.uint8) if max_d else np.zeros(d.size, dtype=np.uint8)
        out[reached] = g[:, None]
    else:
        raise ValueError("mode %r" % (mode,))
    out[~reached] = UNREACHED_RGB
    return out


def occupied_tiles(idx, grid):
    """How many tiles of TILE cells, laid from the low corner of the survivors' index box, hold a survivor."""
    ix, iy, iz = coords(idx, grid)
    if ix.size == 0:
        return 0
    t = np.stack([(ix - ix.min()) // TILE[0], (iy - iy.min()) // TILE[1], (iz - iz.min()) // TILE[2]], axis=1)
    return int(np.unique(t, axis=0).shape[0])
