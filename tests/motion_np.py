"""The contract of vc_hull_motion, vc_hull_warp and vc_paint_motion (include/voxcarve.h) restated in
numpy: block matching between the current hull A and a kept hull B, the prediction of A from B, the colours.  Integers only.

  match_literal    the definition: per listed block and per displacement, the window's cells that differ
  match            the same from shifted XOR volumes and box sums
  stats            the stats of vc_hull_motion from the rows
  warp             P(v) = B(v - d_k) for v in listed block k, and the stats of vc_hull_warp
  paint            the records after vc_paint_motion
  choose           the tie rule on a table of costs
  shifted / random_pair / words / iou   test hulls and their bookkeeping

A hull is a boolean volume occ[iz, ix, iy] (linear index i = (iz nx + ix) ny + iy, the grid's order); grid = (nx, ny, nz); rows are
a dict of arrays over the listed blocks in ascending block index k = (bz NBx + bx) NBy + by: block, ijk (bx, by, bz), d (x, y, z),
cost, cost0, count_a, count_b, ties, flags."""
import numpy as np


def block_dims(grid, b):
    return tuple((int(n) + b - 1) // b for n in grid)


def ellipsoid(grid, centre, semi):
    """occ[iz, ix, iy]: the voxels with ((x - cx) / ax)^2 + ((y - cy) / ay)^2 + ((z - cz) / az)^2 <= 1.0."""
    nx, ny, nz = grid
    z, x, y = np.meshgrid(np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")
    q = ((x - centre[0]) / semi[0]) ** 2 + ((y - centre[1]) / semi[1]) ** 2 + ((z - centre[2]) / semi[2]) ** 2
    return q <= 1.0


def displacements(s):
    """int64 [(2s+1)^3, 3] (dx, dy, dz) in the order of the last tie-break: ascending (dz, dx, dy)."""
    r = np.arange(-s, s + 1)
    dz, dx, dy = np.meshgrid(r, r, r, indexing="ij")
    return np.stack([dx.reshape(-1), dy.reshape(-1), dz.reshape(-1)], axis=1)


def choose(costs, s):
    """(index, ties) for costs [(2s+1)^3] in the order of displacements(s): the smallest cost, then the smallest |d|^2, then the
    smallest (dz, dx, dy); ties = how many displacements attain the smallest cost."""
    costs = np.asarray(costs, dtype=np.int64)
    d = displacements(s)
    d2 = (d * d).sum(axis=1)
    order = np.lexsort((np.arange(costs.size), d2, costs))       # (the last key is the primary one)
    return int(order[0]), int((costs == costs.min()).sum())


def _padded(occ, grid, b, pad):
    """occ[iz, ix, iy] inside a volume of NB b + 2 pad cells per axis, at offset pad: empty outside the grid."""
    nbx, nby, nbz = block_dims(grid, b)
    out = np.zeros((nbz * b + 2 * pad, nbx * b + 2 * pad, nby * b + 2 * pad), dtype=bool)
    nx, ny, nz = grid
    out[pad:pad + nz, pad:pad + nx, pad:pad + ny] = occ
    return out


def _rows(grid, b, s, listed, d, cost, cost0, count_a, count_b, ties):
    nbx, nby, nbz = block_dims(grid, b)
    k = np.asarray(listed, dtype=np.int64)
    d = np.asarray(d, dtype=np.int64).reshape(-1, 3)
    return {"block": k.astype(np.uint32), "ijk": np.stack([(k // nby) % nbx, k % nby, k // (nby * nbx)], axis=1).reshape(-1, 3),
            "d": d.astype(np.int8), "cost": np.asarray(cost, dtype=np.uint32), "cost0": np.asarray(cost0, dtype=np.uint32),
            "count_a": np.asarray(count_a, dtype=np.uint16), "count_b": np.asarray(count_b, dtype=np.uint16),
            "ties": np.asarray(ties, dtype=np.uint16), "flags": (np.abs(d).max(axis=1, initial=0) == s).astype(np.uint8).reshape(-1)}


def match_literal(a, b_occ, grid, b, ap, s):
    """The rows, block by block and displacement by displacement."""
    a, b_occ = np.asarray(a, dtype=bool), np.asarray(b_occ, dtype=bool)
    nbx, nby, nbz = block_dims(grid, b)
    pad = ap + s
    A, B = _padded(a, grid, b, pad), _padded(b_occ, grid, b, pad)
    W = b + 2 * ap
    disp = displacements(s)
    centre = int(np.flatnonzero((disp == 0).all(axis=1))[0])
    out = [[] for _ in range(7)]
    for bz in range(nbz):
        for bx in range(nbx):
            for by in range(nby):
                oz, ox, oy = bz * b + pad, bx * b + pad, by * b + pad
                ca = int(A[oz:oz + b, ox:ox + b, oy:oy + b].sum())
                cb = int(B[oz:oz + b, ox:ox + b, oy:oy + b].sum())
                if ca == 0 and cb == 0:
                    continue
                win = A[oz - ap:oz - ap + W, ox - ap:ox - ap + W, oy - ap:oy - ap + W]
                costs = np.empty(len(disp), dtype=np.int64)
                for j, (dx, dy, dz) in enumerate(disp):
                    z0, x0, y0 = oz - ap - dz, ox - ap - dx, oy - ap - dy          # B(v - d)
                    costs[j] = int((win != B[z0:z0 + W, x0:x0 + W, y0:y0 + W]).sum())
                j, ties = choose(costs, s)
                for lst, v in zip(out, ((bz * nbx + bx) * nby + by, disp[j], costs[j], costs[centre], ca, cb, ties)):
                    lst.append(v)
    return _rows(grid, b, s, *out)


def _box_sums(v, W, b, nb):
    """Sums of v over the windows of W cells that start every b cells, nb of them per axis (v: [nb b + W - b]^3 cells)."""
    v = np.asarray(v, dtype=np.float32)                          # (sums stay below 2^24: exact)
    for axis in (2, 1, 0):
        n = nb[axis]
        m = np.zeros((v.shape[axis], n), dtype=np.float32)       # m[c, j] = 1 where cell c lies in window j
        for j in range(n):
            m[j * b:j * b + W, j] = 1.0
        v = np.moveaxis(np.tensordot(v, m, axes=([axis], [0])), -1, axis)
    return np.rint(v).astype(np.int64)


def match(a, b_occ, grid, b, ap, s):
    """The rows from whole volumes: per displacement the XOR of A with the shifted B, summed over every block's window at once."""
    a, b_occ = np.asarray(a, dtype=bool), np.asarray(b_occ, dtype=bool)
    nbx, nby, nbz = block_dims(grid, b)
    nb = (nbz, nbx, nby)
    pad = ap + s
    A, B = _padded(a, grid, b, pad), _padded(b_occ, grid, b, pad)
    W = b + 2 * ap
    ext = tuple(n * b + 2 * ap for n in nb)                      # the cells any window touches, from -ap on
    Aw = A[s:s + ext[0], s:s + ext[1], s:s + ext[2]]
    disp = displacements(s)
    costs = np.empty((len(disp),) + nb, dtype=np.int64)
    for j, (dx, dy, dz) in enumerate(disp):
        Bs = B[s - dz:s - dz + ext[0], s - dx:s - dx + ext[1], s - dy:s - dy + ext[2]]
        costs[j] = _box_sums((Aw != Bs).astype(np.int32), W, b, nb)
    inner = tuple(slice(pad, pad + n * b) for n in nb)
    ca = _box_sums(A[inner].astype(np.int32), b, b, nb).reshape(-1)
    cb = _box_sums(B[inner].astype(np.int32), b, b, nb).reshape(-1)
    listed = np.flatnonzero((ca > 0) | (cb > 0))
    flat = costs.reshape(len(disp), -1)[:, listed]              # (costs[j][bz, bx, by] flattens to k)
    d2 = (disp * disp).sum(axis=1)
    centre = int(np.flatnonzero((disp == 0).all(axis=1))[0])
    best, ties = [], []
    for col in flat.T:
        order = np.lexsort((np.arange(len(disp)), d2, col))
        best.append(int(order[0]))
        ties.append(int((col == col.min()).sum()))
    best = np.asarray(best, dtype=np.int64)
    return _rows(grid, b, s, listed, disp[best], flat[best, np.arange(listed.size)], flat[centre], ca[listed], cb[listed], ties)


def stats(rows, a, b_occ, grid, b):
    nb = block_dims(grid, b)
    d = np.asarray(rows["d"], dtype=np.int64).reshape(-1, 3)
    return {"blocks": int(nb[0] * nb[1] * nb[2]), "listed": int(len(rows["block"])), "moved": int((d != 0).any(axis=1).sum()),
            "unique": int((np.asarray(rows["ties"]) == 1).sum()), "clipped": int((np.asarray(rows["flags"]) & 1).sum()),
            "cost0_sum": int(np.asarray(rows["cost0"], dtype=np.int64).sum()), "cost_sum": int(np.asarray(rows["cost"], dtype=np.int64).sum()),
            "a": int(np.asarray(a).sum()), "b": int(np.asarray(b_occ).sum())}


def warp(rows, a, b_occ, grid, b):
    """(P, stats): P[iz, ix, iy] = B(v - d_k) for v in listed block k, clipped to the grid; unlisted blocks are empty."""
    a, b_occ = np.asarray(a, dtype=bool), np.asarray(b_occ, dtype=bool)
    nx, ny, nz = grid
    P = np.zeros_like(b_occ)
    for (bx, by, bz), (dx, dy, dz) in zip(np.asarray(rows["ijk"], dtype=np.int64), np.asarray(rows["d"], dtype=np.int64)):
        z, x, y = np.meshgrid(np.arange(bz * b, min(bz * b + b, nz)), np.arange(bx * b, min(bx * b + b, nx)),
                              np.arange(by * b, min(by * b + b, ny)), indexing="ij")
        sz, sx, sy = z - dz, x - dx, y - dy
        ok = (sz >= 0) & (sz < nz) & (sx >= 0) & (sx < nx) & (sy >= 0) & (sy < ny)
        P[z[ok], x[ok], y[ok]] = b_occ[sz[ok], sx[ok], sy[ok]]
    return P, {"warped": int(P.sum()), "common": int((P & a).sum()), "a": int(a.sum())}


def paint(records, rows, grid, b, s):
    """The records after vc_paint_motion: channel = 128 + (127 d) / s, the division towards zero; index and seen byte stay."""
    records = np.asarray(records, dtype=np.uint64)
    nx, ny, nz = grid
    nbx, nby, _ = block_dims(grid, b)
    idx = (records & np.uint64(0xffffffff)).astype(np.int64)
    iy, t = idx % ny, idx // ny
    k = ((t // nx) // b * nbx + (t % nx) // b) * nby + iy // b
    block = np.asarray(rows["block"], dtype=np.int64)
    at = np.searchsorted(block, k)
    assert (at < block.size).all() and np.array_equal(block[at], k), "every record's block is listed"
    d = np.asarray(rows["d"], dtype=np.int64).reshape(-1, 3)[at]
    num = 127 * d
    ch = (128 + np.sign(num) * (np.abs(num) // s)).astype(np.uint64)
    rgb = ch[:, 0] | (ch[:, 1] << np.uint64(8)) | (ch[:, 2] << np.uint64(16))
    return (records & np.uint64(0xff000000ffffffff)) | (rgb << np.uint64(32))


def shifted(occ, shift):
    """occ[iz, ix, iy] moved by shift = (dx, dy, dz); what leaves the grid is lost."""
    out = np.zeros_like(occ)
    dx, dy, dz = shift
    z, x, y = np.nonzero(occ)
    z, x, y = z + dz, x + dx, y + dy
    ok = (z >= 0) & (z < occ.shape[0]) & (x >= 0) & (x < occ.shape[1]) & (y >= 0) & (y < occ.shape[2])
    out[z[ok], x[ok], y[ok]] = True
    return out


def random_pair(grid, seed, s):
    """B: a few random boxes; A: B moved by a random vector within the range, with a little noise on both."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = grid
    b = np.zeros((nz, nx, ny), dtype=bool)
    for _ in range(3):
        lo = [int(rng.integers(0, n)) for n in (nz, nx, ny)]
        hi = [int(min(n, l + rng.integers(1, max(2, n // 2 + 1)))) for n, l in zip((nz, nx, ny), lo)]
        b[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    a = shifted(b, tuple(int(v) for v in rng.integers(-s, s + 1, 3)))
    a ^= rng.random(a.shape) < 0.02
    b ^= rng.random(b.shape) < 0.02
    return a, b


def words(occ):
    """uint64 [ceil(n / 64)]: the occupancy words of vc_fetch_occupancy / vc_fetch_kept."""
    flat = np.asarray(occ, dtype=bool).reshape(-1)
    padded = np.zeros((flat.size + 63) // 64 * 64, dtype=np.uint8)
    padded[:flat.size] = flat
    return np.packbits(padded, bitorder="little").view(np.uint64)


def iou(a, b_occ):
    a, b_occ = np.asarray(a, dtype=bool), np.asarray(b_occ, dtype=bool)
    u = int((a | b_occ).sum())
    return int((a & b_occ).sum()) / u if u else None
