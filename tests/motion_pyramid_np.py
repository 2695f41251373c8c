"""The contract of vc_hull_motion_pyramid, vc_fetch_motion_level and vc_fetch_motion_occupancy (include/voxcarve.h, DESIGN section 8
item 24) restated in numpy: the OR pyramid of two hulls, vc_hull_motion's matching on its coarsest level, and on every finer level a
choice among the displacements around twice the parent block's vector and twice its face neighbours' vectors.  Integers only;
everything on a single level is motion_np's.

  halve / pyramid          the OR levels of a hull
  reach                    the largest component a vector can have
  match_pyramid_literal    the definition: block by block and displacement by displacement, cell by cell
  match_pyramid            the same from packed rows: per block and centre the whole cube of costs at once
  stats / paint            the stats of vc_hull_motion_pyramid, the records after vc_paint_motion (which scales by reach)

Both matchers return a dict: rows, grids, a, b (lists over the levels 0..L: the rows as motion_np's, flags with bit 1; the grid
(nx, ny, nz); the two volumes), evaluated (the displacements tried on the refined levels, each once per block), levels, refine,
search, reach."""
import numpy as np

import motion_np as mn

FLAG_CLIPPED, FLAG_BORROWED = 1, 2
FACES = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))        # (x, y, z)


def halve(occ):
    """occ[iz, ix, iy] one level up: cell v is the OR of the cells 2v + {0, 1}^3 that lie in the grid; ceil(n / 2) cells per axis."""
    occ = np.asarray(occ, dtype=bool)
    nz, nx, ny = occ.shape
    hz, hx, hy = (nz + 1) // 2, (nx + 1) // 2, (ny + 1) // 2
    p = np.zeros((2 * hz, 2 * hx, 2 * hy), dtype=bool)
    p[:nz, :nx, :ny] = occ
    return p.reshape(hz, 2, hx, 2, hy, 2).any(axis=(1, 3, 5))


def level_grid(grid, level):
    g = tuple(int(n) for n in grid)
    for _ in range(level):
        g = tuple((n + 1) // 2 for n in g)
    return g


def pyramid(occ, levels):
    """[occ_0 .. occ_L]."""
    out = [np.asarray(occ, dtype=bool)]
    for _ in range(levels):
        out.append(halve(out[-1]))
    return out


def reach(search, levels, refine):
    return search * 2 ** levels + refine * (2 ** levels - 1)


def _window(vol, z0, x0, y0, W):
    """The W^3 cells of vol[iz, ix, iy] from (z0, x0, y0) on; cells off the grid are empty."""
    out = np.zeros((W, W, W), dtype=bool)
    lo = [max(o, 0) for o in (z0, x0, y0)]
    hi = [min(o + W, n) for o, n in zip((z0, x0, y0), vol.shape)]
    if all(l < h for l, h in zip(lo, hi)):
        out[lo[0] - z0:hi[0] - z0, lo[1] - x0:hi[1] - x0, lo[2] - y0:hi[2] - y0] = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    return out


def _rows(grid, b, cols):
    nbx, nby, _ = mn.block_dims(grid, b)
    k = np.asarray(cols["block"], dtype=np.int64)
    return {"block": k.astype(np.uint32), "ijk": np.stack([(k // nby) % nbx, k % nby, k // (nby * nbx)], axis=1).reshape(-1, 3),
            "d": np.asarray(cols["d"], dtype=np.int64).reshape(-1, 3).astype(np.int8), "cost": np.asarray(cols["cost"], dtype=np.uint32),
            "cost0": np.asarray(cols["cost0"], dtype=np.uint32), "count_a": np.asarray(cols["count_a"], dtype=np.uint16),
            "count_b": np.asarray(cols["count_b"], dtype=np.uint16), "ties": np.asarray(cols["ties"], dtype=np.uint16),
            "flags": np.asarray(cols["flags"], dtype=np.uint8)}


def _centres(bx, by, bz, parent_rows, parent_nb, neighbours):
    """The block's centres (dx, dy, dz), the prediction first: twice the vector of the parent block and of its listed face neighbours."""
    pnbx, pnby, pnbz = parent_nb
    pk = np.asarray(parent_rows["block"], dtype=np.int64)
    pd = np.asarray(parent_rows["d"], dtype=np.int64).reshape(-1, 3)
    px, py, pz = bx >> 1, by >> 1, bz >> 1

    def at(qx, qy, qz):
        if not (0 <= qx < pnbx and 0 <= qy < pnby and 0 <= qz < pnbz):
            return None
        k = (qz * pnbx + qx) * pnby + qy
        i = int(np.searchsorted(pk, k))
        return 2 * pd[i] if i < pk.size and pk[i] == k else None

    c = at(px, py, pz)
    if c is None:
        raise AssertionError("block (%d, %d, %d): its parent is not listed" % (bx, by, bz))
    out = [tuple(int(v) for v in c)]
    if neighbours:
        for ex, ey, ez in FACES:
            v = at(px + ex, py + ey, pz + ez)
            if v is not None:
                out.append(tuple(int(t) for t in v))
    return out


def _flags(d, c, D, r):
    """bit 0: a face neighbour of the winner was not tried; bit 1: the winner lies outside the prediction's own cube."""
    f = 0
    if any((d[0] + e[0], d[1] + e[1], d[2] + e[2]) not in D for e in FACES):
        f |= FLAG_CLIPPED
    if max(abs(d[0] - c[0]), abs(d[1] - c[1]), abs(d[2] - c[2])) > r:
        f |= FLAG_BORROWED
    return f


def _refine_literal(A, B, grid, b, ap, r, parent_rows, parent_grid, neighbours):
    nbx, nby, nbz = mn.block_dims(grid, b)
    pnb = mn.block_dims(parent_grid, b)
    W = b + 2 * ap
    cols = {k: [] for k in ("block", "d", "cost", "cost0", "count_a", "count_b", "ties", "flags")}
    evaluated = 0
    for bz in range(nbz):
        for bx in range(nbx):
            for by in range(nby):
                ca = int(_window(A, bz * b, bx * b, by * b, b).sum())
                cb = int(_window(B, bz * b, bx * b, by * b, b).sum())
                if ca == 0 and cb == 0:
                    continue
                centres = _centres(bx, by, bz, parent_rows, pnb, neighbours)
                c = centres[0]
                D = set()
                for e in centres:
                    for dz in range(e[2] - r, e[2] + r + 1):
                        for dx in range(e[0] - r, e[0] + r + 1):
                            for dy in range(e[1] - r, e[1] + r + 1):
                                D.add((dx, dy, dz))
                oz, ox, oy = bz * b - ap, bx * b - ap, by * b - ap
                win = _window(A, oz, ox, oy, W)

                def cost(d):
                    return int((win != _window(B, oz - d[2], ox - d[0], oy - d[1], W)).sum())      # B(v - d)

                costs = {d: cost(d) for d in D}
                best = min(D, key=lambda d: (costs[d], (d[0] - c[0]) ** 2 + (d[1] - c[1]) ** 2 + (d[2] - c[2]) ** 2, d[2], d[0], d[1]))
                low = costs[best]
                evaluated += len(D)
                for key, v in (("block", (bz * nbx + bx) * nby + by), ("d", best), ("cost", low), ("cost0", cost((0, 0, 0))), ("count_a", ca),
                               ("count_b", cb), ("ties", sum(1 for v in costs.values() if v == low)), ("flags", _flags(best, c, D, r))):
                    cols[key].append(v)
    return _rows(grid, b, cols), evaluated


def _packed(vol):
    """uint64 [nz, nx]: the y lines of vol[iz, ix, iy] (at most 64 cells), bit j = cell j."""
    nz, nx, ny = vol.shape
    p = np.zeros((nz, nx, 64), dtype=np.uint8)
    p[:, :, :ny] = vol
    return np.packbits(p, axis=2, bitorder="little").view("<u8").reshape(nz, nx)


def _cube_costs(win_rows, B, oz, ox, oy, W, e, r):
    """int64 [2r+1, 2r+1, 2r+1] indexed [dz - ez + r, dx - ex + r, dy - ey + r]: the costs of the cube around the centre e."""
    R = W + 2 * r
    reg = _packed(_window(B, oz - e[2] - r, ox - e[0] - r, oy - e[1] - r, R))      # region cell (wz + r - tz, ...) is B(v - e - t)
    mask = np.uint64((1 << W) - 1)
    side = 2 * r + 1
    out = np.empty((side, side, side), dtype=np.int64)
    for ty in range(-r, r + 1):
        rows = (reg >> np.uint64(r - ty)) & mask
        view = np.lib.stride_tricks.sliding_window_view(rows, (W, W))           # [side, side, W, W] from (r - tz, r - tx) on
        c = np.bitwise_count(view ^ win_rows).sum(axis=(2, 3), dtype=np.int64)
        out[:, :, ty + r] = c[::-1, ::-1]
    return out


def _code(d):
    d = np.asarray(d, dtype=np.int64)
    return ((d[..., 2] + 128) * 256 + d[..., 0] + 128) * 256 + d[..., 1] + 128       # ascending code = ascending (dz, dx, dy)


def _refine_packed(A, B, grid, b, ap, r, parent_rows, parent_grid, neighbours):
    nbx, nby, nbz = mn.block_dims(grid, b)
    pnb = mn.block_dims(parent_grid, b)
    W = b + 2 * ap
    t = np.arange(-r, r + 1)
    tz, tx, ty = np.meshgrid(t, t, t, indexing="ij")
    cube = np.stack([tx.reshape(-1), ty.reshape(-1), tz.reshape(-1)], axis=1)   # the order of _cube_costs flattened
    ca = mn._box_sums(mn._padded(A, grid, b, 0).astype(np.int32), b, b, (nbz, nbx, nby)).reshape(-1)
    cb = mn._box_sums(mn._padded(B, grid, b, 0).astype(np.int32), b, b, (nbz, nbx, nby)).reshape(-1)
    cols = {k: [] for k in ("block", "d", "cost", "cost0", "count_a", "count_b", "ties", "flags")}
    evaluated = 0
    for k in np.flatnonzero((ca > 0) | (cb > 0)):
        by, q = int(k % nby), int(k // nby)
        bx, bz = q % nbx, q // nbx
        centres = _centres(bx, by, bz, parent_rows, pnb, neighbours)
        c = np.array(centres[0], dtype=np.int64)
        oz, ox, oy = bz * b - ap, bx * b - ap, by * b - ap
        win = _window(A, oz, ox, oy, W)
        win_rows = _packed(win)
        ds, cs = [], []
        for e in dict.fromkeys(centres):
            ds.append(cube + np.array(e, dtype=np.int64))
            cs.append(_cube_costs(win_rows, B, oz, ox, oy, W, e, r).reshape(-1))
        ds, cs = np.concatenate(ds), np.concatenate(cs)
        codes, first = np.unique(_code(ds), return_index=True)                  # each displacement once
        ds, cs = ds[first], cs[first]
        off = ds - c
        order = np.lexsort((codes, (off * off).sum(axis=1), cs))                # (the last key is the primary one)
        j = int(order[0])
        d = ds[j]
        zero = np.flatnonzero(codes == _code(np.zeros(3, dtype=np.int64)))
        cost0 = int(cs[zero[0]]) if zero.size else int((win != _window(B, oz, ox, oy, W)).sum())
        faces = _code(d + np.array(FACES, dtype=np.int64))
        flags = (0 if np.isin(faces, codes).all() else FLAG_CLIPPED) | (FLAG_BORROWED if np.abs(d - c).max() > r else 0)
        evaluated += int(codes.size)
        for key, v in (("block", int(k)), ("d", d), ("cost", int(cs[j])), ("cost0", cost0), ("count_a", int(ca[k])), ("count_b", int(cb[k])),
                       ("ties", int((cs == cs[j]).sum())), ("flags", flags)):
            cols[key].append(v)
    return _rows(grid, b, cols), evaluated


def _match(single, refine_level, a, b_occ, grid, b, ap, s, levels, refine, neighbours):
    grid = tuple(int(n) for n in grid)
    A, B = pyramid(a, levels), pyramid(b_occ, levels)
    grids = [level_grid(grid, l) for l in range(levels + 1)]
    rows = [None] * (levels + 1)
    rows[levels] = single(A[levels], B[levels], grids[levels], b, ap, s)
    evaluated = 0
    for l in range(levels - 1, -1, -1):
        rows[l], ev = refine_level(A[l], B[l], grids[l], b, ap, refine, rows[l + 1], grids[l + 1], neighbours)
        evaluated += ev
    return {"rows": rows, "grids": grids, "a": A, "b": B, "evaluated": evaluated, "levels": levels, "refine": refine, "search": s,
            "reach": reach(s, levels, refine)}


def match_pyramid_literal(a, b_occ, grid, b, ap, s, levels, refine, neighbours=True):
    """The field of every level, from the contract.  neighbours=False leaves every block its parent's prediction alone (what the
    contract does NOT say; the restatement's test shows the difference)."""
    return _match(mn.match_literal, _refine_literal, a, b_occ, grid, b, ap, s, levels, refine, neighbours)


def match_pyramid(a, b_occ, grid, b, ap, s, levels, refine, neighbours=True):
    return _match(mn.match, _refine_packed, a, b_occ, grid, b, ap, s, levels, refine, neighbours)


def stats(res, a, b_occ, grid, b):
    """The stats of vc_hull_motion_pyramid but motion_ms."""
    out = mn.stats(res["rows"][0], a, b_occ, grid, b)
    L = res["levels"]
    out.update(levels=L, refine=res["refine"], reach=res["reach"], evaluated=int(res["evaluated"]),
               borrowed=int(((np.asarray(res["rows"][0]["flags"]) & FLAG_BORROWED) != 0).sum()),
               listed_level=[int(len(res["rows"][l]["block"])) if l <= L else 0 for l in range(4)],
               dims_level=[list(res["grids"][l]) if l <= L else [0, 0, 0] for l in range(4)])
    return out


def paint(records, res, grid, b):
    """The records after vc_paint_motion on a pyramid's field: motion_np's colours with the reach for the search range."""
    return mn.paint(records, res["rows"][0], grid, b, res["reach"])
