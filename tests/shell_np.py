"""The restatement of vc_hull_shell and vc_fetch_shell_viewer (contract in include/voxcarve.h): the cells of a hull with an exposed
face, in cell order, with their face bytes, at the voxels' resolution or on a grid 2^L times coarser with averaged colours, and
the viewer's float32 arrays of the list -- once as a literal loop (shell_literal, viewer_literal) and once vectorised (shell,
viewer).  Both return the dict {records u64 [T], faces u8 [T], stats}; stats holds what vc_shell_stats_t holds but the time."""
import numpy as np

MAX_LEVEL = 6
# the neighbour across each face, in the order of the face byte's bits: -x, +x, -y, +y, -z, +z as (dx, dy, dz)
FACES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def coarse_dims(grid, level):
    f = 1 << level
    return tuple((n + f - 1) // f for n in grid)


def _check(grid, level):
    if not 0 <= level <= MAX_LEVEL:
        raise ValueError("level %r not in 0..%d" % (level, MAX_LEVEL))
    if grid[0] * grid[1] * grid[2] > 0xffffffff:
        raise ValueError("the grid exceeds the u32 index")


def _stats(S, on, level, dims, faces):
    faces = np.asarray(faces, dtype=np.uint8)
    return {"survivors": int(S), "cells_on": int(on), "shell": int(faces.size),
            "faces": [int(((faces >> k) & 1).sum()) for k in range(6)],
            "level": int(level), "cube_scale": 1 << level, "dims": [int(d) for d in dims]}


def _face_byte(cell, dims, on):
    """Item 2 for one ON cell (x, y, z) of a grid of dims whose ON cells are the set `on`."""
    byte = 0
    for k, (dx, dy, dz) in enumerate(FACES):
        q = (cell[0] + dx, cell[1] + dy, cell[2] + dz)
        inside = all(0 <= q[a] < dims[a] for a in range(3))
        if not inside or q not in on:
            byte |= 1 << k
    return byte


def shell_literal(records, grid, level=0):
    """The contract read out loud: sets of cells, one loop over them."""
    _check(grid, level)
    nx, ny, nz = grid
    records = [int(r) for r in np.asarray(records, dtype=np.uint64)]
    f = 1 << level
    dims = coarse_dims(grid, level)
    fine = {}
    for r in records:
        i = r & 0xffffffff
        fine[((i // ny) % nx, i % ny, i // (nx * ny))] = r
    fine_on = set(fine)
    if level == 0:
        out = []
        for c in fine_on:
            byte = _face_byte(c, grid, fine_on)
            if byte:
                out.append(((c[2] * nx + c[0]) * ny + c[1], fine[c] >> 32, byte))
    else:
        on = set((c[0] // f, c[1] // f, c[2] // f) for c in fine_on)
        sums = {}
        for c, r in fine.items():                                # the level-0 shell voxels the colour camera sees
            if _face_byte(c, grid, fine_on) and (r >> 56) & 1:
                a = sums.setdefault((c[0] // f, c[1] // f, c[2] // f), [0, 0, 0, 0])
                for k in range(3):
                    a[k] += (r >> (32 + 8 * k)) & 255
                a[3] += 1
        out = []
        for c in on:
            byte = _face_byte(c, dims, on)
            if not byte:
                continue
            upper = 0
            if c in sums:
                s = sums[c]
                n = s[3]
                upper = ((s[0] + n // 2) // n) | ((s[1] + n // 2) // n) << 8 | ((s[2] + n // 2) // n) << 16 | 1 << 24
            out.append(((c[2] * dims[0] + c[0]) * dims[1] + c[1], upper, byte))
    out.sort()
    rec = np.array([j | (u << 32) for j, u, _ in out], dtype=np.uint64)
    faces = np.array([b for _, _, b in out], dtype=np.uint8)
    return {"records": rec, "faces": faces,
            "stats": _stats(len(records), len(fine_on) if level == 0 else len(on), level, dims, faces)}


def _face_bytes(occ):
    """u8 volume [nz, nx, ny]: the face byte of every ON cell of the boolean volume occ (0 elsewhere)."""
    pad = np.zeros(tuple(n + 2 for n in occ.shape), dtype=bool)   # a border of OFF cells: outside the grid is exposed
    pad[1:-1, 1:-1, 1:-1] = occ
    nz, nx, ny = occ.shape
    byte = np.zeros(occ.shape, dtype=np.uint8)
    for k, (dx, dy, dz) in enumerate(FACES):
        nb = pad[1 + dz:1 + dz + nz, 1 + dx:1 + dx + nx, 1 + dy:1 + dy + ny]
        byte |= (occ & ~nb).astype(np.uint8) << np.uint8(k)
    return byte


def shell(records, grid, level=0):
    _check(grid, level)
    nx, ny, nz = grid
    records = np.asarray(records, dtype=np.uint64)
    idx = (records & np.uint64(0xffffffff)).astype(np.int64)
    iy, ix, iz = idx % ny, (idx // ny) % nx, idx // (nx * ny)
    occ = np.zeros((nz, nx, ny), dtype=bool)
    occ[iz, ix, iy] = True
    fb = _face_bytes(occ)[iz, ix, iy]                             # per record
    dims = coarse_dims(grid, level)
    if level == 0:
        keep = fb != 0
        return {"records": records[keep].copy(), "faces": fb[keep].copy(), "stats": _stats(records.size, records.size, 0, dims, fb[keep])}
    cx, cy, cz = ix >> level, iy >> level, iz >> level
    cocc = np.zeros((dims[2], dims[0], dims[1]), dtype=bool)
    cocc[cz, cx, cy] = True
    cbyte = _face_bytes(cocc)
    z, x, y = np.nonzero(cbyte)                                   # ascending (cz, cx, cy): ascending j
    j = (z * dims[0] + x) * dims[1] + y
    seen = ((records >> np.uint64(56)) & np.uint64(1)).astype(bool)
    add = (fb != 0) & seen
    cj = ((cz * dims[0] + cx) * dims[1] + cy)[add]
    ncell = dims[0] * dims[1] * dims[2]
    n = np.bincount(cj, minlength=ncell)[j]                       # (counts and sums below 2^26: exact in float64)
    upper = np.zeros(j.size, dtype=np.uint64)
    some = n > 0
    d = np.maximum(n, 1)
    for k, sh in enumerate((32, 40, 48)):
        c = ((records[add] >> np.uint64(sh)) & np.uint64(255)).astype(np.float64)
        s = np.bincount(cj, weights=c, minlength=ncell)[j].astype(np.int64)
        upper |= ((s + d // 2) // d).astype(np.uint64) << np.uint64(8 * k)
    upper = np.where(some, upper | np.uint64(1 << 24), np.uint64(0))
    faces = cbyte[z, x, y]
    return {"records": j.astype(np.uint64) | (upper << np.uint64(32)), "faces": faces,
            "stats": _stats(records.size, int(cocc.sum()), level, dims, faces)}


def viewer_literal(shell_records, grid, axes, level=0, scaling=64.0):
    """Item 4 cell by cell: (positions float32 [T, 3], colours float32 [T, 3])."""
    f = 1 << level
    dims = coarse_dims(grid, level)
    pos, col = [], []
    for r in (int(v) for v in np.asarray(shell_records, dtype=np.uint64)):
        j = r & 0xffffffff
        c = ((j // dims[1]) % dims[0], j % dims[1], j // (dims[0] * dims[1]))
        v = []
        for a in range(3):
            lo, hi = f * c[a], min(f * c[a] + f, grid[a]) - 1
            v.append((np.float64(np.trunc(axes[a][lo])) / np.float64(scaling) + np.float64(np.trunc(axes[a][hi])) / np.float64(scaling))
                     * np.float64(0.5))
        pos.append([np.float32(v[0]), np.float32(-v[2]), np.float32(v[1])])
        col.append([np.float32(np.float64((r >> (32 + 8 * k)) & 255) / np.float64(255.0)) for k in range(3)])
    return np.array(pos, dtype=np.float32).reshape(-1, 3), np.array(col, dtype=np.float32).reshape(-1, 3)


def viewer(shell_records, grid, axes, level=0, scaling=64.0):
    f = 1 << level
    dims = coarse_dims(grid, level)
    rec = np.asarray(shell_records, dtype=np.uint64)
    j = (rec & np.uint64(0xffffffff)).astype(np.int64)
    cell = ((j // dims[1]) % dims[0], j % dims[1], j // (dims[0] * dims[1]))
    v = []
    for a in range(3):
        A = np.trunc(np.asarray(axes[a], dtype=np.float64))
        lo = f * cell[a]
        hi = np.minimum(lo + f, grid[a]) - 1
        v.append((A[lo] / np.float64(scaling) + A[hi] / np.float64(scaling)) * 0.5)
    pos = np.stack([v[0], -v[2], v[1]], axis=1).astype(np.float32)
    rgb = np.stack([((rec >> np.uint64(s)) & np.uint64(255)).astype(np.float64) for s in (32, 40, 48)], axis=1)
    return pos, (rgb / 255.0).astype(np.float32)


def same(a, b):
    """Asserts two shells equal: records, faces (dtype and shape included) and stats."""
    for k in ("records", "faces"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(x, y), (k, x, y)
    assert a["stats"] == b["stats"], (a["stats"], b["stats"])


def same_bits(x, y):
    """Asserts two float32 arrays equal bit for bit (-0.0 is not 0.0)."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.dtype == y.dtype == np.float32 and x.shape == y.shape, (x.dtype, y.dtype, x.shape, y.shape)
    assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
