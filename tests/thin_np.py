"""The restatement of the thinning pass (contract of vc_hull_thin in include/voxcarve.h), in two independent forms that must agree
byte for byte:

  thin_literal   plain loops over a byte per cell, one voxel at a time in ascending linear index within a sub-step, the predicate
                 by flood fill over explicit neighbour lists;
  thin           numpy: the 26-bit codes of a sub-step's candidates gathered from a padded volume, the predicate by bit masks,
                 memoised per code, the sub-step's voxels removed all at once.

Both return {"peel" u16 [S], "voxel" u32 [K], "record" u32 [K], "degree" u8 [K], and the stats of STATS as ints}.  Linear index
i = (iz nx + ix) ny + iy; grid = (nx, ny, nz).  Bit k of a code is the neighbour at offset (dx, dy, dz) with
k27 = (dz + 1) 9 + (dx + 1) 3 + (dy + 1), k = k27 below the centre (13) and k27 - 1 above it."""
import numpy as np

STATS = ("survivors", "anchors", "kept", "removed", "passes", "steps", "stable", "isolated", "endpoints", "junctions")
DIRECTIONS = ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0))     # (dx, dy, dz) of d0 .. d5
MODES = ("curve", "point")
MAX_PASSES = 4096

# the 26 offsets (dx, dy, dz) in the order of the code's bits
OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
BIT = {o: k for k, o in enumerate(OFFSETS)}


def coords(idx, grid):
    nx, ny, _ = grid
    i = np.asarray(idx, dtype=np.int64)
    return (i // ny) % nx, i % ny, i // (nx * ny)


def subfield(ix, iy, iz):
    return (ix & 1) | (iy & 1) << 1 | (iz & 1) << 2


# ---- the predicate, literal: flood fill over explicit neighbour lists --------------------------------------------------------------
def _adjacent26(a, b):
    return a != b and max(abs(a[0] - b[0]), abs(a[1] - b[1]), abs(a[2] - b[2])) == 1


def _adjacent6(a, b):
    return abs(a[0] - b[0]) + abs(a[1] - b[1]) + abs(a[2] - b[2]) == 1


N18 = [o for o in OFFSETS if abs(o[0]) + abs(o[1]) + abs(o[2]) <= 2]
N6 = [o for o in OFFSETS if abs(o[0]) + abs(o[1]) + abs(o[2]) == 1]
# the neighbour lists, by position in OFFSETS: who is 26-adjacent to whom inside N26*, who 6-adjacent inside N18*
NEAR26 = [[k for k, b in enumerate(OFFSETS) if _adjacent26(a, b)] for a in OFFSETS]
IN18 = [o in N18 for o in OFFSETS]
FACES = [k for k, o in enumerate(OFFSETS) if o in N6]
NEAR6_IN_18 = [[k for k, b in enumerate(OFFSETS) if IN18[k] and _adjacent6(a, b)] if IN18[j] else [] for j, a in enumerate(OFFSETS)]


def _flood(start, member, near):
    """How many cells the flood from `start` reaches over the lists `near`, through the cells with member[k]; seen per cell."""
    seen = [False] * 26
    seen[start] = True
    stack = [start]
    n = 1
    while stack:
        for b in near[stack.pop()]:
            if member[b] and not seen[b]:
                seen[b] = True
                n += 1
                stack.append(b)
    return n, seen


def simple_literal(member):
    """member: per offset of OFFSETS whether that neighbour belongs to H."""
    first = -1
    count = 0
    for k in range(26):
        if member[k]:
            count += 1
            if first < 0:
                first = k
    if count == 0:
        return False
    if _flood(first, member, NEAR26)[0] != count:
        return False
    back = [IN18[k] and not member[k] for k in range(26)]
    faces = [k for k in FACES if back[k]]
    if not faces:
        return False
    seen = _flood(faces[0], back, NEAR6_IN_18)[1]
    for f in faces:
        if not seen[f]:
            return False
    return True


def simple_code_literal(code):
    return simple_literal([bool((code >> k) & 1) for k in range(26)])


# ---- the predicate, by bit masks over the 27 cells of the cube ---------------------------------------------------------------------
def _cell(dx, dy, dz):
    return (dz + 1) * 9 + (dx + 1) * 3 + (dy + 1)


_ALL27 = (1 << 27) - 1
_Y0 = sum(1 << _cell(dx, -1, dz) for dx in (-1, 0, 1) for dz in (-1, 0, 1))
_Y2 = sum(1 << _cell(dx, 1, dz) for dx in (-1, 0, 1) for dz in (-1, 0, 1))
_X0 = sum(1 << _cell(-1, dy, dz) for dy in (-1, 0, 1) for dz in (-1, 0, 1))
_X2 = sum(1 << _cell(1, dy, dz) for dy in (-1, 0, 1) for dz in (-1, 0, 1))
_M18 = sum(1 << _cell(*o) for o in N18)
_M6 = sum(1 << _cell(*o) for o in N6)


def _grow_y(g):
    return g | ((g << 1) & ~_Y0 & _ALL27) | ((g >> 1) & ~_Y2)


def _grow_x(g):
    return g | ((g << 3) & ~_X0 & _ALL27) | ((g >> 3) & ~_X2)


def _grow_z(g):
    return g | ((g << 9) & _ALL27) | (g >> 9)


def cube_of(code):
    """The 26-bit code spread over the 27 cells of the cube, the centre clear."""
    return (code & 0x1fff) | ((code >> 13) << 14)


def simple_code(code):
    m = cube_of(code)
    if m == 0:
        return False
    g = m & -m
    while True:
        n = _grow_z(_grow_x(_grow_y(g))) & m
        if n == g:
            break
        g = n
    if g != m:
        return False
    b = ~m & _M18
    faces = b & _M6
    if faces == 0:
        return False
    g = faces & -faces
    while True:
        n = (_grow_y(g) | _grow_x(g) | _grow_z(g)) & b
        if n == g:
            break
        g = n
    return faces & ~g == 0


_MEMO = {}


def simple_codes(codes):
    """bool per code, memoised."""
    out = np.empty(len(codes), dtype=bool)
    for j, c in enumerate(codes.tolist()):
        v = _MEMO.get(c)
        if v is None:
            v = _MEMO[c] = simple_code(c)
        out[j] = v
    return out


def table_bits(codes):
    """The bytes of fetch_thin_table() hold bit c at byte c >> 3, bit c & 7: what they must say about `codes`."""
    return simple_codes(np.asarray(codes, dtype=np.int64))


# ---- shared -----------------------------------------------------------------------------------------------------------------------
def _check_args(idx, grid, mode, anchors, max_passes):
    if mode not in MODES:
        raise ValueError("mode %r" % (mode,))
    if not 1 <= max_passes <= 10000:
        raise ValueError("max_passes %r" % (max_passes,))
    idx = np.asarray(idx, dtype=np.int64)
    assert (np.diff(idx) > 0).all() and (idx.size == 0 or (idx[0] >= 0 and idx[-1] < grid[0] * grid[1] * grid[2]))
    anchors = np.unique(np.asarray([] if anchors is None else anchors, dtype=np.int64))
    if not np.isin(anchors, idx).all():
        raise ValueError("an anchor is no survivor")
    return idx, anchors


def _volume(idx, grid):
    nx, ny, nz = grid
    vol = np.zeros((nz + 2, nx + 2, ny + 2), dtype=bool)
    ix, iy, iz = coords(idx, grid)
    vol[iz + 1, ix + 1, iy + 1] = True
    return vol


def gather_codes(vol, ix, iy, iz):
    code = np.zeros(ix.size, dtype=np.int64)
    for k, (dx, dy, dz) in enumerate(OFFSETS):
        code |= vol[iz + 1 + dz, ix + 1 + dx, iy + 1 + dy].astype(np.int64) << k
    return code


def _finish(idx, grid, peel, vol, anchors, passes, steps, stable):
    kept = np.flatnonzero(peel == 0)
    ix, iy, iz = coords(idx[kept], grid)
    degree = np.array([bin(c).count("1") for c in gather_codes(vol, ix, iy, iz).tolist()], dtype=np.uint8)
    return {"peel": peel, "voxel": idx[kept].astype(np.uint32), "record": kept.astype(np.uint32), "degree": degree,
            "survivors": int(idx.size), "anchors": int(anchors.size), "kept": int(kept.size), "removed": int(idx.size - kept.size),
            "passes": int(passes), "steps": int(steps), "stable": int(stable), "isolated": int((degree == 0).sum()),
            "endpoints": int((degree == 1).sum()), "junctions": int((degree >= 3).sum())}


# ---- the vectorised form ----------------------------------------------------------------------------------------------------------
def thin(idx, grid, mode="curve", anchors=None, max_passes=MAX_PASSES):
    idx, anchors = _check_args(idx, grid, mode, anchors, max_passes)
    vol = _volume(idx, grid)
    ix, iy, iz = coords(idx, grid)
    sub = subfield(ix, iy, iz)
    free = ~np.isin(idx, anchors)
    peel = np.zeros(idx.size, dtype=np.uint16)
    live = np.arange(idx.size)
    passes = steps = 0
    stable = 0
    while passes < max_passes:
        passes += 1
        removed = 0
        for d, (dx, dy, dz) in enumerate(DIRECTIONS):
            live = live[peel[live] == 0]
            cand = live[free[live] & ~vol[iz[live] + 1 + dz, ix[live] + 1 + dx, iy[live] + 1 + dy]]
            if cand.size == 0:
                continue
            steps += 1
            for s in range(8):
                c = cand[sub[cand] == s]
                if c.size == 0:
                    continue
                code = gather_codes(vol, ix[c], iy[c], iz[c])
                go = simple_codes(code)
                if mode == "curve":
                    go &= (code & (code - 1)) != 0               # (a simple voxel has a neighbour: one bit set is an end point)
                c = c[go]
                vol[iz[c] + 1, ix[c] + 1, iy[c] + 1] = False
                peel[c] = 1 + 6 * (passes - 1) + d
                removed += c.size
        if removed == 0:
            stable = 1
            break
    return _finish(idx, grid, peel, vol, anchors, passes, steps, stable)


# ---- the literal form -------------------------------------------------------------------------------------------------------------
def thin_literal(idx, grid, mode="curve", anchors=None, max_passes=MAX_PASSES):
    idx, anchors = _check_args(idx, grid, mode, anchors, max_passes)
    nx, ny, nz = grid
    px, py = nx + 2, ny + 2                                      # H as one byte per cell of the grid padded by one cell
    H = bytearray((nz + 2) * px * py)
    at = []                                                      # per record: its cell in the padded grid
    sub = []
    for i in idx.tolist():
        x, y, z = (i // ny) % nx, i % ny, i // (nx * ny)
        at.append(((z + 1) * px + x + 1) * py + y + 1)
        sub.append(subfield(x, y, z))
        H[at[-1]] = 1
    step = [(dz * px + dx) * py + dy for dx, dy, dz in OFFSETS]
    toward = [(dz * px + dx) * py + dy for dx, dy, dz in DIRECTIONS]
    pinned = set(anchors.tolist())
    free = [int(i) not in pinned for i in idx.tolist()]
    peel = [0] * len(at)
    passes = steps = 0
    stable = 0
    while passes < max_passes:
        passes += 1
        removed = 0
        for d in range(6):
            cand = []
            for r in range(len(at)):
                if peel[r] == 0 and free[r] and not H[at[r] + toward[d]]:
                    cand.append(r)
            if not cand:
                continue
            steps += 1
            for s in range(8):
                for r in cand:                                   # ascending index, one voxel at a time
                    if sub[r] != s:
                        continue
                    p = at[r]
                    member = [H[p + o] == 1 for o in step]
                    if not simple_literal(member) or (mode == "curve" and sum(member) == 1):
                        continue
                    H[p] = 0
                    peel[r] = 1 + 6 * (passes - 1) + d
                    removed += 1
        if removed == 0:
            stable = 1
            break
    peel = np.array(peel, dtype=np.uint16)
    return _finish(idx, grid, peel, _volume(idx[peel == 0], grid), anchors, passes, steps, stable)


# ---- topology, for the tests ------------------------------------------------------------------------------------------------------
def euler_number(idx, grid):
    """Vertices - edges + faces - cubes of the cubical complex whose cubes are the voxels."""
    nx, ny, nz = grid
    vol = np.zeros((nz + 1, nx + 1, ny + 1), dtype=bool)
    ix, iy, iz = coords(idx, grid)
    vol[iz, ix, iy] = True
    total = 0
    for kind in range(8):                                        # which axes the cell spans: 0 a vertex .. 7 a cube
        sz, sx, sy = kind >> 2 & 1, kind >> 1 & 1, kind & 1
        cell = np.zeros((nz + 1, nx + 1, ny + 1), dtype=bool)
        for oz in ((0,) if sz else (0, 1)):                      # a cell that does not span an axis touches the voxels on both sides
            for ox in ((0,) if sx else (0, 1)):
                for oy in ((0,) if sy else (0, 1)):
                    cell |= np.roll(vol, (oz, ox, oy), axis=(0, 1, 2))
        dim = sz + sx + sy
        total += int(cell.sum()) * (-1 if dim & 1 else 1)
    return total


def topology(idx, grid):
    """(26-components of the set, 6-components of its complement on the grid padded by one cell, Euler number).  The components
    by scipy.ndimage.label where there is one (the padded 128^3 grid has two million background voxels), else by components_np."""
    nx, ny, nz = grid
    idx = np.asarray(idx, dtype=np.int64)
    ix, iy, iz = coords(idx, grid)
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        vol = np.zeros((nz + 2, nx + 2, ny + 2), dtype=bool)
        vol[iz + 1, ix + 1, iy + 1] = True
        comp = ndimage.label(vol, structure=np.ones((3, 3, 3), dtype=bool))[1]
        back = ndimage.label(~vol)[1]
    else:
        import components_np as cn
        comp = int(cn.components(idx, grid, 26)["label"].size)
        big = (nx + 2, ny + 2, nz + 2)
        full = np.ones(big[0] * big[1] * big[2], dtype=bool)
        full[((iz + 1) * big[0] + ix + 1) * big[1] + iy + 1] = False
        back = int(cn.components(np.flatnonzero(full), big, 6)["label"].size)
    return int(comp), int(back), euler_number(idx, grid)
