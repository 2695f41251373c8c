"""The motion pass's side of the C ABI (vc_hull_motion, vc_hull_warp; include/voxcarve.h) and what goes with it on the host:
the rows and the stats as the library lays them out, the field in millimetres, the vector of each figure.  Pure Python / numpy;
the matching itself is vc_hull_motion, and CarveEngine.hull_motion / fetch_motion / warp_hull / paint_motion make the calls."""
import ctypes

import numpy as np

BLOCKS = (4, 8, 16)
MAX_APRON, MAX_SEARCH, ROW_BITS = 16, 8, 64
FLAG_CLIPPED = 1
MAX_LEVELS = 3                               # coarser levels of vc_hull_motion_pyramid
FLAG_BORROWED = 2                            # (a pyramid's rows: the vector came from a neighbour's prediction)


class MotionRow(ctypes.Structure):           # vc_motion_t
    _fields_ = [("block", ctypes.c_uint32), ("d", ctypes.c_int8 * 3), ("flags", ctypes.c_uint8), ("cost", ctypes.c_uint32),
                ("cost0", ctypes.c_uint32), ("count_a", ctypes.c_uint16), ("count_b", ctypes.c_uint16), ("ties", ctypes.c_uint16),
                ("reserved", ctypes.c_uint16)]


ROW_DTYPE = np.dtype([("block", "<u4"), ("d", "i1", (3,)), ("flags", "u1"), ("cost", "<u4"), ("cost0", "<u4"), ("count_a", "<u2"),
                      ("count_b", "<u2"), ("ties", "<u2"), ("reserved", "<u2")])
assert ROW_DTYPE.itemsize == ctypes.sizeof(MotionRow) == 24


class MotionStats(ctypes.Structure):         # vc_motion_stats_t
    _fields_ = [("blocks", ctypes.c_uint64), ("listed", ctypes.c_uint64), ("moved", ctypes.c_uint64), ("unique", ctypes.c_uint64),
                ("clipped", ctypes.c_uint64), ("cost0_sum", ctypes.c_uint64), ("cost_sum", ctypes.c_uint64), ("a", ctypes.c_uint64),
                ("b", ctypes.c_uint64), ("motion_ms", ctypes.c_float)]


class PyramidStats(ctypes.Structure):        # vc_motion_pyramid_stats_t
    _fields_ = [("blocks", ctypes.c_uint64), ("listed", ctypes.c_uint64), ("moved", ctypes.c_uint64), ("unique", ctypes.c_uint64),
                ("clipped", ctypes.c_uint64), ("cost0_sum", ctypes.c_uint64), ("cost_sum", ctypes.c_uint64), ("a", ctypes.c_uint64),
                ("b", ctypes.c_uint64), ("levels", ctypes.c_uint32), ("refine", ctypes.c_uint32), ("reach", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("listed_level", ctypes.c_uint64 * 4), ("dims_level", (ctypes.c_uint32 * 3) * 4),
                ("evaluated", ctypes.c_uint64), ("borrowed", ctypes.c_uint64), ("motion_ms", ctypes.c_float)]


class WarpStats(ctypes.Structure):           # vc_warp_stats_t
    _fields_ = [("warped", ctypes.c_uint64), ("common", ctypes.c_uint64), ("a", ctypes.c_uint64), ("warp_ms", ctypes.c_float)]


class TemporalMotionStats(ctypes.Structure):   # vc_temporal_motion_stats_t (the vote aligned by this field)
    _fields_ = [("window", ctypes.c_uint32), ("frames", ctypes.c_uint32), ("on", ctypes.c_uint32), ("off", ctypes.c_uint32),
                ("block", ctypes.c_uint32), ("apron", ctypes.c_uint32), ("search", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("survivors_before", ctypes.c_uint64), ("survivors_after", ctypes.c_uint64), ("added", ctypes.c_uint64),
                ("removed", ctypes.c_uint64), ("raw_changed", ctypes.c_uint64), ("aligned_changed", ctypes.c_uint64),
                ("out_changed", ctypes.c_uint64), ("blocks", ctypes.c_uint64), ("listed", ctypes.c_uint64), ("moved", ctypes.c_uint64),
                ("unique", ctypes.c_uint64), ("clipped", ctypes.c_uint64), ("cost0_sum", ctypes.c_uint64), ("cost_sum", ctypes.c_uint64),
                ("temporal_ms", ctypes.c_float)]


def check_params(block, apron, search):
    """(block, apron, search) as integers, apron=None meaning block // 2; ValueError outside the ranges of vc_hull_motion."""
    block = int(block)
    apron = block // 2 if apron is None else int(apron)
    search = int(search)
    if block not in BLOCKS:
        raise ValueError("motion: block edge %r, expected one of %r" % (block, BLOCKS))
    if not 0 <= apron <= MAX_APRON:
        raise ValueError("motion: apron %r not in 0..%d" % (apron, MAX_APRON))
    if not 1 <= search <= MAX_SEARCH:
        raise ValueError("motion: search range %r not in 1..%d" % (search, MAX_SEARCH))
    if block + 2 * apron + 2 * search > ROW_BITS:
        raise ValueError("motion: block + 2 apron + 2 search = %d exceeds the %d bits of a row" % (block + 2 * apron + 2 * search, ROW_BITS))
    return block, apron, search


def check_pyramid(levels, refine, search):
    """(levels, refine) as integers; ValueError outside the ranges of vc_hull_motion_pyramid: levels in 0..MAX_LEVELS, refine in
    1..search (checked with levels = 0 too, where it is not used)."""
    for name, v in (("levels", levels), ("refine", refine)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("motion: %s %r, expected an integer" % (name, v))
    levels, refine, search = int(levels), int(refine), int(search)
    if not 0 <= levels <= MAX_LEVELS:
        raise ValueError("motion: %r coarser levels, expected 0..%d" % (levels, MAX_LEVELS))
    if not 1 <= refine <= search:
        raise ValueError("motion: refine radius %r not in 1..search = %d" % (refine, search))
    return levels, refine


def reach(search, levels, refine):
    """The largest component a vector of the field can have: search 2^L + refine (2^L - 1)."""
    return int(search) * 2 ** int(levels) + int(refine) * (2 ** int(levels) - 1)


def level_grid(grid, level):
    """(nx, ny, nz) of level `level`: every level has ceil(n / 2) cells per axis of the one below."""
    g = tuple(int(n) for n in grid)
    for _ in range(int(level)):
        g = tuple((n + 1) // 2 for n in g)
    return g


def pyramid_stats_dict(st):
    """A filled PyramidStats as the dict CarveEngine.hull_motion(levels > 0) returns: the keys of MotionStats, then levels, refine,
    reach, listed_level [4], dims_level [4][3] (zeros above `levels`), evaluated, borrowed."""
    out = {name: int(getattr(st, name)) for name in ("blocks", "listed", "moved", "unique", "clipped", "cost0_sum", "cost_sum", "a", "b",
                                                     "levels", "refine", "reach", "evaluated", "borrowed")}
    out["listed_level"] = [int(v) for v in st.listed_level]
    out["dims_level"] = [[int(v) for v in row] for row in st.dims_level]
    out["motion_ms"] = float(st.motion_ms)
    return out


def vote_params(motion):
    """(block, apron, search) of temporal_filter's `motion` (and configure's temporal_motion): True is (8, None, 4), a
    (block, apron, search) tuple goes through check_params (apron None = block // 2); None stays None; ValueError otherwise."""
    if motion is None:
        return None
    if motion is True:
        motion = (8, None, 4)
    if isinstance(motion, (bool, np.bool_)) or not isinstance(motion, (tuple, list)) or len(motion) != 3:
        raise ValueError("temporal motion %r, expected None, True or (block, apron, search)" % (motion,))
    for name, v in zip(("block", "apron", "search"), motion):
        if isinstance(v, bool) or not (isinstance(v, (int, np.integer)) or (v is None and name == "apron")):
            raise ValueError("temporal motion %r: %s %r, expected an integer" % (tuple(motion), name, v))
    return check_params(*motion)


def block_dims(grid, edge):
    """(NBx, NBy, NBz): blocks per axis."""
    return tuple((int(n) + int(edge) - 1) // int(edge) for n in grid)


def block_ijk(block, grid, edge):
    """int64 [L, 3]: (bx, by, bz) of the block indices k = (bz NBx + bx) NBy + by."""
    nbx, nby, _ = block_dims(grid, edge)
    k = np.asarray(block, dtype=np.int64).reshape(-1)
    return np.stack([(k // nby) % nbx, k % nby, k // (nby * nbx)], axis=1)


def rows_dict(raw, grid, edge, apron, search):
    """The structured rows of vc_fetch_motion (ROW_DTYPE) as the dict of arrays CarveEngine.fetch_motion returns."""
    out = {name: np.ascontiguousarray(raw[name]) for name in ("block", "d", "cost", "cost0", "count_a", "count_b", "ties", "flags")}
    out["ijk"] = block_ijk(out["block"], grid, edge)
    out.update(grid=tuple(int(n) for n in grid), edge=int(edge), apron=int(apron), search=int(search))
    return out


def steps_mm(grid, bounds):
    """float64 [3]: the grid steps in mm (0 on an axis of one cell)."""
    return np.array([(float(bounds[2 * a + 1]) - float(bounds[2 * a])) / float(n - 1) if n > 1 else 0.0 for a, n in enumerate(grid)])


def describe(rows, grid, bounds, fps=None):
    """The field in world units.  Returns a dict: centre_mm float64 [L, 3], the centre of each listed block's b^3 cells;
    velocity_mm float64 [L, 3], d times the grid steps, per frame; speed_mm float64 [L]; with fps also velocity_mm_s and
    speed_mm_s; median_mm float64 [3], the component-wise median of velocity_mm over the blocks with ties == 1 (zeros when
    there is none)."""
    step = steps_mm(grid, bounds)
    edge = int(rows["edge"])
    lo = np.array([float(bounds[0]), float(bounds[2]), float(bounds[4])])
    centre = lo + (np.asarray(rows["ijk"], dtype=np.float64).reshape(-1, 3) * edge + 0.5 * (edge - 1)) * step
    vel = np.asarray(rows["d"], dtype=np.float64).reshape(-1, 3) * step
    out = {"centre_mm": centre, "velocity_mm": vel, "speed_mm": np.sqrt((vel * vel).sum(axis=1))}
    sure = np.asarray(rows["ties"]).reshape(-1) == 1
    out["median_mm"] = np.median(vel[sure], axis=0) if sure.any() else np.zeros(3)
    if fps is not None:
        out["velocity_mm_s"] = vel * float(fps)
        out["speed_mm_s"] = out["speed_mm"] * float(fps)
    return out


def figure_motion(rows, record_indices, labels, K):
    """Per figure the motion of its blocks.  record_indices: the records' linear voxel indices (u32 [S]); labels: their figures
    (cluster_hull's labels, [S], values >= K count for nobody).  A block belongs to the figure most of its records belong to;
    equal counts go to the smaller label.  Returns a dict: d float64 [K, 3], the component-wise median of d over the figure's
    blocks with ties == 1 (zeros for a figure without one), blocks int64 [K] (its listed blocks) and unique int64 [K] (those
    the median is taken over), owner int64 [L] (the figure of each row, -1 for none)."""
    K = int(K)
    nx, ny, _ = rows["grid"]
    edge = int(rows["edge"])
    nbx, nby, _ = block_dims(rows["grid"], edge)
    idx = np.asarray(record_indices, dtype=np.int64).reshape(-1)
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    if idx.shape != lab.shape:
        raise ValueError("figure_motion: %d indices and %d labels" % (idx.size, lab.size))
    iy, t = idx % ny, idx // ny
    k = ((t // nx) // edge * nbx + (t % nx) // edge) * nby + iy // edge
    block = np.asarray(rows["block"], dtype=np.int64).reshape(-1)
    L = block.size
    row_of = np.searchsorted(block, k)                           # (listed blocks ascend)
    ok = (lab >= 0) & (lab < K) & (row_of < L)
    ok[ok] = block[row_of[ok]] == k[ok]
    votes = np.zeros((L, max(K, 1)), dtype=np.int64)
    np.add.at(votes, (row_of[ok], lab[ok]), 1)
    owner = np.where(votes.sum(axis=1) > 0, votes.argmax(axis=1), -1)    # (argmax: the first, so the smaller label)
    d = np.asarray(rows["d"], dtype=np.float64).reshape(-1, 3)
    sure = np.asarray(rows["ties"]).reshape(-1) == 1
    out = {"d": np.zeros((K, 3)), "blocks": np.zeros(K, dtype=np.int64), "unique": np.zeros(K, dtype=np.int64), "owner": owner}
    for f in range(K):
        mine = owner == f
        out["blocks"][f] = int(mine.sum())
        out["unique"][f] = int((mine & sure).sum())
        if out["unique"][f]:
            out["d"][f] = np.median(d[mine & sure], axis=0)
    return out
