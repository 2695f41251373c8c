"""Hulls as operands of the set algebra (CarveEngine.upload_hull, combine_hull, compare_hull) and as files: pure host code.

A hull of a grid of n voxels is given as one of
  bool [n]      occupancy in linear index i = (iz nx + ix) ny + iy,
  uint32 [S]    ascending unique linear indices,
  uint64 [S]    records: index in the low 32 bits, R | G << 8 | B << 16 | seen << 24 in the high 32, ascending index.
The first two carry no colours: voxels they add to a result are coloured from the carve's colour camera."""
import numpy as np


def _ascending(idx, n, what):
    if idx.size and int(idx.max()) >= n:
        raise ValueError("%s: index %d at or beyond the grid's %d voxels" % (what, int(idx.max()), n))
    if idx.size > 1 and not np.all(idx[1:] > idx[:-1]):
        raise ValueError("%s: the indices are not strictly ascending (descending or duplicate entries)" % what)


def as_operand(hull, n):
    """("bits", uint8 [8 ceil(n / 64)]) laid out as CarveEngine.fetch_occupancy's words, or ("records", uint64 [S]).
    ValueError for a bool array of another size, descending or duplicate indices, an index at or beyond n, another dtype."""
    n = int(n)
    a = np.asarray(hull)
    if a.dtype == np.bool_:
        if a.size != n:
            raise ValueError("a bool hull of %d elements for a grid of %d voxels" % (a.size, n))
        bits = np.zeros(((n + 63) // 64) * 8, dtype=np.uint8)
        packed = np.packbits(a.reshape(-1), bitorder="little")
        bits[:packed.size] = packed
        return "bits", bits
    if a.ndim != 1:
        raise ValueError("a hull of indices or records is one-dimensional, got shape %s" % (a.shape,))
    if a.dtype == np.uint32:
        _ascending(a, n, "uint32 hull")
        occ = np.zeros(n, dtype=bool)
        occ[a] = True
        return as_operand(occ, n)
    if a.dtype == np.uint64:
        _ascending(a & np.uint64(0xffffffff), n, "uint64 hull")
        return "records", np.ascontiguousarray(a)
    raise ValueError("a hull is a bool, uint32 or uint64 array, got %s" % a.dtype)


def save(path, grid, bounds, records):
    """Writes a reconstruction: the grid (nx, ny, nz), its bounds (6 floats, mm) and the u64 records, as an .npz."""
    grid = np.asarray(grid, dtype=np.int64).reshape(3)
    bounds = np.asarray(bounds, dtype=np.float64).reshape(6)
    records = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1)
    as_operand(records, int(grid.prod()))
    with open(path, "wb") as f:                                  # (a file object: numpy appends no suffix)
        np.savez(f, grid=grid, bounds=bounds, records=records)


def load(path):
    """(grid tuple of 3 ints, bounds tuple of 6 floats, records uint64 [S]) as save wrote them."""
    with np.load(path) as z:
        grid = tuple(int(v) for v in z["grid"])
        bounds = tuple(float(v) for v in z["bounds"])
        records = z["records"].astype(np.uint64)
    as_operand(records, grid[0] * grid[1] * grid[2])
    return grid, bounds, records
