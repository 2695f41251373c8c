"""Restatement of vc_hull_distance and vc_hull_morphology (include/voxcarve.h): the exact squared
Euclidean distance transform of an occupancy volume in um^2, erosion and opening by a ball.  A volume is a bool array
occ[iz, ix, iy] (linear index i = (iz nx + ix) ny + iy, the grid's order); q = (q_x, q_y, q_z) are the steps in micrometres.
Two forms of every field:

  *_literal(occ, q, ...)   the definition: for each voxel the minimum over all sites, one site at a time, in Python integers
                           (small grids).
  inside, outside, ...     separable: one min-plus pass per axis, out[x] = min_i g[i] + q_a^2 (x - i)^2, vectorised over the other
                           two axes in int64 (every value stays below 2^63, see INF).

Fields are uint64 arrays of occ's shape; "no site at all" is NONE = 2^64 - 1.  border = "open" | "off": with "off" one virtual OFF
layer surrounds the grid -- the positions with exactly one coordinate equal to -1 or n_a.  The separable form pads the volume with
OFF on every side instead, which adds that layer's edges and corners; they are never nearer than a face position (the test of
vectorised == literal covers it)."""
import numpy as np

NONE = np.uint64(0xffffffffffffffff)
INF = np.int64(1) << np.int64(62)           # above every real d2 (< 2^62); INF + q_a^2 m^2 <= 2^62 + 2^60 still fits int64
BORDERS = ("open", "off")


def steps_um(grid, bounds):
    """q = (q_x, q_y, q_z): per axis llrint(((max - min) / (n - 1)) * 1000.0), the library's refusals as ValueError."""
    q = []
    for a, n in enumerate(grid):
        if n < 2:
            raise ValueError("axis %d has %d cells" % (a, n))
        s = (float(bounds[2 * a + 1]) - float(bounds[2 * a])) / float(n - 1)
        v = int(np.rint(s * 1000.0))
        if not 1 <= v <= 1 << 20 or (n + 1) * v > 1 << 30:
            raise ValueError("axis %d: step %r um out of range" % (a, v))
        q.append(v)
    return tuple(q)


def volume(idx, grid):
    """bool [nz, nx, ny] from a list of linear indices."""
    nx, ny, nz = grid
    occ = np.zeros(nx * ny * nz, dtype=bool)
    occ[np.asarray(idx, dtype=np.int64)] = True
    return occ.reshape(nz, nx, ny)


def indices(occ):
    return np.flatnonzero(occ.reshape(-1)).astype(np.uint32)


def _check_border(border):
    if border not in BORDERS:
        raise ValueError("border %r, expected one of %s" % (border, BORDERS))


# ---- literal --------------------------------------------------------------------------------------------------------------------
def _sites_literal(occ, border, on):
    nz, nx, ny = occ.shape
    sites = [(ix, iy, iz) for iz in range(nz) for ix in range(nx) for iy in range(ny) if bool(occ[iz, ix, iy]) == on]
    if border == "off" and not on:
        for iz in range(nz):
            for ix in range(nx):
                sites += [(ix, -1, iz), (ix, ny, iz)]
        for iz in range(nz):
            for iy in range(ny):
                sites += [(-1, iy, iz), (nx, iy, iz)]
        for ix in range(nx):
            for iy in range(ny):
                sites += [(ix, iy, -1), (ix, iy, nz)]
    return sites


def _field_literal(shape, sites, q):
    nz, nx, ny = shape
    qx, qy, qz = (int(v) for v in q)
    out = np.empty(shape, dtype=np.uint64)
    for iz in range(nz):
        for ix in range(nx):
            for iy in range(ny):
                best = None
                for wx, wy, wz in sites:
                    d = (qx * (ix - wx)) ** 2 + (qy * (iy - wy)) ** 2 + (qz * (iz - wz)) ** 2
                    if best is None or d < best:
                        best = d
                out[iz, ix, iy] = NONE if best is None else best
    return out


def inside_literal(occ, q, border="open"):
    _check_border(border)
    return _field_literal(occ.shape, _sites_literal(occ, border, False), q)


def outside_literal(occ, q):
    return _field_literal(occ.shape, _sites_literal(occ, "open", True), q)


def erode_literal(occ, q, r2, border="open"):
    return occ & (inside_literal(occ, q, border) > np.uint64(r2))


def open_literal(occ, q, r2, border="open"):
    e = erode_literal(occ, q, r2, border)
    d = _field_literal(occ.shape, _sites_literal(e, "open", True), q)
    return occ & (d != NONE) & (d <= np.uint64(r2))


# ---- separable ------------------------------------------------------------------------------------------------------------------
def _pass(g, axis, w):
    """out[.., x, ..] = min over i of g[.., i, ..] + w (x - i)^2 along `axis` (int64; INF stays >= INF)."""
    g = np.moveaxis(g, axis, 0)
    m = g.shape[0]
    x = np.arange(m, dtype=np.int64).reshape((m,) + (1,) * (g.ndim - 1))
    out = np.full(g.shape, np.iinfo(np.int64).max, dtype=np.int64)
    for i in range(m):
        if (g[i] >= INF).all():
            continue
        np.minimum(out, g[i][None] + np.int64(w) * (x - i) ** 2, out=out)
    np.minimum(out, INF, out=out)
    return np.moveaxis(out, 0, axis)


def field(sites, q):
    """Squared distance of every cell of the bool volume sites[iz, ix, iy] to its nearest True cell; NONE when there is none."""
    qx, qy, qz = (int(v) for v in q)
    g = np.where(sites, np.int64(0), INF)
    g = _pass(g, 2, qy * qy)
    g = _pass(g, 1, qx * qx)
    g = _pass(g, 0, qz * qz)
    out = g.astype(np.uint64)
    out[g >= INF] = NONE
    return out


def inside(occ, q, border="open"):
    """D_in over the whole grid."""
    _check_border(border)
    if border == "off":
        return field(np.pad(~occ, 1, constant_values=True), q)[1:-1, 1:-1, 1:-1]
    return field(~occ, q)


def hull_box(occ, border="open"):
    """The slices (z, x, y) of the survivors' inclusive index box grown by one cell per side and clipped to the grid, and per
    axis whether the unclipped box reaches below 0 / beyond n - 1 (where the "off" layer counts); None on an empty hull."""
    if not occ.any():
        return None
    sl, lo_out, hi_out = [], [], []
    for a in range(3):
        on = np.flatnonzero(occ.any(axis=tuple(b for b in range(3) if b != a)))
        lo, hi = int(on[0]) - 1, int(on[-1]) + 1
        lo_out.append(lo < 0)
        hi_out.append(hi > occ.shape[a] - 1)
        sl.append(slice(max(lo, 0), min(hi, occ.shape[a] - 1) + 1))
    return tuple(sl), lo_out, hi_out


def inside_box(occ, q, border="open"):
    """D_in computed on the hull's box alone (the device's layout): equal to inside() everywhere -- zero off the box."""
    _check_border(border)
    out = np.zeros(occ.shape, dtype=np.uint64)
    hb = hull_box(occ, border)
    if hb is None:
        return out
    sl, lo_out, hi_out = hb
    sites = ~occ[sl]
    if border == "off":
        pad = [(1 if lo_out[a] else 0, 1 if hi_out[a] else 0) for a in range(3)]
        f = field(np.pad(sites, pad, constant_values=True), q)
        f = f[tuple(slice(p[0], f.shape[a] - p[1]) for a, p in enumerate(pad))]
    else:
        f = field(sites, q)
    out[sl] = f
    return out


def outside(occ, q):
    """D_out over the whole grid (the border never contributes)."""
    return field(occ, q)


def erode(occ, q, r2, border="open"):
    """E = { v ON : D_in(v) > r2 }."""
    return occ & (inside_box(occ, q, border) > np.uint64(r2))


def open_(occ, q, r2, border="open"):
    """O = { v ON : min over e in E of d2(v, e) <= r2 }; returns (O, E)."""
    e = erode(occ, q, r2, border)
    out = np.zeros(occ.shape, dtype=bool)
    hb = hull_box(occ)
    if hb is None or not e.any():
        return out, e
    sl = hb[0]
    d = field(e[sl], q)
    out[sl] = occ[sl] & (d != NONE) & (d <= np.uint64(r2))
    return out, e


def radius_r2(radius_mm):
    """r2 of CarveEngine.erode_hull / open_hull: round(radius_mm * 1000) squared, um^2."""
    r = int(round(float(radius_mm) * 1000.0))
    return r * r


def depth_mm(d2):
    return np.sqrt(np.asarray(d2).astype(np.float64)) / 1000
