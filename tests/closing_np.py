"""Restatement of vc_hull_grow (include/voxcarve.h): dilation and closing of an occupancy volume by a
ball in um, and the records of the grown hull.  Built on tests/distance_np.py: a volume is a bool array occ[iz, ix, iy], q = (q_x,
q_y, q_z) the steps in micrometres, every distance an exact integer.  The border is open: nothing outside the grid is a site, and
the dilation is clipped to the grid.  Three forms of both sets:

  dilate_literal, close_literal   the definition: for each voxel a loop over all voxels, in Python integers (small grids)
  dilate, close_                  separable transforms over the whole grid
  dilate_box, close_box           the device's layout: the transforms run over the survivors' index box grown per axis by g_a + 1
                                  cells, g_a = isqrt(r2) // q_a, and clipped to the grid; voxels off the box keep their state
"""
import math
import os
import sys

import numpy as np

import distance_np as dn

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

NONE = dn.NONE


def _above(d, r2):
    """d > r2, with "no site" above every radius."""
    return (d > np.uint64(r2)) | (d == NONE)


# ---- literal --------------------------------------------------------------------------------------------------------------------
def _cells(shape):
    nz, nx, ny = shape
    return [(ix, iy, iz) for iz in range(nz) for ix in range(nx) for iy in range(ny)]


def _d2(v, w, q):
    return (q[0] * (v[0] - w[0])) ** 2 + (q[1] * (v[1] - w[1])) ** 2 + (q[2] * (v[2] - w[2])) ** 2


def dilate_literal(occ, q, r2):
    q = tuple(int(v) for v in q)
    on = [c for c in _cells(occ.shape) if occ[c[2], c[0], c[1]]]
    out = np.zeros(occ.shape, dtype=bool)
    for v in _cells(occ.shape):
        out[v[2], v[0], v[1]] = any(_d2(v, w, q) <= r2 for w in on)
    return out


def close_literal(occ, q, r2):
    q = tuple(int(v) for v in q)
    dl = dilate_literal(occ, q, r2)
    off = [c for c in _cells(occ.shape) if not dl[c[2], c[0], c[1]]]
    out = np.zeros(occ.shape, dtype=bool)
    for v in _cells(occ.shape):
        out[v[2], v[0], v[1]] = bool(dl[v[2], v[0], v[1]]) and all(_d2(v, u, q) > r2 for u in off)
    return out


def erode_grid_literal(occ, q, r2):
    """The adjoint of dilate_literal on the subsets of the grid: the voxels farther than r2 from every OFF voxel of the grid."""
    q = tuple(int(v) for v in q)
    off = [c for c in _cells(occ.shape) if not occ[c[2], c[0], c[1]]]
    out = np.zeros(occ.shape, dtype=bool)
    for v in _cells(occ.shape):
        out[v[2], v[0], v[1]] = bool(occ[v[2], v[0], v[1]]) and all(_d2(v, u, q) > r2 for u in off)
    return out


# ---- separable, whole grid ------------------------------------------------------------------------------------------------------
def dilate(occ, q, r2):
    """Dl = { v : min over ON w of d2(v, w) <= r2 }; empty for an empty hull."""
    if not occ.any():
        return np.zeros(occ.shape, dtype=bool)
    return dn.field(occ, q) <= np.uint64(r2)


def close_(occ, q, r2):
    """C = { v in Dl : min over u not in Dl of d2(v, u) > r2 }; returns (C, Dl)."""
    dl = dilate(occ, q, r2)
    if not dl.any():
        return dl.copy(), dl
    return dl & _above(dn.field(~dl, q), r2), dl


# ---- the device's box -----------------------------------------------------------------------------------------------------------
def reach(q, r2):
    """g_a = isqrt(r2) // q_a per axis x, y, z: the largest k with (k q_a)^2 <= r2."""
    root = math.isqrt(int(r2))
    return tuple(root // int(v) for v in q)


def grown_box(occ, q, r2, extra=1):
    """Slices (z, x, y) of the survivors' inclusive index box grown per axis by g_a + extra cells and clipped to the grid; None on
    an empty hull."""
    if not occ.any():
        return None
    g = reach(q, r2)
    ga = (g[2], g[0], g[1])                                      # the volume's axes: z, x, y
    sl = []
    for a in range(3):
        on = np.flatnonzero(occ.any(axis=tuple(b for b in range(3) if b != a)))
        sl.append(slice(max(int(on[0]) - ga[a] - extra, 0), min(int(on[-1]) + ga[a] + extra, occ.shape[a] - 1) + 1))
    return tuple(sl)


def dilate_box(occ, q, r2):
    out = occ.copy()
    sl = grown_box(occ, q, r2)
    if sl is None:
        return out
    out[sl] = dn.field(occ[sl], q) <= np.uint64(r2)
    return out


def close_box(occ, q, r2):
    """(C, Dl, box cells) with both transforms restricted to the grown box: the second one's sites are the BOX's cells outside Dl."""
    sl = grown_box(occ, q, r2)
    if sl is None:
        return occ.copy(), occ.copy(), 0
    dl_box = dn.field(occ[sl], q) <= np.uint64(r2)
    dl = np.zeros(occ.shape, dtype=bool)
    dl[sl] = dl_box
    c = np.zeros(occ.shape, dtype=bool)
    c[sl] = dl_box & _above(dn.field(~dl_box, q), r2)
    return c, dl, int(dl_box.size)


def box_cells(occ, q, r2):
    sl = grown_box(occ, q, r2)
    return 0 if sl is None else int(np.prod([s.stop - s.start for s in sl]))


def grow(occ, q, r2, op):
    """What the device leaves: (new occupancy, |Dl|, box cells), op = "dilate" | "close"."""
    if op == "dilate":
        d = dilate_box(occ, q, r2)
        return d, int(d.sum()), box_cells(occ, q, r2)
    if op != "close":
        raise ValueError("op %r, expected dilate or close" % (op,))
    c, dl, cells = close_box(occ, q, r2)
    return c, int(dl.sum()), cells


# ---- records ----------------------------------------------------------------------------------------------------------------------
def records_after(records, new_occ, grid, bounds, cam=None, frame=None, H=None, W=None):
    """The 8-byte records of the grown hull and their `added` bytes.  records: uint64 [S] of the hull before (ascending linear index
    in the low 32 bits), kept byte for byte.  A voxel of new_occ without one gets idx | r << 32 | g << 40 | b << 48 | seen << 56:
    the pixel of `frame` (uint8 [H, W, 3] BGR, or None: colour 0) under its centre when cam = (K, dist, R, tvec) projects the centre
    into the H x W image (oracle/carve_np.project_points, pixel_offsets), seen = 1; otherwise 0, 0, 0 and seen = 0, as with
    cam = None."""
    from oracle import carve_np as cnp
    nx, ny, nz = grid
    records = np.asarray(records, dtype=np.uint64)
    old_idx = (records & np.uint64(0xffffffff)).astype(np.int64)
    new_idx = np.flatnonzero(new_occ.reshape(-1)).astype(np.int64)
    is_old = np.isin(new_idx, old_idx)
    assert int(is_old.sum()) == old_idx.size, "the grown hull holds the hull"
    out = np.empty(new_idx.size, dtype=np.uint64)
    out[is_old] = records
    fresh = new_idx[~is_old]
    rec = fresh.astype(np.uint64)
    if cam is not None and fresh.size:
        K, dist, R, t = cam
        off = cnp.pixel_offsets(cnp.project_points(cnp.points_of_indices(fresh, nx, ny, nz, bounds), R, t, K, dist), H, W).astype(np.int64)
        ok = off >= 0
        upper = np.zeros(fresh.size, dtype=np.uint64)
        upper[ok] = np.uint64(1) << np.uint64(24)
        if frame is not None:
            bgr = np.asarray(frame).reshape(-1, 3)[off[ok]].astype(np.uint64)
            upper[ok] |= bgr[:, 2] | (bgr[:, 1] << np.uint64(8)) | (bgr[:, 0] << np.uint64(16))
        rec = rec | (upper << np.uint64(32))
    out[~is_old] = rec
    return out, (~is_old).astype(np.uint8)

