"""Restatement of the silhouette-refined surface mesh (vc_surface_mesh, include/voxcarve.h).

TEST INFRASTRUCTURE ONLY.  Two forms of one contract: `refine` (vectorised over the vertices) and `refine_literal` (vertex by
vertex, step by step, camera by camera in plain Python floats, the operation order of csrc/vc_device.h).

Inputs: the occupancy as bool [n] over the voxel index i = (iz nx + ix) ny + iy (the volume viewed as (nz, nx, ny)), the grid
(nx, ny, nz), bounds, cameras as (K, dist, R, tvec), the masks the carve read as bool [C, H, W] (after its post-filter), m (the
carve's min_views after the clamp to >= 1), steps.  Vertices come in marching-cubes order (oracle/marching_np.py): per word of 64
elements, the crossings along axis 0 in element order, then axis 1, then axis 2; an edge belongs to its lower element.
"""
import numpy as np

from oracle import marching_np
from oracle.carve_np import axis_tables, pixel_offsets, project_points


def mesh_edges(occ, grid):
    """(e int64 [V] lower element, axis int64 [V] in (nz, nx, ny) axes, on_low bool [V]) in vertex order."""
    nx, ny, nz = grid
    flat = np.asarray(occ, dtype=bool).reshape(-1)
    n = flat.size
    assert n == nx * ny * nz
    d0, d1, d2 = nz, nx, ny
    idx = np.arange(n, dtype=np.int64)
    a, b, c = idx // (d1 * d2), (idx // d2) % d1, idx % d2
    strides = (d1 * d2, d2, 1)
    limits = (a < d0 - 1, b < d1 - 1, c < d2 - 1)
    es, axes = [], []
    for axis in range(3):
        lo = idx[limits[axis]]
        cr = lo[flat[lo] != flat[lo + strides[axis]]]
        es.append(cr)
        axes.append(np.full(cr.size, axis, np.int64))
    e, axis = np.concatenate(es), np.concatenate(axes)
    order = np.lexsort((e % 64, axis, e // 64))
    e, axis = e[order], axis[order]
    return e, axis, flat[e]


def edges_from_grid_verts(verts):
    """The edges of marching_cubes(axes="grid", level=0.25) vertices ((iz, ix, iy) index coordinates, float32): the axis is the
    coordinate with a fractional part, 0.75 = the lower element is ON, 0.25 = it is OFF.  Returns (lower (iz, ix, iy) int64
    [V, 3], axis, on_low)."""
    v = np.asarray(verts, dtype=np.float64)
    fl = np.floor(v)
    frac = v - fl
    axis = np.argmax(frac, axis=1)
    f = frac[np.arange(v.shape[0]), axis]
    assert np.all((f == 0.25) | (f == 0.75)) and np.count_nonzero(frac, axis=1).max(initial=1) == 1
    return fl.astype(np.int64), axis.astype(np.int64), f == 0.75


def _endpoints(e, axis, on_low, grid, bounds):
    """base [V, 3] world centre of the lower element, wa [V] world axis of the edge, a_on / a_off [V] its two coordinates."""
    nx, ny, nz = grid
    xs, ys, zs = axis_tables(nx, ny, nz, bounds)
    e = np.asarray(e, dtype=np.int64)
    iy, t = e % ny, e // ny
    ix, iz = t % nx, t // nx
    base = np.stack([xs[ix], ys[iy], zs[iz]], axis=1)
    axis = np.asarray(axis, dtype=np.int64)
    wa = np.where(axis == 0, 2, axis - 1)
    upper = np.where(wa == 0, xs[np.minimum(ix + 1, nx - 1)], np.where(wa == 1, ys[np.minimum(iy + 1, ny - 1)],
                                                                       zs[np.minimum(iz + 1, nz - 1)]))
    lower = base[np.arange(e.size), wa]
    on_low = np.asarray(on_low, dtype=bool)
    return base, wa, np.where(on_low, lower, upper), np.where(on_low, upper, lower)


def _at(base, wa, vals):
    P = base.copy()
    P[np.arange(base.shape[0]), wa] = vals
    return P


def count_views(P, cams, masks):
    """T(P) for points P [N, 3]: the cameras whose mask holds the pixel P projects to."""
    masks = np.asarray(masks, dtype=bool)
    C, H, W = masks.shape
    T = np.zeros(P.shape[0], dtype=np.int64)
    for c, (K, dist, R, tv) in enumerate(cams):
        off = pixel_offsets(project_points(P, R, tv, K, dist), H, W)
        ok = off >= 0
        hit = np.zeros(P.shape[0], dtype=bool)
        hit[ok] = masks[c].reshape(-1)[off[ok]]
        T += hit
    return T


def refine(occ, grid, bounds, cams, masks, m, steps, edges=None, with_interval=False):
    """Vectorised form -> dict verts f64 [V, 3], s f64 [V], refined bool [V], e, axis, on_low (and lo, hi when asked)."""
    e, axis, on_low = mesh_edges(occ, grid) if edges is None else edges
    base, wa, a_on, a_off = _endpoints(e, axis, on_low, grid, bounds)
    d = a_off - a_on
    V = base.shape[0]
    inside = lambda vals: count_views(_at(base, wa, vals), cams, masks) >= m
    refined = inside(a_on) & ~inside(a_off) if V else np.zeros(0, bool)
    lo, hi = np.zeros(V), np.ones(V)
    r = np.nonzero(refined)[0]
    for _ in range(steps):
        if r.size == 0:
            break
        mid = (lo[r] + hi[r]) * 0.5
        ins = count_views(_at(base[r], wa[r], a_on[r] + mid * d[r]), cams, masks) >= m
        lo[r] = np.where(ins, mid, lo[r])
        hi[r] = np.where(ins, hi[r], mid)
    s = np.where(refined, (lo + hi) * 0.5, 0.5)
    out = {"verts": _at(base, wa, a_on + s * d), "s": s, "refined": refined, "e": e, "axis": axis, "on_low": on_low}
    if with_interval:
        out["lo"], out["hi"] = lo, hi
        out["base"], out["wa"], out["a_on"], out["a_off"] = base, wa, a_on, a_off
    return out


# ---------------------------------------------------------------------------------------------------------------- literal form
def _project_literal(cam, X, Y, Z):
    K, dist, R, tv = cam
    R = np.asarray(R, dtype=np.float64).reshape(9).tolist()
    t = np.asarray(tv, dtype=np.float64).reshape(3).tolist()
    K = np.asarray(K, dtype=np.float64).reshape(9).tolist()
    k1, k2, p1, p2, k3 = np.asarray(dist, dtype=np.float64).reshape(5).tolist()
    x = R[0] * X + R[1] * Y + R[2] * Z + t[0]
    y = R[3] * X + R[4] * Y + R[5] * Z + t[1]
    z = R[6] * X + R[7] * Y + R[8] * Z + t[2]
    z = 1.0 / z if z != 0.0 else 1.0
    x = x * z
    y = y * z
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    tx, ty = 2 * x, 2 * y
    a1 = tx * y
    a2 = r2 + tx * x
    a3 = r2 + ty * y
    cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6
    xd = x * cdist + p1 * a1 + p2 * a2
    yd = y * cdist + p1 * a3 + p2 * a1
    return xd * K[0] + K[2], yd * K[4] + K[5]


def _inside_literal(cams, masks, m, P):
    C, H, W = masks.shape
    T = 0
    for c in range(C):
        try:
            u, v = _project_literal(cams[c], *P)
        except (OverflowError, ZeroDivisionError):
            continue
        if not (u >= 0.0 and u < W and v >= 0.0 and v < H):
            continue
        if masks[c, int(v), int(u)]:
            T += 1
    return T >= m


def refine_literal(occ, grid, bounds, cams, masks, m, steps, vertices=None):
    """Vertex by vertex (all, or the listed vertex numbers) -> (verts f64 [k, 3], refined bool [k])."""
    nx, ny, nz = grid
    xs, ys, zs = (a.tolist() for a in axis_tables(nx, ny, nz, bounds))
    masks = np.asarray(masks, dtype=bool)
    flat = np.asarray(occ, dtype=bool).reshape(-1)
    e_all, axis_all, _ = mesh_edges(flat, grid)
    sel = range(e_all.size) if vertices is None else vertices
    verts, refined = [], []
    for k in sel:
        e, axis = int(e_all[k]), int(axis_all[k])
        iy, ix, iz = e % ny, (e // ny) % nx, e // (nx * ny)
        stride = (nx * ny, ny, 1)[axis]
        lo_el, hi_el = e, e + stride
        on_el, off_el = (lo_el, hi_el) if flat[lo_el] else (hi_el, lo_el)
        assert flat[on_el] and not flat[off_el]

        def centre(el):
            return [xs[(el // ny) % nx], ys[el % ny], zs[el // (nx * ny)]]
        P_on, P_off = centre(on_el), centre(off_el)
        wa = (2, 0, 1)[axis]
        assert [P_on[j] == P_off[j] for j in range(3)] == [j != wa for j in range(3)]

        def P(s):
            if s == 0.0:
                return P_on
            if s == 1.0:
                return P_off
            q = list(P_on)
            q[wa] = P_on[wa] + s * (P_off[wa] - P_on[wa])
            return q
        ref = _inside_literal(cams, masks, m, P(0.0)) and not _inside_literal(cams, masks, m, P(1.0))
        s = 0.5
        if ref:
            lo, hi = 0.0, 1.0
            for _ in range(steps):
                mid = (lo + hi) * 0.5
                if _inside_literal(cams, masks, m, P(mid)):
                    lo = mid
                else:
                    hi = mid
            s = (lo + hi) * 0.5
        verts.append(P(s))
        refined.append(ref)
    return np.array(verts, dtype=np.float64).reshape(-1, 3), np.array(refined, dtype=bool)


# -------------------------------------------------------------------------------------------------------------- the whole mesh
def colours(idx, rgb, e, axis, on_low, grid):
    """u8 [V, 3]: the RGB of each vertex's ON element's record (idx ascending)."""
    nx, ny, _ = grid
    stride = np.array([nx * ny, ny, 1], dtype=np.int64)[np.asarray(axis, dtype=np.int64)]
    on = np.where(on_low, e, e + stride)
    idx = np.asarray(idx, dtype=np.int64)
    pos = np.searchsorted(idx, on)
    assert np.all(pos < idx.size) and np.array_equal(idx[pos], on)
    return np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)[pos]


def surface_mesh(occ, idx, rgb, grid, bounds, cams, masks, m, steps, faces=True):
    """The whole contract -> dict verts, faces (None unless asked: marching_np.extract is a Python loop), rgb, refined, stats."""
    nx, ny, nz = grid
    r = refine(occ, grid, bounds, cams, masks, m, steps)
    out = {"verts": r["verts"], "refined": r["refined"], "rgb": colours(idx, rgb, r["e"], r["axis"], r["on_low"], grid), "faces": None}
    if faces:
        out["faces"] = marching_np.extract(np.asarray(occ, dtype=bool).reshape(nz, nx, ny))[1]
    V = r["verts"].shape[0]
    out["stats"] = {"n_verts": V, "refined": int(r["refined"].sum()), "unrefined": V - int(r["refined"].sum())}
    return out


def signed_volume(verts, faces):
    return marching_np.mesh_invariants(verts, faces)[3]
