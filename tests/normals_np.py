"""Restatement of vc_hull_normals, vc_shade_render and vc_surface_normals (include/voxcarve.h): the
surface normal of each record of a hull from the occupancy inside a ball in micrometres, in signed 64-bit integers, and the
float64 shading of a render with it.  A volume is a bool array occ[iz, ix, iy] (linear index i = (iz nx + ix) ny + iy, the
grid's order); q = (q_x, q_y, q_z) are the steps in micrometres (distance_np.steps_um).  Two forms of the normals:

  normals_literal(occ, q, r2)   the definition: per surface voxel, per offset of the ball, in Python integers (small grids).
  normals(occ, q, r2)           vectorised over the surface voxels in int64, one offset at a time.

Both return (n4, stats): n4 int16 [S, 4] in record order (ascending linear index), stats a dict with survivors, surface, zero,
offsets, ext and q."""
import math

import numpy as np

EXT_MAX = 15


def ball(q, r2):
    """(ext, offsets): ext_a = the largest k with (k q_a)^2 <= r2; offsets int64 [K, 3] = the (dx, dy, dz) != 0 with
    (q_x dx)^2 + (q_y dy)^2 + (q_z dz)^2 <= r2.  ValueError where the library refuses: an empty ball, some ext_a > 15."""
    q = [int(v) for v in q]
    r2 = int(r2)
    if r2 < 0:
        raise ValueError("r2 < 0")
    ext = [math.isqrt(r2) // v for v in q]
    if max(ext) == 0:
        raise ValueError("the ball of r2 = %d holds no offset" % r2)
    if max(ext) > EXT_MAX:
        raise ValueError("ext %r above %d" % (ext, EXT_MAX))
    offs = [(dx, dy, dz)
            for dz in range(-ext[2], ext[2] + 1) for dx in range(-ext[0], ext[0] + 1) for dy in range(-ext[1], ext[1] + 1)
            if (dx, dy, dz) != (0, 0, 0) and (q[0] * dx) ** 2 + (q[1] * dy) ** 2 + (q[2] * dz) ** 2 <= r2]
    return tuple(ext), np.array(offs, dtype=np.int64).reshape(-1, 3)


def surface_mask(occ):
    """bool, occ's shape: ON and one of the 6 face neighbours OFF or outside the grid."""
    p = np.pad(occ, 1, constant_values=False)
    c = p[1:-1, 1:-1, 1:-1]
    inner = p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]
    return c & ~inner


def _tdiv(a, b):
    """a / b truncated toward zero, as C divides (b > 0)."""
    return -((-a) // b) if a < 0 else a // b


def store_literal(n):
    """The stored quadruple of a surface record with normal n (Python ints)."""
    m = max(abs(v) for v in n)
    if m == 0:
        return (0, 0, 0, 1)
    return tuple(_tdiv(v * 32767, m) for v in n) + (1,)


def _stats(occ, q, ext, offs, n4, surf_flat):
    return {"survivors": int(occ.sum()), "surface": int(surf_flat.sum()),
            "zero": int((surf_flat & ~n4[:, :3].any(axis=1)).sum()), "offsets": int(len(offs)), "ext": tuple(ext),
            "q": tuple(int(v) for v in q)}


def normals_literal(occ, q, r2):
    ext, offs = ball(q, r2)
    nz, nx, ny = occ.shape
    qx, qy, qz = (int(v) for v in q)
    surf = surface_mask(occ)
    out, sflags = [], []
    for iz in range(nz):
        for ix in range(nx):
            for iy in range(ny):
                if not occ[iz, ix, iy]:
                    continue
                sflags.append(bool(surf[iz, ix, iy]))
                if not surf[iz, ix, iy]:
                    out.append((0, 0, 0, 0))
                    continue
                g = [0, 0, 0]
                for dx, dy, dz in offs.tolist():
                    x, y, z = ix + dx, iy + dy, iz + dz
                    if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and occ[z, x, y]:
                        g[0] += qx * dx
                        g[1] += qy * dy
                        g[2] += qz * dz
                out.append(store_literal([-g[0], -g[1], -g[2]]))
    n4 = np.array(out, dtype=np.int16).reshape(-1, 4)
    return n4, _stats(occ, q, ext, offs, n4, np.array(sflags, dtype=bool))


def normals(occ, q, r2):
    ext, offs = ball(q, r2)
    occ = np.ascontiguousarray(occ, dtype=bool)
    qv = np.array([int(v) for v in q], dtype=np.int64)
    on = np.flatnonzero(occ.reshape(-1))
    surf_flat = surface_mask(occ).reshape(-1)[on]
    n4 = np.zeros((len(on), 4), dtype=np.int16)
    if surf_flat.any():
        e = max(ext)
        pad = np.pad(occ, e, constant_values=False)
        iz, ix, iy = np.unravel_index(on[surf_flat], occ.shape)
        g = np.zeros((len(iz), 3), dtype=np.int64)
        for dx, dy, dz in offs.tolist():
            hit = pad[iz + (e + dz), ix + (e + dx), iy + (e + dy)].astype(np.int64)
            g[:, 0] += hit * dx
            g[:, 1] += hit * dy
            g[:, 2] += hit * dz
        n = -(g * qv[None, :])
        m = np.abs(n).max(axis=1)
        safe = np.where(m == 0, 1, m)[:, None]
        n16 = np.sign(n) * ((np.abs(n) * 32767) // safe)          # toward zero: floor of the magnitudes
        rows = np.concatenate([n16, np.ones((len(n16), 1), dtype=np.int64)], axis=1)
        n4[surf_flat] = rows.astype(np.int16)
    return n4, _stats(occ, q, ext, offs, n4, surf_flat)


def face_normals(occ, q):
    """The cube-face estimate, float64 [S, 3] in record order: minus the sum of q_a d_a over the 6 face neighbours that are ON."""
    occ = np.ascontiguousarray(occ, dtype=bool)
    pad = np.pad(occ, 1, constant_values=False)
    iz, ix, iy = np.nonzero(occ)
    g = np.zeros((len(iz), 3), dtype=np.int64)
    for a, (dx, dy, dz) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        for sgn in (1, -1):
            hit = pad[iz + 1 + sgn * dz, ix + 1 + sgn * dx, iy + 1 + sgn * dy].astype(np.int64)
            g[:, a] += hit * sgn * int(q[a])
    return -g.astype(np.float64)


def unit(n4):
    """float64 [S, 3] unit vectors; rows with a zero normal stay zero."""
    v = np.asarray(n4)[:, :3].astype(np.float64)
    l = np.sqrt((v * v).sum(axis=1))
    return v / np.where(l == 0.0, 1.0, l)[:, None]


def default_r2(q):
    """(3 x the largest step)^2 in um^2."""
    return (3 * max(int(v) for v in q)) ** 2


def shade(idx, flat_rgb, rec_idx, rec_rgb, n4, light, ambient):
    """vc_shade_render for one view: idx uint32 [H, W] and flat_rgb uint8 [H, W, 3] of the render, the records' indices
    (ascending) and RGB, their stored normals, the light (3 float64) and ambient 0..255 -> uint8 [H, W, 3]."""
    out = np.array(flat_rgb, dtype=np.uint8, copy=True)
    hit = idx != 0xFFFFFFFF
    if not hit.any() or len(rec_idx) == 0:
        return out
    pos = np.searchsorted(rec_idx, idx[hit])
    pos = np.minimum(pos, len(rec_idx) - 1)
    n = n4[pos].astype(np.int64)
    has = (n[:, 3] != 0) & n[:, :3].any(axis=1)
    L = np.asarray(light, dtype=np.float64)
    nf = n[:, :3].astype(np.float64)
    dot = (nf[:, 0] * L[0] + nf[:, 1] * L[1]) + nf[:, 2] * L[2]
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]).astype(np.float64)
    ll = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(dot > 0.0, np.minimum(dot / np.sqrt(nn * ll), 1.0), 0.0)
    c = np.where(has, c, 0.0)
    s = int(ambient) + np.floor(np.float64(255 - int(ambient)) * c + 0.5).astype(np.int64)
    rgb = (rec_rgb[pos].astype(np.int64) * s[:, None] + 127) // 255
    cur = out[hit]
    cur[has] = rgb[has].astype(np.uint8)
    out[hit] = cur
    return out
