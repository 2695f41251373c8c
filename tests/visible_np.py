"""Restatement of occlusion-aware colouring (vc_color_visible, include/voxcarve.h).

TEST INFRASTRUCTURE ONLY.  Two forms of one contract: `color_visible` (vectorised) and `color_visible_literal` (one voxel,
one camera, one pixel at a time).  Projection is oracle/carve_np.project_points (float64, op order, no contraction).

Inputs: the survivors' ascending linear indices `idx` (i = iz*nx*ny + ix*ny + iy) and their RGB (what the carve left in
the records, the colour camera's samples), grid (nx, ny, nz), bounds, cameras as (K, dist, R, tvec), every camera's BGR
frame [H, W, 3].  Outputs: depth maps u32 [C, H*W] (float32 bits), camera masks u16 [S], RGB u8 [S, 3].
"""
import math

import numpy as np

from oracle.carve_np import axis_tables, project_points

INF_BITS = np.uint32(0x7f800000)
_SIGNS = [(sx, sy, sz) for sz in (-1, 1) for sx in (-1, 1) for sy in (-1, 1)]


def half_extents(grid, bounds):
    """(hx, hy, hz): half the linspace step of each axis, 0 on an axis with one voxel."""
    out = []
    for a in range(3):
        n, lo, hi = grid[a], bounds[2 * a], bounds[2 * a + 1]
        out.append(((hi - lo) / (n - 1)) / 2 if n > 1 else 0.0)
    return tuple(out)


def default_tolerance(grid, bounds):
    """The voxel diagonal as float32 (CarveEngine.color_visible's default)."""
    hx, hy, hz = half_extents(grid, bounds)
    return float(np.float32(math.sqrt((2 * hx) ** 2 + (2 * hy) ** 2 + (2 * hz) ** 2)))


def surface(idx, grid):
    """bool [S]: survivors with at least one face neighbour that is not a survivor or lies outside the grid."""
    nx, ny, nz = grid
    occ = np.zeros((nz + 2, nx + 2, ny + 2), dtype=bool)
    idx = np.asarray(idx, dtype=np.int64)
    iy, t = idx % ny, idx // ny
    ix, iz = t % nx, t // nx
    occ[iz + 1, ix + 1, iy + 1] = True
    inner = np.ones(idx.shape, dtype=bool)
    for dz, dx, dy in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        inner &= occ[iz + 1 + dz, ix + 1 + dx, iy + 1 + dy]
    return ~inner


def _cam_z(R, t, P):
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    return R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1] + R[2, 2] * P[:, 2] + t[2]


def _f32_bits(d):
    return np.asarray(d, dtype=np.float64).astype(np.float32).view(np.uint32)


def _frame_rgb(frame):
    f = np.asarray(frame, dtype=np.uint8)
    return f.reshape(-1, 3)[:, ::-1].astype(np.int64)        # BGR -> RGB per pixel


def color_visible(idx, rgb, grid, bounds, cams, frames, H, W, tol=None):
    """Vectorised form.  Returns (zmaps u32 [C, H*W], vis u16 [S], rgb u8 [S, 3])."""
    nx, ny, nz = grid
    idx = np.asarray(idx, dtype=np.int64)
    S, C = idx.size, len(cams)
    tol = np.float32(default_tolerance(grid, bounds) if tol is None else tol)
    zmaps = np.full((C, H * W), INF_BITS, dtype=np.uint32)
    vis = np.zeros(S, dtype=np.uint16)
    out = np.array(rgb, dtype=np.uint8).reshape(S, 3).copy()
    if S == 0:
        return zmaps, vis, out
    xs, ys, zs = axis_tables(nx, ny, nz, bounds)
    hx, hy, hz = half_extents(grid, bounds)
    iy, t = idx % ny, idx // ny
    ix, iz = t % nx, t // nx
    surf = np.nonzero(surface(idx, grid))[0]
    cx, cy, cz = xs[ix[surf]], ys[iy[surf]], zs[iz[surf]]
    centre = np.stack([cx, cy, cz], axis=1)
    corners = np.concatenate([np.stack([cx + hx if sx > 0 else cx - hx, cy + hy if sy > 0 else cy - hy,
                                        cz + hz if sz > 0 else cz - hz], axis=1) for sx, sy, sz in _SIGNS])   # [8 Ns, 3]
    Ns = surf.size
    acc = np.zeros((Ns, 3), dtype=np.int64)
    cnt = np.zeros(Ns, dtype=np.int64)
    with np.errstate(all="ignore"):
        for c, (K, dist, R, tv) in enumerate(cams):
            d = _cam_z(R, tv, centre)
            ok = (d > 0) & (_cam_z(R, tv, corners).reshape(8, Ns) > 0).all(axis=0)
            uv = project_points(corners, R, tv, K, dist).reshape(8, Ns, 2)
            umin, umax = uv[..., 0].min(axis=0), uv[..., 0].max(axis=0)
            vmin, vmax = uv[..., 1].min(axis=0), uv[..., 1].max(axis=0)
            ok &= np.isfinite(uv).all(axis=(0, 2))
            x0 = np.maximum(np.floor(umin), 0.0)
            x1 = np.minimum(np.floor(umax), W - 1.0)
            y0 = np.maximum(np.floor(vmin), 0.0)
            y1 = np.minimum(np.floor(vmax), H - 1.0)
            ok &= (x0 <= x1) & (y0 <= y1)
            key = _f32_bits(d)
            z = zmaps[c]
            k = np.nonzero(ok)[0]
            x0, x1, y0, y1 = (a[k].astype(np.int64) for a in (x0, x1, y0, y1))
            w, h = x1 - x0 + 1, y1 - y0 + 1
            small = (w <= 8) & (h <= 8)
            for dy in range(8):                                  # small rectangles: all at once, one offset at a time
                for dx in range(8):
                    m = small & (dy < h) & (dx < w)
                    if m.any():
                        np.minimum.at(z, (y0[m] + dy) * W + x0[m] + dx, key[k[m]])
            z2 = z.reshape(H, W)
            for j in np.nonzero(~small)[0]:                      # large ones: a slice each
                blk = z2[y0[j]:y1[j] + 1, x0[j]:x1[j] + 1]
                np.minimum(blk, key[k[j]], out=blk)
        for c, (K, dist, R, tv) in enumerate(cams):
            d = _cam_z(R, tv, centre)
            uv = project_points(centre, R, tv, K, dist)
            u, v = uv[:, 0], uv[:, 1]
            inside = (d > 0) & (0 <= v) & (v < H) & (0 <= u) & (u < W)
            pix = np.zeros(Ns, dtype=np.int64)
            pix[inside] = v[inside].astype(np.int64) * W + u[inside].astype(np.int64)
            zm = zmaps[c].view(np.float32)[pix]
            seen = inside & (d.astype(np.float32) <= zm + tol)
            vis[surf[seen]] |= np.uint16(1 << c)
            acc[seen] += _frame_rgb(frames[c])[pix[seen]]
            cnt[seen] += 1
    has = cnt > 0
    avg = (acc[has] + (cnt[has] // 2)[:, None]) // cnt[has][:, None]
    out[surf[has]] = avg.astype(np.uint8)
    return zmaps, vis, out


def color_visible_literal(idx, rgb, grid, bounds, cams, frames, H, W, tol=None):
    """The same contract, one voxel, one camera, one pixel at a time."""
    nx, ny, nz = grid
    idx = [int(i) for i in idx]
    C = len(cams)
    tol = np.float32(default_tolerance(grid, bounds) if tol is None else tol)
    xs, ys, zs = axis_tables(nx, ny, nz, bounds)
    hx, hy, hz = half_extents(grid, bounds)
    alive = set(idx)
    zmaps = np.full((C, H * W), INF_BITS, dtype=np.uint32)
    vis = np.zeros(len(idx), dtype=np.uint16)
    out = np.array(rgb, dtype=np.uint8).reshape(len(idx), 3).copy()

    def coords(i):
        return (i // ny) % nx, i % ny, i // (nx * ny)

    def is_surface(i):
        ix, iy, iz = coords(i)
        for nb, inside in ((i + 1, iy + 1 < ny), (i - 1, iy >= 1), (i + ny, ix + 1 < nx), (i - ny, ix >= 1),
                           (i + nx * ny, iz + 1 < nz), (i - nx * ny, iz >= 1)):
            if not inside or nb not in alive:
                return True
        return False

    def point(i):
        ix, iy, iz = coords(i)
        return float(xs[ix]), float(ys[iy]), float(zs[iz])

    def camz(R, tv, p):
        R = np.asarray(R, dtype=np.float64).reshape(3, 3)
        tv = np.asarray(tv, dtype=np.float64).reshape(3)
        return float(R[2, 0] * p[0] + R[2, 1] * p[1] + R[2, 2] * p[2] + tv[2])

    surf = [s for s, i in enumerate(idx) if is_surface(i)]
    with np.errstate(all="ignore"):
        for s in surf:
            X, Y, Z = point(idx[s])
            for c, (K, dist, R, tv) in enumerate(cams):
                d = camz(R, tv, (X, Y, Z))
                if not d > 0:
                    continue
                pts = [(X + hx if sx > 0 else X - hx, Y + hy if sy > 0 else Y - hy, Z + hz if sz > 0 else Z - hz)
                       for sx, sy, sz in _SIGNS]
                if any(not camz(R, tv, p) > 0 for p in pts):
                    continue
                uv = [project_points(np.array([p]), R, tv, K, dist)[0] for p in pts]
                if not all(math.isfinite(a) for q in uv for a in q):
                    continue
                x0 = max(math.floor(min(q[0] for q in uv)), 0)
                x1 = min(math.floor(max(q[0] for q in uv)), W - 1)
                y0 = max(math.floor(min(q[1] for q in uv)), 0)
                y1 = min(math.floor(max(q[1] for q in uv)), H - 1)
                key = int(_f32_bits(d))
                for py in range(y0, y1 + 1):
                    for px in range(x0, x1 + 1):
                        if key < zmaps[c, py * W + px]:
                            zmaps[c, py * W + px] = key
        for s in surf:
            X, Y, Z = point(idx[s])
            tot, n = [0, 0, 0], 0
            for c, (K, dist, R, tv) in enumerate(cams):
                d = camz(R, tv, (X, Y, Z))
                u, v = project_points(np.array([(X, Y, Z)]), R, tv, K, dist)[0]
                if not (d > 0 and 0 <= v < H and 0 <= u < W):
                    continue
                pix = int(v) * W + int(u)
                zm = zmaps[c, pix:pix + 1].view(np.float32)[0]
                if not np.float32(d) <= np.float32(zm + tol):
                    continue
                vis[s] |= 1 << c
                b, g, r = (int(a) for a in np.asarray(frames[c]).reshape(-1, 3)[pix])
                tot = [tot[0] + r, tot[1] + g, tot[2] + b]
                n += 1
            if n:
                out[s] = [(a + n // 2) // n for a in tot]
    return zmaps, vis, out
