"""Restatement of the footprint carve (vc_carve_footprint, include/voxcarve.h).

TEST INFRASTRUCTURE ONLY.  Two forms of one contract: `carve` (vectorised, summed-area tables) and `carve_literal` (one
voxel, one camera, one pixel at a time, plain Python floats and ints, no table).

Projection: `project` below is csrc/vc_device.h operation for operation (float64, every multiply and add its own rounding).
It is oracle/carve_np.project_points without that function's all-zero k4..k6 / s1..s4 / tilt slots: the two agree bit for bit
wherever the result is finite (tests/test_footprint_restatement.py checks that), and a box is built from NaN-ignoring minima
and maxima, so where a corner is NOT finite (cameras inside the volume) it matters which of inf and NaN the device's form
gives -- hence the device's form here.  No behind-camera cull.

The contract:
 1. Cell.  Per axis with n cells, bounds lo, hi and centres c[k] (np.linspace): h = 0.5 * ((hi - lo) / (n - 1)) (0 when
    n == 1); lattice L[k] = c[k] - h for k < n, L[n] = c[n-1] + h.  Voxel (ix, iy, iz) has the 8 corners L[i], L[i+1] per axis.
 2. Box.  The 8 corners and the centre are projected; u_lo, u_hi, v_lo, v_hi = per-coordinate fmin / fmax over the 9 points.
    A NaN centre u or v: the camera does not see the voxel.  bx0 = clamp(floor(u_lo), -1, W), bx1 = clamp(floor(u_hi), -1, W),
    by0, by1 likewise with H.  area = (bx1 - bx0 + 1) * (by1 - by0 + 1); cnt = foreground pixels inside box and image.
 3. Test.  "any": cnt > 0.  ("cover", q): cnt * 256 >= q * area.  "all" = ("cover", 256).
 4. T = cameras that pass; kept when T >= min_views and T >= 1; ascending linear index.  Colour / seen: the colour camera's
    pixel under the CENTRE whenever the centre is inside its image (mask not consulted), else 0, 0, 0 and seen = 0.

masks are the slot's PREPARED masks (after the 2x2 post-filter, what vc_fetch_mask returns), uint8 [H, W], foreground > 0.
"""
import math

import numpy as np

from oracle.carve_np import DEFAULT_BOUNDS, axis_tables

RULES = ("any", "all")


def normalise_rule(rule):
    """-> ("any", 0) or ("cover", q)."""
    if rule == "any":
        return ("any", 0)
    if rule == "all":
        return ("cover", 256)
    kind, q = rule
    if kind != "cover" or int(q) != q or not 1 <= int(q) <= 256:
        raise ValueError("footprint rule %r" % (rule,))
    return ("cover", int(q))


def lattices(grid, bounds=DEFAULT_BOUNDS):
    """(Lx, Ly, Lz): n + 1 float64 values per axis."""
    out = []
    for a, c in enumerate(axis_tables(grid[0], grid[1], grid[2], bounds)):
        n, lo, hi = grid[a], bounds[2 * a], bounds[2 * a + 1]
        h = 0.5 * ((hi - lo) / (n - 1)) if n > 1 else 0.0
        L = np.empty(n + 1, dtype=np.float64)
        L[:n] = c - h
        L[n] = c[n - 1] + h
        out.append(L)
    return tuple(out)


def project(points, cam):
    """csrc/vc_device.h project_point: float64 [N, 2] (u, v) of points [N, 3]; cam = (K, dist, R, tvec)."""
    K, dist, R, t = cam
    A = np.asarray(K, dtype=np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3 = [np.float64(v) for v in np.asarray(dist, dtype=np.float64).reshape(-1)[:5]]
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    P = np.asarray(points, dtype=np.float64)
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        x = R[0, 0] * X + R[0, 1] * Y + R[0, 2] * Z + t[0]
        y = R[1, 0] * X + R[1, 1] * Y + R[1, 2] * Z + t[1]
        z = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + t[2]
        z = np.where(z != 0.0, 1.0 / z, 1.0)
        x = x * z
        y = y * z
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        tx = 2 * x
        ty = 2 * y
        a1 = tx * y
        a2 = r2 + tx * x
        a3 = r2 + ty * y
        cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6
        xd = x * cdist + p1 * a1 + p2 * a2
        yd = y * cdist + p1 * a3 + p2 * a1
        u = xd * A[0, 0] + A[0, 2]
        v = yd * A[1, 1] + A[1, 2]
    return np.stack([u, v], axis=1)


def _decompose(idx, nx, ny):
    idx = np.asarray(idx, dtype=np.int64)
    iy = idx % ny
    t = idx // ny
    return t % nx, iy, t // nx


def _clamp(a, hi):
    with np.errstate(invalid="ignore"):
        f = np.clip(np.floor(a), -1.0, float(hi))
    return np.where(np.isnan(f), -1.0, f).astype(np.int64)


def boxes(idx, grid, cam, H, W, bounds=DEFAULT_BOUNDS):
    """(sees bool [n], bx0, bx1, by0, by1 int64 [n], centre uv float64 [n, 2]) of the voxels `idx` for one camera."""
    nx, ny, nz = grid
    xs, ys, zs = axis_tables(nx, ny, nz, bounds)
    Lx, Ly, Lz = lattices(grid, bounds)
    ix, iy, iz = _decompose(idx, nx, ny)
    uvc = project(np.stack([xs[ix], ys[iy], zs[iz]], axis=1), cam)
    ulo, uhi, vlo, vhi = uvc[:, 0].copy(), uvc[:, 0].copy(), uvc[:, 1].copy(), uvc[:, 1].copy()
    for dz in (0, 1):
        for dx in (0, 1):
            for dy in (0, 1):
                uv = project(np.stack([Lx[ix + dx], Ly[iy + dy], Lz[iz + dz]], axis=1), cam)
                ulo, uhi = np.fmin(ulo, uv[:, 0]), np.fmax(uhi, uv[:, 0])
                vlo, vhi = np.fmin(vlo, uv[:, 1]), np.fmax(vhi, uv[:, 1])
    sees = ~(np.isnan(uvc[:, 0]) | np.isnan(uvc[:, 1]))
    return sees, _clamp(ulo, W), _clamp(uhi, W), _clamp(vlo, H), _clamp(vhi, H), uvc


def table(mask):
    """int64 [H + 1, W + 1]: T[y, x] = foreground pixels in rows < y, columns < x."""
    H, W = mask.shape
    T = np.zeros((H + 1, W + 1), dtype=np.int64)
    T[1:, 1:] = np.cumsum(np.cumsum((np.asarray(mask) > 0).astype(np.int64), axis=0), axis=1)
    return T


def _passes(T, H, W, sees, bx0, bx1, by0, by1, rule):
    a, b = np.maximum(bx0, 0), np.minimum(bx1, W - 1)
    c, d = np.maximum(by0, 0), np.minimum(by1, H - 1)
    ok = (a <= b) & (c <= d)
    a, b, c, d = [np.where(ok, v, 0) for v in (a, b, c, d)]
    cnt = np.where(ok, T[d + 1, b + 1] - T[c, b + 1] - T[d + 1, a] + T[c, a], 0)
    area = (bx1 - bx0 + 1) * (by1 - by0 + 1)
    kind, q = rule
    return sees & ((cnt > 0) if kind == "any" else (cnt * 256 >= q * area))


def center_offsets(uvc, H, W):
    """int(v) * W + int(u) of the centres inside the image, else -1 (int64)."""
    u, v = uvc[:, 0], uvc[:, 1]
    with np.errstate(invalid="ignore"):
        inside = (0 <= v) & (v < H) & (0 <= u) & (u < W)
    off = np.full(u.shape, -1, dtype=np.int64)
    off[inside] = v[inside].astype(np.int64) * W + u[inside].astype(np.int64)
    return off


def viewmasks_of_rules(idx, grid, cams, masks, rules, bounds=DEFAULT_BOUNDS, chunk=1 << 19):
    """One uint16 [n] per rule of `rules`: bit c = camera c passes voxel idx[k] (the boxes, which no rule changes, are made once)."""
    norm = [normalise_rule(r) for r in rules]
    idx = np.asarray(idx, dtype=np.int64)
    H, W = masks[0].shape
    tabs = [table(m) for m in masks]
    vms = [np.zeros(idx.size, dtype=np.uint16) for _ in norm]
    for s in range(0, idx.size, chunk):
        part = idx[s:s + chunk]
        for c, cam in enumerate(cams):
            sees, bx0, bx1, by0, by1, _ = boxes(part, grid, cam, H, W, bounds)
            for vm, rule in zip(vms, norm):
                vm[s:s + chunk] |= _passes(tabs[c], H, W, sees, bx0, bx1, by0, by1, rule).astype(np.uint16) << np.uint16(c)
    return vms


def viewmasks(idx, grid, cams, masks, rule, bounds=DEFAULT_BOUNDS, chunk=1 << 19):
    """uint16 [n]: bit c = camera c passes voxel idx[k] under `rule`."""
    return viewmasks_of_rules(idx, grid, cams, masks, [rule], bounds, chunk)[0]


def carve(grid, cams, masks, rule, frames=None, min_views=None, color_cam=1, bounds=DEFAULT_BOUNDS, index_range=None, viewmask=None):
    """The footprint hull of the grid, or of the linear-index range index_range = (i0, i1) (a z-slab).  Returns dict: idx uint32
    [S] ascending global indices, viewmask uint16 [n] (the range's voxels), rgb uint8 [S, 3], seen uint8 [S], occupancy bool [n].
    viewmask: the result of an earlier call for the same range and rule (it does not depend on min_views), to save the time."""
    nx, ny, nz = grid
    C = len(cams)
    if min_views is None:
        min_views = C
    i0, i1 = (0, nx * ny * nz) if index_range is None else index_range
    H, W = masks[0].shape
    vm = viewmasks(np.arange(i0, i1, dtype=np.int64), grid, cams, masks, rule, bounds) if viewmask is None else viewmask
    T = np.zeros(i1 - i0, dtype=np.int32)
    for c in range(C):
        T += (vm >> c) & 1
    keep = (T >= min_views) & (T >= 1)
    idx = (np.nonzero(keep)[0] + i0).astype(np.uint32)
    rgb = np.zeros((idx.size, 3), dtype=np.uint8)
    seen = np.zeros(idx.size, dtype=np.uint8)
    if color_cam is not None and color_cam >= 0 and idx.size:
        xs, ys, zs = axis_tables(nx, ny, nz, bounds)
        ix, iy, iz = _decompose(idx, nx, ny)
        off = center_offsets(project(np.stack([xs[ix], ys[iy], zs[iz]], axis=1), cams[color_cam]), H, W)
        seen = (off >= 0).astype(np.uint8)
        if frames is not None:
            rgb[off >= 0] = np.asarray(frames[color_cam]).reshape(-1, 3)[off[off >= 0]][:, ::-1]
    return {"idx": idx, "viewmask": vm, "rgb": rgb, "seen": seen, "occupancy": keep}


# ----------------------------------------------------------------------------------------------- literal form
def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def _fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _project_literal(cam, X, Y, Z):
    K, dist, R, t = cam
    R = [[float(R[i][j]) for j in range(3)] for i in range(3)]
    t = [float(v) for v in np.asarray(t).reshape(3)]
    k1, k2, p1, p2, k3 = [float(v) for v in np.asarray(dist).reshape(-1)[:5]]
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    x = R[0][0] * X + R[0][1] * Y + R[0][2] * Z + t[0]
    y = R[1][0] * X + R[1][1] * Y + R[1][2] * Z + t[1]
    z = R[2][0] * X + R[2][1] * Y + R[2][2] * Z + t[2]
    z = 1.0 / z if z != 0.0 else 1.0
    x = x * z
    y = y * z
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    tx = 2 * x
    ty = 2 * y
    a1 = tx * y
    a2 = r2 + tx * x
    a3 = r2 + ty * y
    cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6
    xd = x * cdist + p1 * a1 + p2 * a2
    yd = y * cdist + p1 * a3 + p2 * a1
    return xd * fx + cx, yd * fy + cy


def _clamp_literal(a, hi):
    if a == math.inf:
        return hi
    if a == -math.inf:
        return -1
    return min(max(math.floor(a), -1), hi)


def carve_literal(grid, cams, masks, rule, frames=None, min_views=None, color_cam=1, bounds=DEFAULT_BOUNDS):
    """The same contract, one voxel, one camera, one pixel at a time (small grids only).  Returns (idx, viewmask, rgb, seen)."""
    kind, q = normalise_rule(rule)
    nx, ny, nz = grid
    C = len(cams)
    if min_views is None:
        min_views = C
    H, W = masks[0].shape
    axes = [[float(v) for v in a] for a in axis_tables(nx, ny, nz, bounds)]
    lat = []
    for a in range(3):
        n, lo, hi = grid[a], float(bounds[2 * a]), float(bounds[2 * a + 1])
        h = 0.5 * ((hi - lo) / (n - 1)) if n > 1 else 0.0
        lat.append([axes[a][k] - h for k in range(n)] + [axes[a][n - 1] + h])
    idx, vms, rgb, seen = [], [], [], []
    for i in range(nx * ny * nz):
        iy, t = i % ny, i // ny
        ix, iz = t % nx, t // nx
        centre = (axes[0][ix], axes[1][iy], axes[2][iz])
        vm = 0
        for c in range(C):
            uc, vc = _project_literal(cams[c], *centre)
            if uc != uc or vc != vc:
                continue
            ulo = uhi = uc
            vlo = vhi = vc
            for dx in (0, 1):
                for dy in (0, 1):
                    for dz in (0, 1):
                        u, v = _project_literal(cams[c], lat[0][ix + dx], lat[1][iy + dy], lat[2][iz + dz])
                        ulo, uhi, vlo, vhi = _fmin(ulo, u), _fmax(uhi, u), _fmin(vlo, v), _fmax(vhi, v)
            bx0, bx1, by0, by1 = _clamp_literal(ulo, W), _clamp_literal(uhi, W), _clamp_literal(vlo, H), _clamp_literal(vhi, H)
            area = (bx1 - bx0 + 1) * (by1 - by0 + 1)
            cnt = 0
            for y in range(by0, by1 + 1):
                for x in range(bx0, bx1 + 1):
                    if 0 <= x < W and 0 <= y < H and masks[c][y][x] > 0:
                        cnt += 1
            if (cnt > 0) if kind == "any" else (cnt * 256 >= q * area):
                vm |= 1 << c
        vms.append(vm)
        T = bin(vm).count("1")
        if T >= min_views and T >= 1:
            idx.append(i)
            px, s = (0, 0, 0), 0
            if color_cam is not None and color_cam >= 0:
                u, v = _project_literal(cams[color_cam], *centre)
                if 0 <= u < W and 0 <= v < H:
                    s = 1
                    if frames is not None:
                        b, g, r = frames[color_cam][int(v)][int(u)]
                        px = (int(r), int(g), int(b))
            rgb.append(px)
            seen.append(s)
    return (np.array(idx, dtype=np.uint32), np.array(vms, dtype=np.uint16), np.array(rgb, dtype=np.uint8).reshape(-1, 3),
            np.array(seen, dtype=np.uint8))
