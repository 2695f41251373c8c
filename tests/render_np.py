"""Restatement of vc_render (include/voxcarve.h, "ray-cast images of the current result") in numpy, bit for bit.

Vectorised over pixels, one loop iteration per walk step; every float64 operation is written out element by element in the
contract's order (no matrix products: BLAS may fuse multiply-adds).  Two walks:

  walk_voxels   the contract's walk: one cell per step.
  walk_blocks   the same walk skipping empty blocks of B^3 voxels (what the device does with B = 8): the exit from an empty
                block is the (t, axis)-least of its three boundary events; every other axis then advances past each of its own
                boundary events that comes before the exit in (t, axis) order.  tests/test_render_restatement.py holds it to
                walk_voxels bit for bit.

Both take the occupancy as bool [n] in linear index order i = (iz nx + ix) ny + iy and return per ray
(idx u32, t float64, face u8), idx = 0xFFFFFFFF on a miss.
"""
import numpy as np

MISS = np.uint32(0xFFFFFFFF)
INF = np.inf


def view_params(cam):
    """camera.Camera -> (K4, dist5, R9, t3) float64, as vc_view_t holds them."""
    K = np.asarray(cam.K, dtype=np.float64).reshape(3, 3)
    if K[0, 1] != 0.0:
        raise ValueError("skewed camera matrix")
    K4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], dtype=np.float64)
    return K4, np.asarray(cam.dist, dtype=np.float64).reshape(5), np.asarray(cam.R, dtype=np.float64).reshape(9), \
        np.asarray(cam.tvec, dtype=np.float64).reshape(3)


def grid_params(grid, bounds):
    """(n, s, e) per axis: s = (max - min) / (n - 1), e = min - 0.5 s."""
    n = [int(v) for v in grid]
    s = [(float(bounds[2 * a + 1]) - float(bounds[2 * a])) / float(n[a] - 1) for a in range(3)]
    e = [float(bounds[2 * a]) - 0.5 * s[a] for a in range(3)]
    return n, s, e


def boundary(e, s, k):
    """b(k) = e + (double)k s (k an int array or scalar)."""
    return e + np.asarray(k).astype(np.float64) * s


def pixel_rays(view, H, W, pixels=None):
    """Origin o [3] and directions d [P, 3] of the pixels (flat v W + u; None = all H W in order)."""
    K4, dist, R9, t3 = view
    fx, fy, cx, cy = (float(v) for v in K4)
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    R = [[float(R9[3 * i + j]) for j in range(3)] for i in range(3)]
    t0, t1, t2 = (float(v) for v in t3)
    p = np.arange(H * W, dtype=np.int64) if pixels is None else np.asarray(pixels, dtype=np.int64)
    u = (p % W).astype(np.float64)
    v = (p // W).astype(np.float64)
    xd = ((u + 0.5) - cx) / fx
    yd = ((v + 0.5) - cy) / fy
    x, y = xd, yd
    for _ in range(8):
        r2 = x * x + y * y
        cd = ((1.0 + k1 * r2) + (k2 * r2) * r2) + ((k3 * r2) * r2) * r2
        dx = ((2.0 * p1) * x) * y + p2 * (r2 + (2.0 * x) * x)
        dy = p1 * (r2 + (2.0 * y) * y) + ((2.0 * p2) * x) * y
        x, y = (xd - dx) / cd, (yd - dy) / cd
    d = np.empty((p.size, 3), dtype=np.float64)
    o = np.empty(3, dtype=np.float64)
    for j in range(3):
        d[:, j] = (x * R[0][j] + y * R[1][j]) + R[2][j]
        o[j] = -((R[0][j] * t0 + R[1][j] * t1) + R[2][j] * t2)
    return o, d


def _lin(c, n):
    # c [P, 3] = (ix, iy, iz)
    return (c[:, 2] * n[0] + c[:, 0]) * n[1] + c[:, 1]


def entry(grid, bounds, o, d):
    """Item 3: (live bool [P], t_in [P], cell int64 [P, 3], entry face axis int [P] (-1 = none: t_in == 0))."""
    n, s, e = grid_params(grid, bounds)
    P = d.shape[0]
    live = np.ones(P, dtype=bool)
    near = np.full((P, 3), -INF)
    far = np.full((P, 3), INF)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(3):
            da = d[:, a]
            nz = da != 0.0
            inv = np.where(nz, 1.0 / np.where(nz, da, 1.0), 0.0)
            ta = (boundary(e[a], s[a], 0) - o[a]) * inv
            tb = (boundary(e[a], s[a], n[a]) - o[a]) * inv
            near[:, a] = np.where(nz, np.where(ta < tb, ta, tb), -INF)
            far[:, a] = np.where(nz, np.where(ta < tb, tb, ta), INF)
            outside = (o[a] < boundary(e[a], s[a], 0)) | (o[a] >= boundary(e[a], s[a], n[a]))
            live &= nz | ~outside
        t_in = np.zeros(P)
        t_out = np.full(P, INF)
        for a in range(3):
            t_in = np.where(near[:, a] > t_in, near[:, a], t_in)
            t_out = np.where(far[:, a] < t_out, far[:, a], t_out)
        live &= ~(t_in >= t_out)
        ax = np.full(P, -1, dtype=np.int64)
        for a in (2, 1, 0):                         # the lowest axis wins
            ax = np.where((t_in > 0.0) & (near[:, a] == t_in), a, ax)
        c = np.zeros((P, 3), dtype=np.int64)
        for a in range(3):
            f = np.floor(((o[a] + t_in * d[:, a]) - e[a]) / s[a])
            f = np.where(f >= 0.0, np.where(f <= n[a] - 1, f, n[a] - 1), 0.0)
            cell = f.astype(np.int64)
            cell = np.where(ax == a, np.where(d[:, a] > 0.0, 0, n[a] - 1), cell)
            c[:, a] = cell
    return live, t_in, c, ax


def _face(ax, d):
    """2a + (d_a > 0 ? 0 : 1); 6 where ax == -1."""
    P = ax.size
    pos = d[np.arange(P), np.clip(ax, 0, 2)] > 0.0
    return np.where(ax < 0, 6, 2 * ax + np.where(pos, 0, 1)).astype(np.uint8)


def _tn(n, s, e, o, d, c, a):
    """Next boundary parameter of axis a for the rays' cells c [P, 3] (+inf where d_a == 0)."""
    da = d[:, a]
    nz = da != 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = 1.0 / np.where(nz, da, 1.0)
        t = (boundary(e[a], s[a], c[:, a] + (da > 0.0)) - o[a]) * inv
    return np.where(nz, t, INF)


def _argmin3(tn):
    """Smallest tn, ties to the lowest axis (strict comparisons in axis order)."""
    best = np.zeros(tn.shape[0], dtype=np.int64)
    bt = tn[:, 0].copy()
    for a in (1, 2):
        m = tn[:, a] < bt
        best = np.where(m, a, best)
        bt = np.where(m, tn[:, a], bt)
    return best, bt


def walk_voxels(occ, grid, bounds, o, d, stats=None):
    """The contract's walk (items 3-4).  Returns (idx u32 [P], t float64 [P], face u8 [P]); stats (dict) gets 'cells'."""
    n, s, e = grid_params(grid, bounds)
    occ = np.asarray(occ, dtype=bool).reshape(-1)
    P = d.shape[0]
    live, t, c, ax = entry(grid, bounds, o, d)
    idx = np.full(P, MISS, dtype=np.uint32)
    tt = np.full(P, INF)
    face = np.full(P, 255, dtype=np.uint8)
    act = np.nonzero(live)[0]
    t, c, ax = t[act], c[act], ax[act]
    dd = d[act]
    cells = 0
    while act.size:
        cells += act.size
        i = _lin(c, n)
        hit = occ[i]
        if hit.any():
            idx[act[hit]] = i[hit].astype(np.uint32)
            tt[act[hit]] = t[hit]
            face[act[hit]] = _face(ax[hit], dd[hit])
        keep = ~hit
        act, t, c, ax, dd = act[keep], t[keep], c[keep], ax[keep], dd[keep]
        if not act.size:
            break
        tn = np.stack([_tn(n, s, e, o, dd, c, a) for a in range(3)], axis=1)
        best, bt = _argmin3(tn)
        r = np.arange(act.size)
        c[r, best] += np.where(dd[r, best] > 0.0, 1, -1)
        t = bt
        ax = best
        inside = np.ones(act.size, dtype=bool)
        for a in range(3):
            inside &= (c[:, a] >= 0) & (c[:, a] < n[a])
        act, t, c, ax, dd = act[inside], t[inside], c[inside], ax[inside], dd[inside]
    if stats is not None:
        stats["cells"] = stats.get("cells", 0) + cells
    return idx, tt, face


def block_map(occ, grid, B):
    """bool [nbz, nbx, nby]: block (bx, by, bz) of B^3 voxels holds a survivor."""
    nx, ny, nz = (int(v) for v in grid)
    v = np.asarray(occ, dtype=bool).reshape(nz, nx, ny)
    nb = [(nx + B - 1) // B, (ny + B - 1) // B, (nz + B - 1) // B]
    pad = np.zeros((nb[2] * B, nb[0] * B, nb[1] * B), dtype=bool)
    pad[:nz, :nx, :ny] = v
    return pad.reshape(nb[2], B, nb[0], B, nb[1], B).any(axis=(1, 3, 5))


def walk_blocks(occ, grid, bounds, o, d, B, stats=None):
    """walk_voxels with empty blocks of B^3 voxels skipped whole; the same results bit for bit.
    stats (dict) gets 'cells' (cells looked at) and 'skips' (empty blocks skipped)."""
    n, s, e = grid_params(grid, bounds)
    occ = np.asarray(occ, dtype=bool).reshape(-1)
    bm = block_map(occ, grid, B)
    P = d.shape[0]
    live, t, c, ax = entry(grid, bounds, o, d)
    idx = np.full(P, MISS, dtype=np.uint32)
    tt = np.full(P, INF)
    face = np.full(P, 255, dtype=np.uint8)
    act = np.nonzero(live)[0]
    t, c, ax = t[act], c[act], ax[act]
    dd = d[act]
    cells = skips = 0
    while act.size:
        full = bm[c[:, 2] // B, c[:, 0] // B, c[:, 1] // B]
        cells += int(full.sum())
        skips += int((~full).sum())
        i = _lin(c, n)
        hit = full & occ[i]
        if hit.any():
            idx[act[hit]] = i[hit].astype(np.uint32)
            tt[act[hit]] = t[hit]
            face[act[hit]] = _face(ax[hit], dd[hit])
        keep = ~hit
        act, t, c, ax, dd, full = act[keep], t[keep], c[keep], ax[keep], dd[keep], full[keep]
        if not act.size:
            break
        r = np.arange(act.size)
        # a cell of a block that holds survivors: one voxel step
        tn = np.stack([_tn(n, s, e, o, dd, c, a) for a in range(3)], axis=1)
        best, bt = _argmin3(tn)
        # an empty block: its three exit events, the (t, axis)-least one leaves it
        kb = np.empty_like(c)
        tb = np.empty((act.size, 3))
        for a in range(3):
            pos = dd[:, a] > 0.0
            lo = (c[:, a] // B) * B
            kb[:, a] = np.where(pos, np.minimum(lo + B, n[a]), lo)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                inv = 1.0 / np.where(dd[:, a] != 0.0, dd[:, a], 1.0)
                tb[:, a] = np.where(dd[:, a] != 0.0, (boundary(e[a], s[a], kb[:, a]) - o[a]) * inv, INF)
        xa, xt = _argmin3(tb)
        cs = c.copy()
        for a in range(3):                           # every other axis past its own events before (xt, xa)
            for _ in range(B):
                ta = _tn(n, s, e, o, dd, cs, a)
                m = (~full) & (xa != a) & ((ta < xt) | ((ta == xt) & (a < xa)))
                if not m.any():
                    break
                cs[m, a] += np.where(dd[m, a] > 0.0, 1, -1)
        cs[r, xa] = np.where(dd[r, xa] > 0.0, kb[r, xa], kb[r, xa] - 1)
        c = np.where(full[:, None], c, cs)
        c[r, best] += np.where(full, np.where(dd[r, best] > 0.0, 1, -1), 0)
        t = np.where(full, bt, xt)
        ax = np.where(full, best, xa)
        inside = np.ones(act.size, dtype=bool)
        for a in range(3):
            inside &= (c[:, a] >= 0) & (c[:, a] < n[a])
        act, t, c, ax, dd = act[inside], t[inside], c[inside], ax[inside], dd[inside]
    if stats is not None:
        stats["cells"] = stats.get("cells", 0) + cells
        stats["skips"] = stats.get("skips", 0) + skips
    return idx, tt, face


def shade_rgb(rec_rgb, face, shade):
    """rgb_k = (rec_rgb_k * shade[face] + 127) / 255 in integers."""
    sh = np.asarray(shade, dtype=np.uint32)[face.astype(np.int64)]
    return ((rec_rgb.astype(np.uint32) * sh[:, None] + 127) // 255).astype(np.uint8)


def render(occ, rec_idx, rec_rgb, grid, bounds, views, H, W, shade=None, background=(0, 0, 0), pixels=None, block=None,
           stats=None):
    """The images of vc_render for every view: dict of index u32 [V, P], depth f32 [V, P], face u8 [V, P], rgb u8 [V, P, 3]
    (P = H W, or the given flat pixel indices).  occ: bool [n]; rec_idx u32 [S] ascending and rec_rgb u8 [S, 3] the records.
    block: None = walk_voxels, B = walk_blocks with B^3 blocks (same results)."""
    shade = np.full(7, 255, dtype=np.uint8) if shade is None else np.asarray(shade, dtype=np.uint8).reshape(7)
    bg = np.asarray(background, dtype=np.uint8).reshape(3)
    rec_idx = np.asarray(rec_idx, dtype=np.uint32)
    out = {"index": [], "depth": [], "face": [], "rgb": []}
    for view in views:
        o, d = pixel_rays(view, H, W, pixels)
        if block is None:
            idx, t, face = walk_voxels(occ, grid, bounds, o, d, stats)
        else:
            idx, t, face = walk_blocks(occ, grid, bounds, o, d, block, stats)
        hit = idx != MISS
        rgb = np.empty((idx.size, 3), dtype=np.uint8)
        rgb[:] = bg
        if hit.any():
            k = np.searchsorted(rec_idx, idx[hit])
            assert np.array_equal(rec_idx[k], idx[hit]), "a hit without a record"
            rgb[hit] = shade_rgb(np.asarray(rec_rgb)[k], face[hit], shade)
        out["index"].append(idx)
        out["depth"].append(t.astype(np.float32))
        out["face"].append(face)
        out["rgb"].append(rgb)
    return {k: np.stack(v) for k, v in out.items()}


def brute_force(occ, grid, bounds, o, d):
    """Per ray the survivor whose box [b(c), b(c + 1)] has the smallest slab entry max(0, near) with entry < exit
    (u32 index, MISS when none) and that entry t: the walk's answer for rays away from edges and corners."""
    n, s, e = grid_params(grid, bounds)
    occ = np.asarray(occ, dtype=bool).reshape(-1)
    sv = np.nonzero(occ)[0]
    iy = sv % n[1]
    ix = (sv // n[1]) % n[0]
    iz = sv // (n[0] * n[1])
    cell = [ix, iy, iz]
    P = d.shape[0]
    best_i = np.full(P, MISS, dtype=np.uint32)
    best_t = np.full(P, INF)
    if not sv.size:
        return best_i, best_t
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for p in range(P):
            tin = np.zeros(sv.size)
            tout = np.full(sv.size, INF)
            ok = np.ones(sv.size, dtype=bool)
            for a in range(3):
                lo = boundary(e[a], s[a], cell[a])
                hi = boundary(e[a], s[a], cell[a] + 1)
                if d[p, a] != 0.0:
                    ta = (lo - o[a]) / d[p, a]
                    tb = (hi - o[a]) / d[p, a]
                    tin = np.maximum(tin, np.minimum(ta, tb))
                    tout = np.minimum(tout, np.maximum(ta, tb))
                else:
                    ok &= (o[a] >= lo) & (o[a] < hi)
            ok &= tin < tout
            if ok.any():
                k = np.nonzero(ok)[0]
                j = k[np.argmin(tin[k])]
                best_i[p] = np.uint32(sv[j])
                best_t[p] = tin[j]
    return best_i, best_t
