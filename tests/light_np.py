"""Restatement of vc_light_render (include/voxcarve.h, "lit renders") in numpy, bit for bit: cast
shadows, ambient occlusion and a floor for the images of a render.  Built on render_np (pixel_rays, entry, the walk's tn, tie rule
and blocks) and on the arithmetic of normals_np.shade.  Two forms:

  light(...)           vectorised over the secondary rays, one loop iteration per walk step.  block=B walks with empty blocks of
                       B^3 voxels skipped (what the device does with B = 8); the same results.
  light_literal(...)   the definition: per pixel, per ray, in plain Python floats and ints.

Both take the occupancy as bool [n] in linear index order, the records (ascending indices, RGB, stored normals or None), the
views and the images of render_np.render (or the device's: index u32, depth f32, face u8, rgb u8, each [V, P ...]) and a light
dict: pos (x, y, z, w), ambient, smooth, ao_reach, floor (None or a dict z, rect, cell_mm, rgb).  They return a dict of
rgb u8 [V, P, 3], depth f32 [V, P], kind / shadow / ao u8 [V, P] and stats (the contract's counts)."""
import math

import numpy as np

import render_np as rn

MISS = rn.MISS
RAYS = 16


def ao_table():
    """The sixteen (iu, iv, in) of item 5, in order."""
    axial = [(1, 0), (-1, 0), (0, 1), (0, -1)]
    diag = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    return [(iu, iv, 2) for iu, iv in axial] + [(iu, iv, 2) for iu, iv in diag] + \
           [(iu, iv, 1) for iu, iv in axial] + [(iu, iv, 1) for iu, iv in diag]


def _inside(c, n):
    ok = np.ones(c.shape[0], dtype=bool)
    for a in range(3):
        ok &= (c[:, a] >= 0) & (c[:, a] < n[a])
    return ok


def walk_from(occ, grid, bounds, q, d, c, t, B=None, stats=None):
    """Item 4 of vc_render from given cells: ray r has origin q[r], direction d[r], stands in cell c[r] (inside the grid) at
    parameter t[r].  Returns (hit bool [P], t float64 [P]).  B: empty blocks of B^3 voxels are skipped whole, as
    render_np.walk_blocks skips them."""
    n, s, e = rn.grid_params(grid, bounds)
    occ = np.asarray(occ, dtype=bool).reshape(-1)
    bm = None if B is None else rn.block_map(occ, grid, B)
    P = d.shape[0]
    hit_out = np.zeros(P, dtype=bool)
    t_out = np.full(P, np.inf)
    act = np.arange(P)
    o = np.ascontiguousarray(np.asarray(q, dtype=np.float64).T)          # [3, P]: o[a] is the rays' origin on axis a
    c = np.array(c, dtype=np.int64)
    t = np.array(t, dtype=np.float64)
    dd = np.asarray(d, dtype=np.float64)
    cells = skips = 0
    while act.size:
        full = np.ones(act.size, dtype=bool) if bm is None else bm[c[:, 2] // B, c[:, 0] // B, c[:, 1] // B]
        cells += int(full.sum())
        skips += int((~full).sum())
        hit = full & occ[rn._lin(c, n)]
        hit_out[act[hit]] = True
        t_out[act[hit]] = t[hit]
        keep = ~hit
        act, t, c, dd, o, full = act[keep], t[keep], c[keep], dd[keep], o[:, keep], full[keep]
        if not act.size:
            break
        r = np.arange(act.size)
        tn = np.stack([rn._tn(n, s, e, o, dd, c, a) for a in range(3)], axis=1)
        best, bt = rn._argmin3(tn)
        if bm is None:
            c[r, best] += np.where(dd[r, best] > 0.0, 1, -1)
            t = bt
        else:
            kb = np.empty_like(c)
            tb = np.empty((act.size, 3))
            for a in range(3):
                lo = (c[:, a] // B) * B
                kb[:, a] = np.where(dd[:, a] > 0.0, np.minimum(lo + B, n[a]), lo)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    inv = 1.0 / np.where(dd[:, a] != 0.0, dd[:, a], 1.0)
                    tb[:, a] = np.where(dd[:, a] != 0.0, (rn.boundary(e[a], s[a], kb[:, a]) - o[a]) * inv, np.inf)
            xa, xt = rn._argmin3(tb)
            cs = c.copy()
            for a in range(3):                       # every other axis past its own events before (xt, xa)
                for _ in range(B):
                    ta = rn._tn(n, s, e, o, dd, cs, a)
                    m = (~full) & (xa != a) & ((ta < xt) | ((ta == xt) & (a < xa)))
                    if not m.any():
                        break
                    cs[m, a] += np.where(dd[m, a] > 0.0, 1, -1)
            cs[r, xa] = np.where(dd[r, xa] > 0.0, kb[r, xa], kb[r, xa] - 1)
            c = np.where(full[:, None], c, cs)
            c[r, best] += np.where(full, np.where(dd[r, best] > 0.0, 1, -1), 0)
            t = np.where(full, bt, xt)
        inside = _inside(c, n)
        act, t, c, dd, o = act[inside], t[inside], c[inside], dd[inside], o[:, inside]
    if stats is not None:
        stats["cells"] = stats.get("cells", 0) + cells
        stats["skips"] = stats.get("skips", 0) + skips
    return hit_out, t_out


def secondary(occ, grid, bounds, q, d, c0=None, B=None, stats=None):
    """The secondary rays of items 3 and 6: origins q [P, 3], directions d [P, 3].  c0 int [P, 3]: the walk starts at that cell
    with t = 0 (a start cell outside the grid: open); c0 None: the entry of vc_render's item 3, then the walk.  Returns
    (hit bool [P], t float64 [P])."""
    n, _, _ = rn.grid_params(grid, bounds)
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    P = d.shape[0]
    hit = np.zeros(P, dtype=bool)
    t = np.full(P, np.inf)
    if not P:
        return hit, t
    if c0 is not None:
        c = np.asarray(c0, dtype=np.int64).reshape(-1, 3)
        live = _inside(c, n)
        t0 = np.zeros(P)
    else:
        live, t0, c, _ = rn.entry(grid, bounds, q.T, d)
    k = np.nonzero(live)[0]
    if k.size:
        hit[k], t[k] = walk_from(occ, grid, bounds, q[k], d[k], c[k], t0[k], B, stats)
    return hit, t


def lambert(n, L):
    """The c of vc_shade_render for integer normals n [P, 3] and lights L [P, 3] (float64), as normals_np.shade computes it."""
    n = np.asarray(n, dtype=np.int64)
    nf = n.astype(np.float64)
    dot = (nf[:, 0] * L[:, 0] + nf[:, 1] * L[:, 1]) + nf[:, 2] * L[:, 2]
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]).astype(np.float64)
    ll = (L[:, 0] * L[:, 0] + L[:, 1] * L[:, 1]) + L[:, 2] * L[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(dot > 0.0, np.minimum(dot / np.sqrt(nn * ll), 1.0), 0.0)


def floor_pixels(o, d, idx, depth, floor):
    """Item 6: (is_floor bool [P], tf float64 [P], Q float64 [P, 3]) of a view's pixels."""
    P = d.shape[0]
    if floor is None:
        return np.zeros(P, dtype=bool), np.zeros(P), np.zeros((P, 3))
    x0, x1, y0, y1 = (float(v) for v in floor["rect"])
    dz = d[:, 2]
    nz = dz != 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tf = (float(floor["z"]) - o[2]) / np.where(nz, dz, 1.0)
        ok = nz & (tf > 0.0) & ((idx == MISS) | (tf < depth.astype(np.float64)))
        Q = np.stack([o[a] + tf * d[:, a] for a in range(3)], axis=1)
        ok &= (Q[:, 0] >= x0) & (Q[:, 0] <= x1) & (Q[:, 1] >= y0) & (Q[:, 1] <= y1)
    return ok, tf, Q


def _view_setup(occ, grid, bounds, view, H, W, ren, v, lt, pixels):
    """What both forms share per view: rays, kinds, the listed pixels with their points, frames and start cells."""
    n, s, e = rn.grid_params(grid, bounds)
    o, d = rn.pixel_rays(view, H, W, pixels)
    idx = np.asarray(ren["index"][v], dtype=np.uint32).reshape(-1)
    depth = np.asarray(ren["depth"][v], dtype=np.float32).reshape(-1)
    face = np.asarray(ren["face"][v], dtype=np.uint8).reshape(-1)
    isf, tf, Qf = floor_pixels(o, d, idx, depth, lt.get("floor"))
    kind = np.where(isf, 2, np.where(idx != MISS, 1, 0)).astype(np.uint8)
    job = (kind == 2) | ((kind == 1) & (face != 6))
    j = np.nonzero(job)[0]
    hull = kind[j] == 1
    tq = np.where(hull, depth[j].astype(np.float64), tf[j])
    Q = np.stack([o[a] + tq * d[j, a] for a in range(3)], axis=1)
    fj = np.where(hull, face[j], 0).astype(np.int64)
    axis = np.where(hull, fj // 2, 2)
    sigma = np.where(hull, np.where(fj % 2 == 0, -1, 1), -1 if o[2] < (lt["floor"]["z"] if lt.get("floor") else 0.0) else 1).astype(np.int64)
    i = np.where(hull, idx[j], 0).astype(np.int64)
    c0 = np.stack([(i // n[1]) % n[0], i % n[1], i // (n[0] * n[1])], axis=1)
    c0[np.arange(j.size), axis] += sigma                                # (k = 0: -1, k = 1: +1 -- sigma itself)
    return o, d, idx, depth, face, kind, tf, j, hull, Q, axis, sigma, c0


def _shade(base, n3, E, shadow, ao, ambient):
    c = lambert(n3, E)
    a_term = (int(ambient) * ao.astype(np.int64) * 2 + 16) // 32
    s = a_term + np.where(shadow == 0, np.floor(np.float64(255 - int(ambient)) * c + 0.5).astype(np.int64), 0)
    return ((base.astype(np.int64) * s[:, None] + 127) // 255).astype(np.uint8)


def _bases_and_normals(lt, rec_idx, rec_rgb, n4, idx_j, hull, Q, axis, sigma):
    """Base colours u8 [J, 3] and integer normals [J, 3] of the listed pixels (item 7)."""
    J = idx_j.size
    n3 = np.zeros((J, 3), dtype=np.int64)
    n3[np.arange(J), axis] = sigma
    base = np.zeros((J, 3), dtype=np.uint8)
    S = len(rec_idx)
    if hull.any():
        pos = np.searchsorted(np.asarray(rec_idx, dtype=np.uint32), idx_j[hull])
        ok = pos < S
        b = np.zeros((int(hull.sum()), 3), dtype=np.uint8)
        b[ok] = np.asarray(rec_rgb, dtype=np.uint8)[pos[ok]]
        base[hull] = b
        if lt.get("smooth"):
            q = np.zeros((int(hull.sum()), 4), dtype=np.int64)
            q[ok] = np.asarray(n4)[pos[ok]].astype(np.int64)
            has = (q[:, 3] != 0) & q[:, :3].any(axis=1)
            m = n3[hull]
            m[has] = q[has, :3]
            n3[hull] = m
    if (~hull).any():
        fl = lt["floor"]
        cell = float(fl["cell_mm"])
        kx = np.floor(Q[~hull, 0] / cell).astype(np.int64)
        ky = np.floor(Q[~hull, 1] / cell).astype(np.int64)
        base[~hull] = np.asarray(fl["rgb"], dtype=np.uint8).reshape(2, 3)[(kx + ky) & 1]
    return base, n3


def light(occ, rec_idx, rec_rgb, n4, grid, bounds, views, H, W, ren, lt, pixels=None, block=None, stats=None):
    n, s, e = rn.grid_params(grid, bounds)
    pos = [float(v) for v in lt["pos"]]
    reach = float(lt["ao_reach"])
    out = {"rgb": [], "depth": [], "kind": [], "shadow": [], "ao": []}
    st = {"pixels": 0, "hull_pixels": 0, "floor_pixels": 0, "shadowed": 0, "facing_away": 0, "rays_walked": 0}
    for v, view in enumerate(views):
        o, d, idx, depth, face, kind, tf, j, hull, Q, axis, sigma, c0 = _view_setup(occ, grid, bounds, view, H, W, ren, v, lt, pixels)
        P, J = idx.size, j.size
        rgb = np.array(np.asarray(ren["rgb"][v]).reshape(-1, 3), dtype=np.uint8, copy=True)
        odepth = depth.copy()
        shadow = np.zeros(P, dtype=np.uint8)
        ao = np.full(P, RAYS, dtype=np.uint8)
        st["pixels"] += P
        st["hull_pixels"] += int((kind == 1).sum())
        st["floor_pixels"] += int((kind == 2).sum())
        if J:
            r = np.arange(J)

            def cast(E, sel):
                """hit, t of the rays (Q, E) of the listed pixels `sel`: from the start cell on the hull, by entry on the floor."""
                hit = np.zeros(J, dtype=bool)
                t = np.full(J, np.inf)
                for mode in (True, False):
                    k = np.nonzero(sel & (hull == mode))[0]
                    if k.size:
                        hit[k], t[k] = secondary(occ, grid, bounds, Q[k], E[k], c0[k] if mode else None, block, stats)
                return hit, t

            # 4 the shadow ray
            E = (np.array(pos[:3])[None, :] - Q) if pos[3] != 0.0 else np.broadcast_to(np.array(pos[:3]), (J, 3)).copy()
            away = sigma.astype(np.float64) * E[r, axis] <= 0.0
            hit, t = cast(E, ~away)
            occl = hit & ((t < 1.0) if pos[3] != 0.0 else True)
            sh = np.where(away, 2, np.where(occl, 1, 0)).astype(np.uint8)
            st["rays_walked"] += int((~away).sum())
            # 5 the occlusion rays
            aoj = np.full(J, RAYS, dtype=np.int64)
            if reach > 0.0:
                aoj[:] = 0
                sv = np.array(s)
                for iu, iv, inn in ao_table():
                    A = np.zeros((J, 3))
                    ua, va = (axis + 1) % 3, (axis + 2) % 3
                    A[r, ua] = float(iu) * sv[ua]
                    A[r, va] = float(iv) * sv[va]
                    A[r, axis] = (sigma * inn).astype(np.float64) * sv[axis]
                    hit, t = cast(A, np.ones(J, dtype=bool))
                    aoj += ~(hit & (t < reach / math.sqrt(float(iu * iu + iv * iv + inn * inn))))
                st["rays_walked"] += RAYS * J
            base, n3 = _bases_and_normals(lt, rec_idx, rec_rgb, n4, idx[j], hull, Q, axis, sigma)
            rgb[j] = _shade(base, n3, E, sh, aoj, lt["ambient"])
            odepth[j] = np.where(hull, depth[j], tf[j].astype(np.float32))
            shadow[j] = sh
            ao[j] = aoj.astype(np.uint8)
            st["shadowed"] += int((sh == 1).sum())
            st["facing_away"] += int((sh == 2).sum())
        for key, val in (("rgb", rgb), ("depth", odepth), ("kind", kind), ("shadow", shadow), ("ao", ao)):
            out[key].append(val)
    res = {k: np.stack(val) for k, val in out.items()}
    res["stats"] = st
    return res


# ---- the literal form ----------------------------------------------------------------------------------------------------------
def _b(e, s, k):
    return e + float(k) * s


def _tn1(n, s, e, o, d, c, a):
    if d[a] == 0.0:
        return math.inf
    return (_b(e[a], s[a], c[a] + (1 if d[a] > 0.0 else 0)) - o[a]) * (1.0 / d[a])


def _entry1(n, s, e, o, d):
    """Item 3 of vc_render for one ray in Python floats: None on a miss, else (t_in, cell)."""
    near, far = [-math.inf] * 3, [math.inf] * 3
    for a in range(3):
        if d[a] != 0.0:
            inv = 1.0 / d[a]
            ta, tb = (_b(e[a], s[a], 0) - o[a]) * inv, (_b(e[a], s[a], n[a]) - o[a]) * inv
            near[a], far[a] = (ta, tb) if ta < tb else (tb, ta)
        elif o[a] < _b(e[a], s[a], 0) or o[a] >= _b(e[a], s[a], n[a]):
            return None
    t_in, t_out = 0.0, math.inf
    for a in range(3):
        if near[a] > t_in:
            t_in = near[a]
        if far[a] < t_out:
            t_out = far[a]
    if t_in >= t_out:
        return None
    ax = -1
    if t_in > 0.0:
        for a in (2, 1, 0):
            if near[a] == t_in:
                ax = a
    c = []
    for a in range(3):
        if ax == a:
            c.append(0 if d[a] > 0.0 else n[a] - 1)
        else:
            f = math.floor(((o[a] + t_in * d[a]) - e[a]) / s[a])
            c.append(int(f) if 0 <= f <= n[a] - 1 else (0 if f < 0 else n[a] - 1))
    return t_in, c


def ray_literal(occ, n, s, e, q, d, c0):
    """One secondary ray in Python floats -> (hit, t).  c0: the start cell (t = 0), or None for entry then walk."""
    if c0 is not None:
        c, t = list(c0), 0.0
        if not all(0 <= c[a] < n[a] for a in range(3)):
            return False, math.inf
    else:
        ent = _entry1(n, s, e, q, d)
        if ent is None:
            return False, math.inf
        t, c = ent
    for _ in range(n[0] + n[1] + n[2] + 1):
        if occ[(c[2] * n[0] + c[0]) * n[1] + c[1]]:
            return True, t
        tn = [_tn1(n, s, e, q, d, c, a) for a in range(3)]
        best = 0
        for a in (1, 2):
            if tn[a] < tn[best]:
                best = a
        c[best] += 1 if d[best] > 0.0 else -1
        t = tn[best]
        if not all(0 <= c[a] < n[a] for a in range(3)):
            break
    return False, math.inf


def light_literal(occ, rec_idx, rec_rgb, n4, grid, bounds, views, H, W, ren, lt, pixels=None):
    n, s, e = rn.grid_params(grid, bounds)
    occ = np.asarray(occ, dtype=bool).reshape(-1)
    pos = [float(v) for v in lt["pos"]]
    reach, amb, fl = float(lt["ao_reach"]), int(lt["ambient"]), lt.get("floor")
    rec_idx = [int(v) for v in rec_idx]
    table = ao_table()
    out = {"rgb": [], "depth": [], "kind": [], "shadow": [], "ao": []}
    st = {"pixels": 0, "hull_pixels": 0, "floor_pixels": 0, "shadowed": 0, "facing_away": 0, "rays_walked": 0}
    for v, view in enumerate(views):
        ov, dv = rn.pixel_rays(view, H, W, pixels)
        o = [float(x) for x in ov]
        P = dv.shape[0]
        rgb = np.array(np.asarray(ren["rgb"][v]).reshape(-1, 3), dtype=np.uint8, copy=True)
        depth = np.array(np.asarray(ren["depth"][v]).reshape(-1), dtype=np.float32, copy=True)
        kind = np.zeros(P, dtype=np.uint8)
        shadow = np.zeros(P, dtype=np.uint8)
        ao = np.full(P, RAYS, dtype=np.uint8)
        idxs = np.asarray(ren["index"][v]).reshape(-1)
        faces = np.asarray(ren["face"][v]).reshape(-1)
        st["pixels"] += P
        for p in range(P):
            d = [float(x) for x in dv[p]]
            idx, face = int(idxs[p]), int(faces[p])
            hit = idx != 0xFFFFFFFF
            t1 = float(depth[p])
            is_floor = False
            if fl is not None and d[2] != 0.0:
                tf = (float(fl["z"]) - o[2]) / d[2]
                if tf > 0.0 and (not hit or tf < t1):
                    Q = [o[a] + tf * d[a] for a in range(3)]
                    x0, x1, y0, y1 = (float(x) for x in fl["rect"])
                    is_floor = x0 <= Q[0] <= x1 and y0 <= Q[1] <= y1
            if is_floor:
                kind[p] = 2
                st["floor_pixels"] += 1
                a, sigma, c0 = 2, (-1 if o[2] < float(fl["z"]) else 1), None
                cell = float(fl["cell_mm"])
                base = [int(x) for x in np.asarray(fl["rgb"]).reshape(2, 3)[(math.floor(Q[0] / cell) + math.floor(Q[1] / cell)) & 1]]
                nrm = [0, 0, sigma]
                depth[p] = np.float32(tf)
            elif hit:
                kind[p] = 1
                st["hull_pixels"] += 1
                if face == 6:
                    continue
                Q = [o[a] + t1 * d[a] for a in range(3)]
                a, sigma = face // 2, (-1 if face % 2 == 0 else 1)
                c0 = [(idx // n[1]) % n[0], idx % n[1], idx // (n[0] * n[1])]
                c0[a] += sigma
                lo, hi = 0, len(rec_idx)
                while lo < hi:
                    mid = (lo + hi) >> 1
                    if rec_idx[mid] < idx:
                        lo = mid + 1
                    else:
                        hi = mid
                base = [int(x) for x in rec_rgb[lo]] if lo < len(rec_idx) else [0, 0, 0]
                nrm = [0, 0, 0]
                nrm[a] = sigma
                if lt.get("smooth") and lo < len(rec_idx):
                    q4 = [int(x) for x in n4[lo]]
                    if q4[3] != 0 and any(q4[:3]):
                        nrm = q4[:3]
            else:
                continue
            E = [pos[b] - Q[b] for b in range(3)] if pos[3] != 0.0 else pos[:3]
            if float(sigma) * E[a] <= 0.0:
                sh = 2
                st["facing_away"] += 1
            else:
                h, t = ray_literal(occ, n, s, e, Q, E, c0)
                sh = 1 if h and (pos[3] == 0.0 or t < 1.0) else 0
                st["shadowed"] += sh
                st["rays_walked"] += 1
            k_open = RAYS
            if reach > 0.0:
                k_open = 0
                for iu, iv, inn in table:
                    A = [0.0, 0.0, 0.0]
                    A[(a + 1) % 3] = float(iu) * s[(a + 1) % 3]
                    A[(a + 2) % 3] = float(iv) * s[(a + 2) % 3]
                    A[a] = float(sigma * inn) * s[a]
                    h, t = ray_literal(occ, n, s, e, Q, A, c0)
                    if not (h and t < reach / math.sqrt(float(iu * iu + iv * iv + inn * inn))):
                        k_open += 1
                st["rays_walked"] += RAYS
            sterm = (amb * k_open * 2 + 16) // 32
            if sh == 0:
                dot = (float(nrm[0]) * E[0] + float(nrm[1]) * E[1]) + float(nrm[2]) * E[2]
                nn = float(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2])
                ll = (E[0] * E[0] + E[1] * E[1]) + E[2] * E[2]
                c = min(dot / math.sqrt(nn * ll), 1.0) if dot > 0.0 else 0.0
                sterm += int(math.floor(float(255 - amb) * c + 0.5))
            rgb[p] = [(bk * sterm + 127) // 255 for bk in base]
            shadow[p] = sh
            ao[p] = k_open
        for key, val in (("rgb", rgb), ("depth", depth), ("kind", kind), ("shadow", shadow), ("ao", ao)):
            out[key].append(val)
    res = {k: np.stack(val) for k, val in out.items()}
    res["stats"] = st
    return res
