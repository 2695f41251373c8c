"""Restatement of the free-viewpoint texturing pass (vc_texture_render, include/voxcarve.h).

TEST INFRASTRUCTURE ONLY.  Two forms of one contract: `texture_view` (vectorised over the hit pixels of one view) and
`texture_literal` (pixel by pixel, step by step, camera by camera in plain Python floats).  The pixel ray is vc_render's
(render_np.pixel_rays), the projection the carve's (oracle/carve_np.project_points in the vectorised form, the operation order of
csrc/vc_device.h in the literal one).

Inputs per view: the render's hit mask bool [P], depth f32 [P] and rgb u8 [P, 3] (P = H W, flat v W + u), the view as
render_np.view_params gives it; the carve's cameras as (K, dist, R, tvec), the masks the carve read as bool [C, Hc, Wc] (after its
post-filter) and m (its min_views after the clamp to >= 1); the depth maps of vc_color_visible as u32 [C, Hc Wc] (float32 bits);
every camera's BGR frame [Hc, Wc, 3].  Outputs: rgb u8 [P, 3], depth f32 [P], count u8 [P], best_cam u8 [P], refined u8 [P] and
the contract's stats.
"""
import math
import sys

import numpy as np

import render_np as rn
import surface_np as sn
from oracle.carve_np import pixel_offsets, project_points

MAX_STEPS, MAX_BEST, MAX_SHARPEN = 24, 16, 6
FILTERS = {"nearest": 0, "bilinear": 1}


def camera_centre(cam):
    """C_j = -((R[0][j] t0 + R[1][j] t1) + R[2][j] t2), as the render makes a view's origin."""
    _, _, R, tv = cam
    R = np.asarray(R, dtype=np.float64).reshape(3, 3).tolist()
    t0, t1, t2 = np.asarray(tv, dtype=np.float64).reshape(3).tolist()
    return [-((R[0][j] * t0 + R[1][j] * t1) + R[2][j] * t2) for j in range(3)]


def _cam_z(cam, P):
    _, _, R, tv = cam
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(tv, dtype=np.float64).reshape(3)
    return R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1] + R[2, 2] * P[:, 2] + t[2]


def _points(o, d, t):
    return np.stack([o[j] + t * d[:, j] for j in range(3)], axis=1)


def _frame_rgb(frame):
    return np.asarray(frame, dtype=np.uint8).reshape(-1, 3)[:, ::-1].astype(np.int64)        # BGR -> RGB per pixel


def bracket(o, d, t0, cams, masks, m, steps, reach):
    """Item 3 for rays (o, d [N, 3]) with render depths t0 f64 [N] -> dict t, refined, lo, hi, lo0, clamped."""
    N = t0.size
    inside = lambda t: sn.count_views(_points(o, d, t), cams, masks) >= m
    lo, hi = t0.copy(), t0.copy()
    refined = np.zeros(N, dtype=bool)
    clamped = np.zeros(N, dtype=bool)
    if steps > 0 and N:
        in0 = inside(t0)
        back = t0 - reach
        clamped = in0 & ~(back > 0.0)
        lo = np.where(in0, np.where(back > 0.0, back, 0.0), t0)
        hi = np.where(in0, t0, t0 + reach)
        refined = ~inside(lo) & inside(hi)
    lo0 = lo.copy()
    r = np.nonzero(refined)[0]
    for _ in range(steps):
        if r.size == 0:
            break
        mid = (lo[r] + hi[r]) * 0.5
        ins = sn.count_views(_points(o, d[r], mid), cams, masks) >= m
        hi[r] = np.where(ins, mid, hi[r])
        lo[r] = np.where(ins, lo[r], mid)
    t = np.where(refined, (lo + hi) * 0.5, t0)
    return {"t": t, "refined": refined, "lo": lo, "hi": hi, "lo0": lo0, "clamped": clamped}


def weights(P, o, cams, zmaps, Hc, Wc, tol, sharpen):
    """Items 4 and 5: (w int64 [C, N], uv f64 [C, N, 2]); w = 0 where the camera is no candidate."""
    N, C = P.shape[0], len(cams)
    tol = np.float32(tol)
    w = np.zeros((C, N), dtype=np.int64)
    uvs = np.zeros((C, N, 2), dtype=np.float64)
    b = [o[j] - P[:, j] for j in range(3)]
    bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    with np.errstate(all="ignore"):
        for c, cam in enumerate(cams):
            K, dist, R, tv = cam
            dz = _cam_z(cam, P)
            uv = project_points(P, R, tv, K, dist)
            uvs[c] = uv
            off = pixel_offsets(uv, Hc, Wc)
            cand = (dz > 0.0) & (off >= 0)
            zm = np.asarray(zmaps[c], dtype=np.uint32).view(np.float32)[np.where(cand, off, 0)]
            cand &= dz.astype(np.float32) <= zm + tol
            cc = camera_centre(cam)
            a = [cc[j] - P[:, j] for j in range(3)]
            dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
            aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
            nn = aa * bb
            ok = (dot > 0.0) & np.isfinite(nn) & (nn >= sys.float_info.min)
            cw = np.where(ok, np.minimum(dot / np.sqrt(np.where(ok, nn, 1.0)), 1.0), 0.0)
            for _ in range(sharpen):
                cw = cw * cw
            w[c] = np.where(cand, np.floor(cw * 65535.0 + 0.5).astype(np.int64), 0)
    return w, uvs


def keep_best(w, best):
    """(kept bool [C, N], rank int64 [C, N]): the `best` largest weights, ties to the lower camera index; zero weights never stay."""
    C = w.shape[0]
    rank = np.zeros_like(w)
    for c in range(C):
        for e in range(C):
            rank[c] += (w[e] > w[c]) | ((w[e] == w[c]) & (e < c))
    return (w > 0) & (rank < best), rank


def sample(frame, uv, Hc, Wc, filt):
    """Item 6: RGB int64 [N, 3] of the BGR frame at float pixel coordinates uv [N, 2] (inside the image)."""
    f = _frame_rgb(frame)
    u, v = uv[:, 0], uv[:, 1]
    if filt == 0:
        return f[v.astype(np.int64) * Wc + u.astype(np.int64)]
    fu, fv = u - 0.5, v - 0.5
    x0, y0 = np.floor(fu), np.floor(fv)
    ax = np.floor((fu - x0) * 256.0).astype(np.int64)[:, None]
    ay = np.floor((fv - y0) * 256.0).astype(np.int64)[:, None]
    xa, xb = np.clip(x0.astype(np.int64), 0, Wc - 1), np.clip(x0.astype(np.int64) + 1, 0, Wc - 1)
    ya, yb = np.clip(y0.astype(np.int64), 0, Hc - 1), np.clip(y0.astype(np.int64) + 1, 0, Hc - 1)
    p00, p10, p01, p11 = f[ya * Wc + xa], f[ya * Wc + xb], f[yb * Wc + xa], f[yb * Wc + xb]
    return ((p00 * (256 - ax) + p10 * ax) * (256 - ay) + (p01 * (256 - ax) + p11 * ax) * ay + 32768) >> 16


def texture_view(view, H, W, hit, depth, rgb, cams, masks, m, zmaps, frames, steps=8, reach=0.0, tol=0.0, best=2, sharpen=2,
                 filt=1, with_interval=False):
    """Vectorised form for one view -> dict rgb, depth, count, best_cam, refined, stats (and the bracket when asked)."""
    masks = np.asarray(masks, dtype=bool)
    C, Hc, Wc = masks.shape
    P_all = H * W
    hit = np.asarray(hit, dtype=bool).reshape(P_all)
    px = np.nonzero(hit)[0]
    out_rgb = np.array(rgb, dtype=np.uint8).reshape(P_all, 3).copy()
    out_depth = np.full(P_all, np.inf, dtype=np.float32)
    count = np.zeros(P_all, dtype=np.uint8)
    best_cam = np.full(P_all, 255, dtype=np.uint8)
    refined = np.zeros(P_all, dtype=np.uint8)
    o, d = rn.pixel_rays(view, H, W, px)
    t0 = np.asarray(depth, dtype=np.float32).reshape(P_all)[px].astype(np.float64)
    br = bracket(o, d, t0, cams, masks, m, steps, float(reach))
    out_depth[px] = br["t"].astype(np.float32)
    refined[px] = br["refined"]
    P = _points(o, d, br["t"])
    w, uvs = weights(P, o, cams, zmaps, Hc, Wc, tol, sharpen)
    kept, rank = keep_best(w, best)
    ws = np.zeros(px.size, dtype=np.int64)
    acc = np.zeros((px.size, 3), dtype=np.int64)
    cnt = np.zeros(px.size, dtype=np.int64)
    top = np.full(px.size, 255, dtype=np.int64)
    for c in range(C):
        k = np.nonzero(kept[c])[0]
        if not k.size:
            continue
        acc[k] += w[c, k][:, None] * sample(frames[c], uvs[c, k], Hc, Wc, filt)
        ws[k] += w[c, k]
        cnt[k] += 1
        top[k] = np.where(rank[c, k] == 0, c, top[k])
    has = ws > 0
    out_rgb[px[has]] = ((acc[has] + (ws[has] // 2)[:, None]) // ws[has][:, None]).astype(np.uint8)
    count[px] = cnt
    best_cam[px] = top
    out = {"rgb": out_rgb, "depth": out_depth, "count": count, "best_cam": best_cam, "refined": refined,
           "stats": {"pixels": P_all, "hits": int(px.size), "refined": int(br["refined"].sum()), "textured": int(has.sum()),
                     "fallback": int(px.size - has.sum())}}
    if with_interval:
        out.update(px=px, o=o, d=d, t0=t0, lo=br["lo"], hi=br["hi"], lo0=br["lo0"], clamped=br["clamped"], w=w, kept=kept)
    return out


def texture(views, H, W, hit, depth, rgb, cams, masks, m, zmaps, frames, **kw):
    """Every view of a render (hit [V, P], depth [V, P], rgb [V, P, 3]) -> the outputs stacked [V, ...] and the summed stats."""
    outs = [texture_view(view, H, W, hit[k], depth[k], rgb[k], cams, masks, m, zmaps, frames, **kw) for k, view in enumerate(views)]
    res = {key: np.stack([o[key] for o in outs]) for key in ("rgb", "depth", "count", "best_cam", "refined")}
    res["stats"] = {key: sum(o["stats"][key] for o in outs) for key in outs[0]["stats"]}
    return res


# ---------------------------------------------------------------------------------------------------------------- literal form
def _project_literal(cam, X, Y, Z):
    """(u, v, camera z) of one point: csrc/vc_device.h's project_point, operation for operation."""
    K, dist, R, tv = cam
    R = np.asarray(R, dtype=np.float64).reshape(9).tolist()
    t = np.asarray(tv, dtype=np.float64).reshape(3).tolist()
    K = np.asarray(K, dtype=np.float64).reshape(9).tolist()
    k1, k2, p1, p2, k3 = np.asarray(dist, dtype=np.float64).reshape(5).tolist()
    x = R[0] * X + R[1] * Y + R[2] * Z + t[0]
    y = R[3] * X + R[4] * Y + R[5] * Z + t[1]
    dz = R[6] * X + R[7] * Y + R[8] * Z + t[2]
    z = 1.0 / dz if dz != 0.0 else 1.0
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
    return xd * K[0] + K[2], yd * K[4] + K[5], dz


def _sample_literal(frame, u, v, Hc, Wc, filt):
    f = np.asarray(frame, dtype=np.uint8)

    def rgb(y, x):
        b, g, r = (int(a) for a in f[y, x])
        return r, g, b
    if filt == 0:
        return rgb(int(v), int(u))
    fu, fv = u - 0.5, v - 0.5
    x0, y0 = math.floor(fu), math.floor(fv)
    ax, ay = int(math.floor((fu - x0) * 256.0)), int(math.floor((fv - y0) * 256.0))
    xa, xb = min(max(x0, 0), Wc - 1), min(max(x0 + 1, 0), Wc - 1)
    ya, yb = min(max(y0, 0), Hc - 1), min(max(y0 + 1, 0), Hc - 1)
    p00, p10, p01, p11 = rgb(ya, xa), rgb(ya, xb), rgb(yb, xa), rgb(yb, xb)
    return tuple(((p00[k] * (256 - ax) + p10[k] * ax) * (256 - ay) + (p01[k] * (256 - ax) + p11[k] * ax) * ay + 32768) >> 16
                 for k in range(3))


def texture_literal(view, H, W, hit, depth, rgb, cams, masks, m, zmaps, frames, steps=8, reach=0.0, tol=0.0, best=2, sharpen=2,
                    filt=1, pixels=None):
    """The same contract one pixel at a time (all pixels, or the listed flat indices) -> dict of rgb [k, 3], depth f32 [k],
    count, best_cam, refined [k] in the order of the pixels."""
    masks = np.asarray(masks, dtype=bool)
    C, Hc, Wc = masks.shape
    hit = np.asarray(hit, dtype=bool).reshape(-1)
    depth = np.asarray(depth, dtype=np.float32).reshape(-1)
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    tol = np.float32(tol)
    reach = float(reach)
    centres = [camera_centre(cam) for cam in cams]
    sel = range(H * W) if pixels is None else [int(p) for p in pixels]
    out = {"rgb": [], "depth": [], "count": [], "best_cam": [], "refined": []}

    def emit(c, t, n, top, ref):
        out["rgb"].append([int(a) for a in c]); out["depth"].append(np.float32(t)); out["count"].append(n)
        out["best_cam"].append(top); out["refined"].append(ref)

    with np.errstate(all="ignore"):
        for p in sel:
            if not hit[p]:
                emit(rgb[p], np.inf, 0, 255, 0)
                continue
            o, d = rn.pixel_rays(view, H, W, [p])
            o, d = o.tolist(), d[0].tolist()
            t0 = float(depth[p])
            at = lambda t: [o[j] + t * d[j] for j in range(3)]
            inside = lambda t: sn._inside_literal(cams, masks, m, at(t))
            t, ref = t0, 0
            if steps > 0:
                lo, hi = (max(t0 - reach, 0.0), t0) if inside(t0) else (t0, t0 + reach)
                if not inside(lo) and inside(hi):
                    ref = 1
                    for _ in range(steps):
                        mid = (lo + hi) * 0.5
                        if inside(mid):
                            hi = mid
                        else:
                            lo = mid
                    t = (lo + hi) * 0.5
            P = at(t)
            b = [o[j] - P[j] for j in range(3)]
            bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
            heap = []                                   # the candidates, heaviest first, ties to the lower camera: by insertion
            for c in range(C):
                u, v, dz = _project_literal(cams[c], *P)
                if not (dz > 0.0 and 0.0 <= v < Hc and 0.0 <= u < Wc):
                    continue
                zm = np.asarray(zmaps[c], dtype=np.uint32)[int(v) * Wc + int(u):][:1].view(np.float32)[0]
                if not np.float32(dz) <= np.float32(zm + tol):
                    continue
                a = [centres[c][j] - P[j] for j in range(3)]
                dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
                aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
                nn = aa * bb
                cw = min(dot / math.sqrt(nn), 1.0) if dot > 0.0 and math.isfinite(nn) and nn >= sys.float_info.min else 0.0
                for _ in range(sharpen):
                    cw = cw * cw
                wc = int(math.floor(cw * 65535.0 + 0.5))
                k = 0
                while k < len(heap) and heap[k][0] >= wc:
                    k += 1
                heap.insert(k, (wc, c, u, v))
                del heap[best:]
            heap = [h for h in heap if h[0] > 0]
            ws = sum(h[0] for h in heap)
            if ws == 0:
                emit(rgb[p], t, 0, 255, ref)
                continue
            tot = [0, 0, 0]
            for wc, c, u, v in heap:
                s = _sample_literal(frames[c], u, v, Hc, Wc, filt)
                tot = [tot[k] + wc * s[k] for k in range(3)]
            emit([(a + ws // 2) // ws for a in tot], t, len(heap), heap[0][1], ref)
    return {"rgb": np.array(out["rgb"], dtype=np.uint8).reshape(-1, 3), "depth": np.array(out["depth"], dtype=np.float32),
            "count": np.array(out["count"], dtype=np.uint8), "best_cam": np.array(out["best_cam"], dtype=np.uint8),
            "refined": np.array(out["refined"], dtype=np.uint8)}
