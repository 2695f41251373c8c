"""Restatement of photo-consistency carving (vc_photo_carve, include/voxcarve.h).

TEST INFRASTRUCTURE ONLY.  Two forms of one contract: `photo_carve` (vectorised, built on visible_np.color_visible) and
`photo_carve_literal` (round by round, voxel by voxel, camera by camera, on visible_np.color_visible_literal).

Inputs: the carve result A1 as ascending linear indices `idx` and their RGB, grid, bounds, cameras as (K, dist, R, tvec), every
camera's BGR frame [H, W, 3], tol (None = the voxel diagonal), T = var_threshold, m = min_views, R = max_rounds.
Output: dict with idx (F, ascending), rgb u8 [|F|, 3] (coloured as color_visible colours the input records restricted to F),
zmaps u32 [C, H*W] and vis u16 [|F|] of color_visible on F, rounds u8 [S0] (0 = kept), n_rounds (rounds evaluated, the empty
round that shows convergence included) and converged.
"""
import numpy as np

import visible_np as vn
from oracle.carve_np import axis_tables, project_points


def _centres(idx, grid, bounds):
    nx, ny, nz = grid
    xs, ys, zs = axis_tables(nx, ny, nz, bounds)
    idx = np.asarray(idx, dtype=np.int64)
    iy, t = idx % ny, idx // ny
    ix, iz = t % nx, t // nx
    return np.stack([xs[ix], ys[iy], zs[iz]], axis=1)


def inconsistent(idx, vis, grid, bounds, cams, frames, H, W, var_threshold, min_views):
    """bool [S]: n = popcount(vis) >= m and D = sum_k (n q_k - s_k^2) > T n^2, over the visible cameras' samples at the centre."""
    S = len(idx)
    vis = np.asarray(vis, dtype=np.int64)
    s = np.zeros((S, 3), dtype=np.int64)
    q = np.zeros((S, 3), dtype=np.int64)
    n = np.zeros(S, dtype=np.int64)
    rows = np.nonzero(vis)[0]
    if rows.size:
        P = _centres(np.asarray(idx)[rows], grid, bounds)
        for c, (K, dist, R, tv) in enumerate(cams):
            on = np.nonzero((vis[rows] >> c) & 1)[0]
            if on.size == 0:
                continue
            with np.errstate(all="ignore"):
                uv = project_points(P[on], R, tv, K, dist)
            pix = uv[:, 1].astype(np.int64) * W + uv[:, 0].astype(np.int64)     # visible: inside the image, v, u >= 0
            ch = vn._frame_rgb(frames[c])[pix]
            s[rows[on]] += ch
            q[rows[on]] += ch * ch
            n[rows[on]] += 1
    D = (n[:, None] * q - s * s).sum(axis=1)
    return (n >= min_views) & (D > np.int64(var_threshold) * n * n)


def photo_carve(idx, rgb, grid, bounds, cams, frames, H, W, var_threshold=1200, min_views=2, max_rounds=32, tol=None):
    """Vectorised form."""
    idx0 = np.asarray(idx, dtype=np.int64)
    rgb0 = np.array(rgb, dtype=np.uint8).reshape(idx0.size, 3)
    rounds = np.zeros(idx0.size, dtype=np.uint8)
    alive = np.ones(idx0.size, dtype=bool)
    r, converged = 0, False
    while r < max_rounds:
        r += 1
        cur = np.nonzero(alive)[0]
        _, vis, _ = vn.color_visible(idx0[cur], rgb0[cur], grid, bounds, cams, frames, H, W, tol)
        bad = inconsistent(idx0[cur], vis, grid, bounds, cams, frames, H, W, var_threshold, min_views)
        if not bad.any():
            converged = True
            break
        rounds[cur[bad]] = r
        alive[cur[bad]] = False
    keep = np.nonzero(alive)[0]
    zmaps, vis, out = vn.color_visible(idx0[keep], rgb0[keep], grid, bounds, cams, frames, H, W, tol)
    return {"idx": idx0[keep].astype(np.uint32), "rgb": out, "zmaps": zmaps, "vis": vis, "rounds": rounds, "n_rounds": r,
            "converged": converged}


def photo_carve_literal(idx, rgb, grid, bounds, cams, frames, H, W, var_threshold=1200, min_views=2, max_rounds=32, tol=None):
    """The same contract, one round, one voxel, one camera at a time."""
    nx, ny, nz = grid
    xs, ys, zs = axis_tables(nx, ny, nz, bounds)
    idx0 = [int(i) for i in idx]
    rgb0 = np.array(rgb, dtype=np.uint8).reshape(len(idx0), 3)
    rounds = [0] * len(idx0)
    r, converged = 0, False
    while r < max_rounds:
        r += 1
        cur = [k for k in range(len(idx0)) if rounds[k] == 0]
        _, vis, _ = vn.color_visible_literal([idx0[k] for k in cur], rgb0[cur], grid, bounds, cams, frames, H, W, tol)
        removed = []
        for j, k in enumerate(cur):                       # every decision of the round reads A_r only
            i = idx0[k]
            X, Y, Z = float(xs[(i // ny) % nx]), float(ys[i % ny]), float(zs[i // (nx * ny)])
            n, s, q = 0, [0, 0, 0], [0, 0, 0]
            for c, (K, dist, R, tv) in enumerate(cams):
                if not (int(vis[j]) >> c) & 1:
                    continue
                with np.errstate(all="ignore"):
                    u, v = project_points(np.array([(X, Y, Z)]), R, tv, K, dist)[0]
                b, g, rr = (int(a) for a in np.asarray(frames[c]).reshape(-1, 3)[int(v) * W + int(u)])
                n += 1
                for ch, val in enumerate((rr, g, b)):
                    s[ch] += val
                    q[ch] += val * val
            D = sum(n * q[ch] - s[ch] * s[ch] for ch in range(3))
            if n >= min_views and D > int(var_threshold) * n * n:
                removed.append(k)
        if not removed:
            converged = True
            break
        for k in removed:
            rounds[k] = r
    keep = [k for k in range(len(idx0)) if rounds[k] == 0]
    zmaps, vis, out = vn.color_visible_literal([idx0[k] for k in keep], rgb0[keep], grid, bounds, cams, frames, H, W, tol)
    return {"idx": np.array([idx0[k] for k in keep], dtype=np.uint32), "rgb": out, "zmaps": zmaps, "vis": vis,
            "rounds": np.array(rounds, dtype=np.uint8), "n_rounds": r, "converged": converged}


def occupancy_words(idx, n):
    """u64 [ceil(n / 64)]: bit i & 63 of word i >> 6 set for every index in idx (vc_fetch_occupancy's layout)."""
    words = np.zeros((n + 63) // 64, dtype=np.uint64)
    idx = np.asarray(idx, dtype=np.uint64)
    np.bitwise_or.at(words, (idx >> np.uint64(6)).astype(np.int64), np.uint64(1) << (idx & np.uint64(63)))
    return words
