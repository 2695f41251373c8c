"""Restatement of vc_hull_clusters and vc_paint_clusters (include/voxcarve.h): K-means of the hull's
survivors on the floor plane, in integers.  A volume is a bool array occ[iz, ix, iy] (linear index i = (iz nx + ix) ny + iy, the
grid's order; distance_np.volume makes one from record indices); a floor position is a column col = ix ny + iy at
P = (q_x ix, q_y iy) micrometres from the grid's (x_min, y_min) corner, q = steps_um_xy(grid, bounds).  Two forms:

  clusters_literal(occ, q, K, ...)   the contract read aloud: one survivor, one column, one centre at a time, in Python integers
  clusters(occ, q, K, ...)           vectorised over the columns in int64 (every sum stays below 2^62)

Both return the same dict (see clusters).  describe(records, grid, result, hist_iz) gives what the fetch calls return per record
and per cluster, paint(records, labels, palette) what vc_paint_clusters leaves in the records."""
import numpy as np

MAX_K = 16
MAX_ITERS = 255
EMPTY_LO, EMPTY_HI = 0xffffffff, 0            # lo / hi of a cluster without a survivor: lo > hi on every axis
NO_LABEL = 255                                # floor label of a column without a survivor
INIT_LIMIT = 1 << 30                          # |init| may not exceed it: d2 then stays inside int64


def steps_um_xy(grid, bounds):
    """(q_x, q_y): item 2 of vc_hull_distance for the x and y axes, the library's refusals as ValueError."""
    q = []
    for a in range(2):
        n = grid[a]
        if n < 2:
            raise ValueError("axis %d has %d cells" % (a, n))
        s = (float(bounds[2 * a + 1]) - float(bounds[2 * a])) / float(n - 1)
        v = int(np.rint(s * 1000.0))
        if not 1 <= v <= 1 << 20 or (n + 1) * v > 1 << 30:
            raise ValueError("axis %d: step %r um out of range" % (a, v))
        q.append(v)
    return tuple(q)


def _check(K, max_iters, init):
    if not 1 <= K <= MAX_K:
        raise ValueError("K = %r not in 1..%d" % (K, MAX_K))
    if not 1 <= max_iters <= MAX_ITERS:
        raise ValueError("max_iters = %r not in 1..%d" % (max_iters, MAX_ITERS))
    if init is not None:
        init = [[int(v) for v in c] for c in init]
        if len(init) != K or any(len(c) != 2 for c in init):
            raise ValueError("init must hold K centres (x, y)")
        if any(abs(v) > INIT_LIMIT for c in init for v in c):
            raise ValueError("init centre beyond 2^30 um")
    return init


def floor_map(occ):
    """u32 [nx ny]: survivors per column."""
    return np.asarray(occ, dtype=bool).sum(axis=0, dtype=np.uint32).reshape(-1)


# ---- literal --------------------------------------------------------------------------------------------------------------------
def clusters_literal(occ, q, K, max_iters=32, min_column=1, init=None):
    init = _check(K, max_iters, init)
    nz, nx, ny = occ.shape
    qx, qy = int(q[0]), int(q[1])
    n = [0] * (nx * ny)
    for iz in range(nz):
        for ix in range(nx):
            for iy in range(ny):
                if occ[iz, ix, iy]:
                    n[((iz * nx + ix) * ny + iy) % (nx * ny)] += 1
    w = [c if c >= min_column else 0 for c in n]
    P = [(qx * (col // ny), qy * (col % ny)) for col in range(nx * ny)]
    d2 = lambda p, c: (p[0] - c[0]) ** 2 + (p[1] - c[1]) ** 2
    Wtot = sum(w)
    centres = [tuple(c) for c in init] if init is not None else [(0, 0)] * K
    labels = [0 if n[col] else NO_LABEL for col in range(nx * ny)]
    W = [0] * K
    iterations, converged = 0, 1
    if Wtot:
        if init is None:
            M = ((sum(w[c] * P[c][0] for c in range(nx * ny)) + Wtot // 2) // Wtot,
                 (sum(w[c] * P[c][1] for c in range(nx * ny)) + Wtot // 2) // Wtot)
            weighted = [c for c in range(nx * ny) if w[c] > 0]
            best = None
            for c in weighted:                                   # ascending col: a tie keeps the earlier one
                if best is None or d2(P[c], M) < d2(P[best], M):
                    best = c
            centres = [P[best]]
            for j in range(1, K):
                best, best_v = None, -1
                for c in weighted:
                    v = min(d2(P[c], ci) for ci in centres)
                    if v > best_v:
                        best, best_v = c, v
                centres.append(P[best])
        converged = 0
        for r in range(1, max_iters + 1):
            for col in range(nx * ny):
                if n[col]:
                    k_best = 0
                    for k in range(1, K):
                        if d2(P[col], centres[k]) < d2(P[col], centres[k_best]):
                            k_best = k
                    labels[col] = k_best
            new = list(centres)
            for k in range(K):
                cols = [c for c in range(nx * ny) if n[c] and labels[c] == k]
                W[k] = sum(w[c] for c in cols)
                if W[k] > 0:
                    new[k] = ((sum(w[c] * P[c][0] for c in cols) + W[k] // 2) // W[k],
                              (sum(w[c] * P[c][1] for c in cols) + W[k] // 2) // W[k])
            iterations = r
            same = new == centres
            centres = new
            if same:
                converged = 1
                break
    return {"centres": np.array(centres, dtype=np.int64).reshape(K, 2), "floor_map": np.array(n, dtype=np.uint32),
            "floor_labels": np.array(labels, dtype=np.uint8), "cluster_weight": np.array(W, dtype=np.uint64),
            "iterations": iterations, "converged": converged, "weight": Wtot, "columns": sum(1 for c in n if c),
            "survivors": sum(n), "q": (qx, qy)}


# ---- vectorised -----------------------------------------------------------------------------------------------------------------
def _d2(Px, Py, c):
    dx, dy = Px - np.int64(c[0]), Py - np.int64(c[1])
    return dx * dx + dy * dy


def clusters(occ, q, K, max_iters=32, min_column=1, init=None):
    """K-means of the columns, weighted by their survivors.  Returns a dict: centres int64 [K, 2] (um), floor_map u32 [nx ny],
    floor_labels u8 [nx ny] (255 = no survivor), cluster_weight u64 [K] (W_k of the last round), iterations, converged, weight
    (Wtot), columns (with a survivor), survivors, q."""
    init = _check(K, max_iters, init)
    nz, nx, ny = occ.shape
    qx, qy = int(q[0]), int(q[1])
    n = floor_map(occ)
    w = np.where(n >= min_column, n, 0).astype(np.int64)
    col = np.arange(nx * ny, dtype=np.int64)
    Px, Py = qx * (col // ny), qy * (col % ny)
    Wtot = int(w.sum())
    centres = np.array(init if init is not None else np.zeros((K, 2)), dtype=np.int64).reshape(K, 2)
    labels = np.where(n > 0, 0, NO_LABEL).astype(np.uint8)
    W = np.zeros(K, dtype=np.int64)
    iterations, converged = 0, 1
    on = np.flatnonzero(n > 0)
    if Wtot:
        if init is None:
            M = ((int((w * Px).sum()) + Wtot // 2) // Wtot, (int((w * Py).sum()) + Wtot // 2) // Wtot)
            cand = np.flatnonzero(w > 0)
            first = cand[np.argmin(_d2(Px[cand], Py[cand], M))]      # argmin / argmax return the first of equal values
            centres[0] = (Px[first], Py[first])
            near = _d2(Px[cand], Py[cand], centres[0])
            for j in range(1, K):
                c = cand[np.argmax(near)]
                centres[j] = (Px[c], Py[c])
                near = np.minimum(near, _d2(Px[cand], Py[cand], centres[j]))
        converged = 0
        for r in range(1, max_iters + 1):
            d = np.stack([_d2(Px[on], Py[on], centres[k]) for k in range(K)])
            lab = np.argmin(d, axis=0)
            labels[on] = lab
            new = centres.copy()
            for k in range(K):
                m = on[lab == k]
                W[k] = w[m].sum()
                if W[k] > 0:
                    Wk = int(W[k])
                    new[k] = ((int((w[m] * Px[m]).sum()) + Wk // 2) // Wk, (int((w[m] * Py[m]).sum()) + Wk // 2) // Wk)
            iterations = r
            same = np.array_equal(new, centres)
            centres = new
            if same:
                converged = 1
                break
    return {"centres": centres, "floor_map": n, "floor_labels": labels, "cluster_weight": W.astype(np.uint64),
            "iterations": iterations, "converged": converged, "weight": Wtot, "columns": int(on.size),
            "survivors": int(n.sum(dtype=np.int64)), "q": (qx, qy)}


# ---- per record and per cluster -------------------------------------------------------------------------------------------------
def describe(records, grid, result, hist_iz=None):
    """What the fetch calls return for u64 records [S] of the volume `result` was made from: labels u8 [S]; per cluster voxels
    u64 [K], weight u64 [K], columns u32 [K], lo / hi u32 [K, 3] (inclusive box in (ix, iy, iz); EMPTY_LO / EMPTY_HI without a
    survivor), centres; histograms u32 [K, 512] over the records with seen = 1 and hist_iz[0] <= iz <= hist_iz[1] (default: every
    layer), bin (r >> 5) << 6 | (g >> 5) << 3 | (b >> 5)."""
    nx, ny, nz = grid
    rec = np.asarray(records, dtype=np.uint64)
    K = result["centres"].shape[0]
    idx = (rec & np.uint64(0xffffffff)).astype(np.int64)
    col, iz = idx % (nx * ny), idx // (nx * ny)
    ix, iy = col // ny, col % ny
    labels = result["floor_labels"][col]
    lo_z, hi_z = (0, nz - 1) if hist_iz is None else hist_iz
    r, g, b = [((rec >> np.uint64(s)) & np.uint64(255)).astype(np.int64) for s in (32, 40, 48)]
    seen = ((rec >> np.uint64(56)) & np.uint64(1)).astype(bool)
    bins = ((r >> 5) << 6) | ((g >> 5) << 3) | (b >> 5)
    out = {"labels": labels.astype(np.uint8), "centres": result["centres"], "weight": result["cluster_weight"],
           "voxels": np.zeros(K, np.uint64), "columns": np.zeros(K, np.uint32), "lo": np.full((K, 3), EMPTY_LO, np.uint32),
           "hi": np.full((K, 3), EMPTY_HI, np.uint32), "histograms": np.zeros((K, 512), np.uint32)}
    fl, n = result["floor_labels"], result["floor_map"]
    for k in range(K):
        m = labels == k
        out["voxels"][k] = m.sum()
        out["columns"][k] = ((fl == k) & (n > 0)).sum()
        if m.any():
            out["lo"][k] = (ix[m].min(), iy[m].min(), iz[m].min())
            out["hi"][k] = (ix[m].max(), iy[m].max(), iz[m].max())
        h = m & seen & (iz >= lo_z) & (iz <= hi_z)
        out["histograms"][k] = np.bincount(bins[h], minlength=512)
    return out


def paint(records, labels, palette):
    """The records after vc_paint_clusters: RGB = palette[label] (u8 [K, 3]), index and seen byte unchanged."""
    rec = np.asarray(records, dtype=np.uint64)
    pal = np.asarray(palette, dtype=np.uint64)[np.asarray(labels, dtype=np.int64)]
    rgb = (pal[:, 0] << np.uint64(32)) | (pal[:, 1] << np.uint64(40)) | (pal[:, 2] << np.uint64(48))
    return (rec & np.uint64(0xff000000ffffffff)) | rgb


def centres_world_mm(centres, bounds):
    """The centres in world millimetres: min + um / 1000."""
    c = np.asarray(centres, dtype=np.float64)
    return np.stack([float(bounds[0]) + c[:, 0] / 1000.0, float(bounds[2]) + c[:, 1] / 1000.0], axis=1)


# ---- the scene of the tests: three figures on the floor --------------------------------------------------------------------------
FIGURE_CENTRES = ((-100.0, -600.0, -768.0), (700.0, -200.0, -768.0), (100.0, 600.0, -768.0))
FIGURE_RADII = (160.0, 140.0, 700.0)


def three_figures(H=120, W=160, n_cameras=8):
    """(cams, masks): synthetic.ring_cameras(n_cameras, H, W) and, per camera, the OR of the noise-free ellipsoid masks of three
    upright figures (FIGURE_RADII) at FIGURE_CENTRES."""
    from voxcarve import synthetic
    cams = synthetic.ring_cameras(n_cameras, H, W)
    per = [synthetic.ellipsoid_masks(cams, H, W, radii=FIGURE_RADII, centre=c, noise=0) for c in FIGURE_CENTRES]
    return cams, [np.maximum(np.maximum(a, b), c) for a, b, c in zip(*per)]
