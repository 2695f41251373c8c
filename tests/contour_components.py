"""numpy restatement of the device formulation of the contour stage (csrc/vc_contour.h), held to tests/contour_literal.py.

Components of the image padded with a ring of zeros: foreground 8-connected, background 4-connected, the padding's
background component is the frame.  A component's label is its raster-first pixel; its parent is the component of that
pixel's left neighbour (the frame has none).  contourArea of a component's border = the area of the cells between pixel
centres (the padded image's (H+1) x (W+1) cells) attributed to it and to all its descendants, in half units:
    4 corners fg          2 -> the fg component
    3 corners fg          1 -> the fg component, 1 -> the bg corner's component
    2 fg, edge-adjacent   2 -> the bg component
    2 fg, diagonal        1 -> each bg corner's component
    0 or 1 corner fg      2 -> the bg component
Outer borders have a negative oriented area, hole borders a positive one.  The per-pixel output rule is in fill_figures."""
import numpy as np


def _find(par, a):
    r = a
    while par[r] != r:
        r = par[r]
    while par[a] != r:
        par[a], a = r, par[a]
    return r


def components(mask):
    """(labels [H+2, W+2] int64 = raster-first padded linear index of each pixel's component, fg [H+2, W+2] bool)."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    fg = np.zeros((H + 2, W + 2), dtype=bool)
    fg[1:-1, 1:-1] = m
    Wp = W + 2
    n = (H + 2) * Wp
    par = list(range(n))
    flat = fg.ravel().tolist()

    def union(a, b):
        ra, rb = _find(par, a), _find(par, b)
        if ra != rb:
            if ra < rb:
                par[rb] = ra
            else:
                par[ra] = rb
    for i in range(n):
        y, x = divmod(i, Wp)
        v = flat[i]
        if x > 0 and flat[i - 1] == v:
            union(i, i - 1)
        if y > 0 and flat[i - Wp] == v:
            union(i, i - Wp)
        if v and y > 0:
            if x > 0 and flat[i - Wp - 1]:
                union(i, i - Wp - 1)
            if x + 1 < Wp and flat[i - Wp + 1]:
                union(i, i - Wp + 1)
    lab = np.array([_find(par, i) for i in range(n)], dtype=np.int64).reshape(H + 2, Wp)
    return lab, fg


def fill_figures(mask, figure_threshold, figure_inner_threshold):
    m = np.asarray(mask)
    H, W = m.shape
    lab, fg = components(m)
    Wp = W + 2
    roots = np.unique(lab)
    frame = 0                                             # padded pixel 0 is background and raster-first
    parent = {}
    for r in roots.tolist():
        parent[r] = None if r == frame else int(lab.ravel()[r - 1])
    # cell attribution (half units)
    own = {r: 0 for r in roots.tolist()}
    c = [fg[:-1, :-1], fg[:-1, 1:], fg[1:, :-1], fg[1:, 1:]]
    L = [lab[:-1, :-1], lab[:-1, 1:], lab[1:, :-1], lab[1:, 1:]]
    nfg = sum(x.astype(np.int64) for x in c)
    for cy in range(H + 1):
        for cx in range(W + 1):
            k = nfg[cy, cx]
            f = [c[j][cy, cx] for j in range(4)]
            l = [int(L[j][cy, cx]) for j in range(4)]
            if k == 4:
                own[l[0]] += 2
            elif k == 3:
                own[l[f.index(True)]] += 1                # the three fg corners are 8-connected: one component
                own[l[f.index(False)]] += 1
            elif k == 2 and f[0] == f[3]:                 # diagonal pair
                for j in range(4):
                    if not f[j]:
                        own[l[j]] += 1
            else:
                own[l[f.index(False)]] += 2
    # subtree sums: children before parents (a child's label is larger than its parent's)
    tot = dict(own)
    for r in sorted(roots.tolist(), reverse=True):
        if parent[r] is not None:
            tot[parent[r]] += tot[r]
    isfg = {r: bool(fg.ravel()[r]) for r in roots.tolist()}
    fig = {r: r != frame and tot[r] / 2.0 >= figure_threshold for r in roots.tolist()}
    sgn = {r: (-tot[r] if isfg[r] else tot[r]) / 2.0 for r in roots.tolist()}
    out = np.zeros((H, W), dtype=np.uint8)
    memo = {}
    for y in range(1, H + 1):
        for x in range(1, W + 1):
            X = int(lab[y, x])
            if X not in memo:
                # deepest figure on the path X -> root, and the child Z of it on that path
                F, Z, node, prev = None, None, X, None
                while node is not None:
                    if fig[node]:
                        F, Z = node, prev
                        break
                    prev, node = node, parent[node]
                memo[X] = (F, Z)
            F, Z = memo[X]
            if F is None:
                continue
            if F == X:
                out[y - 1, x - 1] = 255
                continue
            if sgn[Z] >= figure_inner_threshold:
                if isfg[Z] and X == Z:
                    P = parent[Z]
                    if (lab[y - 1, x] == P or lab[y + 1, x] == P or lab[y, x - 1] == P or lab[y, x + 1] == P):
                        out[y - 1, x - 1] = 255
                continue
            out[y - 1, x - 1] = 255
    return out
