"""Literal restatement of the reference's contour stage, background_subtraction.py:171-193, written from the published
algorithms cv2 implements -- the referee the device formulation is held to (tests only; no cv2 here).

  cv2.findContours(mask, RETR_TREE, CHAIN_APPROX_SIMPLE)
      Suzuki & Abe, "Topological structural analysis of digitized binary images by border following" (CVGIP 30, 1985),
      Algorithm 1, on the image padded with a ring of zeros (OpenCV does the same).  Foreground is 8-connected.  Borders are
      traced with OpenCV's chain codes (code k = direction k * 45 degrees counter-clockwise on screen, 0 = +x); the start
      search runs clockwise from the zero neighbour (left for an outer border, right for a hole border), the trace
      counter-clockwise.  CHAIN_APPROX_SIMPLE writes a point where the chain code changes.  Hierarchy: the paper's LNBD rule;
      the list is the tree in pre-order, a node's children in reverse order of discovery (cvInsertNodeIntoTree prepends).
  cv2.contourArea(c, oriented)
      shoelace sum over (prev.x * p.y - prev.y * p.x), halved; |.| unless oriented.
  cv2.fillPoly(img, [c], v)
      even-odd scanline fill of the closed polygon through the pixel centres; `boundary` decides whether lattice points on
      the polygon itself are set (both choices are checked to give the same stage output).
  cv2.drawContours(img, [c], -1, v)
      thickness 1, LINE_8: the closed polyline; consecutive points of a traced contour are joined by straight chain runs, so
      every 8-connected line algorithm draws the same pixels.
"""
import numpy as np

# OpenCV's chain code deltas (x, y): 0 right, then counter-clockwise on screen (y grows downwards)
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)


def _trace(f, y0, x0, is_hole, nbd):
    """Border following from (y0, x0) of the padded label image f (modified in place); returns the contour as a list
    of (x, y) in image coordinates (padding removed), CHAIN_APPROX_SIMPLE."""
    s = s_end = 0 if is_hole else 4
    while True:                                          # (3.1) clockwise from the zero neighbour
        s = (s - 1) & 7
        y1, x1 = y0 + DY[s], x0 + DX[s]
        if f[y1][x1] != 0 or s == s_end:
            break
    if f[y1][x1] == 0:                                   # isolated pixel
        f[y0][x0] = -nbd
        return [(x0 - 1, y0 - 1)]
    pts = []
    y3, x3 = y0, x0
    prev_s = s ^ 4
    while True:
        s_end = s                                        # (3.3) counter-clockwise from the direction after the one we came from
        k = s
        while True:
            k += 1
            y4, x4 = y3 + DY[k & 7], x3 + DX[k & 7]
            if f[y4][x4] != 0:
                break
        sn = k & 7
        if k >= 8 and (sn - 1) & 0xffffffff < s_end:    # (3.4) the right neighbour (code 0) was examined and is 0
            f[y3][x3] = -nbd
        elif f[y3][x3] == 1:
            f[y3][x3] = nbd
        if sn != prev_s:
            pts.append((x3 - 1, y3 - 1))
            prev_s = sn
        if (y4, x4) == (y0, x0) and (y3, x3) == (y1, x1):   # (3.5)
            break
        y3, x3 = y4, x4
        s = (sn + 4) & 7
    return pts


def find_contours_tree(mask):
    """(contours, hierarchy) as cv2.findContours(mask, RETR_TREE, CHAIN_APPROX_SIMPLE) returns them: contours a list of int
    arrays [n, 2] (x, y); hierarchy int [N, 4] (next, previous, first child, parent), -1 for none."""
    m = np.asarray(mask)
    H, W = m.shape
    f = [[0] * (W + 2)]
    for row in (m != 0).astype(np.int64).tolist():
        f.append([0] + row + [0])
    f.append([0] * (W + 2))
    # border 1 = the frame (a hole border)
    is_hole = {1: True}
    parent = {1: None}
    cont = {}
    nbd = 1
    for y in range(1, H + 1):
        lnbd = 1
        row = f[y]
        for x in range(1, W + 1):
            v = row[x]
            if v == 0:
                continue
            start = None
            if v == 1 and row[x - 1] == 0:
                start = False                            # outer border
            elif v >= 1 and row[x + 1] == 0:
                start = True                             # hole border
                if v > 1:
                    lnbd = v
            if start is not None:
                nbd += 1
                is_hole[nbd] = start
                bp = lnbd                                 # B' = the border LNBD names
                parent[nbd] = parent[bp] if is_hole[bp] == start else bp
                if parent[nbd] is None:
                    parent[nbd] = 1
                cont[nbd] = _trace(f, y, x, start, nbd)
            v = row[x]
            if v != 1:
                lnbd = abs(v)
    # pre-order of the tree, children in reverse discovery order
    children = {k: [] for k in list(cont) + [1]}
    for k in sorted(cont):
        children[parent[k]].append(k)
    order = []

    def visit(k):
        for c in reversed(children[k]):
            order.append(c)
            visit(c)
    import sys
    lim = sys.getrecursionlimit()
    sys.setrecursionlimit(max(lim, 4 * len(cont) + 1000))
    try:
        visit(1)
    finally:
        sys.setrecursionlimit(lim)
    pos = {k: i for i, k in enumerate(order)}
    hier = np.full((len(order), 4), -1, dtype=np.int64)
    for k in order:
        sib = list(reversed(children[parent[k]]))
        j = sib.index(k)
        i = pos[k]
        hier[i, 0] = pos[sib[j + 1]] if j + 1 < len(sib) else -1
        hier[i, 1] = pos[sib[j - 1]] if j > 0 else -1
        hier[i, 2] = pos[list(reversed(children[k]))[0]] if children[k] else -1
        hier[i, 3] = pos[parent[k]] if parent[k] != 1 else -1
    contours = [np.array(cont[k], dtype=np.int64).reshape(-1, 2) for k in order]
    return contours, hier, [is_hole[k] for k in order]


def contour_area(c, oriented=False):
    a = 0.0
    px, py = c[-1]
    for x, y in c:
        a += float(px) * float(y) - float(py) * float(x)
        px, py = x, y
    a *= 0.5
    return a if oriented else abs(a)


def _segments(c):
    n = len(c)
    pts = [(int(x), int(y)) for x, y in c]
    return [(pts[i], pts[(i + 1) % n]) for i in range(n)]


def _line_points(a, b):
    (x0, y0), (x1, y1) = a, b
    dx, dy = x1 - x0, y1 - y0
    steps = max(abs(dx), abs(dy))
    assert dx == 0 or dy == 0 or abs(dx) == abs(dy), "a traced contour's segments are chain runs"
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    return [(x0 + k * sx, y0 + k * sy) for k in range(steps + 1)]


def draw_contour(img, c, value):
    for a, b in _segments(c):
        for x, y in _line_points(a, b):
            img[y, x] = value


def fill_poly(img, c, value, boundary=True):
    """Even-odd fill of the closed polygon c over the pixel centres of img; boundary lattice points set iff boundary."""
    H, W = img.shape
    segs = _segments(c)
    ys = [p[1] for p in c]
    lo, hi = max(min(ys), 0), min(max(ys), H - 1)
    on_edge = set()
    for a, b in segs:
        on_edge.update(_line_points(a, b))
    for y in range(lo, hi + 1):
        xs = []
        for (x0, y0), (x1, y1) in segs:
            if y0 == y1:
                continue
            if min(y0, y1) <= y < max(y0, y1):         # half-open: exact parity for points off the polygon
                xs.append(x0 + (y - y0) * (x1 - x0) / (y1 - y0))
        if not xs:
            continue
        xs = np.sort(np.array(xs))
        xr = np.arange(int(np.floor(xs[0])), int(np.ceil(xs[-1])) + 1)
        xr = xr[(xr >= 0) & (xr < W)]
        odd = (len(xs) - np.searchsorted(xs, xr, side="right")) % 2 == 1
        for x in xr[odd]:
            if (int(x), y) not in on_edge:
                img[y, x] = value
    if boundary:
        for x, y in on_edge:
            img[y, x] = value


def fill_figures(mask, figure_threshold, figure_inner_threshold, boundary=True):
    """background_subtraction.py:171-193, loop for loop."""
    contours, hierarchy, _ = find_contours_tree(mask)
    foreground = np.zeros(np.asarray(mask).shape, dtype=np.uint8)
    for idx, contour in enumerate(contours):
        if contour_area(contour) >= figure_threshold:
            draw_contour(foreground, contour, 255)
            fill_poly(foreground, contour, 255, boundary)
            inner_idx = hierarchy[idx][2]
            while inner_idx != -1:
                if contour_area(contours[inner_idx], True) >= figure_inner_threshold:
                    fill_poly(foreground, contours[inner_idx], 0, boundary)
                    draw_contour(foreground, contours[inner_idx], 255)
                inner_idx = hierarchy[inner_idx][0]
    return foreground
