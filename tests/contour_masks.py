"""Seeded mask families for the contour stage's tests: blobs, salt noise, their mixes, nested rings."""
import numpy as np

SIZES = [(1, 1), (3, 2), (2, 3), (7, 9), (16, 16), (37, 129), (60, 80)]
THRESHOLDS = [(5000, 115), (5000, 175), (0, 0), (50, -20), (1e9, 0)]


def _blur(a, k):
    for axis in (0, 1):
        c = np.cumsum(np.pad(a, [(k, k) if ax == axis else (0, 0) for ax in (0, 1)], mode="edge"), axis=axis)
        n = a.shape[axis]
        lo = np.take(c, np.arange(n), axis=axis)
        hi = np.take(c, np.arange(2 * k, 2 * k + n), axis=axis)
        a = (hi - lo) / (2 * k)
    return a


def blobs(rng, H, W, k=None, level=None):
    k = k or max(1, min(H, W) // 8)
    a = _blur(rng.random((H, W)), k) if min(H, W) > 2 else rng.random((H, W))
    level = np.quantile(a, rng.uniform(0.3, 0.7)) if level is None else level
    return np.where(a > level, 255, 0).astype(np.uint8)


def noise(rng, H, W, p=None):
    p = rng.uniform(0.1, 0.9) if p is None else p
    return np.where(rng.random((H, W)) < p, 255, 0).astype(np.uint8)


def mix(rng, H, W):
    m = blobs(rng, H, W)
    flip = rng.random((H, W)) < rng.uniform(0.01, 0.15)
    return np.where(flip, 255 - m, m).astype(np.uint8)


def rings(depth, gap=1, pad=2):
    """Concentric square rings of width 1 and `gap` background between them, `depth` foreground rings."""
    n = 2 * depth * (1 + gap) + 2 * pad + 1
    m = np.zeros((n, n), np.uint8)
    for d in range(depth):
        o = pad + d * (1 + gap)
        m[o:n - o, o:n - o] = 255
        m[o + 1:n - o - 1, o + 1:n - o - 1] = 0
    return m


def family(seed, count, sizes=SIZES):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        H, W = sizes[i % len(sizes)]
        kind = i % 3
        out.append(blobs(rng, H, W) if kind == 0 else noise(rng, H, W) if kind == 1 else mix(rng, H, W))
    return out
