"""What goes with CarveEngine.cluster_hull on the host: the default palette of paint_clusters and the matching of colour
signatures (fetch_cluster_histograms) between two clusterings.  Pure Python / numpy; the clustering itself is vc_hull_clusters."""
import itertools

import numpy as np

# 16 distinct colours, RGB; entry k paints figure k
PALETTE = np.array([(230, 25, 75), (60, 180, 75), (0, 130, 200), (255, 225, 25), (245, 130, 48), (145, 30, 180), (70, 240, 240),
                    (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40),
                    (128, 0, 0), (170, 255, 195), (0, 0, 128)], dtype=np.uint8)
MATCH_MAX_K = 8


def _normalised(h):
    h = np.asarray(h, dtype=np.float64)
    s = h.sum(axis=1, keepdims=True)
    return h / np.where(s == 0.0, 1.0, s)


def match_costs(ref_hist, hist):
    """float64 [K, K]: cost[i, j] = sum over bins of (a - b)^2 / (a + b), a = the normalised reference histogram i, b = the
    normalised histogram j; bins empty in both are skipped.  0 = equal signatures, 2 = disjoint ones."""
    a, b = _normalised(ref_hist), _normalised(hist)
    if a.shape != b.shape or a.ndim != 2:
        raise ValueError("match: histograms of shapes %r and %r" % (a.shape, b.shape))
    num = (a[:, None, :] - b[None, :, :]) ** 2
    den = a[:, None, :] + b[None, :, :]
    return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0).sum(axis=2)


def match(ref_hist, hist):
    """The permutation p (a tuple, p[k] = the cluster of `hist` that is reference figure k) that minimises
    sum_k cost[k, p[k]] (match_costs), searched exactly over itertools.permutations: K <= 8, ValueError above.  Equal totals
    keep the permutation that comes first in lexicographic order, so equal histograms give the identity."""
    K = np.asarray(ref_hist).shape[0]
    if K > MATCH_MAX_K:
        raise ValueError("match: K = %d, the exact search stops at %d" % (K, MATCH_MAX_K))
    cost = match_costs(ref_hist, hist)
    best, best_cost = None, None
    rows = np.arange(K)
    for p in itertools.permutations(range(K)):
        c = float(cost[rows, list(p)].sum())
        if best is None or c < best_cost:
            best, best_cost = p, c
    return best
