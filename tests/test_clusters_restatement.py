"""The restatement of the floor-plane K-means (tests/clusters_np.py; contract of vc_hull_clusters in include/voxcarve.h) against
its own literal form and against what the contract promises: random occupancies with K = 1..5, both kinds of start, a floor under
the column weights, fewer weighted columns than K, the empty volume; K = 1 is the weighted mean; three figures carved on the CPU
are found where they stand and a warm start stops in round 1; what a speck does to the seeding and what min_column does about it;
voxcarve.clusters.match."""
import itertools

import numpy as np
import pytest

import clusters_np as cn
import distance_np as dn
import fixtures_util as fx

KEYS = ("centres", "floor_map", "floor_labels", "cluster_weight")
SCALARS = ("iterations", "converged", "weight", "columns", "survivors", "q")


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    for k in SCALARS:
        assert a[k] == b[k], k


def _both(occ, q, K, **kw):
    a, b = cn.clusters(occ, q, K, **kw), cn.clusters_literal(occ, q, K, **kw)
    _same(a, b)
    return a


@pytest.mark.parametrize("shape,q", [((4, 5, 7), (30000, 17000)), ((6, 9, 13), (12090, 16130))])       # (nz, nx, ny)
@pytest.mark.parametrize("min_column", [1, 3])
def test_vectorised_equals_literal(shape, q, min_column):
    for seed, fill in ((1, 0.5), (2, 0.15)):
        rng = np.random.default_rng(seed)
        occ = rng.random(shape) < fill
        ncol = shape[1] * shape[2]
        for K in range(1, 6):
            r = _both(occ, q, K, min_column=min_column)
            assert r["survivors"] == int(occ.sum()) and r["floor_map"].sum() == r["survivors"]
            assert r["weight"] == int(r["floor_map"][r["floor_map"] >= min_column].sum())
            assert ((r["floor_labels"] == cn.NO_LABEL) == (r["floor_map"] == 0)).all()
            if r["weight"]:
                assert r["iterations"] >= 1 and int(r["cluster_weight"].sum()) == r["weight"]
            init = np.stack([rng.integers(0, q[0] * shape[1], K), rng.integers(0, q[1] * shape[2], K)], axis=1)
            _both(occ, q, K, min_column=min_column, init=init)
            _both(occ, q, K, min_column=min_column, max_iters=1)
        assert ncol == r["floor_map"].size


def test_fewer_weighted_columns_than_k_and_the_empty_volume():
    occ = np.zeros((4, 5, 7), dtype=bool)
    q = (1000, 2000)
    r = _both(occ, q, 3)
    assert r["iterations"] == 0 and r["converged"] == 1 and not r["centres"].any() and (r["floor_labels"] == cn.NO_LABEL).all()
    r = _both(occ, q, 2, init=[[5, 6], [7, 8]])
    assert r["centres"].tolist() == [[5, 6], [7, 8]]
    occ[:, 1, 2] = True
    occ[:2, 3, 5] = True
    r = _both(occ, q, 4)                                         # two columns, four centres: two duplicates that end up empty
    assert sorted(r["cluster_weight"].tolist()) == [0, 0, 2, 4] and r["converged"] == 1
    assert sorted(map(tuple, r["centres"].tolist())) == [(1000, 4000)] * 3 + [(3000, 10000)]
    # a floor no column reaches: no rounds, every label 0
    r = _both(occ, q, 2, min_column=5)
    assert r["weight"] == 0 and r["iterations"] == 0 and r["converged"] == 1
    assert set(r["floor_labels"][r["floor_map"] > 0].tolist()) == {0}
    with pytest.raises(ValueError):
        cn.clusters(occ, q, 0)
    with pytest.raises(ValueError):
        cn.clusters(occ, q, 17)
    with pytest.raises(ValueError):
        cn.clusters(occ, q, 2, max_iters=256)
    with pytest.raises(ValueError):
        cn.clusters(occ, q, 1, init=[[1 << 31, 0]])


def test_k1_is_the_weighted_mean():
    rng = np.random.default_rng(7)
    occ = rng.random((6, 9, 13)) < 0.4
    q = (12090, 16130)
    r = _both(occ, q, 1)
    n = occ.sum(axis=0).astype(np.int64)
    ix, iy = np.mgrid[0:9, 0:13]
    W = int(n.sum())
    want = ((int((n * ix).sum()) * q[0] + W // 2) // W, (int((n * iy).sum()) * q[1] + W // 2) // W)
    assert tuple(r["centres"][0]) == want and r["converged"] == 1 and r["iterations"] == 2
    assert int(r["cluster_weight"][0]) == W


@pytest.fixture(scope="module")
def figures():
    """The three-figure scene carved at 64^3 on the CPU: (occ, q, bounds)."""
    from oracle import carve_np
    from voxcarve.engine import DEFAULT_BOUNDS
    cams, masks = cn.three_figures()
    out = carve_np.carve(64, 64, 64, fx.oracle_cams(cams), masks)
    return dn.volume(out["idx"], (64, 64, 64)), cn.steps_um_xy((64, 64, 64), DEFAULT_BOUNDS), DEFAULT_BOUNDS


def test_three_figures(figures):
    occ, q, bounds = figures
    assert q == (24381, 32508) and int(occ.sum()) == 6143
    r = cn.clusters(occ, q, 3, max_iters=32)
    assert r["converged"] == 1 and r["columns"] == 313
    mm = cn.centres_world_mm(r["centres"], bounds)
    truth = np.array(cn.FIGURE_CENTRES)[:, :2]
    taken = []
    for c in mm:
        d = np.abs(truth - c)
        hit = np.flatnonzero((d[:, 0] <= q[0] / 1000.0) & (d[:, 1] <= q[1] / 1000.0))
        assert hit.size == 1, (c, truth)
        taken.append(int(hit[0]))
    assert sorted(taken) == [0, 1, 2]                            # each true centre exactly once
    rec = np.flatnonzero(occ.reshape(-1)).astype(np.uint64)
    d = cn.describe(rec, (64, 64, 64), r)
    assert int(d["voxels"].sum()) == 6143 and (d["voxels"] > 1500).all()
    warm = cn.clusters(occ, q, 3, init=r["centres"])
    assert warm["iterations"] == 1 and warm["converged"] == 1 and np.array_equal(warm["floor_labels"], r["floor_labels"])
    assert np.array_equal(warm["centres"], r["centres"])
    for K, mc in itertools.product((2, 4), (1, 8)):
        assert cn.clusters(occ, q, K, min_column=mc)["converged"] == 1


def test_a_speck_pulls_the_seeding_and_min_column_stops_it(figures):
    """Farthest-first seeding takes an outlying speck for a figure: with one stray voxel in a corner of the floor, K = 3 spends a
    centre on it and merges two figures; with min_column = 2 the speck weighs nothing and the split is the clean scene's."""
    occ, q, bounds = figures
    clean = cn.clusters(occ, q, 3)
    noisy = occ.copy()
    noisy[40, 62, 1] = True
    pulled = cn.clusters(noisy, q, 3)
    assert 1 in pulled["cluster_weight"].tolist()               # a centre sits on the speck alone
    floored = cn.clusters(noisy, q, 3, min_column=2)
    assert np.array_equal(np.sort(floored["centres"], axis=0), np.sort(cn.clusters(occ, q, 3, min_column=2)["centres"], axis=0))
    assert sorted(floored["cluster_weight"].tolist()) == sorted(cn.clusters(occ, q, 3, min_column=2)["cluster_weight"].tolist())
    assert 1 not in clean["cluster_weight"].tolist()


def test_describe_and_paint():
    rng = np.random.default_rng(11)
    shape, grid = (6, 9, 13), (9, 13, 6)
    occ = rng.random(shape) < 0.3
    idx = np.flatnonzero(occ.reshape(-1)).astype(np.uint64)
    rgb = rng.integers(0, 256, (idx.size, 3)).astype(np.uint64)
    seen = (rng.random(idx.size) < 0.8).astype(np.uint64)
    rec = idx | (rgb[:, 0] << np.uint64(32)) | (rgb[:, 1] << np.uint64(40)) | (rgb[:, 2] << np.uint64(48)) | (seen << np.uint64(56))
    r = cn.clusters(occ, (1000, 1500), 3)
    d = cn.describe(rec, grid, r, hist_iz=(1, 4))
    iz = (idx // np.uint64(9 * 13)).astype(np.int64)
    assert int(d["histograms"].sum()) == int(((seen == 1) & (iz >= 1) & (iz <= 4)).sum())
    assert np.array_equal(d["voxels"], np.bincount(d["labels"], minlength=3).astype(np.uint64))
    assert int(d["columns"].sum()) == r["columns"]
    for k in range(3):                                           # literal boxes
        m = d["labels"] == k
        cols = (idx[m] % np.uint64(9 * 13)).astype(np.int64)
        assert d["lo"][k].tolist() == [(cols // 13).min(), (cols % 13).min(), iz[m].min()]
        assert d["hi"][k].tolist() == [(cols // 13).max(), (cols % 13).max(), iz[m].max()]
    pal = np.array([[1, 2, 3], [40, 50, 60], [255, 0, 128]], dtype=np.uint8)
    painted = cn.paint(rec, d["labels"], pal)
    assert np.array_equal(painted & np.uint64(0xff000000ffffffff), rec & np.uint64(0xff000000ffffffff))
    got = np.stack([(painted >> np.uint64(s)) & np.uint64(255) for s in (32, 40, 48)], 1).astype(np.uint8)
    assert np.array_equal(got, pal[d["labels"]])
    e = cn.describe(rec[:0], grid, cn.clusters(np.zeros(shape, bool), (1000, 1500), 2))
    assert (e["lo"] == cn.EMPTY_LO).all() and (e["hi"] == cn.EMPTY_HI).all() and not e["voxels"].any()


def test_match():
    from voxcarve.clusters import match, match_costs, PALETTE
    rng = np.random.default_rng(5)
    ref = rng.integers(0, 50, (4, 512)).astype(np.uint32)
    ref[:, rng.integers(0, 512, 100)] = 0                        # empty bins on both sides
    assert match(ref, ref) == (0, 1, 2, 3)
    perm = (2, 0, 3, 1)                                          # hist[perm[k]] is figure k, seen a little differently
    hist = np.zeros_like(ref)
    for k in range(4):
        hist[perm[k]] = ref[k] * 3 + rng.integers(0, 3, 512).astype(np.uint32) * (ref[k] > 0)
    assert match(ref, hist) == perm
    c = match_costs(ref, hist)
    assert c.shape == (4, 4) and c.dtype == np.float64 and (c >= 0).all() and (c <= 2.0 + 1e-12).all()
    assert match(np.zeros((2, 512)), np.zeros((2, 512))) == (0, 1)
    with pytest.raises(ValueError):
        match(np.ones((9, 512)), np.ones((9, 512)))
    assert match(np.eye(8, 512), np.eye(8, 512)[::-1]) == tuple(range(7, -1, -1))
    assert PALETTE.shape == (16, 3) and PALETTE.dtype == np.uint8 and len(set(map(tuple, PALETTE.tolist()))) == 16
