"""Connected components of the hull, CPU side: the vectorised restatement (tests/components_np.py) against the literal
breadth-first search on seeded random occupancies (word-straddling ny, degenerate shapes, every connectivity, size floors and
rank limits with ties), against scipy.ndimage.label's partition, and the fragment counts of the committed 64^3 / 128^3 hulls."""
import numpy as np
import pytest

import components_np as cn
import fixtures_util as fx

SHAPES = [(1, 1, 1), (1, 9, 1), (1, 70, 1), (7, 50, 3), (4, 63, 3), (3, 64, 4), (5, 65, 2), (2, 130, 3), (6, 6, 6)]
RULES = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (2, 2), (4, 1), (1000, 0), (0, 1000)]


def _random_idx(rng, grid, density):
    n = grid[0] * grid[1] * grid[2]
    return np.flatnonzero(rng.random(n) < density).astype(np.uint32)


def _agree(idx, grid, conn, mv, kl):
    a = cn.components(idx, grid, conn, mv, kl)
    b = cn.components_literal(idx, grid, conn, mv, kl)
    for k in ("labels", "label", "size", "lo", "hi", "kept", "keep", "idx"):
        assert np.array_equal(a[k], b[k]), (k, grid, conn, mv, kl)
    return a


@pytest.mark.parametrize("grid", SHAPES)
@pytest.mark.parametrize("conn", cn.CONNECTIVITIES)
def test_vectorised_equals_literal(grid, conn):
    rng = np.random.default_rng(1000 * grid[0] + 10 * grid[1] + grid[2] + conn)
    for density in (0.05, 0.15, 0.3, 0.45, 0.6):
        idx = _random_idx(rng, grid, density)
        for mv, kl in RULES[:: 1 if density in (0.15, 0.45) else 3]:
            a = _agree(idx, grid, conn, mv, kl)
            assert a["size"].sum() == idx.size
            assert np.array_equal(np.sort(np.unique(a["labels"])), a["label"])
            assert np.all(a["label"][:-1] < a["label"][1:])


def test_ties_are_broken_by_label():
    # three single voxels and two pairs, far apart: ranks 0, 1 are the pairs (lower label first), then singles by label
    grid = (1, 20, 1)
    idx = np.array([0, 3, 4, 7, 10, 11, 15], dtype=np.uint32)
    for conn in cn.CONNECTIVITIES:
        a = _agree(idx, grid, conn, 0, 3)
        assert a["label"].tolist() == [0, 3, 7, 10, 15]
        assert a["size"].tolist() == [1, 2, 1, 2, 1]
        assert a["kept"].tolist() == [True, True, False, True, False]
        assert a["idx"].tolist() == [0, 3, 4, 10, 11]


def test_columns_do_not_wrap():
    # i and i + 1 across a column end are not neighbours; diagonal neighbours across the end of a column are not either
    grid = (2, 3, 2)
    idx = np.array([2, 3], dtype=np.uint32)         # (ix 0, iy 2) and (ix 1, iy 0)
    for conn in cn.CONNECTIVITIES:
        assert _agree(idx, grid, conn, 0, 0)["label"].size == 2
    idx = np.array([2, 4], dtype=np.uint32)         # (0, 2) and (1, 1): edge neighbours
    assert _agree(idx, grid, 6, 0, 0)["label"].size == 2
    assert _agree(idx, grid, 18, 0, 0)["label"].size == 1


def test_many_seeded_occupancies():
    rng = np.random.default_rng(7)
    n = 0
    for _ in range(160):
        grid = (int(rng.integers(1, 6)), int(rng.choice([1, 2, 5, 63, 64, 65, 130])), int(rng.integers(1, 5)))
        idx = _random_idx(rng, grid, float(rng.uniform(0.05, 0.6)))
        conn = int(rng.choice(cn.CONNECTIVITIES))
        _agree(idx, grid, conn, int(rng.integers(0, 4)), int(rng.integers(0, 4)))
        n += 1
    assert n == 160


@pytest.mark.parametrize("conn", cn.CONNECTIVITIES)
def test_partition_equals_scipy(conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    rank = {6: 1, 18: 2, 26: 3}[conn]
    rng = np.random.default_rng(conn)
    for grid in [(9, 65, 7), (12, 12, 12), (3, 130, 5)]:
        for density in (0.1, 0.3, 0.5):
            idx = _random_idx(rng, grid, density)
            a = cn.components(idx, grid, conn)
            nx, ny, nz = grid
            vol = np.zeros(nx * ny * nz, dtype=bool)
            vol[idx] = True
            lab, k = ndimage.label(vol.reshape(nz, nx, ny), structure=ndimage.generate_binary_structure(3, rank))
            sl = lab.reshape(-1)[idx]
            assert k == a["label"].size
            # same partition: the map scipy label -> our label is a bijection
            pairs = np.unique(np.stack([sl, a["labels"]], axis=1), axis=0)
            assert pairs.shape[0] == k


@pytest.mark.parametrize("n,counts,bodies", [(64, (9, 4, 4), (6969, 6977, 6977)), (128, (11, 3, 2), (57018, 57037, 57041))])
def test_fixture_fragments(n, counts, bodies):
    idx, _, _ = fx.expected(n)
    for conn, k, body in zip(cn.CONNECTIVITIES, counts, bodies):
        a = cn.components(idx, (n, n, n), conn)
        assert a["label"].size == k and int(a["size"].max()) == body
        b = cn.components(idx, (n, n, n), conn, keep_largest=1)
        assert b["idx"].size == body and b["kept"].sum() == 1
        c = cn.components(idx, (n, n, n), conn, min_voxels=3)
        assert c["idx"].size == int(a["size"][a["size"] >= 3].sum())
    if n == 64:
        lit = cn.components_literal(idx, (n, n, n), 6, min_voxels=2)
        assert np.array_equal(lit["idx"], cn.components(idx, (n, n, n), 6, min_voxels=2)["idx"])
