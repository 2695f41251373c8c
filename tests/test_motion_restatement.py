"""The restatement of the block motion between two hulls (tests/motion_np.py) against itself and against the cases whose answer is
known: shifted ellipsoids, noise, the aperture problem, the search range, the tie rule; voxcarve.motion on the host.  No GPU."""
import functools

import numpy as np
import pytest

import motion_np as mn

GRIDS = [(5, 7, 3), (9, 11, 7), (12, 64, 10), (37, 53, 29)]
PARAMS = [(4, 0, 1), (4, 2, 2), (8, 4, 4), (16, 8, 8)]
ROW_KEYS = ("block", "ijk", "d", "cost", "cost0", "count_a", "count_b", "ties", "flags")


def same_rows(got, want, where=""):
    for key in ROW_KEYS:
        assert np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)), (where, key)


@pytest.mark.parametrize("b,ap,s", PARAMS)
@pytest.mark.parametrize("grid", GRIDS)
def test_vectorised_equals_literal(grid, b, ap, s):
    a, bo = mn.random_pair(grid, 100 * b + grid[0], s)
    got, lit = mn.match(a, bo, grid, b, ap, s), mn.match_literal(a, bo, grid, b, ap, s)
    same_rows(got, lit, (grid, b, ap, s))
    assert len(got["block"]) > 0 and np.all(np.diff(got["block"].astype(np.int64)) > 0)
    assert np.all(got["cost"] <= got["cost0"]) and np.all(got["ties"] >= 1)
    assert mn.stats(got, a, bo, grid, b) == mn.stats(lit, a, bo, grid, b)


def test_rows_of_64_bits():
    grid = (9, 11, 7)
    a, bo = mn.random_pair(grid, 5, 8)
    same_rows(mn.match(a, bo, grid, 16, 16, 8), mn.match_literal(a, bo, grid, 16, 16, 8))


ONE = {"grid": (48, 48, 48), "centre": (24, 24, 24), "semi": (14, 10, 18), "shift": (2, -1, 3)}
TWO = {"grid": (64, 64, 64), "bodies": (((16, 32, 32), (9, 12, 20), (3, -2, 1)), ((46, 30, 30), (10, 9, 22), (-1, 3, -2)))}


@functools.lru_cache(maxsize=None)
def one_body():
    b = mn.ellipsoid(ONE["grid"], ONE["centre"], ONE["semi"])
    a = mn.ellipsoid(ONE["grid"], tuple(c + d for c, d in zip(ONE["centre"], ONE["shift"])), ONE["semi"])
    return a, b, mn.match(a, b, ONE["grid"], 8, 4, 4)


@functools.lru_cache(maxsize=None)
def two_bodies():
    grid = TWO["grid"]
    a = np.zeros((grid[2], grid[0], grid[1]), dtype=bool)
    b = np.zeros_like(a)
    for centre, semi, shift in TWO["bodies"]:
        b |= mn.ellipsoid(grid, centre, semi)
        a |= mn.ellipsoid(grid, tuple(c + d for c, d in zip(centre, shift)), semi)
    return a, b, mn.match(a, b, grid, 8, 4, 4)


def body_shift(rows):
    """int64 [L, 3]: the shift of the body on each row's side of x = 32 (block edge 8: blocks 0..3 lie left of it)."""
    left = np.asarray(rows["ijk"])[:, 0] < 4
    return np.where(left[:, None], np.array(TWO["bodies"][0][2]), np.array(TWO["bodies"][1][2]))


def test_one_body_is_found_exactly():
    a, b, rows = one_body()
    assert len(rows["block"]) == 62                              # (the prototype's count)
    assert np.all(rows["ties"] == 1)
    assert np.array_equal(rows["d"].astype(np.int64), np.tile(ONE["shift"], (62, 1)))
    P, st = mn.warp(rows, a, b, ONE["grid"], 8)
    assert np.array_equal(P, a) and st["warped"] == st["common"] == st["a"] == int(a.sum())
    s = mn.stats(rows, a, b, ONE["grid"], 8)
    assert s["cost_sum"] == 0 and s["cost0_sum"] == 25157 and s["moved"] == s["unique"] == s["listed"] == 62 and s["clipped"] == 0
    assert s["blocks"] == 216
    assert abs(mn.iou(a, b) - 0.694) < 5e-4


def test_two_bodies_each_carry_their_own_shift():
    a, b, rows = two_bodies()
    assert len(rows["block"]) == 112 and np.all(rows["ties"] == 1)
    assert np.array_equal(rows["d"].astype(np.int64), body_shift(rows))
    assert int((np.asarray(rows["ijk"])[:, 0] < 4).sum()) == 56
    # (8, not 0: the windows of the blocks next to x = 32 reach into the other body, which moves another way)
    st = mn.stats(rows, a, b, TWO["grid"], 8)
    assert (st["cost_sum"], st["cost0_sum"], st["moved"], st["unique"], st["clipped"]) == (8, 62722, 112, 112, 0)
    assert mn.iou(a, b) < 0.6
    P, _ = mn.warp(rows, a, b, TWO["grid"], 8)
    assert np.array_equal(P, a) and mn.iou(a, P) == 1.0


def test_noise_leaves_the_vectors():
    a, b, clean = two_bodies()
    rng = np.random.default_rng(1)
    flat = a.reshape(-1).copy()
    on = np.flatnonzero(flat)
    flat[rng.choice(on, size=on.size // 100, replace=False)] = False
    noisy = flat.reshape(a.shape)
    rows = mn.match(noisy, b, TWO["grid"], 8, 4, 4)
    at = np.searchsorted(rows["block"], clean["block"])
    assert np.array_equal(rows["block"][at], clean["block"])     # (B alone lists every clean block)
    assert np.array_equal(rows["d"][at].astype(np.int64), body_shift(clean))


def test_equal_hulls_do_not_move():
    a, _, _ = one_body()
    rows = mn.match(a, a, ONE["grid"], 8, 4, 4)
    assert len(rows["block"]) > 0 and not rows["d"].any() and not rows["cost"].any() and not rows["cost0"].any() and not rows["flags"].any()


@pytest.mark.parametrize("b,ap,s", [(4, 0, 1), (8, 4, 4), (4, 2, 2)])
def test_solid_window_ties_everywhere(b, ap, s):
    grid = (3 * b + 16, 3 * b + 16, 3 * b + 16)
    solid = np.ones((grid[2], grid[0], grid[1]), dtype=bool)
    rows = mn.match(solid, solid, grid, b, ap, s)
    k = int(np.flatnonzero((rows["ijk"] == (grid[0] // b // 2,) * 3).all(axis=1))[0])   # a block whose search region lies inside
    assert rows["ties"][k] == (2 * s + 1) ** 3 and not rows["d"][k].any() and rows["cost"][k] == 0 and rows["flags"][k] == 0
    # an empty old hull: every displacement costs the window's voxels
    rows = mn.match(solid, np.zeros_like(solid), grid, b, ap, s)
    assert np.all(rows["ties"] == (2 * s + 1) ** 3) and not rows["d"].any() and np.array_equal(rows["cost"], rows["cost0"])


def test_shift_beyond_the_range_is_flagged():
    s = 4
    b = mn.ellipsoid(ONE["grid"], ONE["centre"], ONE["semi"])
    a = mn.ellipsoid(ONE["grid"], (ONE["centre"][0] + s + 1, ONE["centre"][1], ONE["centre"][2]), ONE["semi"])
    rows = mn.match(a, b, ONE["grid"], 8, 4, s)
    d = rows["d"].astype(np.int64)
    assert np.array_equal(rows["flags"] & 1, (np.abs(d).max(axis=1) == s).astype(np.uint8))
    at_range = d[:, 0] == s
    assert at_range.sum() >= len(d) // 2 and np.all(rows["flags"][at_range] == 1)
    assert np.all(rows["cost"][at_range & (rows["ties"] == 1)] > 0)                      # (the true vector lies outside)
    assert mn.stats(rows, a, b, ONE["grid"], 8)["clipped"] == int((rows["flags"] & 1).sum()) > 0


def test_tie_rule_by_hand():
    # costs: the three rules one after the other
    s = 1
    disp = mn.displacements(s)
    costs = np.full(27, 9)
    assert mn.choose(costs, s) == (13, 27) and not disp[13].any()
    costs[[0, 26]] = 3                                           # (-1, -1, -1) and (1, 1, 1): |d|^2 equal, the smaller dz first
    assert mn.choose(costs, s) == (0, 2)
    costs[int(np.flatnonzero((disp == (0, 1, 0)).all(axis=1))[0])] = 3               # |d|^2 = 1 beats 3
    j, ties = mn.choose(costs, s)
    assert tuple(disp[j]) == (0, 1, 0) and ties == 3
    costs[int(np.flatnonzero((disp == (-1, 0, 0)).all(axis=1))[0])] = 3              # dz equal: the smaller dx
    assert tuple(disp[mn.choose(costs, s)[0]]) == (-1, 0, 0)
    costs[int(np.flatnonzero((disp == (0, 0, 1)).all(axis=1))[0])] = 2               # the cost comes first
    assert tuple(disp[mn.choose(costs, s)[0]]) == (0, 0, 1) and mn.choose(costs, s)[1] == 1
    # a hull: one old voxel, six new ones around it; each of the six unit steps explains one of them
    grid = (8, 8, 8)
    b = np.zeros((8, 8, 8), dtype=bool)
    a = np.zeros_like(b)
    b[4, 4, 4] = True
    for axis in range(3):
        for step in (-1, 1):
            p = [4, 4, 4]
            p[axis] += step
            a[tuple(p)] = True
    for rows in (mn.match(a, b, grid, 8, 0, 2), mn.match_literal(a, b, grid, 8, 0, 2)):
        assert rows["block"].tolist() == [0] and rows["ties"].tolist() == [6] and rows["cost"].tolist() == [5] and rows["cost0"].tolist() == [7]
        assert rows["d"].tolist() == [[0, 0, -1]]                # the smallest dz
        assert rows["count_a"].tolist() == [6] and rows["count_b"].tolist() == [1]


def test_paint_channels():
    grid = (8, 8, 8)
    rows = {"block": np.array([0], dtype=np.uint32), "d": np.array([[-3, 1, 4]], dtype=np.int8)}
    rec = np.array([5 | (0x01aabbcc << 32), 100 | (0x00112233 << 32)], dtype=np.uint64)
    out = mn.paint(rec, rows, grid, 8, 4)
    want = 128 - (127 * 3) // 4, 128 + 127 // 4, 255
    assert want == (33, 159, 255)
    for r, o in zip(rec, out):
        assert int(o) & 0xffffffff == int(r) & 0xffffffff and int(o) >> 56 == int(r) >> 56
        assert ((int(o) >> 32) & 0xff, (int(o) >> 40) & 0xff, (int(o) >> 48) & 0xff) == want


def test_figure_motion_and_describe_on_two_bodies():
    from voxcarve import motion
    a, b, rows = two_bodies()
    grid = TWO["grid"]
    bounds = (-512.0, 1024.0, -1024.0, 1024.0, -2048.0, 512.0)
    rows = dict(rows, grid=grid, edge=8, apron=4, search=4)
    assert np.array_equal(motion.block_ijk(rows["block"], grid, 8), rows["ijk"])
    idx = np.flatnonzero(a.reshape(-1))
    labels = ((idx // grid[1]) % grid[0] >= 32).astype(np.uint8)
    fm = motion.figure_motion(rows, idx, labels, 2)
    assert np.array_equal(fm["d"], np.array([TWO["bodies"][0][2], TWO["bodies"][1][2]], dtype=np.float64))
    # (a block that only the old hull touches holds no record: it is nobody's)
    assert fm["unique"].tolist() == fm["blocks"].tolist() and all(40 < v <= 56 for v in fm["blocks"])
    assert int((fm["owner"] < 0).sum()) == 112 - int(fm["blocks"].sum())
    # equal counts go to the smaller label; a figure nobody votes for has no motion
    small = {"grid": (8, 8, 8), "edge": 8, "block": np.array([0], dtype=np.uint32), "d": np.array([[1, 2, 3]], dtype=np.int8),
             "ties": np.array([1], dtype=np.uint16)}
    half = motion.figure_motion(small, [0, 1, 9], [1, 0, 7], 3)
    assert half["owner"].tolist() == [0] and half["d"].tolist() == [[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    assert half["blocks"].tolist() == [1, 0, 0]
    desc = motion.describe(rows, grid, bounds, fps=30)
    step = motion.steps_mm(grid, bounds)
    assert np.allclose(step, [1536 / 63, 2048 / 63, 2560 / 63])
    assert np.allclose(desc["velocity_mm"], rows["d"] * step) and np.allclose(desc["velocity_mm_s"], desc["velocity_mm"] * 30)
    assert np.allclose(desc["centre_mm"][0], np.array([-512.0, -1024.0, -2048.0]) + (rows["ijk"][0] * 8 + 3.5) * step)
    assert desc["median_mm"].shape == (3,) and "velocity_mm_s" not in motion.describe(rows, grid, bounds)
    assert motion.check_params(8, None, 4) == (8, 4, 4) and motion.check_params(16, 16, 8) == (16, 16, 8)   # 64 itself is allowed
    for bad in ((5, 0, 1), (8, 17, 1), (8, 4, 0), (8, 4, 9), (16, 16, 9)):
        with pytest.raises(ValueError):
            motion.check_params(*bad)


def test_words_layout():
    occ = np.zeros((3, 5, 7), dtype=bool)
    occ[2, 4, 6] = occ[0, 0, 0] = occ[0, 9 // 7, 9 % 7] = True
    w = mn.words(occ)
    assert w.size == 2 and int(w[0]) == 1 | (1 << 9) and int(w[1]) == 1 << (104 - 64)
