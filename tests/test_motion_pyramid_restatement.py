"""The restatement of vc_hull_motion_pyramid (tests/motion_pyramid_np.py) against itself and against motion_np: the literal and the
packed-row version agree; L = 0 is motion_np.match; every listed block's parent is listed; flag bit 0 on one level is today's; and
what the pyramid is for -- two bodies that move further than the search range, apart from each other, and one body that moves 21
voxels -- with the numbers this restatement gives."""
import functools

import numpy as np
import pytest

import motion_np as mn
import motion_pyramid_np as mp

GRIDS = [(5, 7, 3), (9, 11, 7), (12, 64, 10), (37, 53, 29), (24, 130, 20)]
SETTINGS = [(4, 0, 1, 1, 1), (8, 4, 4, 2, 1), (8, 4, 4, 3, 2), (16, 8, 8, 1, 8), (16, 16, 8, 1, 8)]
ROW_KEYS = ("block", "ijk", "d", "cost", "cost0", "count_a", "count_b", "ties", "flags")

TWO_GRID = (96, 96, 64)
# test_two_bodies' ellipsoids (tests/test_gpu_motion.py) with their centres at 3 / 2 of x and y for the wider grid: centre, semi-axes, shift
TWO_BODIES = (((24, 48, 32), (9, 12, 20), (11, -9, 6)), ((69, 45, 30), (10, 9, 22), (-7, 10, -5)))


def pair(grid, b, s, levels, refine):
    """motion_np.random_pair with the shift drawn from [-reach, reach]."""
    return mn.random_pair(grid, 7 * b + grid[1] + levels, mp.reach(s, levels, refine))


def same_rows(got, want):
    for key in ROW_KEYS:
        assert np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)), key


@functools.lru_cache(maxsize=None)
def two_bodies():
    a = np.zeros((TWO_GRID[2], TWO_GRID[0], TWO_GRID[1]), dtype=bool)
    bo = np.zeros_like(a)
    for centre, semi, shift in TWO_BODIES:
        bo |= mn.ellipsoid(TWO_GRID, centre, semi)
        a |= mn.ellipsoid(TWO_GRID, tuple(c + d for c, d in zip(centre, shift)), semi)
    return a, bo


def two_bodies_exact(rows):
    """Per row the shift of the body its block belongs to (the bodies lie on either side of x = 48, block column 6)."""
    left = np.asarray(rows["ijk"])[:, 0] < 6
    return np.where(left[:, None], np.array(TWO_BODIES[0][2]), np.array(TWO_BODIES[1][2]))


@pytest.mark.parametrize("setting", SETTINGS[:3])
@pytest.mark.parametrize("grid", GRIDS)
def test_literal_and_packed_agree(grid, setting):
    b, ap, s, L, r = setting
    a, bo = pair(grid, b, s, L, r)
    lit = mp.match_pyramid_literal(a, bo, grid, b, ap, s, L, r)
    got = mp.match_pyramid(a, bo, grid, b, ap, s, L, r)
    for l in range(L + 1):
        same_rows(got["rows"][l], lit["rows"][l])
        assert np.array_equal(got["a"][l], lit["a"][l]) and np.array_equal(got["b"][l], lit["b"][l])
    assert got["evaluated"] == lit["evaluated"] and got["grids"] == lit["grids"]
    assert mp.stats(got, a, bo, grid, b) == mp.stats(lit, a, bo, grid, b)


@pytest.mark.parametrize("setting", SETTINGS[3:])
@pytest.mark.parametrize("grid", [(5, 7, 3), (9, 11, 7)])
def test_literal_and_packed_agree_on_a_wide_refine(grid, setting):
    """r = s = 8: 17^3 displacements per centre, which the literal version walks on the two small grids only."""
    b, ap, s, L, r = setting
    a, bo = pair(grid, b, s, L, r)
    lit = mp.match_pyramid_literal(a, bo, grid, b, ap, s, L, r)
    got = mp.match_pyramid(a, bo, grid, b, ap, s, L, r)
    for l in range(L + 1):
        same_rows(got["rows"][l], lit["rows"][l])
    assert got["evaluated"] == lit["evaluated"] > 0


def test_halve_is_the_or_of_the_children():
    rng = np.random.default_rng(5)
    occ = rng.random((3, 5, 7)) < 0.2                            # [iz, ix, iy]: odd on every axis
    h = mp.halve(occ)
    assert h.shape == (2, 3, 4) and mp.level_grid((5, 7, 3), 1) == (3, 4, 2) and mp.level_grid((5, 7, 3), 2) == (2, 2, 1)
    for z in range(2):
        for x in range(3):
            for y in range(4):
                assert h[z, x, y] == occ[2 * z:2 * z + 2, 2 * x:2 * x + 2, 2 * y:2 * y + 2].any()
    assert mp.reach(8, 3, 8) == 120 and mp.reach(4, 0, 1) == 4 and mp.reach(4, 2, 1) == 19


@pytest.mark.parametrize("grid", GRIDS)
def test_one_level_is_motion_np(grid):
    for b, ap, s in ((4, 0, 1), (8, 4, 4)):
        a, bo = pair(grid, b, s, 0, 1)
        got = mp.match_pyramid(a, bo, grid, b, ap, s, 0, 1)
        want = mn.match(a, bo, grid, b, ap, s)
        same_rows(got["rows"][0], want)
        st = mp.stats(got, a, bo, grid, b)
        assert {k: st[k] for k in mn.stats(want, a, bo, grid, b)} == mn.stats(want, a, bo, grid, b)
        assert (st["levels"], st["reach"], st["evaluated"], st["borrowed"]) == (0, s, 0, 0)
        assert st["listed_level"] == [st["listed"], 0, 0, 0] and st["dims_level"] == [list(grid), [0] * 3, [0] * 3, [0] * 3]


@pytest.mark.parametrize("setting", SETTINGS[:3])
@pytest.mark.parametrize("grid", GRIDS)
def test_every_listed_blocks_parent_is_listed(grid, setting):
    b, ap, s, L, r = setting
    a, bo = pair(grid, b, s, L, r)
    res = mp.match_pyramid(a, bo, grid, b, ap, s, L, r)
    for l in range(L):
        pnb = mn.block_dims(res["grids"][l + 1], b)
        ijk = np.asarray(res["rows"][l]["ijk"]) >> 1
        parents = (ijk[:, 2] * pnb[0] + ijk[:, 0]) * pnb[1] + ijk[:, 1]
        assert np.isin(parents, np.asarray(res["rows"][l + 1]["block"], dtype=np.int64)).all()
        d = np.asarray(res["rows"][l]["d"], dtype=np.int64)
        assert np.abs(d).max(initial=0) <= mp.reach(s, L - l, r)


def test_flag_bit_0_on_one_level_is_todays():
    """A single centre at 0 with r = s tries [-s, s]^3: a face neighbour of the winner is missing exactly when a component is +-s."""
    grid, b, ap, s = (12, 64, 10), 4, 2, 2
    a, bo = pair(grid, b, s, 0, 1)
    none = mn.match(np.zeros_like(mp.halve(a)), np.zeros_like(mp.halve(a)), mp.level_grid(grid, 1), b, ap, s)
    assert len(none["block"]) == 0
    # every block listed on the parent level with d = 0: the blocks of a level-1 grid, all of them
    pgrid = mp.level_grid(grid, 1)
    pnb = mn.block_dims(pgrid, b)
    n = pnb[0] * pnb[1] * pnb[2]
    parents = {"block": np.arange(n, dtype=np.uint32), "d": np.zeros((n, 3), dtype=np.int8)}
    rows, _ = mp._refine_packed(a, bo, grid, b, ap, s, parents, pgrid, True)
    want = mn.match(a, bo, grid, b, ap, s)
    for key in ("block", "d", "cost", "cost0", "ties"):
        assert np.array_equal(np.asarray(rows[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)), key
    assert np.array_equal(rows["flags"], want["flags"]) and (rows["flags"] == 1).any() and (rows["flags"] == 0).any()


def test_two_bodies_beyond_the_range():
    """96 x 96 x 64, 8 / 4 / 4, shifts of (+11, -9, +6) and (-7, +10, -5): a single level finds no vector; two coarser levels at
    r = 1 find every vector that is determined, and the warp is exact."""
    a, bo = two_bodies()
    one = mn.match(a, bo, TWO_GRID, 8, 4, 4)
    assert len(one["block"]) == 155 and int((one["d"].astype(np.int64) == two_bodies_exact(one)).all(axis=1).sum()) == 0
    assert int(one["cost"].sum()) == 121768
    assert round(mn.iou(a, bo), 3) == 0.064 and round(mn.iou(a, mn.warp(one, a, bo, TWO_GRID, 8)[0]), 3) == 0.294
    res = mp.match_pyramid(a, bo, TWO_GRID, 8, 4, 4, 2, 1)
    rows = res["rows"][0]
    st = mp.stats(res, a, bo, TWO_GRID, 8)
    exact = (rows["d"].astype(np.int64) == two_bodies_exact(rows)).all(axis=1)
    assert (st["listed"], st["unique"], st["moved"], st["cost_sum"], st["cost0_sum"]) == (155, 123, 155, 0, 219508)
    assert (st["listed_level"], st["evaluated"], st["reach"]) == ([155, 36, 11, 0], 10272, 19)
    assert int(exact.sum()) == 124 and exact[rows["ties"] == 1].all()
    P, wst = mn.warp(rows, a, bo, TWO_GRID, 8)
    assert mn.iou(a, P) == 1.0 and wst["warped"] == wst["common"] == wst["a"] == 17214
    # about 54 displacements per block where the single level tries 729
    assert st["evaluated"] / (st["listed_level"][0] + st["listed_level"][1]) < 62


def test_two_bodies_need_the_neighbours():
    """The same case with the parent's prediction alone: at the coarsest level one window spans both bodies and gives one of them the
    other's vector, and no refinement by 1 brings it back."""
    a, bo = two_bodies()
    res = mp.match_pyramid(a, bo, TWO_GRID, 8, 4, 4, 2, 1, neighbours=False)
    rows = res["rows"][0]
    P, _ = mn.warp(rows, a, bo, TWO_GRID, 8)
    assert mn.iou(a, P) < 0.8 and round(mn.iou(a, P), 3) == 0.708
    assert int(rows["cost"].astype(np.int64).sum()) == 34192 and int((rows["flags"] & mp.FLAG_BORROWED).sum()) == 0


def test_one_body_21_voxels():
    """One ellipsoid moved by (+21, -17, +10), L = 2, r = 2 (reach 22): every determined vector is exact, the warp too."""
    grid, shift = (96, 96, 64), (21, -17, 10)
    bo = mn.ellipsoid(grid, (36, 52, 26), (10, 9, 14))
    a = mn.shifted(bo, shift)
    assert a.sum() == bo.sum()
    res = mp.match_pyramid(a, bo, grid, 8, 4, 4, 2, 2)
    rows = res["rows"][0]
    sure = rows["ties"] == 1
    assert (len(rows["block"]), int(sure.sum())) == (68, 37)
    assert (rows["d"][sure].astype(np.int64) == np.array(shift)).all()
    assert mn.iou(a, mn.warp(rows, a, bo, grid, 8)[0]) == 1.0
    assert mn.iou(a, mn.warp(mn.match(a, bo, grid, 8, 4, 4), a, bo, grid, 8)[0]) == 0.0


def test_paint_scales_by_the_reach():
    grid, (b, ap, s, L, r) = (12, 64, 10), (8, 4, 4, 2, 1)
    a, bo = pair(grid, b, s, L, r)
    res = mp.match_pyramid(a, bo, grid, b, ap, s, L, r)
    idx = np.flatnonzero(a.reshape(-1)).astype(np.uint64)
    rec = idx | (np.uint64(0x01abcdef) << np.uint64(32))
    out = mp.paint(rec, res, grid, b)
    assert res["reach"] == 19 and np.array_equal(out, mn.paint(rec, res["rows"][0], grid, b, 19))
    assert np.abs(res["rows"][0]["d"].astype(np.int64)).max() > 4 and not np.array_equal(out, mn.paint(rec, res["rows"][0], grid, b, 4))
    ch = (out >> np.uint64(32)) & np.uint64(0xff)
    assert ch.min() >= 1 and ch.max() <= 255
