"""Coarse-to-fine block motion on the device (vc_hull_motion_pyramid, vc_fetch_motion_level, vc_fetch_motion_occupancy;
csrc/vc_motion_pyramid.h) against the restatement (tests/motion_pyramid_np.py), bit for bit: the rows of every level, the stats, the
level words of A and B, the warped register's words and count, the painted records; grids whose lines are word-aligned, packed two
and four to a word, straddling words and longer than two words; refine radii up to the search range and the 64-bit-wide row; empty and
equal hulls; block grids with an odd number of blocks; L = 0 against vc_hull_motion byte for byte; the two calls in turn; two bodies
that move beyond the search range; every refusal; the field's lifetime; configure(motion_levels=1) over three frames."""
import ctypes
import functools

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import motion_np as mn
import motion_pyramid_np as mp

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)
GRIDS = [(5, 7, 3), (9, 11, 7), (12, 64, 10), (37, 53, 29), (24, 130, 20)]
SETTINGS = [(4, 0, 1, 1, 1), (8, 4, 4, 2, 1), (8, 4, 4, 3, 2), (16, 8, 8, 1, 8)]
WIDE = (16, 16, 8, 1, 8)                                         # block + 2 apron + 2 search = 64: the row fills its word
ROW_KEYS = ("block", "ijk", "d", "cost", "cost0", "count_a", "count_b", "ties", "flags")
TWO_GRID = (96, 96, 64)
TWO_BODIES = (((24, 48, 32), (9, 12, 20), (11, -9, 6)), ((69, 45, 30), (10, 9, 22), (-7, 10, -5)))


@pytest.fixture(scope="module")
def meng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _start(e, grid, seed=3):
    """A grid with cameras and a carve result to replace (set_hull needs one)."""
    cams3, masks3, _ = fx.random_scene(seed, C=3, fg=0.7)
    e.set_grid(*grid)
    e.set_cameras(cams3, *masks3[0].shape)
    e.upload_masks(masks3)
    e.carve(min_views=1)


def _inject(e, a, b, reg=0):
    """A becomes the current result, B the hull of register `reg` (register 3 carries A in)."""
    e.set_hull(a, reg=3)
    e.upload_hull(b, reg)


@functools.lru_cache(maxsize=None)
def _case(grid, setting):
    """A hull pair whose shift is drawn from [-reach, reach], and the restatement's field of every level."""
    b, ap, s, L, r = setting
    a, bo = mn.random_pair(grid, 7 * b + grid[1] + L, mp.reach(s, L, r))
    return a, bo, mp.match_pyramid(a, bo, grid, b, ap, s, L, r)


def _same_rows(got, want):
    for key in ROW_KEYS:
        assert np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)), key


def _same_levels(e, res):
    """The rows and the words of A and B of every level; the scalars of the fetches."""
    L = res["levels"]
    for l in range(L + 1):
        rows = e.fetch_motion_level(l)
        _same_rows(rows, res["rows"][l])
        assert rows["grid"] == tuple(res["grids"][l]) and (rows["levels"], rows["refine"], rows["reach"]) == (L, res["refine"], res["reach"])
        assert np.array_equal(e.fetch_motion_occupancy(l, 0), mn.words(res["a"][l])), l
        assert np.array_equal(e.fetch_motion_occupancy(l, 1), mn.words(res["b"][l])), l
    _same_rows(e.fetch_motion(), res["rows"][0])


def _check_all(e, a, bo, res, grid, setting, src=0, dst=1):
    """hull_motion(levels=L), the per-level fetches, warp_hull and paint_motion against the restatement; what must not change."""
    b, ap, s, L, r = setting
    rec0 = e.fetch_records().copy()
    kept0 = e.fetch_kept(src)["words"].copy()
    e.fetch_combined()
    st = e.hull_motion(src, b, ap, s, levels=L, refine=r)
    assert st.pop("motion_ms") > 0
    want = mp.stats(res, a, bo, grid, b)
    assert st == want, (st, want)
    _same_levels(e, res)
    rows = e.fetch_motion()
    assert (rows["grid"], rows["edge"], rows["apron"], rows["search"]) == (tuple(grid), b, ap, s)
    # nothing changed: the records, the register, the generation (the combine's product is still current)
    assert np.array_equal(e.fetch_records(), rec0) and np.array_equal(e.fetch_kept(src)["words"], kept0)
    assert e.fetch_combined().size == rec0.size
    P, wst = mn.warp(res["rows"][0], a, bo, grid, b)
    got = e.warp_hull(src, dst)
    assert got.pop("warp_ms") > 0
    iou = got.pop("predicted_iou")
    assert got == wst, (got, wst)
    assert iou == mn.iou(a, P)
    k = e.fetch_kept(dst)
    assert k["count"] == wst["warped"] and not k["has_records"] and np.array_equal(k["words"], mn.words(P))
    _same_levels(e, res)                                         # (the warp leaves the field current, on every level)
    e.paint_motion()
    assert np.array_equal(e.fetch_records(), mp.paint(rec0, res, grid, b))
    _same_rows(e.fetch_motion_level(L), res["rows"][L])          # (a colour pass leaves it too)
    return st


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("grid", GRIDS)
def test_injected_pairs_equal_restatement(meng, grid, setting):
    a, bo, res = _case(grid, setting)
    _start(meng, grid)
    _inject(meng, a, bo)
    st = _check_all(meng, a, bo, res, grid, setting)
    assert st["listed"] > 0 and st["evaluated"] > 0


@pytest.mark.parametrize("grid", [(9, 11, 7), (12, 64, 10)])
def test_rows_of_64_bits(meng, grid):
    """16 / 16 / 8 with r = 8: the search region and the refine region are both 64 cells wide."""
    a, bo, res = _case(grid, WIDE)
    _start(meng, grid)
    _inject(meng, a, bo)
    assert _check_all(meng, a, bo, res, grid, WIDE)["listed"] > 0


def test_empty_and_equal_hulls(meng):
    grid, setting = (9, 11, 7), (4, 2, 2, 2, 1)
    a, bo, _ = _case(grid, (8, 4, 4, 2, 1))
    none = np.zeros_like(a)
    _start(meng, grid)
    for x, y in ((none, bo), (a, none), (a, a), (none, none)):
        _inject(meng, x, y)
        st = _check_all(meng, x, y, mp.match_pyramid(x, y, grid, *setting), grid, setting)
        if x is y:
            assert st["moved"] == 0 and st["cost_sum"] == st["cost0_sum"] == 0 and st["borrowed"] == 0
        if not x.any() and not y.any():
            assert st["listed_level"] == [0, 0, 0, 0] and st["evaluated"] == 0
            assert all(len(meng.fetch_motion_level(l)["block"]) == 0 for l in range(3))


def test_a_parent_with_one_child(meng):
    """(20, 24, 12) in blocks of 4 is 5 x 6 x 3 blocks over 3 x 3 x 2 parents: the last parent in x and in z has one child there."""
    grid, setting = (20, 24, 12), (4, 1, 2, 1, 1)
    a, bo, res = _case(grid, setting)
    assert mn.block_dims(grid, 4) == (5, 6, 3) and mn.block_dims(res["grids"][1], 4) == (3, 3, 2)
    assert (res["rows"][0]["ijk"][:, 0] == 4).any() and (res["rows"][0]["ijk"][:, 2] == 2).any()
    _start(meng, grid)
    _inject(meng, a, bo)
    _check_all(meng, a, bo, res, grid, setting)


def test_no_levels_is_vc_hull_motion_byte_for_byte(meng):
    """L = 0 through the new entry point: rows, the nine stats and the warp of vc_hull_motion; refine is checked and not used."""
    from voxcarve import motion
    grid, (b, ap, s) = (37, 53, 29), (8, 4, 4)
    a, bo = mn.random_pair(grid, 11, s)
    _start(meng, grid)
    _inject(meng, a, bo)
    old = meng.hull_motion(0, b, ap, s)
    old_rows = np.zeros(old["listed"], dtype=motion.ROW_DTYPE)
    L, ctx = meng._L, meng._ctx
    assert L.vc_fetch_motion(ctx, old_rows.ctypes.data_as(ctypes.c_void_p), None) == 0
    old_warp = meng.warp_hull(0, 1)
    old_words = meng.fetch_kept(1)["words"].copy()
    for refine in (1, 3):
        st = motion.PyramidStats()
        assert L.vc_hull_motion_pyramid(ctx, 0, b, ap, s, 0, refine, 0, ctypes.byref(st)) == 0, L.vc_last_error(ctx)
        new = motion.pyramid_stats_dict(st)
        assert {k: new[k] for k in old if k != "motion_ms"} == {k: v for k, v in old.items() if k != "motion_ms"}
        assert (new["levels"], new["refine"], new["reach"], new["evaluated"], new["borrowed"]) == (0, refine, s, 0, 0)
        assert new["listed_level"] == [old["listed"], 0, 0, 0] and new["dims_level"] == [list(grid), [0] * 3, [0] * 3, [0] * 3]
        for fetch in (lambda p: L.vc_fetch_motion(ctx, p, None), lambda p: L.vc_fetch_motion_level(ctx, 0, p, None)):
            rows = np.zeros(old["listed"], dtype=motion.ROW_DTYPE)
            assert fetch(rows.ctypes.data_as(ctypes.c_void_p)) == 0
            assert rows.tobytes() == old_rows.tobytes()
        w = meng.warp_hull(0, 1)
        assert {k: w[k] for k in ("warped", "common", "a")} == {k: old_warp[k] for k in ("warped", "common", "a")}
        assert np.array_equal(meng.fetch_kept(1)["words"], old_words)
    assert meng.hull_motion(0, b, ap, s, levels=0, refine=2).keys() == old.keys()


def test_the_two_calls_in_turn(meng):
    """vc_hull_motion after a pyramid call leaves a single-level field (its paint divides by the search range again), and back."""
    from voxcarve._lib import VoxcarveError
    grid, setting = (12, 64, 10), (8, 4, 4, 2, 1)
    b, ap, s, L, r = setting
    a, bo, res = _case(grid, setting)
    one = mn.match(a, bo, grid, b, ap, s)
    _start(meng, grid)
    _inject(meng, a, bo)
    rec0 = meng.fetch_records().copy()
    for _ in range(2):
        meng.hull_motion(0, b, ap, s, levels=L, refine=r)
        _same_levels(meng, res)
        meng.paint_motion()
        assert np.array_equal(meng.fetch_records(), mp.paint(rec0, res, grid, b))
        st = meng.hull_motion(0, b, ap, s)
        st.pop("motion_ms")
        assert st == mn.stats(one, a, bo, grid, b)
        rows = meng.fetch_motion()
        _same_rows(rows, one)
        assert sorted(rows) == sorted(ROW_KEYS + ("grid", "edge", "apron", "search"))      # the dict it always was
        level0 = meng.fetch_motion_level(0)
        _same_rows(level0, one)
        assert (level0["levels"], level0["reach"]) == (0, s)
        with pytest.raises(VoxcarveError, match="vc_fetch_motion_level: level 1, the field has the levels 0..0"):
            meng.fetch_motion_level(1)
        with pytest.raises(VoxcarveError, match="vc_fetch_motion_occupancy: level 1"):
            meng.fetch_motion_occupancy(1, 0)
        assert np.array_equal(meng.fetch_motion_occupancy(0, 1), mn.words(bo))
        meng.paint_motion()
        assert np.array_equal(meng.fetch_records(), mn.paint(rec0, one, grid, b, s))


def test_two_bodies_beyond_the_range(meng):
    """The case of tests/test_motion_pyramid_restatement.py on the device, with its numbers."""
    grid = TWO_GRID
    a = np.zeros((grid[2], grid[0], grid[1]), dtype=bool)
    bo = np.zeros_like(a)
    for centre, semi, shift in TWO_BODIES:
        bo |= mn.ellipsoid(grid, centre, semi)
        a |= mn.ellipsoid(grid, tuple(c + d for c, d in zip(centre, shift)), semi)
    _start(meng, grid)
    _inject(meng, a, bo)
    one = meng.hull_motion(0)
    assert (one["listed"], one["cost_sum"]) == (155, 121768)
    assert round(meng.warp_hull(0, 1)["predicted_iou"], 3) == 0.294
    st = meng.hull_motion(0, levels=2, refine=1)                 # 8 / 4 / 4
    assert (st["listed"], st["unique"], st["moved"], st["cost_sum"], st["cost0_sum"]) == (155, 123, 155, 0, 219508)
    assert (st["listed_level"], st["evaluated"], st["reach"], st["borrowed"]) == ([155, 36, 11, 0], 10272, 19, 0)
    rows = meng.fetch_motion()
    left = rows["ijk"][:, 0] < 6
    exact = (rows["d"].astype(np.int64) == np.where(left[:, None], np.array(TWO_BODIES[0][2]), np.array(TWO_BODIES[1][2]))).all(axis=1)
    assert int(exact.sum()) == 124 and exact[rows["ties"] == 1].all()
    w = meng.warp_hull(0, 1)
    assert w["predicted_iou"] == 1.0 and w["warped"] == w["common"] == w["a"] == int(a.sum()) == 17214


def test_refusals(built):
    import voxcarve
    from voxcarve import motion
    from voxcarve._lib import VoxcarveError
    grid = (9, 11, 7)
    a, bo, _ = _case(grid, (8, 4, 4, 2, 1))
    with voxcarve.CarveEngine(0) as e:
        cams3, masks3, _ = fx.random_scene(3, C=3, fg=0.7)
        e.set_grid(*grid)
        e.set_cameras(cams3, *masks3[0].shape)
        e.upload_masks(masks3)
        with pytest.raises(VoxcarveError, match="vc_hull_motion_pyramid: no carve result"):
            e.hull_motion(0, levels=1)
        e.carve(min_views=1)
        with pytest.raises(VoxcarveError, match="register 0 is empty"):
            e.hull_motion(0, levels=1)
        with pytest.raises(VoxcarveError, match="register 4, there are 4"):
            e.hull_motion(4, levels=1)
        _inject(e, a, bo)
        for kw in ({"levels": 4}, {"levels": -1}, {"levels": 1, "refine": 0}, {"levels": 1, "refine": 5}, {"levels": 0, "refine": 0},
                   {"levels": 0, "refine": 5}, {"levels": True}, {"levels": 1.0}):
            with pytest.raises(ValueError):
                e.hull_motion(0, 8, 4, 4, **kw)
        for bad in ((5, 0, 1), (8, 17, 1), (8, 4, 0), (8, 4, 9)):
            with pytest.raises(ValueError):
                e.hull_motion(0, *bad, levels=1)
        L, ctx = e._L, e._ctx
        st = motion.PyramidStats()
        for args, text in (((0, 8, 4, 4, 4, 1, 0), "4 coarser levels, at most 3"), ((0, 8, 4, 4, 1, 0, 0), "refine radius 0 not in 1..search = 4"),
                           ((0, 8, 4, 4, 1, 5, 0), "refine radius 5 not in 1..search = 4"), ((0, 8, 4, 4, 0, 5, 0), "refine radius 5"),
                           ((0, 8, 4, 4, 1, 1, 1), "flags must be 0"), ((0, 5, 0, 1, 1, 1, 0), "block edge 5, expected 4, 8 or 16"),
                           ((0, 8, 17, 1, 1, 1, 0), "apron 17 not in 0..16"), ((0, 8, 4, 0, 1, 1, 0), "search range 0 not in 1..8"),
                           ((0, 8, 4, 9, 1, 1, 0), "search range 9 not in 1..8"), ((0, 16, 16, 9, 1, 1, 0), "search range 9"),
                           ((0, 16, 16, 8, 1, 9, 0), "refine radius 9")):
            assert L.vc_hull_motion_pyramid(ctx, *args, ctypes.byref(st)) != 0
            assert "vc_hull_motion_pyramid: " + text in L.vc_last_error(ctx).decode(), (args, L.vc_last_error(ctx))
        assert L.vc_hull_motion_pyramid(ctx, 0, 8, 4, 4, 1, 1, 0, None) != 0 and "stats must not be NULL" in L.vc_last_error(ctx).decode()
        # no field yet: every refused call above left none
        for call, what in ((lambda: e.fetch_motion_level(1), "vc_fetch_motion_level"), (lambda: e.fetch_motion_occupancy(0, 0), "vc_fetch_motion_occupancy"),
                           (e.fetch_motion, "vc_fetch_motion"), (e.paint_motion, "vc_paint_motion")):
            with pytest.raises(VoxcarveError, match="%s: no motion field" % what):
                call()
        e.hull_motion(0, 16, 16, 8, levels=1, refine=8)          # b + 2a + 2s = 64 itself is allowed, with r = s
        e.hull_motion(0, levels=2)
        for call, text in ((lambda: e.fetch_motion_level(3), "vc_fetch_motion_level: level 3, the field has the levels 0..2"),
                           (lambda: e.fetch_motion_occupancy(3, 0), "vc_fetch_motion_occupancy: level 3, the field has the levels 0..2"),
                           (lambda: e.fetch_motion_occupancy(2, 2), "which = 2, expected 0 .A. or 1 .B.")):
            with pytest.raises(VoxcarveError, match=text):
                call()
        n = ctypes.c_uint64(0)
        assert L.vc_fetch_motion_level(ctx, 2, None, ctypes.byref(n)) == 0 and n.value == len(e.fetch_motion_level(2)["block"])
        assert L.vc_fetch_motion_occupancy(ctx, 2, 1, None, ctypes.byref(n)) == 0 and n.value == 1       # (3, 3, 2): 18 cells
        assert L.vc_fetch_motion_level(ctx, 2, None, None) == 0 and L.vc_fetch_motion_occupancy(ctx, 2, 1, None, None) == 0
        # a stale field: the generation, the register
        e.upload_hull(bo, 0)
        for call in (lambda: e.fetch_motion_level(1), lambda: e.fetch_motion_occupancy(1, 1)):
            with pytest.raises(VoxcarveError, match="no motion field"):
                call()
        e.set_slab(0, 3)
        e.carve(min_views=1)
        with pytest.raises(VoxcarveError, match="narrower than the grid"):
            e.hull_motion(0, levels=1)
        e.set_slab(0, grid[2])
        e.carve(min_views=1, records=False)
        with pytest.raises(VoxcarveError, match="VC_FLAG_NO_RECORDS"):
            e.hull_motion(0, levels=1)


def test_field_lifetime(meng):
    from voxcarve._lib import VoxcarveError
    grid, setting = (12, 64, 10), (8, 4, 4, 2, 1)
    a, bo, res = _case(grid, setting)
    _start(meng, grid)

    def fresh():
        _inject(meng, a, bo)
        meng.hull_motion(0, levels=2, refine=1)
        _same_levels(meng, res)

    def stale(warp="no motion field"):
        for call, text in ((meng.fetch_motion, "no motion field"), (meng.paint_motion, "no motion field"), (lambda: meng.warp_hull(0, 1), warp),
                           (lambda: meng.fetch_motion_level(0), "no motion field"), (lambda: meng.fetch_motion_level(2), "no motion field"),
                           (lambda: meng.fetch_motion_occupancy(1, 0), "no motion field"), (lambda: meng.fetch_motion_occupancy(0, 1), "no motion field")):
            with pytest.raises(VoxcarveError, match=text):
                call()

    fresh()
    meng.carve(min_views=1)                                      # a carve
    stale()
    fresh()
    assert meng.combine_hull("or", 0)["added"] > 0               # a pass that changes the survivors
    stale()
    fresh()
    meng.keep_hull(0)                                            # the register rewritten
    stale()
    fresh()
    meng.upload_hull(bo, 0)
    stale()
    fresh()
    meng.release_hull(0)
    stale(warp="register 0 is empty")                            # (the warp names its empty source first)
    fresh()
    meng.keep_hull(2)                                            # another register: nothing to the field
    meng.release_hull(2)
    meng.warp_hull(0, 2)
    _same_levels(meng, res)
    meng.set_grid(*grid)                                         # the geometry
    with pytest.raises(VoxcarveError):
        meng.fetch_motion_level(1)


def test_motion_stage_over_three_frames(built):
    """configure(motion_block=8, motion_levels=1): the first frame only keeps; from the second on the stage matches coarse to fine."""
    import os
    from voxcarve import assignment
    masks = fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    sets = [(frames, [np.roll(m, 4 * t, axis=1) for m in masks]) for t in range(3)]
    n = 64
    try:
        for bad in ({"motion_levels": 4}, {"motion_refine": 0}, {"motion_refine": 5}, {"motion_levels": None}):
            with pytest.raises(ValueError):
                assignment.configure(motion_block=8, **bad)
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=os.path.join(fx.GOLDEN, "data"), motion_block=8,
                             motion_levels=1, motion_paint=True)
        assignment.set_voxel_positions(n, n // 2, n)
        e = assignment._engine
        with pytest.raises(RuntimeError, match="no motion field"):
            assignment.motion()                                  # the first frame only keeps
        prev = dn.volume((e.fetch_records() & LOW).astype(np.uint32), e.grid)
        for _ in range(2):
            pos, col = assignment.set_voxel_positions(n, n // 2, n)
            m = assignment.motion()
            st, rows = dict(m["stats"]), m["rows"]
            rec = e.fetch_records()
            a = dn.volume((rec & LOW).astype(np.uint32), e.grid)
            res = mp.match_pyramid(a, prev, e.grid, 8, 4, 4, 1, 1)
            _same_rows(rows, res["rows"][0])
            assert st.pop("motion_ms") > 0 and st == mp.stats(res, a, prev, e.grid, 8) and st["listed"] > 0
            assert (rows["levels"], rows["refine"], rows["reach"]) == (1, 1, 9)
            assert m["description"]["velocity_mm"].shape == (st["listed"], 3)
            assert np.array_equal(rec, mp.paint(rec, res, e.grid, 8)) and len(pos) == rec.size    # painted, then handed out
            assert np.array_equal(e.fetch_kept(1)["words"], mn.words(a))
            prev = a
    finally:
        assignment.configure(frame_source=None, motion_block=0, motion_paint=False, motion_levels=0, motion_refine=1)
