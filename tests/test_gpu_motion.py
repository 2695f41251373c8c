"""Block motion between two hulls on the device (vc_hull_motion, vc_fetch_motion, vc_hull_warp, vc_paint_motion; csrc/vc_motion.h)
against the restatement (tests/motion_np.py), bit for bit: rows, stats, the warped register's words and count, the painted records,
on injected hull pairs and on a pair of real carves; grids of one block per axis, of lines that are word-aligned, that straddle words
and that are longer than two words; the 64-bit-wide row of (16, 8, 8); empty and equal hulls; two bodies; every refusal; the field's
lifetime; configure(motion_block=8) over three frames."""
import functools

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import motion_np as mn

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)
GRIDS = [(5, 7, 3), (9, 11, 7), (12, 64, 10), (37, 53, 29), (24, 130, 20)]
PARAMS = [(4, 0, 1), (8, 4, 4), (16, 8, 8)]
STAT_KEYS = ("blocks", "listed", "moved", "unique", "clipped", "cost0_sum", "cost_sum", "a", "b")


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
def _case(grid, b, ap, s):
    a, bo = mn.random_pair(grid, 7 * b + grid[1], s)
    return a, bo, mn.match(a, bo, grid, b, ap, s)


def _same_rows(got, want):
    for key in ("block", "ijk", "d", "cost", "cost0", "count_a", "count_b", "ties", "flags"):
        assert np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)), key


def _check_all(e, a, bo, want, grid, b, ap, s, src=0, dst=1, probe=None):
    """hull_motion, fetch_motion, warp_hull, compare_hull(dst) and paint_motion against the restatement; what must not change.
    probe: a fetch of a product of the current generation (default: the added bytes of the combine that brought A in)."""
    rec0 = e.fetch_records().copy()
    kept0 = e.fetch_kept(src)["words"].copy()
    probe = e.fetch_combined if probe is None else probe
    probe()
    st = e.hull_motion(src, b, ap, s)
    assert st.pop("motion_ms") > 0
    assert st == mn.stats(want, a, bo, grid, b), (st, mn.stats(want, a, bo, grid, b))
    rows = e.fetch_motion()
    _same_rows(rows, want)
    assert (rows["grid"], rows["edge"], rows["apron"], rows["search"]) == (tuple(grid), b, ap, s)
    # nothing changed: the records, the register, the generation (the probe's product is still current)
    assert np.array_equal(e.fetch_records(), rec0) and np.array_equal(e.fetch_kept(src)["words"], kept0)
    assert probe().size == rec0.size
    P, wst = mn.warp(want, a, bo, grid, b)
    got = e.warp_hull(src, dst)
    assert got.pop("warp_ms") > 0
    iou = got.pop("predicted_iou")
    assert got == wst, (got, wst)
    assert iou == mn.iou(a, P)
    k = e.fetch_kept(dst)
    assert k["count"] == wst["warped"] and not k["has_records"] and np.array_equal(k["words"], mn.words(P))
    cmp_ = e.compare_hull(dst)
    assert cmp_["common"] == wst["common"] and cmp_["b"] == wst["warped"] and cmp_["a"] == wst["a"]
    _same_rows(e.fetch_motion(), want)                           # (the warp leaves the field current)
    e.paint_motion()
    assert np.array_equal(e.fetch_records(), mn.paint(rec0, want, grid, b, s))
    _same_rows(e.fetch_motion(), want)                           # (a colour pass leaves it too)
    return st


@pytest.mark.parametrize("b,ap,s", PARAMS)
@pytest.mark.parametrize("grid", GRIDS)
def test_injected_pairs_equal_restatement(meng, grid, b, ap, s):
    a, bo, want = _case(grid, b, ap, s)
    _start(meng, grid)
    _inject(meng, a, bo)
    st = _check_all(meng, a, bo, want, grid, b, ap, s)
    assert st["listed"] > 0


@pytest.mark.parametrize("grid", [(9, 11, 7), (12, 64, 10)])
def test_rows_of_64_bits(meng, grid):
    """16 / 16 / 8 is the one setting whose search region is 64 cells wide: a mask of 64 ones, a row that fills its word."""
    a, bo, want = _case(grid, 16, 16, 8)
    _start(meng, grid)
    _inject(meng, a, bo)
    assert _check_all(meng, a, bo, want, grid, 16, 16, 8)["listed"] > 0


def test_real_carve_pair_equals_restatement(meng):
    """B is the carve of the masks rolled by three columns, kept with keep_hull; A the carve of the masks as they are."""
    grid = (37, 53, 29)
    cams3, masks3, _ = fx.random_scene(4, C=3, fg=0.7)
    meng.set_grid(*grid)
    meng.set_cameras(cams3, *masks3[0].shape)
    meng.upload_masks([np.roll(m, 3, axis=1) for m in masks3])
    assert meng.carve(min_views=2) > 0
    bo = dn.volume((meng.fetch_records() & LOW).astype(np.uint32), grid)
    meng.keep_hull(0)
    meng.upload_masks(masks3)
    assert meng.carve(min_views=2) > 0
    a = dn.volume((meng.fetch_records() & LOW).astype(np.uint32), grid)
    assert (a != bo).any()
    for b, ap, s in ((8, 4, 4), (4, 2, 2)):
        meng.hull_distance()
        _check_all(meng, a, bo, mn.match(a, bo, grid, b, ap, s), grid, b, ap, s, probe=meng.fetch_record_distance)
        meng.carve(min_views=2)                                  # (the camera colours again)


def test_empty_and_equal_hulls(meng):
    grid = (9, 11, 7)
    a, bo, _ = _case(grid, 8, 4, 4)
    none = np.zeros_like(a)
    _start(meng, grid)
    for x, y in ((none, bo), (a, none), (a, a), (none, none)):
        _inject(meng, x, y)
        st = _check_all(meng, x, y, mn.match(x, y, grid, 4, 2, 2), grid, 4, 2, 2)
        if x is y:
            assert st["moved"] == 0 and st["cost_sum"] == st["cost0_sum"] == 0
        if not x.any() and not y.any():
            assert st["listed"] == 0 and len(meng.fetch_motion()["block"]) == 0


def test_two_bodies(meng):
    grid = (64, 64, 64)
    bodies = (((16, 32, 32), (9, 12, 20), (3, -2, 1)), ((46, 30, 30), (10, 9, 22), (-1, 3, -2)))
    a = np.zeros((64, 64, 64), dtype=bool)
    bo = np.zeros_like(a)
    for centre, semi, shift in bodies:
        bo |= mn.ellipsoid(grid, centre, semi)
        a |= mn.ellipsoid(grid, tuple(c + d for c, d in zip(centre, shift)), semi)
    _start(meng, grid)
    _inject(meng, a, bo)
    st = meng.hull_motion(0)                                     # the defaults: 8, 4, 4
    # (cost_sum is 8, not 0: the windows of the blocks next to x = 32 reach into the other body, which moves another way)
    assert (st["listed"], st["unique"], st["moved"], st["cost_sum"], st["cost0_sum"]) == (112, 112, 112, 8, 62722)
    rows = meng.fetch_motion()
    left = rows["ijk"][:, 0] < 4
    assert left.sum() == 56
    assert np.array_equal(rows["d"].astype(np.int64), np.where(left[:, None], np.array(bodies[0][2]), np.array(bodies[1][2])))
    assert meng.compare_hull(0)["iou"] < 0.6
    w = meng.warp_hull(0, 1)
    assert w["predicted_iou"] == 1.0 and w["warped"] == w["common"] == w["a"] == int(a.sum())
    assert meng.compare_hull(1)["only_a"] == meng.compare_hull(1)["only_b"] == 0
    # the field per figure and in millimetres
    from voxcarve import motion
    idx = (meng.fetch_records() & LOW).astype(np.int64)
    fm = motion.figure_motion(rows, idx, ((idx // 64) % 64 >= 32).astype(np.uint8), 2)
    assert fm["d"].tolist() == [[3.0, -2.0, 1.0], [-1.0, 3.0, -2.0]]
    desc = motion.describe(rows, meng.grid, meng.bounds, fps=30)
    assert np.allclose(desc["velocity_mm"], rows["d"] * motion.steps_mm(meng.grid, meng.bounds))


def test_refusals(built):
    import voxcarve
    from voxcarve._lib import VoxcarveError
    grid = (9, 11, 7)
    a, bo, _ = _case(grid, 8, 4, 4)
    with voxcarve.CarveEngine(0) as e:
        cams3, masks3, _ = fx.random_scene(3, C=3, fg=0.7)
        e.set_grid(*grid)
        e.set_cameras(cams3, *masks3[0].shape)
        e.upload_masks(masks3)
        with pytest.raises(VoxcarveError, match="vc_hull_motion: no carve result"):
            e.hull_motion(0)
        e.carve(min_views=1)
        with pytest.raises(VoxcarveError, match="register 0 is empty"):
            e.hull_motion(0)
        with pytest.raises(VoxcarveError, match="register 4, there are 4"):
            e.hull_motion(4)
        _inject(e, a, bo)
        for bad in ((5, 0, 1), (8, 17, 1), (8, 4, 0), (8, 4, 9)):
            with pytest.raises(ValueError):
                e.hull_motion(0, *bad)
        L, ctx = e._L, e._ctx
        from voxcarve import motion
        st, ws = motion.MotionStats(), motion.WarpStats()
        import ctypes
        for args, text in (((0, 5, 0, 1, 0), "block edge 5"), ((0, 8, 17, 1, 0), "apron 17"), ((0, 8, 4, 0, 0), "search range 0"),
                           ((0, 8, 4, 9, 0), "search range 9"), ((0, 8, 4, 4, 1), "flags must be 0")):
            assert L.vc_hull_motion(ctx, *args, ctypes.byref(st)) != 0 and text in L.vc_last_error(ctx).decode()
        assert L.vc_hull_motion(ctx, 0, 8, 4, 4, 0, None) != 0 and "stats must not be NULL" in L.vc_last_error(ctx).decode()
        for call, what in ((e.fetch_motion, "vc_fetch_motion"), (e.paint_motion, "vc_paint_motion"), (lambda: e.warp_hull(0, 1), "vc_hull_warp")):
            with pytest.raises(VoxcarveError, match="%s: no motion field" % what):
                call()
        e.hull_motion(0, 16, 16, 8)                              # b + 2a + 2s = 64 itself is allowed
        e.hull_motion(0)
        with pytest.raises(VoxcarveError, match="source and target are both register 0"):
            e.warp_hull(0, 0)
        with pytest.raises(VoxcarveError, match="register 4, there are 4"):
            e.warp_hull(0, 4)
        with pytest.raises(VoxcarveError, match="made against register 0, not 3"):
            e.warp_hull(3, 1)
        with pytest.raises(VoxcarveError, match="register 2 is empty"):
            e.warp_hull(2, 1)
        assert L.vc_hull_warp(ctx, 0, 1, 1, ctypes.byref(ws)) != 0 and "flags must be 0" in L.vc_last_error(ctx).decode()
        assert L.vc_hull_warp(ctx, 0, 1, 0, None) != 0
        with pytest.raises(VoxcarveError, match="register 1 is empty"):
            e.fetch_kept(1)                                      # (no refused warp wrote its target)
        e.set_slab(0, 3)
        e.carve(min_views=1)
        with pytest.raises(VoxcarveError, match="narrower than the grid"):
            e.hull_motion(0)
        e.set_slab(0, grid[2])
        e.carve(min_views=1, records=False)
        with pytest.raises(VoxcarveError, match="VC_FLAG_NO_RECORDS"):
            e.hull_motion(0)


def test_field_lifetime(meng):
    from voxcarve._lib import VoxcarveError
    grid = (12, 64, 10)
    a, bo, want = _case(grid, 8, 4, 4)
    _start(meng, grid)

    def fresh():
        _inject(meng, a, bo)
        meng.hull_motion(0)
        _same_rows(meng.fetch_motion(), want)

    def stale(warp="no motion field"):
        for call, text in ((meng.fetch_motion, "no motion field"), (meng.paint_motion, "no motion field"), (lambda: meng.warp_hull(0, 1), warp)):
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
    _same_rows(meng.fetch_motion(), want)
    meng.set_grid(*grid)                                         # the geometry
    with pytest.raises(VoxcarveError):
        meng.fetch_motion()


def test_colour_passes_leave_the_field(meng):
    grid = (37, 53, 29)
    cams3, masks3, frames3 = fx.random_scene(4, C=3, fg=0.7)
    meng.set_grid(*grid)
    meng.set_cameras(cams3, *masks3[0].shape)
    meng.upload_masks(masks3)
    for c in range(3):
        meng.upload_frame(c, frames3[c])
    assert meng.carve(min_views=2) > 0
    meng.keep_hull(0)
    meng.upload_masks([np.roll(m, 2, axis=1) for m in masks3])
    for c in range(3):
        meng.upload_frame(c, frames3[c])
    assert meng.carve(min_views=2) > 0
    meng.hull_motion(0)
    rows = meng.fetch_motion()
    meng.color_visible()
    meng.cluster_hull(2)
    meng.paint_clusters()
    meng.paint_motion()
    _same_rows(meng.fetch_motion(), rows)
    assert meng.clusters_valid()                                 # (paint_motion is a colour pass too)
    assert meng.warp_hull(0, 1)["warped"] > 0


def test_motion_stage_over_three_frames(built):
    """configure(motion_block=8): the first frame only keeps; from the second on the stage matches against register 1."""
    import os
    from voxcarve import assignment
    masks = fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    sets = [(frames, [np.roll(m, 4 * t, axis=1) for m in masks]) for t in range(3)]
    n = 64
    try:
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=os.path.join(fx.GOLDEN, "data"), motion_block=8,
                             motion_paint=True)
        with pytest.raises(RuntimeError, match="no motion field"):
            assignment.motion()
        assignment.set_voxel_positions(n, n // 2, n)
        e = assignment._engine
        with pytest.raises(RuntimeError, match="no motion field"):
            assignment.motion()                                  # the first frame only keeps
        prev = dn.volume((e.fetch_records() & LOW).astype(np.uint32), e.grid)
        assert np.array_equal(e.fetch_kept(1)["words"], mn.words(prev))
        for _ in range(2):
            pos, col = assignment.set_voxel_positions(n, n // 2, n)
            m = assignment.motion()
            st, rows = m["stats"], m["rows"]
            rec = e.fetch_records()
            a = dn.volume((rec & LOW).astype(np.uint32), e.grid)
            want = mn.match(a, prev, e.grid, 8, 4, 4)
            _same_rows(rows, want)
            assert {k: st[k] for k in STAT_KEYS} == mn.stats(want, a, prev, e.grid, 8) and st["listed"] > 0
            assert m["description"]["velocity_mm"].shape == (st["listed"], 3)
            assert np.array_equal(rec, mn.paint(rec, want, e.grid, 8, 4)) and len(pos) == rec.size    # painted, then handed out
            assert np.array_equal(e.fetch_kept(1)["words"], mn.words(a))
            prev = a
    finally:
        assignment.configure(frame_source=None, motion_block=0, motion_paint=False)
