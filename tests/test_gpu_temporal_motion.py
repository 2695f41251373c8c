"""The motion-compensated vote on the device (vc_hull_temporal_motion, vc_fetch_temporal_motion; csrc/vc_temporal_motion.h)
against the restatement (tests/temporal_motion_np.py), bit for bit after every call of a sequence: every stat, the field's rows,
all 8 bytes of every record in order, the vote and `added` bytes, the occupancy words and every snapshot of the ring.  Hulls are
injected (set_hull after a carve): random boxes that move by a vector within the search range with 2 % of the cells flipped, one
or two bodies.  Grids of two words with many segments per word, of an odd word count, of word-aligned lines, of lines that
straddle words and of lines longer than two words; windows 1, 2, 3, 5 and 15 so that the ring wraps; thresholds and motion
parameters changed half way; an empty hull and a solid grid inside a sequence; a figure that leaves the grid; a voxel kept by an
old speck in an unlisted block; restored voxels with and without a colour camera; the state rules; every refusal;
configure(temporal_window=3, temporal_motion=True)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import motion_np as mo
import temporal_motion_np as tm
import temporal_np as tn

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)
ROW_KEYS = ("block", "ijk", "d", "cost", "cost0", "count_a", "count_b", "ties", "flags")


@pytest.fixture(scope="module")
def veng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _words(e):
    raw = np.empty((e.n_voxels + 63) // 64, dtype=np.uint64)
    e._check(e._L.vc_fetch_occupancy(e._ctx, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "vc_fetch_occupancy")
    return raw


def _same_rows(got, want):
    for key in ROW_KEYS:
        assert np.array_equal(np.asarray(got[key]).astype(np.int64).reshape(-1), np.asarray(want[key]).astype(np.int64).reshape(-1)), key


def _start(e, grid, seed=3, cc=1):
    """A grid with cameras, frames and a carve result to replace (set_hull needs one); the ring starts over."""
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    e.set_grid(*grid)
    e.set_cameras(cams3, *masks3[0].shape)
    e.upload_masks(masks3)
    if cc is not None:
        e.upload_frame(cc, frames3[cc])
    e.carve(min_views=1)
    e.temporal_reset()
    return cams3, frames3


class Follower:
    """The restatement beside an engine: every step injects a hull, votes on both and compares everything the device exposes."""

    def __init__(self, e, cams, frames=None, cc=1):
        self.e, self.v = e, tm.AlignedVote()
        self.cam = None if cc is None else fx.oracle_cams(cams)[cc]
        self.frame = None if frames is None or cc is None else frames[cc]
        self.cc = cc

    def step(self, hull, window, on, off, params):
        e = self.e
        e.carve(min_views=1, color_cam=self.cc)                  # (another result: one push per result)
        e.set_hull(hull, reg=3)
        rec = e.fetch_records().copy()
        occ = dn.volume((rec & LOW).astype(np.uint32), e.grid)
        assert np.array_equal(occ, hull)
        window_, on_, off_ = e.temporal_thresholds(window, on, off)
        b, ap, s = params
        out, c, ws = self.v.push(occ, window_, on_, off_, b, ap, s)
        H, W = e.image_size
        want, wvotes, wadded = tn.records_after(rec, occ, out, c, e.grid, e.bounds, self.cam, self.frame, H, W)
        st = e.temporal_filter(window, on, off, motion=params)
        ms = st.pop("temporal_ms")
        assert st == ws, (st, ws)
        assert ms > 0 and e.count == want.size
        _same_rows(e.fetch_temporal_motion(), self.v.rows)
        got = e.fetch_records()
        assert np.array_equal(got & LOW, want & LOW), "indices and order"
        assert np.array_equal(got, want), "records"
        votes, added = e.fetch_temporal()
        assert np.array_equal(votes, wvotes), "vote bytes"
        assert np.array_equal(added, wadded), "added bytes"
        assert np.array_equal(_words(e), mo.words(out)), "occupancy words"
        for age in range(ws["frames"]):
            assert np.array_equal(e.temporal_history(age), mo.words(self.v.history(age))), "history %d" % age
        return st, want, wadded


@functools.lru_cache(maxsize=None)
def _sequence(grid, seed, frames, s, bodies):
    return tm.moving_boxes(grid, seed, frames, s, bodies=bodies)


def _run(e, grid, window, pairs, params_list, seed, bodies=1):
    """2 window + 2 frames; thresholds and motion parameters change half way; an empty hull and a solid grid inside."""
    cams3, frames3 = _start(e, grid)
    f = Follower(e, cams3, frames3)
    n_frames = 2 * window + 2
    hulls = _sequence(grid, seed, n_frames, min(p[2] for p in params_list), bodies)
    tot = {"moved": 0, "added": 0, "removed": 0, "listed": 0}
    for t in range(n_frames):
        hull = hulls[t]
        if window > 1 and t == window // 2 + 1:
            hull = np.zeros_like(hull)                           # an empty hull
        elif window > 1 and t == window + 2:
            hull = np.ones_like(hull)                            # a solid grid
        on, off = pairs[(t * len(pairs)) // n_frames]
        params = params_list[(t * len(params_list)) // n_frames]
        st, _, _ = f.step(hull, window, on, off, params)
        for k in tot:
            tot[k] += st[k]
    return tot, f


@pytest.mark.parametrize("grid,window,pairs,params_list", [
    ((5, 7, 3), 1, [(1, 1)], [(4, 0, 1)]),
    ((5, 7, 3), 3, [(2, 1), (3, 3)], [(4, 0, 1), (8, 4, 4)]),
    ((5, 7, 3), 15, [(8, 4)], [(4, 0, 1)]),
    ((9, 11, 7), 2, [(2, 2), (1, 1)], [(4, 0, 1), (16, 8, 8)]),
    ((9, 11, 7), 5, [(None, None), (4, 2)], [(8, 4, 4), (4, 0, 1)]),
    ((12, 64, 10), 3, [(2, 2), (3, 1)], [(16, 8, 8), (8, 4, 4)]),
    ((12, 64, 10), 5, [(5, 1), (3, 2)], [(4, 0, 1)]),
    ((37, 53, 29), 2, [(2, 1)], [(8, 4, 4)]),
    ((37, 53, 29), 5, [(3, 3), (4, 2)], [(4, 0, 1)]),
    ((24, 130, 20), 3, [(2, 2), (2, 1)], [(8, 4, 4), (4, 0, 1)])])
def test_sequences_equal_restatement(veng, grid, window, pairs, params_list):
    tot, _ = _run(veng, grid, window, pairs, params_list, seed=grid[1] + window)
    assert tot["listed"] > 0 and tot["moved"] > 0
    if window == 1:
        assert tot["added"] == tot["removed"] == 0               # window 1 is the identity
    else:
        assert tot["removed"] > 0 and (tot["added"] > 0 or grid == (5, 7, 3))    # (105 cells: the votes only ever drop there)


def test_two_bodies_moving_differently(veng):
    grid = (37, 53, 29)
    cams3, frames3 = _start(veng, grid)
    f = Follower(veng, cams3, frames3)
    bodies = (((9, 14, 14), (5, 8, 9), (2, 1, 0)), ((27, 36, 13), (6, 9, 8), (-1, -2, 1)))
    rng = np.random.default_rng(9)
    distinct = 0
    for t in range(5):
        hull = np.zeros((29, 37, 53), dtype=bool)
        for centre, semi, step in bodies:
            hull |= mo.ellipsoid(grid, tuple(c + t * d for c, d in zip(centre, step)), semi)
        hull ^= rng.random(hull.shape) < 0.02
        st, _, _ = f.step(hull, 3, 2, 2, (8, 4, 4))
        d = np.asarray(f.v.rows["d"]).reshape(-1, 3)
        distinct = max(distinct, len({tuple(v) for v in d.tolist() if any(v)}))
    assert distinct >= 2 and st["aligned_changed"] < st["raw_changed"]


def test_solid_and_empty_blocks_report_ties(veng):
    """Solid after solid: every block's search region of B is solid, ties = (2s + 1)^3 and d = 0; empty after empty lists nothing."""
    grid = (12, 64, 10)
    cams3, frames3 = _start(veng, grid)
    f = Follower(veng, cams3, frames3)
    solid, none = np.ones((10, 12, 64), dtype=bool), np.zeros((10, 12, 64), dtype=bool)
    noisy = _sequence(grid, 4, 2, 1, 1)[0]
    for hull, listed in ((solid, None), (noisy, None), (none, None), (none, 0), (solid, None)):
        st, _, _ = f.step(hull, 3, 2, 1, (4, 0, 1))
        if listed is not None:
            assert st["listed"] == listed and st["cost_sum"] == 0
    # interior blocks of solid on solid (the grid's border blocks see the empty outside within the search range)
    f2 = Follower(veng, cams3, frames3)
    veng.temporal_reset()
    f2.step(solid, 2, 1, 1, (4, 0, 1))
    st, _, _ = f2.step(solid, 2, 1, 1, (4, 0, 1))
    rows = f2.v.rows
    inner = (rows["ijk"][:, 0] == 1) & (rows["ijk"][:, 2] == 1) & (rows["ijk"][:, 1] > 0) & (rows["ijk"][:, 1] < 15)
    assert inner.any() and (rows["ties"][inner] == 27).all() and not np.asarray(rows["d"]).any() and st["moved"] == 0


def test_a_figure_that_leaves_the_grid(veng):
    """A box that walks out through the x = 0 face: its blocks gather from sources outside the grid, which are empty."""
    grid = (9, 11, 7)
    cams3, frames3 = _start(veng, grid)
    f = Follower(veng, cams3, frames3)
    base = np.zeros((7, 9, 11), dtype=bool)
    base[1:6, 2:7, 2:9] = True
    clipped = 0
    for t in range(6):
        st, _, _ = f.step(mo.shifted(base, (-2 * t, 0, 0)), 3, 2, 2, (4, 2, 2))
        d = np.asarray(f.v.rows["d"]).reshape(-1, 3)
        clipped += int((d[:, 0] < 0).sum())
    assert clipped > 0 and st["survivors_before"] == 0           # (the figure has left; the field said so on the way)


def test_an_old_speck_in_an_unlisted_block_keeps_its_vote(veng):
    """Two on, one off, window 3, 4 / 0 / 1.  A speck away from the body, inside its block (no displacement of the range moves it
    out of the block's window, so its block gets d = 0), is in the hulls of frames 0 and 1.  At frame 3 neither H_3 nor H_2 has a
    voxel in that block: it is unlisted, the aligned snapshot of frame 1 and P keep the speck where it was (d = 0, not the
    emptying of vc_hull_warp), and with keep_off = 1 the voxel is still in the output."""
    grid = (12, 64, 10)
    cams3, frames3 = _start(veng, grid)
    f = Follower(veng, cams3, frames3)
    body = np.zeros((10, 12, 64), dtype=bool)
    body[2:8, 2:10, 4:20] = True
    speck = (5, 1, 61)                                           # (iz, ix, iy): block (bx, by, bz) = (0, 15, 1) of edge 4, far from the body
    kept = []
    for t in range(4):
        hull = mo.shifted(body, (0, t, 0))
        if t < 2:
            hull[speck] = True
        st, want, _ = f.step(hull, 3, 2, 1, (4, 0, 1))
        idx = (speck[0] * 12 + speck[1]) * 64 + speck[2]
        kept.append(bool(np.isin(idx, (want & LOW).astype(np.int64))))
        if t == 3:
            k = ((speck[0] // 4) * 3 + speck[1] // 4) * 16 + speck[2] // 4
            assert k not in f.v.rows["block"].tolist()           # unlisted: neither H_3 nor H_2 has a voxel there
    # frames 0, 1: in the hull; frame 2: two of three snapshots hold it; frame 3: one aligned snapshot does, and P (keep_off = 1)
    assert kept == [True, True, True, True]


@pytest.mark.parametrize("cc", [1, None])
def test_restored_voxels_with_and_without_a_colour_camera(veng, cc):
    grid = (37, 53, 29)
    cams3, frames3 = _start(veng, grid)
    restored = _restore(Follower(veng, cams3, frames3, cc=cc), grid)
    fresh = np.concatenate(restored)
    assert fresh.size > 0
    if cc is None:
        assert ((fresh >> np.uint64(32)) == 0).all()
    else:
        assert (((fresh >> np.uint64(32)) & np.uint64(0xffffff)) != 0).any() and ((fresh >> np.uint64(56)) == 1).any()


def _restore(f, grid):
    out = []
    for t, hull in enumerate(_sequence(grid, 21, 5, 2, 1)):
        _, want, added = f.step(hull, 3, 2, 2, (8, 4, 2))
        out.append(want[added == 1])
    return out


def test_state_rules(veng):
    from voxcarve._lib import VoxcarveError
    grid = (12, 64, 10)
    cams3, frames3 = _start(veng, grid)
    hulls = _sequence(grid, 31, 8, 1, 1)
    e = veng
    f = Follower(e, cams3, frames3)
    f.step(hulls[0], 3, 2, 2, (4, 0, 1))
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*vc_hull_temporal_motion.*one push per result"):
        e.temporal_filter(3, motion=(4, 0, 1))
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*one push per result"):
        e.temporal_filter(3)
    st, _, _ = f.step(hulls[1], 3, 2, 2, (4, 0, 1))
    assert st["frames"] == 2
    # a plain call after a compensated one restarts the ring, and the reverse
    e.carve(min_views=1)
    e.set_hull(hulls[2], reg=3)
    assert e.temporal_filter(3)["frames"] == 1
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no field"):
        e.fetch_temporal_motion()
    e.fetch_temporal()
    e.carve(min_views=1)
    e.set_hull(hulls[3], reg=3)
    assert e.temporal_filter(3)["frames"] == 2
    f = Follower(e, cams3, frames3)                              # (the restatement starts over with the device)
    st, _, _ = f.step(hulls[4], 3, 2, 2, (4, 0, 1))
    assert st["frames"] == 1 and st["listed"] == 0 and len(e.fetch_temporal_motion()["block"]) == 0
    st, _, _ = f.step(hulls[5], 3, 2, 2, (4, 0, 1))
    assert st["frames"] == 2 and st["listed"] > 0
    # temporal_reset and set_grid restart it; the votes go with the ring
    e.temporal_reset()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no votes"):
        e.fetch_temporal()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no field"):
        e.fetch_temporal_motion()
    f = Follower(e, cams3, frames3)
    assert f.step(hulls[6], 3, 2, 2, (4, 0, 1))[0]["frames"] == 1
    f.step(hulls[7], 3, 2, 2, (4, 0, 1))
    e.set_grid(*grid)                                            # the geometry: no reset call, the ring starts over by itself
    e.set_cameras(cams3, *e.image_size)
    e.upload_masks(fx.random_scene(3, C=3, fg=0.7)[1])
    e.upload_frame(1, frames3[1])
    e.carve(min_views=1)
    f = Follower(e, cams3, frames3)
    assert f.step(hulls[0], 3, 2, 2, (4, 0, 1))[0]["frames"] == 1
    # a carve invalidates the field with the votes
    e.carve(min_views=1)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no field"):
        e.fetch_temporal_motion()


def test_the_users_field_and_registers_are_untouched(veng):
    grid = (9, 11, 7)
    cams3, frames3 = _start(veng, grid)
    e = veng
    hulls = _sequence(grid, 41, 3, 1, 1)
    f = Follower(e, cams3, frames3)
    f.step(hulls[0], 3, 2, 2, (4, 0, 1))
    e.carve(min_views=1)
    for reg in range(3):
        e.upload_hull(hulls[reg] ^ hulls[(reg + 1) % 3], reg)
    e.set_hull(hulls[1], reg=3)
    e.hull_motion(0, 8, 4, 4)                                    # the user's own field, other parameters
    before = {key: np.asarray(e.fetch_motion()[key]).copy() for key in ROW_KEYS}
    kept = [e.fetch_kept(reg)["words"].copy() for reg in range(4)]
    rec = e.fetch_records().copy()
    occ = dn.volume((rec & LOW).astype(np.uint32), grid)
    out, c, ws = f.v.push(occ, 3, 2, 2, 4, 0, 1)
    st = e.temporal_filter(3, 2, 2, motion=(4, 0, 1))
    assert st["listed"] == ws["listed"] > 0
    for reg in range(4):
        assert np.array_equal(e.fetch_kept(reg)["words"], kept[reg])
    if st["added"] == st["removed"] == 0:                        # O_t = H_t: the generation stays, the user's field with it
        _same_rows(e.fetch_motion(), before)
    else:                                                        # another result: stale as after any pass, but not rewritten
        from voxcarve._lib import VoxcarveError
        with pytest.raises(VoxcarveError, match="no motion field"):
            e.fetch_motion()
    _same_rows(e.fetch_temporal_motion(), f.v.rows)


def test_a_call_that_changes_nothing_invalidates_nothing(veng):
    """The first push of a ring has O_t = H_t: the user's field, made on this result, and the distance field stay current."""
    grid = (9, 11, 7)
    cams3, frames3 = _start(veng, grid)
    e = veng
    hull = _sequence(grid, 41, 3, 1, 1)[0]
    e.upload_hull(_sequence(grid, 41, 3, 1, 1)[1], 0)
    e.set_hull(hull, reg=3)
    e.hull_motion(0, 8, 4, 4)
    before = {key: np.asarray(e.fetch_motion()[key]).copy() for key in ROW_KEYS}
    e.hull_distance()
    d = e.fetch_record_distance().copy()
    rec = e.fetch_records().copy()
    st = e.temporal_filter(3, 2, 2, motion=True)
    assert st["added"] == st["removed"] == 0 and st["frames"] == 1 and (st["block"], st["apron"], st["search"]) == (8, 4, 4)
    assert st["listed"] == st["moved"] == st["cost0_sum"] == st["aligned_changed"] == st["raw_changed"] == 0 and st["blocks"] == 2 * 2 * 1
    assert np.array_equal(e.fetch_records(), rec) and np.array_equal(e.fetch_record_distance(), d)
    _same_rows(e.fetch_motion(), before)
    votes, added = e.fetch_temporal()
    assert (votes == 1).all() and not added.any()


def test_refusals(built):
    import voxcarve
    from voxcarve import motion
    from voxcarve._lib import VoxcarveError
    grid = (9, 11, 7)
    with voxcarve.CarveEngine(0) as e:
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*vc_hull_temporal_motion: no carve result"):
            e.temporal_filter(motion=True)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no field"):
            e.fetch_temporal_motion()
        cams3, masks3, frames3 = fx.random_scene(3, C=3, fg=0.7)
        e.set_grid(*grid)
        e.set_cameras(cams3, *masks3[0].shape)
        e.upload_masks(masks3)
        S = e.carve(min_views=1)
        hull = e.fetch_records().copy()
        st = motion.TemporalMotionStats()
        call = e._L.vc_hull_temporal_motion
        err = lambda: e._L.vc_last_error(e._ctx).decode()
        ok = (5, 3, 3, 8, 4, 4, 0)
        for args, text in (((5, 3, 3, 8, 4, 4, 1), "flags must be 0"), ((0, 1, 1, 8, 4, 4, 0), "window 0"), ((16, 1, 1, 8, 4, 4, 0), "window 16"),
                           ((5, 0, 0, 8, 4, 4, 0), "keep_on 0"), ((5, 6, 1, 8, 4, 4, 0), "keep_on 6"), ((5, 3, 0, 8, 4, 4, 0), "keep_off 0"),
                           ((5, 3, 4, 8, 4, 4, 0), "keep_off 4"), ((5, 3, 3, 5, 0, 1, 0), "block edge 5"), ((5, 3, 3, 8, 17, 1, 0), "apron 17"),
                           ((5, 3, 3, 8, 4, 0, 0), "search range 0"), ((5, 3, 3, 8, 4, 9, 0), "search range 9"),
                           ((5, 3, 3, 16, 16, 9, 0), "search range 9")):
            assert call(e._ctx, *args, ctypes.byref(st)) == -1 and "vc_hull_temporal_motion" in err() and text in err(), (args, err())
        # (b + 2a + 2s > 64 cannot be reached inside the three ranges: 16 + 32 + 16 = 64, which is allowed, below)
        assert call(e._ctx, *ok, None) == -1 and "stats must not be NULL" in err()
        for bad in ((5,), (8, 4), (8, 17, 1), False):
            with pytest.raises(ValueError):
                e.temporal_filter(5, motion=bad)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*age 0"):        # nothing was pushed by any of them
            e.temporal_history(0)
        assert e.count == S and np.array_equal(e.fetch_records(), hull)
        e.touch_masks(0)
        e.fetch_mask(0)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*vc_hull_temporal_motion.*prepared again"):
            e.temporal_filter(motion=True)
        e.carve(min_views=1)
        assert e.temporal_filter(motion=(16, 16, 8))["frames"] == 1            # b + 2a + 2s = 64 itself is allowed
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*one push per result"):
            e.temporal_filter(motion=True)
        assert e._L.vc_fetch_temporal_motion(e._ctx, None, None) == 0          # either may be NULL
        e.carve(min_views=1, records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.temporal_filter(motion=True)
        e.set_slab(0, 3)
        e.carve(min_views=1)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.temporal_filter(motion=True)
        e.set_slab(0, grid[2])
        e.carve_begin(min_views=1)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
            e.temporal_filter(motion=True)
        e.carve_end()
        assert e.temporal_filter(motion=True)["frames"] == 1     # (set_slab started the ring over)


def test_configure_temporal_motion(built):
    """configure(temporal_window=3, temporal_motion=True): three frames of the masks rolled by 2 t columns against the restatement."""
    from voxcarve import assignment
    masks = fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    sets = [(frames, [np.roll(m, 2 * t, axis=1) for m in masks]) for t in range(3)]
    n = 64
    try:
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=os.path.join(fx.GOLDEN, "data"), temporal_window=3,
                             temporal_motion=True)
        with pytest.raises(RuntimeError):
            assignment.temporal()
        outs, stats = [], []
        for t in range(3):
            pos, _ = assignment.set_voxel_positions(n, n // 2, n)
            stats.append(dict(assignment.temporal()))
            outs.append(assignment._engine.fetch_records().copy())
            assert len(pos) == stats[-1]["survivors_after"] == outs[-1].size
        assert [s["frames"] for s in stats] == [1, 2, 3] and [s["listed"] > 0 for s in stats] == [False, True, True]
        # equal to carve + the restatement
        e = assignment._engine
        e.temporal_reset()
        v = tm.AlignedVote()
        for t in range(3):
            e.upload_masks(sets[t][1], slot=0)
            e.carve(slot=0, min_views=4, color_cam=assignment._settings["color_camera"])
            occ = dn.volume((e.fetch_records() & LOW).astype(np.uint32), e.grid)
            out, _, ws = v.push(occ, 3, 2, 2, 8, 4, 4)
            st = e.temporal_filter(3, motion=True)
            st.pop("temporal_ms")
            stats[t].pop("temporal_ms")
            assert st == stats[t] == ws
            assert np.array_equal(e.fetch_records(), outs[t]) and np.array_equal(_words(e), mo.words(out))
            _same_rows(e.fetch_temporal_motion(), v.rows)
    finally:
        assignment.configure(frame_source=None, temporal_window=0, temporal_motion=None)
