"""The vote over the last frames' hulls on the device (vc_hull_temporal, vc_fetch_temporal, vc_fetch_temporal_history,
vc_temporal_reset; csrc/vc_temporal.h) against the restatement (tests/temporal_np.py), bit for bit after every call of a sequence:
indices, order, all 8 bytes of every record, the vote and `added` bytes, the occupancy words, every snapshot of the ring and every
stat.  Random scenes whose hulls change from frame to frame on grids of 2, 11, 889 and 120 words, windows 1, 2, 5 and 15 with
plain votes and hysteresis, thresholds changed mid-sequence, an empty hull and a solid grid inside a sequence, restored voxels
inside and outside the colour camera's image, no colour camera; closings, dilations and erosions between the votes of one
sequence (the record merge both adding passes share); the real cameras at 64^3 with seeded mask noise in both carve
modes; the state rules; the readers of the voted hull; a call that changes nothing; every refusal; the launch counts;
configure(temporal_window=...); 512^3 on invariants."""
import ctypes
import os

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import temporal_np as tn

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)


@pytest.fixture(scope="module")
def teng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _words(e):
    raw = np.empty((e.n_voxels + 63) // 64, dtype=np.uint64)
    e._check(e._L.vc_fetch_occupancy(e._ctx, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "vc_fetch_occupancy")
    return raw


def _want_words(occ):
    return np.packbits(np.asarray(occ, dtype=bool).reshape(-1), bitorder="little").tobytes().ljust((occ.size + 63) // 64 * 8, b"\0")


def _same_words(words, occ):
    return words.tobytes() == _want_words(occ)


class Follower:
    """The restatement beside an engine: every step votes on both and compares everything the device exposes."""

    def __init__(self, e, cams, frames=None, cc=1):
        self.e, self.v = e, tn.Vote()
        self.cam = None if cc is None else fx.oracle_cams(cams)[cc]
        self.frame = None if frames is None or cc is None else frames[cc]

    def step(self, window=5, on=None, off=None):
        e = self.e
        rec = e.fetch_records().copy()
        occ = dn.volume((rec & LOW).astype(np.uint32), e.grid)
        window_, on_, off_ = e.temporal_thresholds(window, on, off)
        out, c, ws = self.v.push(occ, window_, on_, off_)
        H, W = e.image_size
        want, wvotes, wadded = tn.records_after(rec, occ, out, c, e.grid, e.bounds, self.cam, self.frame, H, W)
        st = e.temporal_filter(window, on, off)
        ms = st.pop("temporal_ms")
        assert st == ws, (st, ws)
        assert ms > 0 and e.count == want.size
        got = e.fetch_records()
        assert np.array_equal(got & LOW, want & LOW), "indices and order"
        assert np.array_equal(got, want), "records"
        votes, added = e.fetch_temporal()
        assert np.array_equal(votes, wvotes), "vote bytes"
        assert np.array_equal(added, wadded), "added bytes"
        assert _same_words(_words(e), out), "occupancy words"
        for age in range(ws["frames"]):
            assert _same_words(e.temporal_history(age), self.v.history(age)), "history %d" % age
        return st, want, wadded


def _scene_masks(seed, t, fg, C=3):
    """Frame t of a sequence: the scene's own masks with a fifth of the pixels drawn again, so consecutive hulls overlap."""
    _, base, _ = fx.random_scene(seed, C=C, fg=fg)
    rng = np.random.default_rng(100 * seed + t)
    return [np.where(rng.random(m.shape) < 0.2, np.where(rng.random(m.shape) < fg, 255, 0), m).astype(np.uint8) for m in base]


def _start(e, grid, cams, masks, frames=None, bounds=None, cc=1):
    H, W = masks[0].shape
    if bounds is None:
        e.set_grid(*grid)
    else:
        e.set_grid(*grid, bounds=bounds)
    e.set_cameras(cams, H, W)
    e.upload_masks(masks)
    if frames is not None and cc is not None:
        e.upload_frame(cc, frames[cc])


@pytest.mark.parametrize("grid,seed,mv,window,pairs", [
    ((5, 7, 3), 3, 1, 1, [(1, 1)]), ((5, 7, 3), 4, 2, 2, [(2, 1), (1, 1)]), ((5, 7, 3), 5, 1, 5, [(3, 3), (5, 1)]),
    ((9, 11, 7), 6, 1, 5, [(None, None), (4, 2)]), ((9, 11, 7), 7, 2, 15, [(15, 1), (8, 8)]), ((9, 11, 7), 8, 1, 2, [(2, 2), (1, 1)]),
    ((37, 53, 29), 3, 1, 5, [(3, 3), (4, 2)]), ((37, 53, 29), 4, 2, 15, [(8, 4)]), ((37, 53, 29), 9, 2, 2, [(2, 1)]),
    ((12, 64, 10), 7, 2, 5, [(5, 1), (3, 2)]), ((12, 64, 10), 5, 1, 1, [(1, 1)])])
def test_random_sequences_equal_restatement(teng, grid, seed, mv, window, pairs):
    """2 window + 2 frames, so the ring wraps; the thresholds change half way; an empty hull and a solid grid inside the sequence;
    restored voxels carry real colours, and some lie outside the colour camera's image (seen = 0)."""
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    H, W = masks3[0].shape
    _start(teng, grid, cams3, masks3, frames3)
    teng.temporal_reset()
    f = Follower(teng, cams3, frames3)
    n_frames = 2 * window + 2
    restored = coloured = unseen = dropped = 0
    for t in range(n_frames):
        if window > 1 and t == window // 2 + 1:
            masks = [np.zeros((H, W), np.uint8)] * 3                                # an empty hull
        elif window > 1 and t == window + 2:
            masks = [np.full((H, W), 255, np.uint8)] * 3                            # every voxel some camera sees
        else:
            masks = _scene_masks(seed, t, 0.7)
        teng.upload_masks(masks)
        S = teng.carve(min_views=mv)
        if t == window // 2 + 1 and window > 1:
            assert S == 0
        on, off = pairs[(t * len(pairs)) // n_frames]
        st, want, added = f.step(window, on, off)
        fresh = want[added == 1]
        restored += fresh.size
        coloured += int((((fresh >> np.uint64(32)) & np.uint64(0xffffff)) != 0).sum())
        unseen += int(((fresh >> np.uint64(56)) == 0).sum())
        dropped += st["removed"]
    if window > 1:
        assert restored > 0 and coloured > 0 and dropped > 0
        if grid == (37, 53, 29):
            assert unseen > 0
    else:
        assert restored == dropped == 0                              # window 1 is the identity


@pytest.mark.parametrize("grid,seed,mv,window,mm", [((9, 130, 12), 6, 1, 3, 250), ((37, 53, 29), 4, 2, 5, 100), ((12, 64, 10), 7, 2, 2, 250)])
def test_votes_on_grown_hulls(teng, grid, seed, mv, window, mm):
    """The two passes that add voxels in one sequence, through the record merge they share: a closing before the vote on odd frames
    (the vote moves records a closing made, `added` colours included), a dilation straight after the vote on every third (a merge
    after a merge) and an erosion after both (a compaction of merged records).  Lines that straddle occupancy words with a partial
    last word; several 64-word groups with n % 64 != 0; lines of exactly one word in two groups."""
    from test_gpu_closing import _check_grow
    from test_gpu_distance import _check_morph
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    _start(teng, grid, cams3, masks3, frames3)
    teng.temporal_reset()
    f = Follower(teng, cams3, frames3)
    closed = voted_in = voted_out = kept = dropped = first_of_word = 0
    for t in range(2 * window + 2):
        teng.upload_masks(_scene_masks(seed, t, 0.7))
        teng.carve(min_views=mv)
        grown = np.empty(0, np.uint64)
        if t % 2 == 1:
            st, want, added = _check_grow(teng, "close", cams3, frames3, mm=mm)
            closed += st["added"]
            grown = want[added == 1] & LOW
        before = teng.fetch_records() & LOW
        st, want, added = f.step(window, (window + 2) // 2, 1)
        voted_in += st["added"]
        voted_out += st["removed"]
        stays = np.isin(grown, want & LOW)
        kept += int(stays.sum())
        dropped += int((~stays).sum())
        first_of_word += int((~np.isin((want[added == 1] & LOW) >> np.uint64(6), before >> np.uint64(6))).sum())
        if t % 3 == 2:
            _check_grow(teng, "dilate", cams3, frames3, mm=mm)
            _check_morph(teng, "erode", mm)
    print("closings added %d, votes added %d and removed %d, grown voxels kept %d and dropped %d, restored as the first of a word %d"
          % (closed, voted_in, voted_out, kept, dropped, first_of_word))
    assert closed > 0 and voted_in > 0 and voted_out > 0 and kept > 0 and dropped > 0
    if grid != (12, 64, 10):
        assert first_of_word > 0


def test_solid_grid_in_a_sequence(teng, cams, masks, frames):
    """A grid every camera sees whole, so a solid hull exists: solid, noisy, empty and solid again through a window of 3."""
    H, W = masks[0].shape
    full = [np.full((H, W), 255, np.uint8)] * 4
    grid, bounds = (10, 16, 6), (60.0, 660.0, -253.0, 347.0, -901.0, -301.0)
    _start(teng, grid, cams, full, frames, bounds=bounds)
    teng.temporal_reset()
    f = Follower(teng, cams, frames)
    rng = np.random.default_rng(5)
    for t, kind in enumerate(("solid", "noisy", "empty", "solid", "noisy", "solid", "solid", "solid")):
        if kind == "solid":
            ms = full
        elif kind == "empty":
            ms = [np.zeros((H, W), np.uint8)] * 4
        else:
            ms = [np.where(rng.random((H, W)) < 0.3, 0, 255).astype(np.uint8) for _ in range(4)]
        teng.upload_masks(ms)
        S = teng.carve()
        assert kind != "solid" or S == 10 * 16 * 6
        st, _, _ = f.step(3, 2, 1)
    assert st["survivors_after"] == 10 * 16 * 6 and st["added"] == st["removed"] == st["out_changed"] == 0


def test_no_colour_camera_and_no_image(built):
    import voxcarve
    cams3, masks3, frames3 = fx.random_scene(11, C=3, fg=0.7)
    with voxcarve.CarveEngine(0) as e:
        _start(e, (9, 11, 7), cams3, masks3)                     # no image uploaded
        for cc, frames in ((None, None), (2, None)):
            e.temporal_reset()
            f = Follower(e, cams3, frames, cc=cc)
            restored = 0
            for t in range(6):
                e.upload_masks(_scene_masks(11, t, 0.7))
                e.carve(min_views=1, color_cam=cc)
                st, want, added = f.step(3, 2, 2)
                fresh = want[added == 1]
                restored += fresh.size
                if cc is None:
                    assert ((fresh >> np.uint64(32)) == 0).all()
                else:
                    assert (((fresh >> np.uint64(32)) & np.uint64(0xffffff)) == 0).all()      # seen, colour 0
            assert restored > 0


@pytest.mark.parametrize("mode", ["fused", "lut"])
def test_real_cameras_64_with_mask_noise(teng, cams, masks, frames, mode):
    """The recipe of DESIGN section 8 item 17 on the device: 12 frames through a 3-of-5 vote, then hysteresis 4 on / 2 off."""
    n = 64
    _start(teng, (n, n, n), cams, masks, frames)
    if mode == "lut":
        teng.build_lut()
    teng.temporal_reset()
    f = Follower(teng, cams, frames)
    raw = voted = 0
    for t in range(12):
        teng.upload_masks(tn.noisy_masks(masks, t))
        teng.carve(mode=mode)
        st, want, added = f.step(5, 3, 3) if t < 9 else f.step(5, 4, 2)
        assert ((want[added == 1] >> np.uint64(56)) == 1).all()   # the real cameras see the whole volume
        if 5 <= t < 9:
            raw += st["raw_changed"]
            voted += st["out_changed"]
    print("64^3, frames 5..8: %d voxels change between raw hulls, %d between voted hulls" % (raw, voted))
    assert 10 * voted <= raw


def test_state_rules(teng):
    """A window change, set_grid, set_cameras and temporal_reset start the ring over; a refused or a second call on the same result
    leaves ring and P alone, so the next call equals the restatement that never saw it."""
    from voxcarve._lib import VoxcarveError
    grid, seed = (9, 11, 7), 6
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    _start(teng, grid, cams3, masks3, frames3)
    teng.temporal_reset()
    f = Follower(teng, cams3, frames3)

    def frame(t):
        teng.upload_masks(_scene_masks(seed, t, 0.7))
        teng.carve(min_views=1)

    for t in range(4):
        frame(t)
        f.step(5, 3, 3)
    # a second call on the same result, and refused calls: nothing is pushed
    for call in (lambda: teng.temporal_filter(5, 3, 3), lambda: teng.temporal_filter(5, 1, 1)):
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*one push per result"):
            call()
    frame(4)
    st = _tstats()
    assert teng._L.vc_hull_temporal(teng._ctx, 5, 6, 1, 0, ctypes.byref(st)) == -1
    assert teng._L.vc_hull_temporal(teng._ctx, 16, 3, 3, 0, ctypes.byref(st)) == -1
    assert teng._L.vc_hull_temporal(teng._ctx, 5, 3, 3, 1, ctypes.byref(st)) == -1
    st5, _, _ = f.step(5, 3, 3)
    assert st5["frames"] == 5
    # another window starts over (and back again: the old ring is gone)
    frame(5)
    st, _, _ = f.step(3, 2, 2)
    assert st["frames"] == 1 and st["added"] == st["removed"] == 0
    frame(6)
    assert f.step(5, 3, 3)[0]["frames"] == 1
    frame(7)
    assert f.step(5, 3, 3)[0]["frames"] == 2
    # temporal_reset
    teng.temporal_reset()
    f.v.reset()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no votes"):
        teng.fetch_temporal()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*age 0"):
        teng.temporal_history(0)
    frame(8)
    assert f.step(5, 3, 3)[0]["frames"] == 1
    frame(9)
    assert f.step(5, 3, 3)[0]["frames"] == 2
    # set_cameras and set_grid (to the same values) start over too
    H, W = masks3[0].shape
    for change in (lambda: teng.set_cameras(cams3, H, W), lambda: teng.set_grid(*grid)):
        change()
        f.v.reset()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*age 0"):
            teng.temporal_history(0)
        teng.upload_masks(masks3)
        teng.upload_frame(1, frames3[1])
        frame(10)
        assert f.step(5, 3, 3)[0]["frames"] == 1
        frame(11)
        assert f.step(5, 3, 3)[0]["frames"] == 2
    # a pass that changes the result between two votes: its output is what the next call pushes
    frame(12)
    f.step(5, 3, 3)
    before = teng.count
    if teng.filter_components(keep_largest=1)["survivors_after"] < before:
        f.step(5, 3, 3)


def _tstats():
    from voxcarve import _lib
    return _lib.VcTemporalStats()


def _noisy_sequence(e, masks, frames_n, mode="fused", window=5):
    """frames_n noisy frames through the vote; leaves the last voted hull as the current result."""
    for t in range(frames_n):
        e.upload_masks(tn.noisy_masks(masks, t))
        e.carve(mode=mode)
        st = e.temporal_filter(window)
    return st


def test_readers_see_the_voted_hull(teng, cams, masks, frames):
    """Every reader of the step after a vote that restored and dropped voxels, each against its own restatement fed with the voted
    hull: fetch*, filter_components, close / open, color_visible, render, marching_cubes(volume=None), pack / expand_entries."""
    import visible_np as vn
    from test_gpu_closing import _check_grow
    from test_gpu_components import _check as check_components
    from test_gpu_distance import _check_morph
    from test_gpu_render import _check as check_render
    n = 64
    H, W = masks[0].shape
    _start(teng, (n, n, n), cams, masks, frames)
    for c in range(4):
        teng.upload_frame(c, frames[c])
    teng.temporal_reset()

    def voted():
        teng.temporal_reset()
        st = _noisy_sequence(teng, masks, 6)
        assert st["added"] > 0 and st["removed"] > 0 and st["frames"] == 5
        return teng.fetch_records().copy()

    rec = voted()
    idx, rgb, seen = teng.fetch()
    assert np.array_equal(idx, (rec & LOW).astype(np.uint32)) and seen.all() and idx.size == teng.count
    occ = teng.fetch_occupancy()
    assert np.array_equal(np.flatnonzero(occ), idx)
    v, fc = teng.marching_cubes(volume=None)
    v2, f2 = teng.marching_cubes(volume=occ.reshape(n, n, n))
    assert np.array_equal(v, v2) and np.array_equal(fc, f2) and fc.size > 0
    check_render(teng, cams[:2], H, W)
    ent = teng.pack_entries()
    assert int(np.bitwise_count(ent[:, 0]).sum()) == rec.size
    assert teng.expand_entries(ent) == rec.size
    assert np.array_equal(teng.fetch_gathered() & LOW, rec & LOW)
    check_components(teng, 26, 0, 0)
    voted()
    _check_grow(teng, "close", cams, frames, mm=40)
    voted()
    _check_morph(teng, "open", 25)
    rec0 = voted()
    teng.color_visible()
    i0 = (rec0 & LOW).astype(np.uint32)
    rgb0 = np.stack([(rec0 >> np.uint64(k)) & np.uint64(0xff) for k in (32, 40, 48)], axis=1).astype(np.uint8)
    _, vis, rgb1 = vn.color_visible(i0, rgb0, teng.grid, teng.bounds, fx.oracle_cams(cams), frames, H, W, None)
    wrec = (rec0 & np.uint64(0xff000000ffffffff)) | (rgb1[:, 0].astype(np.uint64) << np.uint64(32)) | \
        (rgb1[:, 1].astype(np.uint64) << np.uint64(40)) | (rgb1[:, 2].astype(np.uint64) << np.uint64(48))
    assert np.array_equal(teng.fetch_visibility(), vis) and np.array_equal(teng.fetch_records(), wrec)
    teng.fetch_temporal()                                        # (a recolouring leaves the set of survivors alone)
    # what a vote that changes the hull invalidates
    teng.temporal_reset()
    _noisy_sequence(teng, masks, 5)
    teng.upload_masks(tn.noisy_masks(masks, 5))
    teng.carve()
    teng.filter_components(min_voxels=1)
    teng.hull_distance()
    teng.color_visible()
    assert teng.temporal_filter(5)["added"] > 0
    from voxcarve._lib import VoxcarveError
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no component labels"):
        teng.fetch_component_labels()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no distance field"):
        teng.fetch_record_distance()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG"):
        teng.fetch_visibility()
    teng.carve()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no votes"):
        teng.fetch_temporal()


def test_a_call_that_changes_nothing_keeps_what_the_result_carries(teng, cams, masks, frames):
    """O_t = H_t (the first call after a reset; a constant sequence): records, occupancy, visibility, component labels and the
    distance field stay valid, the vote bytes are the call's own, and no merge is launched."""
    n = 64
    _start(teng, (n, n, n), cams, masks, frames)
    for c in range(4):
        teng.upload_frame(c, frames[c])
    teng.temporal_reset()
    teng.set_option("timing_detail", 1)
    try:
        for t in range(3):
            teng.carve()
            teng.filter_components(min_voxels=1)
            teng.color_visible()
            teng.hull_distance()
            vis, lab, rec = teng.fetch_visibility().copy(), teng.fetch_component_labels().copy(), teng.fetch_records().copy()
            d = teng.fetch_record_distance().copy()
            teng.timing(reset=True)
            st = teng.temporal_filter(5, 4, 2)
            k = teng.timing()["kernels"]
            assert st["added"] == st["removed"] == 0 and st["frames"] == t + 1 and st["raw_changed"] == 0
            assert st["out_changed"] == (rec.size if t == 0 else 0)
            assert k["k_temporal_vote"]["launches"] == 1 and k["temporal_rank"]["launches"] == 3 and "temporal_merge" not in k
            assert np.array_equal(teng.fetch_visibility(), vis) and np.array_equal(teng.fetch_component_labels(), lab)
            assert np.array_equal(teng.fetch_records(), rec) and np.array_equal(teng.fetch_record_distance(), d)
            votes, added = teng.fetch_temporal()
            assert not added.any() and (votes == t + 1).all()
    finally:
        teng.set_option("timing_detail", 0)


def test_timing_reports_the_kernels(built, cams, masks, frames):
    import voxcarve
    with voxcarve.CarveEngine(0) as e:
        _start(e, (64, 64, 64), cams, masks, frames)
        e.set_option("timing_detail", 1)
        _noisy_sequence(e, masks, 5)
        e.upload_masks(tn.noisy_masks(masks, 5))
        e.carve()
        e.timing(reset=True)
        st = e.temporal_filter(5)
        k = e.timing()["kernels"]
        assert st["added"] > 0 and st["removed"] > 0
        # rank: k_count_groups, k_cc_wcount, k_cc_woff; merge: k_merge_old, k_temporal_new
        assert k["k_temporal_vote"]["launches"] == 1 and k["temporal_rank"]["launches"] == 3 and k["temporal_merge"]["launches"] == 2
        assert all(k[name]["ms_sum"] > 0 for name in ("k_temporal_vote", "temporal_rank", "temporal_merge"))
        assert "k_grow_mark" not in k and "grow_merge" not in k


def test_refusals(built, cams, masks, frames):
    """Every refusal of the contract's items 8, 9 and 11 but one: a communicator of more than one rank needs two processes with a
    device each, and the message comes from the check every post-carve pass shares."""
    import voxcarve
    from voxcarve._lib import VoxcarveError
    H, W = masks[0].shape
    with voxcarve.CarveEngine(0) as e:
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.temporal_filter()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no votes"):
            e.fetch_temporal()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*age 0"):
            e.temporal_history(0)
        e.temporal_reset()
        _start(e, (64, 64, 64), cams, masks, frames)
        S = e.carve()
        hull = e.fetch_records().copy()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no votes"):
            e.fetch_temporal()
        st = _tstats()
        call = e._L.vc_hull_temporal
        err = lambda: e._L.vc_last_error(e._ctx).decode()
        assert call(e._ctx, 5, 3, 3, 1, ctypes.byref(st)) == -1 and "flags" in err()
        assert call(e._ctx, 5, 3, 3, 0, None) == -1 and "stats" in err()
        for window in (0, 16):
            assert call(e._ctx, window, 1, 1, 0, ctypes.byref(st)) == -1 and "window" in err()
        for on, off in ((0, 0), (6, 1), (0, 1)):
            assert call(e._ctx, 5, on, off, 0, ctypes.byref(st)) == -1 and "keep_on" in err()
        for on, off in ((3, 0), (3, 4)):
            assert call(e._ctx, 5, on, off, 0, ctypes.byref(st)) == -1 and "keep_off" in err()
        assert e._L.vc_fetch_temporal_history(e._ctx, 0, None) == -1
        for bad in ((0,), (16,), (5, 6), (5, 3, 4), (2.5,)):
            with pytest.raises(ValueError):
                e.temporal_filter(*bad)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*age 0"):        # nothing was pushed by any of them
            e.temporal_history(0)
        assert e.count == S and np.array_equal(e.fetch_records(), hull)
        # a slot prepared again since the carve: its images are not the ones the colours came from
        e.touch_masks(0)
        e.fetch_mask(0)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*prepared again"):
            e.temporal_filter()
        e.carve()
        assert e.temporal_filter()["frames"] == 1
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*one push per result"):
            e.temporal_filter()
        e.fetch_temporal()
        e._check(e._L.vc_fetch_temporal(e._ctx, None, None), "vc_fetch_temporal")      # either may be NULL
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*age 1"):
            e.temporal_history(1)
        assert _same_words(e.temporal_history(0), dn.volume((hull & LOW).astype(np.uint32), e.grid))
        e.carve(records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.temporal_filter()
        e.set_slab(0, 32)
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.temporal_filter()
        e.set_slab(0, 64)
        e.carve_begin()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
            e.temporal_filter()
        e.carve_end()
        assert e.temporal_filter()["frames"] == 1                # (set_slab started the ring over)


def test_configure_temporal_window(built, cams, masks):
    from voxcarve import assignment
    frames = [np.dstack([m // 2 + 60, m // 3 + 40, 255 - m // 2]).astype(np.uint8) for m in masks]
    data = os.path.join(fx.GOLDEN, "data")
    sets = [(frames, tn.noisy_masks(masks, t)) for t in range(7)]
    try:
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=data, temporal_window=5)
        with pytest.raises(RuntimeError):
            assignment.temporal()
        outs, stats = [], []
        for t in range(7):
            pos, col = assignment.set_voxel_positions(64, 32, 64)
            stats.append(dict(assignment.temporal()))
            outs.append(assignment._engine.fetch_records().copy())
            assert len(pos) == stats[-1]["survivors_after"] == outs[-1].size
            assert np.array_equal(assignment.voxels_status().reshape(-1), assignment._engine.fetch_occupancy().reshape(-1))
        assert [s["frames"] for s in stats] == [1, 2, 3, 4, 5, 5, 5] and stats[6]["on"] == stats[6]["off"] == 3
        # equal to carve + temporal_filter by hand
        e = assignment._engine
        e.temporal_reset()
        for t in range(7):
            e.upload_masks(sets[t][1], slot=0)
            e.carve(slot=0, min_views=4, color_cam=assignment._settings["color_camera"])
            st = e.temporal_filter(5)
            st.pop("temporal_ms")
            stats[t].pop("temporal_ms")
            assert st == stats[t] and np.array_equal(e.fetch_records(), outs[t])
        # with hysteresis, then a closing: the closing sees the voted hull
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=data, temporal_window=5, temporal_keep=4,
                             temporal_keep_off=2, hull_close_mm=40)
        for t in range(6):
            pos, _ = assignment.set_voxel_positions(64, 32, 64)
        ts = assignment.temporal()
        assert (ts["on"], ts["off"]) == (4, 2) and len(pos) >= ts["survivors_after"]
    finally:
        assignment.configure(frame_source=None, temporal_window=0, temporal_keep=None, temporal_keep_off=None, hull_close_mm=0.0)


def test_real_512_invariants(teng, cams, masks, frames):
    """At 512^3 the restatement of whole sequences is too slow for the suite; the counts against popcounts of the fetched words and
    histories, the order, and the old records byte for byte."""
    n = 512
    _start(teng, (n, n, n), cams, masks, frames)
    teng.temporal_reset()
    hulls = []
    for t in range(3):
        teng.upload_masks(tn.noisy_masks(masks, t))
        teng.carve()
        rec = teng.fetch_records().copy()
        raw = _words(teng)
        st = teng.temporal_filter(3, 2, 2)
        hulls.append(raw)
        out = _words(teng)
        got = teng.fetch_records()
        votes, added = teng.fetch_temporal()
        for age in range(st["frames"]):
            assert np.array_equal(teng.temporal_history(age), hulls[t - age])
        pop = lambda w: int(np.bitwise_count(w).sum())
        assert st["frames"] == t + 1 and st["survivors_before"] == rec.size == pop(raw)
        assert st["survivors_after"] == got.size == pop(out) == teng.count
        assert st["added"] == pop(out & ~raw) == int(added.sum()) and st["removed"] == pop(raw & ~out)
        assert st["raw_changed"] == (pop(raw ^ hulls[t - 1]) if t else 0)
        idx = (got & LOW).astype(np.int64)
        assert (np.diff(idx) > 0).all()
        assert np.array_equal(np.flatnonzero(np.unpackbits(out.view(np.uint8), bitorder="little")[:n ** 3]), idx)
        kept = rec[((out[(rec & LOW).astype(np.int64) >> 6] >> ((rec & LOW) & np.uint64(63))) & np.uint64(1)).astype(bool)]
        assert np.array_equal(got[added == 0], kept)              # old records byte for byte
        count = sum(((h[idx >> 6] >> (idx.astype(np.uint64) & np.uint64(63))) & np.uint64(1)).astype(np.uint8) for h in hulls[-st["frames"]:])
        assert np.array_equal(votes, count) and (votes >= st["on"]).all()
    assert st["added"] > 0 and st["removed"] > 0
