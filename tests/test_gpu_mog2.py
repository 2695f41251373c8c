"""The MOG2 background model on the device (k_mog2_apply through vc_mog2_*, vc_foreground_front, vc_foreground_to_slot) against the
restatement of OpenCV's bgfg_gaussmix2.cpp (tests/mog2_np.py): mask, every state bit and nmodes after every frame, the drop-in
trainer with extract_foreground_mask, MOG and MOG2 cameras mixed in one carve slot, and set_voxel_positions with
DeviceVideoSource(model="MOG2").  Parity with cv2 itself: unpinned."""
import os

import numpy as np
import pytest

import contour_literal as lit
import fixtures_util as fx
import mog2_np

pytestmark = pytest.mark.gpu

PARAMS = [[5000, 115, False, False, True, True], [5000, 115, False, False, True, True],
          [5000, 175, False, True, True, True], [5000, 115, False, False, False, True]]   # assignment.py:28-33
RATES = [-1] * 12 + [0.05] * 4 + [0, 0] + [1.0] + [-1] * 3 + [0, 0.3]                       # test_mog_background_model_on_device's


@pytest.fixture(scope="module")
def m2eng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _frames(rng, shape, n):
    """Flat and textured background, sensor noise, a second mode that comes and goes, a darkened band every third frame, a moving
    inverted square in the second half."""
    H, W = shape
    bg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    bg[: H // 2] = (bg[: H // 2] // 8) + 130
    alt = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    out = []
    for t in range(n):
        f = (alt if t % 5 == 4 else bg).astype(np.int64) + rng.integers(-6, 7, (H, W, 3))
        if t % 3 == 2:
            f[: max(H // 3, 1)] = (f[: max(H // 3, 1)] * 7) // 10
        if t >= n // 2 and H > 8 and W > 8:
            y, x = (3 * t) % (H - 6), (5 * t) % (W - 6)
            f[y:y + 6, x:x + 6] = 255 - f[y:y + 6, x:x + 6]
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


def _same_state(dev, ref, where):
    state, nmodes, hw, nf = dev.state()
    assert hw == ref.shape and nf == ref.nframes, where
    assert np.array_equal(nmodes, ref.nmodes), where
    assert np.array_equal(state.view(np.uint32), ref.state.view(np.uint32)), where


def test_mog2_background_model_on_device(m2eng):
    from voxcarve import background_subtraction as bs
    rng = np.random.default_rng(505)
    cases = (((486, 644), {}, RATES),
             ((9, 13), dict(history=24, varThreshold=650, detectShadows=False), RATES),
             ((1, 1), dict(nmixtures=1, shadowThreshold=0.7, shadowValue=60), RATES),
             ((64, 50), dict(nmixtures=8, shadowThreshold=0.35, shadowValue=200, varThreshold=25), RATES),
             ((1080, 1920), {}, [-1] * 5 + [0, 0.05, 0]))
    for shape, kw, rates in cases:
        dev = bs.BackgroundSubtractorMOG2(engine=m2eng, **kw)
        ref = mog2_np.MOG2(**kw)
        frames = _frames(rng, shape, len(rates))
        seen = set()
        for t, (f, lr) in enumerate(zip(frames, rates)):
            got, want = dev.apply(f, None, lr), ref.apply(f, lr)
            seen |= set(np.unique(want).tolist())
            assert got.dtype == np.uint8 and np.array_equal(got, want), (shape, t, lr, int((got != want).sum()))
            _same_state(dev, ref, (shape, t, lr))
        if shape[0] > 1:
            assert {0, 255} <= seen, (shape, seen)
            if kw.get("detectShadows", True):
                assert kw.get("shadowValue", 127) in seen, (shape, seen)
        # a new image size starts the model over, as apply() does
        f2 = rng.integers(0, 256, (shape[0] + 1, shape[1], 3), dtype=np.uint8)
        assert np.array_equal(dev.apply(f2, None, 0), ref.apply(f2, 0)) and dev.state()[3] == 1
        _same_state(dev, ref, (shape, "resized"))
        dev.close()


def test_mog2_errors_leave_the_engine_usable(m2eng):
    from voxcarve import background_subtraction as bs
    from voxcarve._lib import VoxcarveError
    rng = np.random.default_rng(9)
    frames = _frames(rng, (20, 30), 6)
    mog = bs.BackgroundSubtractorMOG(engine=m2eng)
    dev = bs.BackgroundSubtractorMOG2(engine=m2eng)
    ref = mog2_np.MOG2()

    def still_usable(t):
        assert np.array_equal(dev.apply(frames[t], None, -1), ref.apply(frames[t], -1))
        _same_state(dev, ref, t)

    still_usable(0)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG"):
        bs.BackgroundSubtractorMOG2(nmixtures=9, engine=m2eng)
    still_usable(1)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no background model"):
        m2eng.mog_apply(dev._model, frames[2], -1)
    still_usable(2)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no MOG2 background model"):
        m2eng.mog2_apply(mog._model, frames[3], -1)
    still_usable(3)
    gone = bs.BackgroundSubtractorMOG2(engine=m2eng)
    handle = gone._model
    gone.close()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no MOG2 background model"):
        m2eng.mog2_apply(handle, frames[4], -1)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG"):
        m2eng.mog2_state(handle)
    still_usable(4)
    mog.close()
    dev.close()


def _scene(rng, H, W, n_bg, n_fg, shift=0):
    """Grey textured background (so that a darkened copy reads as a shadow in HSV too), frames with a large figure with a hole
    and a shadow band beside it."""
    yy, xx = np.mgrid[0:H, 0:W]
    grey = (60 + ((xx * 3 + yy * 2) % 150)).astype(np.int64)
    bg = np.stack([grey, grey, grey], -1)
    noisy = lambda img: np.clip(img + rng.integers(-3, 4, (H, W, 1)), 0, 255).astype(np.uint8)
    bgs = [noisy(bg) for _ in range(n_bg)]
    fgs = []
    for t in range(n_fg):
        cy, cx = H // 2 + (t * 5 + shift) % (H // 8), W // 3 + (t * 9 + shift) % (W // 4)
        body = ((yy - cy) / (H * 0.3)) ** 2 + ((xx - cx) / (W * 0.12)) ** 2 < 1
        hole = ((yy - cy) / (H * 0.08)) ** 2 + ((xx - cx) / (W * 0.04)) ** 2 < 1
        shade = (xx > cx + W * 0.14) & (xx < cx + W * 0.3) & (np.abs(yy - cy) < H * 0.25)
        f = bg.copy()
        f[shade] = (f[shade] * 7) // 10
        fig = body & ~hole
        f[fig] = np.stack([255 - grey[fig], grey[fig] // 3, 200 + 0 * grey[fig]], -1)
        fgs.append(noisy(f))
    return bgs, fgs


def _trained(bgs_per_cam, eng, kinds, shadows=True):
    """Per camera a device model and its restatement, trained on the camera's background frames (HSV)."""
    from oracle import foreground_np as fg, mog_np
    from voxcarve import background_subtraction as bs
    dev, ref = [], []
    for bgs, kind in zip(bgs_per_cam, kinds):
        if kind == "MOG2":
            dev.append(bs.train_MOG2_background_model(history=len(bgs), var_threshold=650 if not shadows else 16,
                                                      detect_shadows=shadows, engine=eng, frames=bgs))
            r = mog2_np.MOG2(history=len(bgs), varThreshold=650 if not shadows else 16, detectShadows=shadows)
        else:
            dev.append(bs.train_MOG_background_model(history=len(bgs), n_mixtures=50, bg_ratio=0.90, noise_sigma=0, engine=eng, frames=bgs))
            r = mog_np.MOG(history=len(bgs), nmixtures=50, backgroundRatio=0.90, noiseSigma=0)
        for f in bgs:
            r.apply(fg.bgr_to_hsv(f), -1)
        ref.append(r)
    return dev, ref


def _restated(fs, params, refs):
    """extract_foreground_mask of one frame set, restated, up to the contour stage's output (no post-filter); the models learn as
    the device's do (learning rate 0: MOG2 still writes)."""
    from oracle import foreground_np as fg
    pre = [fg.pre_filter(refs[c].apply(fg.bgr_to_hsv(f), 0), params[c][2], params[c][3]) for c, f in enumerate(fs)]
    return pre, [lit.fill_figures(m, params[c][0], params[c][1]) for c, m in enumerate(pre)]


def test_train_mog2_then_extract_foreground_mask(m2eng):
    from oracle import foreground_np as fg, postfilter_np as pf
    from voxcarve import background_subtraction as bs
    rng = np.random.default_rng(12)
    bgs, fgs = _scene(rng, 240, 320, 10, 4)
    (dev,), (ref,) = _trained([bgs], m2eng, ["MOG2"], shadows=True)
    state, nmodes, _, nf = dev.state()
    assert nf == len(bgs) and np.array_equal(state.view(np.uint32), ref.state.view(np.uint32)) and np.array_equal(nmodes, ref.nmodes)
    saw_shadow = False
    for t, f in enumerate(fgs):
        flags = (True, True, True, True) if t % 2 else (False, True, False, True)
        p = (2000, 115)
        got = bs.extract_foreground_mask(f, dev, 0, p[0], p[1], *flags, engine=m2eng, contour_stage="device")
        pre = fg.pre_filter(ref.apply(fg.bgr_to_hsv(f), 0), flags[0], flags[1])
        saw_shadow |= bool((pre == 127).any())
        filled = lit.fill_figures(pre, p[0], p[1])
        assert np.array_equal(m2eng.fill_figures(pre, p[0], p[1]), filled), t
        want = np.where(pf.post_filter(filled, flags[2], flags[3]) > 0, 255, 0).astype(np.uint8)
        assert np.array_equal(got, want), (t, flags)
        assert got.any()
        state, nmodes, _, _ = dev.state()
        assert np.array_equal(state.view(np.uint32), ref.state.view(np.uint32)) and np.array_equal(nmodes, ref.nmodes)
    assert saw_shadow
    # vc_foreground_front with learning: the same as the three restated steps
    for lr, op, cl in ((0.02, False, True), (-1, True, False)):
        one = m2eng.foreground_front(dev._model, fgs[0], lr, op, cl)
        assert np.array_equal(one, fg.pre_filter(ref.apply(fg.bgr_to_hsv(fgs[0]), lr), op, cl)), (lr, op, cl)
    from voxcarve._lib import VoxcarveError
    with pytest.raises(VoxcarveError, match="train_MOG2_background_model.*cv2"):
        bs.train_MOG2_background_model("data/cam1", "background.avi", engine=m2eng)
    dev.close()


def _cams_and_scene(seed, H, W, n_fg):
    rng = np.random.default_rng(seed)
    per = [_scene(rng, H, W, 6, n_fg, shift=13 * c) for c in range(4)]
    return [p[0] for p in per], [[p[1][t] for p in per] for t in range(n_fg)]


def test_foreground_to_slot_mixed_models_equals_host_path(m2eng, cams):
    from oracle import carve_c, postfilter_np as pf
    H, W = 486, 644
    bgs, frame_sets = _cams_and_scene(41, H, W, 3)
    kinds = ["MOG", "MOG2", "MOG", "MOG2"]
    dev, ref = _trained(bgs, m2eng, kinds, shadows=True)
    grid = (96, 96, 96)
    m2eng.set_grid(*grid)
    m2eng.set_cameras(cams, H, W)
    m2eng.set_mask_postfilter([p[4] for p in PARAMS], [p[5] for p in PARAMS])
    oc = fx.oracle_cams(cams)
    saw_shadow = False
    for k, fs in enumerate(frame_sets):
        m2eng.foreground_to_slot(dev, fs, PARAMS, slot=0)
        pre, filled = _restated(fs, PARAMS, ref)
        saw_shadow |= any((pre[c] == 127).any() for c in (1, 3))
        masks = [np.where(pf.post_filter(filled[c], PARAMS[c][4], PARAMS[c][5]) > 0, 255, 0).astype(np.uint8) for c in range(4)]
        for c in range(4):
            assert np.array_equal(m2eng.fetch_mask(c, 0), masks[c]), (k, c)
        for c in (1, 3):
            state, nmodes, _, _ = dev[c].state()
            assert np.array_equal(state.view(np.uint32), ref[c].state.view(np.uint32)) and np.array_equal(nmodes, ref[c].nmodes), (k, c)
        want = carve_c.carve(*grid, oc, masks, fs, color_cam=1)
        m2eng.touch_masks(0)
        n = m2eng.carve(slot=0, color_cam=1)
        idx, rgb, _ = m2eng.fetch()
        assert n == want["count"] and np.array_equal(idx, want["idx"]) and np.array_equal(rgb[:, ::-1], want["bgr"]), k
        assert n > 0
    assert saw_shadow
    m2eng.set_mask_postfilter([False] * 4, [False] * 4)
    for m in dev:
        m.close()


def test_set_voxel_positions_with_device_video_source_mog2(built):
    from oracle import postfilter_np as pf
    from voxcarve import assignment
    H, W = 486, 644
    bgs, frame_sets = _cams_and_scene(43, H, W, 3)
    data = os.path.join(fx.GOLDEN, "data")
    ref = []
    from oracle import foreground_np as fg
    for b in bgs:                                            # the reference's comparison script's MOG2 (:400-401)
        r = mog2_np.MOG2(history=len(b), varThreshold=650, detectShadows=False)
        for f in b:
            r.apply(fg.bgr_to_hsv(f), -1)
        ref.append(r)
    sets = []
    for fs in frame_sets:
        _, filled = _restated(fs, PARAMS, ref)
        masks = [np.where(pf.post_filter(m, PARAMS[c][4], PARAMS[c][5]) > 0, 255, 0).astype(np.uint8) for c, m in enumerate(filled)]
        sets.append((fs, masks))
    results = {}
    for name, src in (("static", assignment.StaticFrameSource(sets)),
                      ("device", assignment.DeviceVideoSource([[fs[c] for fs in frame_sets] for c in range(4)], bgs, model="MOG2"))):
        assignment.configure(frame_source=src, data_path=data)
        out = []
        for _ in range(len(frame_sets)):
            out.append(assignment.set_voxel_positions(64, 32, 64))
        assert assignment.set_voxel_positions(64, 32, 64) == ([], [])
        results[name] = out
    assignment.configure(frame_source=None)
    assert any(len(p) for p, _ in results["static"])
    for (p0, c0), (p1, c1) in zip(results["static"], results["device"]):
        assert np.array_equal(p0, p1) and np.array_equal(c0, c1)
    with pytest.raises(ValueError):
        assignment.DeviceVideoSource([[fs[c] for fs in frame_sets] for c in range(4)], bgs, model="KNN")
