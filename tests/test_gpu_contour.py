"""The contour stage on the device (vc_fill_figures, csrc/vc_contour.h) and extract_foreground_mask straight into a carve slot
(vc_foreground_to_slot), against the literal restatement of background_subtraction.py:171-193 (contour_literal) and the
restated front / back halves (oracle.foreground_np, oracle.mog_np, oracle.postfilter_np).  Parity with cv2 itself: unpinned."""
import os

import numpy as np
import pytest

import contour_literal as lit
import contour_masks as cm
import fixtures_util as fx

pytestmark = pytest.mark.gpu

PARAMS = [[5000, 115, False, False, True, True], [5000, 115, False, False, True, True],
          [5000, 175, False, True, True, True], [5000, 115, False, False, False, True]]   # assignment.py:28-33


@pytest.fixture(scope="module")
def ceng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _scene(rng, H, W, n_bg, n_fg, seed_shift=0):
    """Background frames and frames with a large figure (holes, an island, a thin arm) moving across a textured background."""
    yy, xx = np.mgrid[0:H, 0:W]
    bg = np.stack([(xx * 255 // max(W - 1, 1)), (yy * 255 // max(H - 1, 1)), ((xx + yy) * 7) % 256], -1).astype(np.int64)
    bgs = [np.clip(bg + rng.integers(-4, 5, (H, W, 3)), 0, 255).astype(np.uint8) for _ in range(n_bg)]
    fgs = []
    for t in range(n_fg):
        cy, cx = H // 2 + (t * 7 + seed_shift) % (H // 6), W // 3 + (t * 11 + seed_shift) % (W // 3)
        body = ((yy - cy) / (H * 0.3)) ** 2 + ((xx - cx) / (W * 0.12)) ** 2 < 1
        hole = ((yy - cy) / (H * 0.08)) ** 2 + ((xx - cx) / (W * 0.04)) ** 2 < 1
        island = ((yy - cy) / (H * 0.02)) ** 2 + ((xx - cx) / (W * 0.01)) ** 2 < 1
        small = ((yy - cy + H // 5) / 4.0) ** 2 + ((xx - cx) / 6.0) ** 2 < 1
        arm = (np.abs(yy - cy + H // 10) < 2) & (xx > cx) & (xx < cx + W // 4)
        fig = (body & ~hole) | island | arm
        fig &= ~small
        f = bg.copy()
        f[fig] = 255 - f[fig]
        f[rng.random((H, W)) < 0.002] = 0                          # salt that survives the model as noise
        fgs.append(np.clip(f + rng.integers(-4, 5, (H, W, 3)), 0, 255).astype(np.uint8))
    return bgs, fgs


def _restated_masks(bgs, fgs_t, params, mogs):
    """extract_foreground_mask up to the contour stage's output (no post-filter), restated, one frame set; mogs trained."""
    from oracle import foreground_np as fg
    out = []
    for c, f in enumerate(fgs_t):
        p = params[c]
        m = fg.pre_filter(mogs[c].apply(fg.bgr_to_hsv(f), 0), p[2], p[3])
        out.append(lit.fill_figures(m, p[0], p[1]))
    return out


def _trained(bgs_per_cam, eng):
    from oracle import foreground_np as fg, mog_np
    from voxcarve import background_subtraction as bs
    dev, ref = [], []
    for bgs in bgs_per_cam:
        dev.append(bs.train_MOG_background_model(history=len(bgs), n_mixtures=50, bg_ratio=0.90, noise_sigma=0, engine=eng, frames=bgs))
        r = mog_np.MOG(history=len(bgs), nmixtures=50, backgroundRatio=0.90, noiseSigma=0)
        for f in bgs:
            r.apply(fg.bgr_to_hsv(f), -1)
        ref.append(r)
    return dev, ref


def test_fill_figures_equals_literal(ceng):
    for m in cm.family(1, 63):
        for T, t in cm.THRESHOLDS + [(8, 2), (3, -4)]:
            assert np.array_equal(ceng.fill_figures(m, T, t), lit.fill_figures(m, T, t)), (m.shape, T, t)
    rng = np.random.default_rng(5)
    for m in (cm.blobs(rng, 486, 644, k=40), cm.mix(rng, 486, 644), cm.noise(rng, 486, 644, 0.5), cm.rings(60),
              cm.blobs(rng, 1080, 1920, k=90)):
        for T, t in cm.THRESHOLDS:
            assert np.array_equal(ceng.fill_figures(m, T, t), lit.fill_figures(m, T, t)), (m.shape, T, t)
    for c, m in enumerate(fx.golden_masks()):
        for T, t in ((5000, 115), (5000, 175), (0, 0), (50, -20)):
            got = ceng.fill_figures(m, T, t)
            assert np.array_equal(got, lit.fill_figures(m, T, t)), (c, T, t)
        assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 255}


def test_fill_figures_on_mog_masks_and_extract_foreground_mask(ceng):
    from oracle import foreground_np as fg, postfilter_np as pf
    from voxcarve import background_subtraction as bs
    rng = np.random.default_rng(11)
    bgs, fgs = _scene(rng, 240, 320, 8, 4)
    (dev,), (ref,) = _trained([bgs], ceng)
    for t, f in enumerate(fgs):
        for flags in ((False, False, True, True), (False, True, True, True), (True, True, False, False)):
            p = (5000, 115) if t % 2 else (2000, 175)
            got = bs.extract_foreground_mask(f, dev, 0, p[0], p[1], *flags, engine=ceng, contour_stage="device")
            pre = fg.pre_filter(ref.apply(fg.bgr_to_hsv(f), 0), flags[0], flags[1])
            filled = lit.fill_figures(pre, p[0], p[1])
            assert np.array_equal(ceng.fill_figures(pre, p[0], p[1]), filled)
            want = pf.post_filter(filled, flags[2], flags[3])
            want = np.where(want > 0, 255, 0).astype(np.uint8)
            assert np.array_equal(got, want), (t, flags)
            assert got.any()
    assert np.array_equal(bs.fill_figures_device(pre, 5000, 115, engine=ceng), lit.fill_figures(pre, 5000, 115))


def _cams_and_scene(seed, H, W, n_fg):
    rng = np.random.default_rng(seed)
    per = [_scene(rng, H, W, 6, n_fg, seed_shift=17 * c) for c in range(4)]
    return [p[0] for p in per], [[p[1][t] for p in per] for t in range(n_fg)]


def test_foreground_to_slot_then_carve_equals_host_path(ceng, cams):
    H, W = 486, 644
    bgs, frame_sets = _cams_and_scene(21, H, W, 3)
    dev, ref = _trained(bgs, ceng)
    ceng.set_grid(128, 128, 128)
    ceng.set_cameras(cams, H, W)
    ceng.set_mask_postfilter([p[4] for p in PARAMS], [p[5] for p in PARAMS])
    from oracle import postfilter_np as pf
    restated = [_restated_masks(bgs, fs, PARAMS, ref) for fs in frame_sets]
    for k, fs in enumerate(frame_sets):
        ceng.foreground_to_slot(dev, fs, PARAMS, slot=0)
        for c in range(4):
            want = np.where(pf.post_filter(restated[k][c], PARAMS[c][4], PARAMS[c][5]) > 0, 255, 0)
            assert np.array_equal(ceng.fetch_mask(c, 0), want), (k, c)
        for cc in (1, 3):
            ceng.touch_masks(0)
            n = ceng.carve(slot=0, color_cam=cc)
            got = ceng.fetch_records()
            ceng.upload_masks(restated[k], slot=1)
            for c in range(4):
                ceng.upload_frame(c, fs[c], slot=1)
            assert ceng.carve(slot=1, color_cam=cc) == n
            assert np.array_equal(ceng.fetch_records(), got), (k, cc)
        assert n > 0
    # two slots in rotation, steps in flight
    want = []
    for k, fs in enumerate(frame_sets):
        ceng.upload_masks(restated[k], slot=2)
        for c in range(4):
            ceng.upload_frame(c, fs[c], slot=2)
        ceng.carve(slot=2)
        want.append(ceng.fetch_records())
    for k in range(len(frame_sets)):
        fs = frame_sets[k]
        ceng.foreground_to_slot(dev, fs, PARAMS, slot=k % 2)
        ceng.carve_begin(slot=k % 2)
        if k >= 1:
            ceng.carve_end()
            assert np.array_equal(ceng.fetch_records(), want[k - 1]), k - 1
    ceng.carve_end()
    assert np.array_equal(ceng.fetch_records(), want[-1])
    # errors: nothing of the slot touched
    from voxcarve._lib import VoxcarveError
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no background model"):
        ceng.foreground_to_slot([dev[0], dev[1], dev[2], 63], frame_sets[0], PARAMS, slot=0)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*3 background models for 4 cameras"):
        ceng.foreground_to_slot(dev[:3], frame_sets[0], PARAMS, slot=0)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*images of 240 x 320"):
        ceng.foreground_to_slot(dev, [f[:240, :320] for f in frame_sets[0]], PARAMS, slot=0)
    ceng.touch_masks(0)                                       # slot 0 still holds the last frame set
    assert ceng.carve(slot=0) == len(want[-1]) and np.array_equal(ceng.fetch_records(), want[-1])


def test_set_voxel_positions_with_device_video_source(built):
    from oracle import postfilter_np as pf
    from voxcarve import assignment
    import voxcarve
    H, W = 486, 644
    bgs, frame_sets = _cams_and_scene(33, H, W, 3)
    data = os.path.join(fx.GOLDEN, "data")
    with voxcarve.CarveEngine(0) as e:
        _, ref = _trained(bgs, e)
    sets = []
    for fs in frame_sets:
        filled = _restated_masks(bgs, fs, PARAMS, ref)
        masks = [np.where(pf.post_filter(m, PARAMS[c][4], PARAMS[c][5]) > 0, 255, 0).astype(np.uint8) for c, m in enumerate(filled)]
        sets.append((fs, masks))
    results = {}
    for name, src in (("static", assignment.StaticFrameSource(sets)),
                      ("device", assignment.DeviceVideoSource([[fs[c] for fs in frame_sets] for c in range(4)], bgs))):
        assignment.configure(frame_source=src, data_path=data)
        out = []
        for _ in range(len(frame_sets)):
            pos, col = assignment.set_voxel_positions(64, 32, 64)
            out.append((pos, col))
        assert assignment.set_voxel_positions(64, 32, 64) == ([], [])          # end of video
        results[name] = out
    assignment.configure(frame_source=None)
    assert any(len(p) for p, _ in results["static"])
    for (p0, c0), (p1, c1) in zip(results["static"], results["device"]):
        assert np.array_equal(p0, p1) and np.array_equal(c0, c1)
