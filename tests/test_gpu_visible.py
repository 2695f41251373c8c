"""Occlusion-aware colouring on the device (vc_color_visible, vc_fetch_visibility, vc_fetch_depth; csrc/vc_visible.h) against
the restatement (tests/visible_np.py): every depth map, every camera mask and every record bit for bit, on the real cameras, a
large grid, 16 cameras at 1080p, cameras next to and inside the grid, a grid one voxel thick, thresholds below C and an empty hull;
the error paths; and set_voxel_positions with color_mode="visible" through both frame sources."""
import os

import numpy as np
import pytest

import fixtures_util as fx
import visible_np as vn
from oracle import carve_np
from voxcarve import synthetic
from voxcarve.camera import Camera

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def veng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _setup(e, grid, cams, masks, frames, bounds=None):
    H, W = masks[0].shape
    if bounds is None:
        e.set_grid(*grid)
    else:
        e.set_grid(*grid, bounds=bounds)
    e.set_cameras(cams, H, W)
    e.upload_masks(masks)
    for c, f in enumerate(frames):
        e.upload_frame(c, f)


def _check(e, cams, frames, min_views=None, mode="fused", tol=None):
    """Carve, colour by visibility, compare with the restatement of the carve's own records; returns the survivor count."""
    H, W = e.image_size
    S = e.carve(min_views=min_views, mode=mode)
    rec0 = e.fetch_records().copy()
    e.color_visible(depth_tolerance=tol)
    rec1 = e.fetch_records()
    idx = (rec0 & 0xffffffff).astype(np.uint32)
    rgb0 = np.stack([(rec0 >> np.uint64(k)) & np.uint64(0xff) for k in (32, 40, 48)], axis=1).astype(np.uint8)
    zmaps, vis, rgb = vn.color_visible(idx, rgb0, e.grid, e.bounds, fx.oracle_cams(cams), frames, H, W, tol)
    want = (rec0 & np.uint64(0xff000000ffffffff)) | (rgb[:, 0].astype(np.uint64) << np.uint64(32)) | \
        (rgb[:, 1].astype(np.uint64) << np.uint64(40)) | (rgb[:, 2].astype(np.uint64) << np.uint64(48))
    assert rec1.size == S
    for c in range(len(cams)):
        assert np.array_equal(e.fetch_depth(c).view(np.uint32).reshape(-1), zmaps[c]), ("depth map", c)
    assert np.array_equal(e.fetch_visibility(), vis), "camera masks"
    assert np.array_equal(rec1, want), "records"
    return S, vis


@pytest.mark.parametrize("n", [64, 128, 256])
def test_golden_cameras_equal_restatement(veng, cams, masks, frames, n):
    _setup(veng, (n, n, n), cams, masks, frames)
    S, vis = _check(veng, cams, frames)
    assert S > 0 and (vis != 0).sum() > S // 20
    if n == 64:                                              # table mode: same records in, same colours out
        veng.build_lut()
        _check(veng, cams, frames, mode="lut")


def test_sixteen_cameras_1080p(veng):
    H, W = 1080, 1920
    cams = synthetic.ring_cameras(16, H, W)
    masks = synthetic.ellipsoid_masks(cams, H, W)
    frames = synthetic.random_frames(16, H, W)
    _setup(veng, (128, 128, 128), cams, masks, frames)
    S, vis = _check(veng, cams, frames)
    assert S > 0 and (vis != 0).sum() > S // 10


def test_cameras_next_to_and_inside_the_grid_min_views_below_c(veng, cams, masks, frames):
    H, W = masks[0].shape
    K = np.array([[490.0, 0, W / 2], [0, 490.0, H / 2], [0, 0, 1.0]])
    R = np.eye(3)                                            # looking along +z
    near = Camera(K, np.zeros(5), None, -R @ np.array([256.0, 0.0, -2048.0 - 300.0]), R=R)    # 300 mm below the z_min layer
    inside = Camera(K, np.zeros(5), None, -R @ np.array([256.0, 0.0, -2048.0 + 300.0]), R=R)  # inside the grid: corners behind it
    allc = list(cams) + [near, inside]
    full = np.full((H, W), 255, np.uint8)
    fr = list(frames) + fx.synthetic_frames(6, H, W)[4:]
    _setup(veng, (64, 64, 64), allc, list(masks) + [full, full], fr)
    S, vis = _check(veng, allc, fr, min_views=4)
    assert S > 0 and ((vis >> 4) & 1).any() and ((vis >> 5) & 1).any()
    assert np.isinf(veng.fetch_depth(5)).mean() < 0.5        # huge rectangles from inside the grid


def test_splat_knobs_change_nothing(veng, cams, masks, frames):
    H, W = masks[0].shape
    K = np.array([[490.0, 0, W / 2], [0, 490.0, H / 2], [0, 0, 1.0]])
    inside = Camera(K, np.zeros(5), None, -np.array([256.0, 0.0, -2048.0 + 300.0]), R=np.eye(3))
    allc = list(cams) + [inside]
    fr = list(frames) + fx.synthetic_frames(5, H, W)[4:]
    _setup(veng, (48, 64, 40), allc, list(masks) + [np.full((H, W), 255, np.uint8)], fr)
    try:
        for check, big in ((0, 64), (1, 1), (0, 1 << 30)):      # no plain look first; every rectangle queued; none queued
            veng.set_option("visible_check", check)
            veng.set_option("visible_big_rect", big)
            _check(veng, allc, fr, min_views=3)
    finally:
        veng.set_option("visible_check", 1)
        veng.set_option("visible_big_rect", 64)


def test_one_voxel_thick_grid_and_zero_tolerance(veng, cams, masks, frames):
    _setup(veng, (96, 1, 80), cams, masks, frames)
    S, _ = _check(veng, cams, frames, min_views=2)
    assert S > 0
    _setup(veng, (64, 64, 64), cams, masks, frames)
    _check(veng, cams, frames, min_views=3, tol=0.0)


def test_empty_hull(veng, cams, masks, frames):
    H, W = masks[0].shape
    _setup(veng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    S, vis = _check(veng, cams, frames)
    assert S == 0 and vis.size == 0
    assert np.isinf(veng.fetch_depth(0)).all()


def test_errors_and_a_carve_restores_camera_colours(veng, cams, masks, frames):
    import voxcarve
    from voxcarve._lib import VoxcarveError
    H, W = masks[0].shape
    with voxcarve.CarveEngine(0) as e:
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.color_visible()
        e.set_grid(64, 64, 64)
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*camera 0 has no frame"):
            e.color_visible()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no visibility"):
            e.fetch_visibility()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no depth maps"):
            e.fetch_depth(0)
        for c in (0, 2, 3):
            e.upload_frame(c, frames[c])                         # after the carve: prepared by color_visible itself
        for bad in (-1.0, float("nan")):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*negative or NaN"):
                e.color_visible(depth_tolerance=bad)
        assert e._L.vc_color_visible(e._ctx, 0, 1.0, 1) == -1
        e.carve(records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.color_visible()
        e.set_slab(0, 32)
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.color_visible()
        e.set_slab(0, 64)
        S = e.carve()
        before = e.fetch_records().copy()
        e.color_visible()
        assert not np.array_equal(e.fetch_records(), before)
        assert e.fetch_visibility().size == S
        assert e.carve() == S
        assert np.array_equal(e.fetch_records(), before)        # the colour camera's colours again
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no visibility"):
            e.fetch_visibility()


def test_set_voxel_positions_visible_mode_both_sources(built):
    import test_gpu_contour as tc
    import voxcarve
    from oracle import carve_c
    from voxcarve import assignment
    from voxcarve.engine import viewer_colors, viewer_positions, voxel_keys
    H, W = 486, 644
    bgs, frame_sets = tc._cams_and_scene(57, H, W, 2)
    data = os.path.join(fx.GOLDEN, "data")
    fsrc = assignment.DeviceVideoSource([[fs[c] for fs in frame_sets] for c in range(4)], bgs)
    try:
        assignment.configure(frame_source=fsrc, data_path=data, color_mode="visible")
        dev, sets = [], []
        for fs in frame_sets:
            dev.append(assignment.set_voxel_positions(64, 32, 64))
            sets.append((fs, [assignment._engine.fetch_mask(c) for c in range(4)]))     # the masks the device carved
        cams = assignment._engine.cameras
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=data, color_mode="visible")
        static = [assignment.set_voxel_positions(64, 32, 64) for _ in sets]
        assert assignment.set_voxel_positions(64, 32, 64) == ([], [])
        with pytest.raises(ValueError):
            assignment.configure(color_mode="mean")
    finally:
        assignment.configure(frame_source=None, color_mode="camera")
    grid = (64, 64, 64)
    with voxcarve.CarveEngine(0) as e:
        e.set_grid(*grid)
        axes = e.axes()
    assert any(len(p) for p, _ in static)
    for (fs, ms), (p0, c0), (p1, c1) in zip(sets, static, dev):
        want = carve_c.carve(*grid, fx.oracle_cams(cams), ms, fs)
        _, _, rgb = vn.color_visible(want["idx"], want["bgr"][:, ::-1], grid, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(cams), fs, H, W)
        assert np.array_equal(p0, viewer_positions(voxel_keys(want["idx"], grid, axes)))
        assert np.array_equal(c0, viewer_colors(rgb))
        assert np.array_equal(p0, p1) and np.array_equal(c0, c1)
