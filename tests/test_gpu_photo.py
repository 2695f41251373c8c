"""Photo-consistency carving on the device (vc_photo_carve, vc_fetch_photo_rounds; csrc/vc_photo.h) against the restatement
(tests/photo_np.py): records (order, colours, seen byte), round numbers, camera masks, every depth map, occupancy words and stats
bit for bit -- the real cameras at 64^3 / 128^3 / 256^3 with random and textured frames, the textured pit scene with the real
cameras and with 16 ring cameras at 1080p, both carve modes, min_views variants and the empty hull; every refusal; the next carve,
color_visible, marching cubes and set_voxel_positions(hull="photo") after a photo carve."""
import os

import numpy as np
import pytest

import fixtures_util as fx
import photo_np as pn
from oracle import carve_np
from voxcarve import synthetic
from test_photo_restatement import pit_setup

pytestmark = pytest.mark.gpu

REAL_PIT = dict(centre=(360.0, 40.0, -300.0), half=(350.0, 350.0, 300.0), opening=(200.0, 200.0), depth=150.0)


@pytest.fixture(scope="module")
def peng(built):
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


def _split(rec):
    idx = (rec & 0xffffffff).astype(np.uint32)
    rgb = np.stack([(rec >> np.uint64(k)) & np.uint64(0xff) for k in (32, 40, 48)], axis=1).astype(np.uint8)
    return idx, rgb


def _check(e, cams, frames, T=1200, m=2, R=32, mode="fused", min_views=None, tol=None):
    """Carve, photo-carve, compare everything with the restatement of the carve's own records; returns (restated, stats)."""
    H, W = e.image_size
    S0 = e.carve(min_views=min_views, mode=mode)
    rec0 = e.fetch_records().copy()
    st = e.photo_carve(var_threshold=T, min_views=m, max_rounds=R, depth_tolerance=tol)
    idx0, rgb0 = _split(rec0)
    want = pn.photo_carve(idx0, rgb0, e.grid, e.bounds, fx.oracle_cams(cams), frames, H, W, var_threshold=T, min_views=m,
                          max_rounds=R, tol=tol)
    keep = want["rounds"] == 0
    F = want["idx"].size
    assert st["survivors_before"] == S0 and st["survivors_after"] == F == e.count
    assert st["rounds"] == want["n_rounds"] and st["converged"] == want["converged"]
    assert st["photo_ms"] > 0
    assert np.array_equal(e.fetch_photo_rounds(), want["rounds"]), "rounds"
    rec = e.fetch_records()
    wrec = (rec0[keep] & np.uint64(0xff000000ffffffff)) | (want["rgb"][:, 0].astype(np.uint64) << np.uint64(32)) | \
        (want["rgb"][:, 1].astype(np.uint64) << np.uint64(40)) | (want["rgb"][:, 2].astype(np.uint64) << np.uint64(48))
    assert np.array_equal(rec, wrec), "records"
    idx, rgb, seen = e.fetch()
    assert np.array_equal(idx, want["idx"]) and np.array_equal(rgb, want["rgb"])
    assert np.array_equal(e.fetch_visibility(), want["vis"]), "camera masks"
    for c in range(len(cams)):
        assert np.array_equal(e.fetch_depth(c).view(np.uint32).reshape(-1), want["zmaps"][c]), ("depth map", c)
    occ = np.zeros(e.n_voxels, dtype=bool)
    occ[want["idx"]] = True
    assert np.array_equal(e.fetch_occupancy(), occ), "occupancy"
    return want, st


@pytest.mark.parametrize("n", [64, 128, 256])
def test_golden_cameras_random_frames_equal_restatement(peng, cams, masks, frames, n):
    _setup(peng, (n, n, n), cams, masks, frames)
    want, st = _check(peng, cams, frames, R=4 if n > 64 else 32)
    assert (want["rounds"] != 0).any()
    if n == 64:
        peng.build_lut()
        _check(peng, cams, frames, mode="lut")
        for m, T in ((3, 600), (4, 0)):
            _check(peng, cams, frames, m=m, T=T, R=3)


@pytest.mark.parametrize("n", [64, 128, 256])
def test_golden_cameras_textured_pit_equal_restatement(peng, cams, n):
    H, W = 486, 644
    masks, frames = synthetic.textured_scene(cams, H, W, **REAL_PIT)
    _setup(peng, (n, n, n), cams, masks, frames)
    want, st = _check(peng, cams, frames, R=32 if n < 256 else 6)
    assert st["survivors_before"] > 0


def test_ring_pit_scene_and_sixteen_cameras_1080p(peng):
    H, W = 240, 320
    cams, bounds, grid = pit_setup(H, W, 64)
    masks, frames = synthetic.textured_scene(cams, H, W)
    _setup(peng, grid, cams, masks, frames, bounds=bounds)
    want, st = _check(peng, cams, frames, R=64)
    assert st["converged"] and st["survivors_after"] < st["survivors_before"]
    H, W = 1080, 1920
    cams = synthetic.ring_cameras(16, H, W)
    masks, frames = synthetic.textured_scene(cams, H, W)
    ctr, half = np.array(synthetic.VOLUME_CENTRE), 1.15 * np.array(synthetic.PIT_HALF)
    lo, hi = ctr - half, ctr + half
    _setup(peng, (48, 48, 48), cams, masks, frames, bounds=(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))
    _check(peng, cams, frames, R=8)


def test_empty_hull(peng, cams, masks, frames):
    H, W = masks[0].shape
    _setup(peng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    want, st = _check(peng, cams, frames)
    assert st == {"rounds": 1, "converged": True, "survivors_before": 0, "survivors_after": 0, "photo_ms": st["photo_ms"]}
    assert peng.fetch_photo_rounds().size == 0 and np.isinf(peng.fetch_depth(0)).all()


def test_after_a_photo_carve(peng, cams, masks, frames):
    """color_visible changes nothing, marching cubes meshes F, photo-carving F again removes nothing when converged, the next
    carve restores the visual hull."""
    _setup(peng, (96, 96, 96), cams, masks, frames)
    S = peng.carve()
    hull = peng.fetch_records().copy()
    st = peng.photo_carve(max_rounds=64)
    assert st["converged"] and st["survivors_after"] < S
    rec = peng.fetch_records().copy()
    vis = peng.fetch_visibility().copy()
    peng.color_visible()
    assert np.array_equal(peng.fetch_records(), rec) and np.array_equal(peng.fetch_visibility(), vis)
    verts, faces = peng.marching_cubes(volume=None)
    occ = peng.fetch_occupancy().reshape(96, 96, 96)
    v2, f2 = peng.marching_cubes(volume=occ)
    assert np.array_equal(verts, v2) and np.array_equal(faces, f2) and faces.size > 0
    idx = (rec & 0xffffffff).astype(np.int64)
    want = np.zeros(96 ** 3, dtype=bool)
    want[idx] = True
    assert np.array_equal(occ.reshape(-1), want)
    again = peng.photo_carve(max_rounds=64)
    assert again["rounds"] == 1 and again["converged"] and again["survivors_after"] == again["survivors_before"] == rec.size
    assert np.array_equal(peng.fetch_records(), rec)
    assert peng.carve() == S
    assert np.array_equal(peng.fetch_records(), hull)
    from voxcarve._lib import VoxcarveError
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no photo rounds"):
        peng.fetch_photo_rounds()


def test_refusals(peng, cams, masks, frames):
    import voxcarve
    from voxcarve._lib import VoxcarveError, VcPhotoStats
    import ctypes
    H, W = masks[0].shape
    with voxcarve.CarveEngine(0) as e:
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.photo_carve()
        e.set_grid(64, 64, 64)
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*camera 0 has no frame"):
            e.photo_carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no photo rounds"):
            e.fetch_photo_rounds()
        for c in (0, 2, 3):
            e.upload_frame(c, frames[c])
        for bad in (-1.0, float("nan")):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*negative or NaN"):
                e.photo_carve(depth_tolerance=bad)
        for kw in ({"min_views": 1}, {"min_views": 5}, {"max_rounds": 0}, {"max_rounds": 256}):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*(min_views|max_rounds)"):
                e.photo_carve(**kw)
        st = VcPhotoStats()
        assert e._L.vc_photo_carve(e._ctx, 0, 1.0, 1200, 2, 4, 1, ctypes.byref(st)) == -1
        assert "flags" in e._L.vc_last_error(e._ctx).decode()
        assert e._L.vc_photo_carve(e._ctx, 0, 1.0, 1200, 2, 4, 0, None) == -1
        assert "stats" in e._L.vc_last_error(e._ctx).decode()
        e.carve(records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.photo_carve()
        e.set_slab(0, 32)
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.photo_carve()
        e.set_slab(0, 64)
        e.carve_begin()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
            e.photo_carve()
        e.carve_end()
        S = e.count
        st = e.photo_carve(max_rounds=2)
        assert st["survivors_before"] == S and e.fetch_photo_rounds().size == S


def test_set_voxel_positions_photo_hull_both_sources(built):
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
        assignment.configure(frame_source=fsrc, data_path=data, hull="photo", photo_var_threshold=900)
        dev, sets, status = [], [], []
        for fs in frame_sets:
            dev.append(assignment.set_voxel_positions(64, 32, 64))
            status.append(assignment.voxels_status().copy())
            sets.append((fs, [assignment._engine.fetch_mask(c) for c in range(4)]))     # the masks the device carved
        cams = assignment._engine.cameras
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=data, hull="photo", photo_var_threshold=900)
        static = [assignment.set_voxel_positions(64, 32, 64) for _ in sets]
        assert assignment.set_voxel_positions(64, 32, 64) == ([], [])
        with pytest.raises(ValueError):
            assignment.configure(hull="convex")
    finally:
        assignment.configure(frame_source=None, color_mode="camera", hull="visual")
    grid = (64, 64, 64)
    with voxcarve.CarveEngine(0) as e:
        e.set_grid(*grid)
        axes = e.axes()
    assert any(len(p) for p, _ in static)
    for (fs, ms), (p0, c0), (p1, c1), occ in zip(sets, static, dev, status):
        hull = carve_c.carve(*grid, fx.oracle_cams(cams), ms, fs)
        want = pn.photo_carve(hull["idx"], hull["bgr"][:, ::-1], grid, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(cams), fs, H, W,
                              var_threshold=900)
        assert np.array_equal(p0, viewer_positions(voxel_keys(want["idx"], grid, axes)))
        assert np.array_equal(c0, viewer_colors(want["rgb"]))
        assert np.array_equal(p0, p1) and np.array_equal(c0, c1)
        dense = np.zeros(64 ** 3, dtype=bool)
        dense[want["idx"]] = True
        assert np.array_equal(occ, dense.reshape(64, 64, 64))
