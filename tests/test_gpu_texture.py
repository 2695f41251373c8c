"""The texturing pass on the device (vc_texture_render, vc_fetch_textured; csrc/vc_texture.h) against the restatement
(tests/texture_np.py): rgb, depth bits, count, best_cam, refined and the contract's stats bit for bit -- the real cameras at 64^3
in both carve modes from the calibrated cameras and from orbit views over the options, 16 cameras, thin and odd grids, a view
from inside the hull, after photo_carve and filter_components, the empty and the solid hull; every refusal, with the images, the
render and the records left alone; assignment.render_views(textured=True) and demo.py --textured."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures_util as fx
import render_np as rn
import texture_np as tn
from voxcarve import _lib, camera, synthetic

pytestmark = pytest.mark.gpu

REAL_PIT = dict(centre=(360.0, 40.0, -300.0), half=(350.0, 350.0, 300.0), opening=(200.0, 200.0), depth=150.0)
DEFAULT = object()


@pytest.fixture(scope="module")
def teng(built):
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


def _inputs(e, cams):
    """What the pass reads besides the render, fetched once per hull: the masks the carve read and color_visible's maps."""
    C = len(cams)
    bm = np.stack([e.fetch_mask(c) > 0 for c in range(C)])
    zmaps = np.stack([e.fetch_depth(c).view(np.uint32).reshape(-1) for c in range(C)])
    return bm, zmaps


def _check(e, cams, frames, m, views, H, W, inputs, steps=8, reach=DEFAULT, tol=DEFAULT, best=2, sharpen=2, filt="bilinear",
           rendered=None):
    """Render (unless given), texture on the device, the same from the restatement; returns (render, device output)."""
    r = e.render(views, H, W) if rendered is None else rendered
    diag = e.default_depth_tolerance()
    reach = diag if reach is DEFAULT else reach
    tol = diag if tol is DEFAULT else tol
    got = e.texture_render(steps=steps, reach_mm=reach, depth_tolerance=tol, best=best, sharpen=sharpen, filter=filt)
    bm, zmaps = inputs
    V = len(views)
    want = tn.texture([rn.view_params(v) for v in views], H, W, (r["index"] != 0xFFFFFFFF).reshape(V, -1), r["depth"].reshape(V, -1),
                      r["rgb"].reshape(V, -1, 3), fx.oracle_cams(cams), bm, m, zmaps, frames, steps=steps, reach=reach, tol=tol,
                      best=best, sharpen=sharpen, filt=tn.FILTERS[filt])
    what = (steps, reach, tol, best, sharpen, filt)
    assert np.array_equal(got["rgb"].reshape(V, -1, 3), want["rgb"]), what
    assert np.array_equal(got["depth"].reshape(V, -1).view(np.uint32), want["depth"].view(np.uint32)), what
    assert np.array_equal(got["count"].reshape(V, -1), want["count"]), what
    assert np.array_equal(got["best_cam"].reshape(V, -1), want["best_cam"]), what
    assert np.array_equal(got["refined"].reshape(V, -1), want["refined"] != 0), what
    for k, v in want["stats"].items():
        assert got["stats"][k] == v, (k, what)
    assert got["stats"]["hits"] == r["stats"]["hits"]
    if steps and got["stats"]["hits"]:
        assert got["stats"]["point_tests"] > 0
    return r, got


# steps, reach, tol, best, sharpen, filter: every value the options take, not their product
OPTIONS = [(8, DEFAULT, DEFAULT, 2, 2, "bilinear"), (0, DEFAULT, DEFAULT, 1, 0, "nearest"), (1, DEFAULT, 0.0, 4, 6, "bilinear"),
           (24, DEFAULT, DEFAULT, 2, 2, "nearest"), (8, 0.0, DEFAULT, 4, 0, "bilinear"), (24, 200.0, 0.0, 1, 6, "nearest")]


@pytest.mark.parametrize("mode", ["fused", "lut"])
def test_real_cameras_equal_restatement(teng, cams, masks, frames, mode):
    H, W = masks[0].shape
    _setup(teng, (64, 64, 64), cams, masks, frames)
    if mode == "lut":
        teng.build_lut()
    orbit = camera.orbit(2, 4500.0, 25.0, 90.0, 61, 83)
    for m in (4, 3):
        teng.carve(mode=mode, min_views=m)
        teng.color_visible()
        inputs = _inputs(teng, cams)
        rendered = None
        for opt in OPTIONS if m == 4 else OPTIONS[:2]:
            rendered, got = _check(teng, cams, frames, m, orbit, 61, 83, inputs, *opt, rendered=rendered)
        assert got["stats"]["hits"] > 500
        rendered = None
        for opt in OPTIONS[:3] if m == 4 else OPTIONS[3:4]:        # the calibrated cameras (lens distortion) at their own size
            rendered, got = _check(teng, cams, frames, m, cams, H, W, inputs, *opt, rendered=rendered)
        if m == 4:
            r8 = _check(teng, cams, frames, m, cams, H, W, inputs, rendered=rendered)[1]
            assert 0 < r8["stats"]["refined"] <= r8["stats"]["hits"] and r8["stats"]["textured"] > 0
            assert np.array_equal(teng.render(cams, H, W)["rgb"], rendered["rgb"])      # the render's own images are untouched


def test_sixteen_cameras(teng):
    H, W = 135, 240
    cams = synthetic.ring_cameras(16, H, W)
    masks = synthetic.ellipsoid_masks(cams, H, W)
    frames = synthetic.random_frames(16, H, W)
    _setup(teng, (40, 72, 24), cams, masks, frames)
    for m in (16, 13):
        teng.carve(min_views=m)
        teng.color_visible()
        inputs = _inputs(teng, cams)
        r, got = _check(teng, cams, frames, m, [cams[0], cams[5]], H, W, inputs, best=16, sharpen=0)
        assert got["count"].max() > 4
        _check(teng, cams, frames, m, [cams[0], cams[5]], H, W, inputs, best=4, sharpen=2, filt="nearest", rendered=r)


def test_odd_grids_empty_and_solid_hull(teng, cams, masks, frames):
    H, W = masks[0].shape
    orbit = camera.orbit(2, 4500.0, 25.0, 90.0, 61, 83)
    for grid in ((2, 130, 9), (40, 40, 2)):
        _setup(teng, grid, cams, masks, frames)
        teng.carve()
        teng.color_visible()
        _check(teng, cams, frames, 4, orbit, 61, 83, _inputs(teng, cams))
    _setup(teng, (16, 16, 16), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert teng.carve() == 0
    teng.color_visible()
    _, got = _check(teng, cams, frames, 4, orbit, 61, 83, _inputs(teng, cams))
    assert got["stats"]["hits"] == 0 and got["stats"]["pixels"] == 2 * 61 * 83 and np.isinf(got["depth"]).all()
    assert (got["best_cam"] == 255).all() and not got["count"].any()
    # a solid hull: a small box around the centroid of the real hull, every mask full
    _setup(teng, (64, 64, 64), cams, masks, frames)
    teng.carve()
    idx = (teng.fetch_records() & np.uint64(0xffffffff)).astype(np.int64)
    xs, ys, zs = teng.axes()
    c = np.array([xs[(idx // 64) % 64].mean(), ys[idx % 64].mean(), zs[idx // 4096].mean()])
    _setup(teng, (16, 16, 16), cams, [np.full((H, W), 255, np.uint8)] * 4, frames,
           bounds=(c[0] - 30, c[0] + 30, c[1] - 30, c[1] + 30, c[2] - 30, c[2] + 30))
    assert teng.carve() == 16 ** 3
    teng.color_visible()
    near = camera.orbit(2, 600.0, 25.0, 300.0, 61, 83, centre=tuple(c))
    _, got = _check(teng, cams, frames, 4, near, 61, 83, _inputs(teng, cams), steps=8, reach=100.0)
    assert got["stats"]["hits"] > 100 and got["stats"]["refined"] == 0          # every point within reach is inside every mask


def test_view_from_inside_the_hull(teng, cams, masks, frames):
    _setup(teng, (64, 64, 64), cams, masks, frames)
    teng.carve()
    teng.color_visible()
    idx = (teng.fetch_records() & np.uint64(0xffffffff)).astype(np.int64)
    xs, ys, zs = teng.axes()
    P = np.stack([xs[(idx // 64) % 64], ys[idx % 64], zs[idx // 4096]], 1)
    eye = P[np.argmin(((P - P.mean(0)) ** 2).sum(1))]                           # the centre of the survivor nearest the centroid
    view = camera.look_at(eye, eye + np.array([100.0, 30.0, 20.0]), 60.0, 61, 83)
    r, got = _check(teng, cams, frames, 4, [view], 61, 83, _inputs(teng, cams), steps=8)
    assert (r["face"] == 6).all() and (r["depth"] == 0.0).all()                # t0 = 0: lo is clamped to 0, nothing brackets
    assert not got["refined"].any() and (got["depth"] == 0.0).all()


def test_after_photo_carve_and_filter_components(teng, cams, masks, frames):
    H, W = 486, 644
    pm, pf = synthetic.textured_scene(cams, H, W, **REAL_PIT)
    _setup(teng, (64, 64, 64), cams, pm, pf)
    teng.carve()
    teng.photo_carve()
    orbit = camera.orbit(3, 3000.0, 50.0, 120.0, 61, 83, centre=REAL_PIT["centre"])
    _, got = _check(teng, cams, pf, 4, orbit, 61, 83, _inputs(teng, cams))
    assert 0 < got["stats"]["refined"] < got["stats"]["hits"]                   # the pit's floor disagrees with the point test
    _setup(teng, (64, 64, 64), cams, masks, frames)
    teng.carve(min_views=3)
    teng.filter_components(keep_largest=1)
    with pytest.raises(_lib.VoxcarveError, match="vc_color_visible"):
        teng.render(camera.orbit(2, 4500.0, 25.0, 90.0, 61, 83), 61, 83)
        teng.texture_render()
    teng.color_visible()
    _check(teng, cams, frames, 3, camera.orbit(2, 4500.0, 25.0, 90.0, 61, 83), 61, 83, _inputs(teng, cams))


def test_refusals_leave_everything_alone(built, cams, masks, frames):
    import voxcarve
    H, W = masks[0].shape
    L = _lib.load()
    orbit = camera.orbit(2, 4500.0, 25.0, 90.0, 61, 83)

    def raw(e, slot=0, steps=8, reach=20.0, tol=20.0, best=2, sharpen=2, filt=1, flags=0, stats=True):
        st = _lib.VcTextureStats()
        return L.vc_texture_render(e._ctx, slot, steps, reach, tol, best, sharpen, filt, flags, ctypes.byref(st) if stats else None)

    def state(e):
        n = 61 * 83
        rgb, depth, cnt, top, ref = (np.empty(n * 3, np.uint8), np.empty(n, np.float32), np.empty(n, np.uint8), np.empty(n, np.uint8),
                                     np.empty(n, np.uint8))
        u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        assert L.vc_fetch_textured(e._ctx, 1, u8(rgb), depth.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), u8(cnt), u8(top), u8(ref)) == 0
        ridx, rrgb = np.empty(n, np.uint32), np.empty(n * 3, np.uint8)
        assert L.vc_fetch_render(e._ctx, 1, ridx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, u8(rrgb), None) == 0
        return tuple(a.tobytes() for a in (rgb, depth, cnt, top, ref, ridx, rrgb, e.fetch_records()))

    def refused(e, before, what, **kw):
        assert raw(e, **kw) == -1, kw
        assert what in L.vc_last_error(e._ctx).decode(), (kw, L.vc_last_error(e._ctx).decode())
        if before is not None:
            assert state(e) == before, kw

    with voxcarve.CarveEngine(0) as e:
        assert L.vc_fetch_textured(e._ctx, 0, None, None, None, None, None) == -1
        refused(e, None, "no carve result")
        _setup(e, (32, 32, 32), cams, masks, frames)
        refused(e, None, "no carve result")
        e.carve()
        refused(e, None, "vc_render")
        e.render(orbit, 61, 83)
        refused(e, None, "vc_color_visible")
        assert L.vc_fetch_textured(e._ctx, 0, None, None, None, None, None) == -1
        e.color_visible()                                                           # (colours only: the render stays current)
        e.render(orbit, 61, 83)
        assert raw(e) == 0
        assert L.vc_fetch_textured(e._ctx, 0, None, None, None, None, None) == 0
        assert L.vc_fetch_textured(e._ctx, 2, None, None, None, None, None) == -1
        s = state(e)
        refused(e, s, "stats", stats=False)
        refused(e, s, "flags", flags=1)
        refused(e, s, "steps", steps=25)
        for best in (0, 17):
            refused(e, s, "best", best=best)
        refused(e, s, "sharpen", sharpen=7)
        refused(e, s, "filter", filt=2)
        for bad in (-1.0, float("nan"), float("inf")):
            refused(e, s, "reach", reach=bad)
            refused(e, s, "tolerance", tol=bad)
        refused(e, s, "slot 1", slot=1)
        e.upload_masks(masks, slot=1)
        e.upload_frame(0, frames[0], slot=1)
        refused(e, s, "camera 1 has no frame", slot=1)
        e.carve_begin()
        refused(e, None, "in flight")
        e.carve_end()
        refused(e, None, "vc_render")                                               # a new result: the render is stale
        assert state(e)[:7] == s[:7]                                                # (its images and the textured ones stay)
        e.carve(records=False)
        refused(e, None, "VC_FLAG_NO_RECORDS")
        e.carve()
        e.color_visible()
        e.render(orbit, 61, 83)
        assert L.vc_fetch_textured(e._ctx, 0, None, None, None, None, None) == -1  # the new render dropped the textured images
        assert raw(e) == 0 and raw(e, steps=24, best=16, sharpen=6, reach=0.0, tol=0.0) == 0
        s = state(e)
        e.touch_masks(0)
        e.fetch_mask(0)                                                             # the frame set is prepared again
        refused(e, s, "prepared again")
        assert raw(e, steps=0) == 0                                                 # no point test, no masks
        e.carve()
        e.color_visible()
        e.render(orbit, 61, 83)
        assert raw(e) == 0
        s = state(e)
        e.upload_frame(2, frames[1])                                                # a new image waits for the next preparation
        refused(e, s, "prepared again")
        assert raw(e, steps=0) == 0
        refused(e, state(e), "prepared again")
        e.set_slab(0, 16)
        e.carve()
        refused(e, None, "slab")


def test_assignment_and_demo_end_to_end(built, cams, masks, frames, tmp_path):
    from voxcarve import assignment
    saved = dict(assignment._settings)
    assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=fx.GOLDEN + "/data", color_mode="visible")
    try:
        assignment.set_voxel_positions(64, 32, 64)
        e = assignment._engine
        orbit = camera.orbit(2, 4500.0, 25.0, 90.0, 61, 83)
        rec = e.fetch_records().copy()
        got = assignment.render_views(orbit, 83, 61, textured=True, texture_steps=6)
        want = e.render_textured(orbit, 61, 83, steps=6)
        for k in ("rgb", "rgb_voxels", "depth", "depth_voxels", "count", "best_cam", "refined", "index"):
            assert np.array_equal(got[k], want[k]), k
        assert got["texture_stats"]["textured"] > 0 and not np.array_equal(got["rgb"], got["rgb_voxels"])
        assert np.array_equal(got["rgb_voxels"], e.render(orbit, 61, 83)["rgb"])
        assert np.array_equal(e.fetch_records(), rec)                              # no hidden side effect on the records
        with pytest.raises(ValueError, match="textured"):
            assignment.render_views(orbit, 83, 61, textured=True, smooth=True)
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), color_mode="camera")
        assignment.set_voxel_positions(64, 32, 64)
        with pytest.raises(ValueError, match="visible"):
            assignment.render_views(orbit, 83, 61, textured=True)
        with pytest.raises(_lib.VoxcarveError, match="color_visible"):     # no colouring by visibility ran on this hull
            assignment._engine.render_textured(orbit, 61, 83)
    finally:
        assignment.configure(frame_source=None, **saved)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "views"
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "demo.py"), "64", "-", "--render", str(out), "--textured"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "textured:" in r.stdout and len(os.listdir(out)) == 12
    assert all(os.path.getsize(os.path.join(out, f)) > 1000 for f in os.listdir(out))
