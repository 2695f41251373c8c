"""The ray caster on the device (vc_render, vc_fetch_render; csrc/vc_render.h) against the restatement (tests/render_np.py):
index, depth (as bits), face and colour bit for bit -- the real cameras with their distortion and orbit views at 64^3 and 128^3 in
both carve modes, after color_visible, photo_carve (a view into the pit) and filter_components, grids whose columns straddle
occupancy words, a camera inside the grid, axis-aligned views, the empty and the solid hull, 1024^3 (the bench's workload) on
sampled pixels; every refusal, the fetch rules, the images' lifetime, the stats, render_views and silhouette_agreement."""
import ctypes
import math

import numpy as np
import pytest

import fixtures_util as fx
import render_np as rn
from voxcarve import _lib, camera, synthetic

pytestmark = pytest.mark.gpu

SHADE = (200, 190, 225, 215, 255, 150, 240)
BG = (9, 8, 7)


@pytest.fixture(scope="module")
def reng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _setup(e, grid, cams, masks, frames=None, bounds=None):
    H, W = masks[0].shape
    if bounds is None:
        e.set_grid(*grid)
    else:
        e.set_grid(*grid, bounds=bounds)
    e.set_cameras(cams, H, W)
    e.upload_masks(masks)
    if frames is not None:
        for c, f in enumerate(frames):
            e.upload_frame(c, f)


def _state(e):
    rec = e.fetch_records() if e.count else np.zeros(0, np.uint64)
    idx = (rec & np.uint64(0xffffffff)).astype(np.uint32)
    rgb = np.stack([(rec >> np.uint64(s)) & np.uint64(255) for s in (32, 40, 48)], 1).astype(np.uint8) if rec.size else \
        np.zeros((0, 3), np.uint8)
    return e.fetch_occupancy(), idx, rgb


def _check(e, views, H, W, pixels=None, shade=SHADE, bg=BG):
    """Device render of the current result against render_np (walk_blocks with 8^3 blocks: equal to the voxel walk, the CPU
    tests hold it to that); returns the device output."""
    got = e.render(views, H, W, shade=shade, background=bg)
    occ, idx, rgb = _state(e)
    want = rn.render(occ, idx, rgb, e.grid, e.bounds, [rn.view_params(v) for v in views], H, W, shade=shade, background=bg,
                     pixels=pixels, block=8)
    V = len(views)
    sel = (lambda a: a.reshape(V, H * W, *a.shape[3:])) if pixels is None else \
        (lambda a: a.reshape(V, H * W, *a.shape[3:])[:, np.asarray(pixels)])
    assert np.array_equal(sel(got["index"]), want["index"])
    assert np.array_equal(sel(got["depth"]).view(np.uint32), want["depth"].view(np.uint32))
    assert np.array_equal(sel(got["face"]), want["face"])
    assert np.array_equal(sel(got["rgb"]), want["rgb"])
    st = got["stats"]
    assert st["pixels"] == V * H * W
    assert st["hits"] == int((got["index"] != rn.MISS).sum())
    if pixels is None:
        assert st["hits"] == int((want["index"] != rn.MISS).sum())
    return got


def _orbit(n=6, H=240, W=320, radius=4000.0, el=25.0, centre=synthetic.VOLUME_CENTRE):
    return camera.orbit(n, radius, el, 0.9 * W, H, W, centre=centre)


@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("mode", ["fused", "lut"])
def test_real_cameras_and_orbits_equal_restatement(reng, cams, masks, frames, n, mode):
    _setup(reng, (n, n, n), cams, masks, frames)
    if mode == "lut":
        reng.build_lut()
    assert reng.carve(mode=mode) > 0
    H, W = masks[0].shape
    got = _check(reng, cams, H, W)
    assert got["stats"]["hits"] > 0.01 * got["stats"]["pixels"]
    _check(reng, _orbit(), 240, 320)


def test_after_color_visible_and_filter_components(reng, cams, masks, frames):
    _setup(reng, (64, 64, 64), cams, masks, frames)
    reng.carve()
    reng.color_visible()
    _check(reng, cams[:2], *masks[0].shape)
    st = reng.filter_components(min_voxels=50)
    assert st["survivors_after"] < st["survivors_before"]
    _check(reng, _orbit(3), 240, 320)


def test_after_photo_carve_view_into_the_pit(reng):
    H, W = 240, 320
    ring = synthetic.ring_cameras(8, H, W)
    ctr, half = np.array(synthetic.VOLUME_CENTRE), 1.15 * np.array(synthetic.PIT_HALF)
    masks, frames = synthetic.textured_scene(ring, H, W)
    lo, hi = ctr - half, ctr + half
    _setup(reng, (64, 64, 64), ring, masks, frames, bounds=(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))
    reng.carve()
    before = reng.render([camera.look_at(ctr + (150.0, 100.0, -2500.0), ctr, 600.0, H, W)], H, W)["depth"]
    st = reng.photo_carve(max_rounds=32)
    assert st["survivors_after"] < st["survivors_before"]
    into = camera.look_at(ctr + (150.0, 100.0, -2500.0), ctr, 600.0, H, W)      # from above (up is -z), into the pit
    got = _check(reng, [into] + ring[:2], H, W)
    assert (got["depth"][0] > before[0]).sum() > 50                              # the pit is deeper than the visual hull


def test_non_cubic_grids_inside_camera_axis_views(reng, cams, masks, frames):
    H, W = masks[0].shape
    ctr = np.array(synthetic.VOLUME_CENTRE)
    for grid in ((40, 72, 24), (33, 97, 18), (8, 130, 9)):
        _setup(reng, grid, cams, masks, frames)
        reng.carve()
        inside = camera.look_at(ctr + (0.0, 0.0, 300.0), ctr + (900.0, 300.0, 200.0), 150.0, 120, 160)
        # cx, cy on a pixel centre: column 80 / row 60 have direction components of exactly 0
        ax = [camera.Camera(np.array([[200.0, 0, 80.5], [0, 200.0, 60.5], [0, 0, 1]]), np.zeros(5), None,
                            -(R @ (ctr - 5000.0 * R[2])), R=R)
              for R in (np.eye(3), np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]]), np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]))]
        _check(reng, [inside] + ax + cams[:1], 120, 160)


def test_empty_and_solid_hull(reng, cams, masks, frames):
    H, W = masks[0].shape
    _setup(reng, (48, 48, 48), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert reng.carve() == 0
    got = _check(reng, _orbit(2), 60, 80)
    assert got["stats"]["hits"] == 0 and (got["rgb"] == BG).all() and np.isinf(got["depth"]).all()
    # solid: every mask full, the grid on the box of the real hull (every camera sees all of it)
    _setup(reng, (64, 64, 64), cams, masks, frames)
    reng.carve()
    idx, _, _ = reng.fetch()
    keys = np.stack(np.unravel_index(idx, (64, 64, 64)), 1)                      # (iz, ix, iy)
    xs, ys, zs = reng.axes()
    lo = np.array([xs[keys[:, 1].min()], ys[keys[:, 2].min()], zs[keys[:, 0].min()]])
    hi = np.array([xs[keys[:, 1].max()], ys[keys[:, 2].max()], zs[keys[:, 0].max()]])
    _setup(reng, (48, 48, 48), cams, [np.full((H, W), 255, np.uint8)] * 4, frames,
           bounds=(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))
    assert reng.carve() == 48 ** 3
    ctr = (lo + hi) / 2
    got = _check(reng, _orbit(2, 60, 80, centre=ctr) + [camera.look_at(ctr, ctr + (1.0, 2.0, 3.0), 40.0, 60, 80)], 60, 80)
    assert (got["face"][2] == 6).all() and (got["depth"][2] == 0).all()


def test_1024_cubed_one_1080p_view_sampled(reng, cams, masks, frames):
    _setup(reng, (1024, 1024, 1024), cams, masks, frames)
    assert reng.carve() > 10 ** 6
    H, W = 1080, 1920
    view = _orbit(1, H, W, radius=4500.0)[0]
    rng = np.random.default_rng(5)
    pix = np.concatenate([rng.integers(0, H * W, 4096), 540 * W + np.arange(W), np.arange(H) * W + 960])
    got = _check(reng, [view], H, W, pixels=pix)
    assert got["stats"]["hits"] > 10 ** 5


def test_block_skipping_off_gives_the_same_images(reng, cams, masks, frames):
    _setup(reng, (128, 128, 128), cams, masks, frames)
    reng.carve()
    views = _orbit(2)
    a = reng.render(views, 240, 320, shade=SHADE)
    reng.set_option("render_blocks", 0)
    try:
        b = reng.render(views, 240, 320, shade=SHADE)
    finally:
        reng.set_option("render_blocks", 1)
    for k in ("index", "face", "rgb"):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))
    assert b["stats"]["blocks_skipped"] == 0 and a["stats"]["blocks_skipped"] > 0
    assert b["stats"]["cells_visited"] > a["stats"]["cells_visited"]


def _raw(e, views, H, W, flags=0, n=None):
    arr = (_lib.VcView * max(len(views), 1))()
    for k, v in enumerate(views):
        arr[k].K[:] = list(v[0]); arr[k].dist[:] = list(v[1]); arr[k].R[:] = list(v[2]); arr[k].t[:] = list(v[3])
    return e._L.vc_render(e._ctx, len(views) if n is None else n, ctypes.cast(arr, ctypes.c_void_p), H, W, None, None, flags, None)


def test_refusals_fetch_rules_and_lifetime(built, cams, masks, frames):
    import voxcarve
    H, W = masks[0].shape
    good = rn.view_params(_orbit(1)[0])
    with voxcarve.CarveEngine(0) as e:
        buf = np.empty(4, np.uint32)
        assert e._L.vc_fetch_render(e._ctx, 0, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, None, None) == -1
        assert _raw(e, [good], 2, 2) == -1                                           # no carve result
        _setup(e, (32, 32, 32), cams, masks, frames)
        assert _raw(e, [good], 2, 2) == -1
        e.carve(viewmask=False, records=False)
        assert _raw(e, [good], 2, 2) == -1                                           # VC_FLAG_NO_RECORDS
        e.carve()
        e.carve_begin()
        assert _raw(e, [good], 2, 2) == -1                                           # a step in flight
        e.carve_end()
        assert _raw(e, [good], 2, 2) == 0
        for H_, W_ in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
            assert _raw(e, [good], H_, W_) == -1
        assert _raw(e, [good] * 2, 16384, 8193) == -1                                # more than 2^28 pixels
        assert _raw(e, [], 4, 4, n=0) == -1
        assert _raw(e, [good], 4, 4, flags=1) == -1
        for j, bad in ((0, 0.0), (1, -1.0), (0, math.nan), (5, math.inf)):
            K4, d5, R9, t3 = (np.array(a, dtype=np.float64) for a in good)
            flat = np.concatenate([K4, d5, R9, t3])
            flat[j] = bad
            assert _raw(e, [(flat[:4], flat[4:9], flat[9:18], flat[18:])], 4, 4) == -1
        with pytest.raises(ValueError):
            skew = camera.look_at((0.0, 0.0, -4000.0), synthetic.VOLUME_CENTRE, 100.0, 8, 8)
            skew.K[0, 1] = 0.5
            e.render([skew], 8, 8)
        e.set_slab(0, 16)
        e.carve()
        assert _raw(e, [good], 4, 4) == -1                                           # slab narrower than the grid
        e.set_grid(32, 1, 32)
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.carve()
        assert _raw(e, [good], 4, 4) == -1                                           # an axis shorter than 2
        # images survive refusals and a new carve; a second render replaces them; fetch beyond n_views fails
        _setup(e, (32, 32, 32), cams, masks, frames)
        e.carve()
        views = _orbit(2, 30, 40)
        first = e.render(views, 30, 40)
        assert _raw(e, [good], 4, 4, flags=1) == -1
        e.upload_masks([np.zeros((H, W), np.uint8)] * 4)
        assert e.carve() == 0
        again = np.empty((30, 40), np.uint32)
        e._check(e._L.vc_fetch_render(e._ctx, 1, again.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, None, None), "fetch")
        assert np.array_equal(again, first["index"][1]) and (again != rn.MISS).any()
        assert e._L.vc_fetch_render(e._ctx, 2, again.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, None, None) == -1
        second = e.render(views[:1], 30, 40)
        assert (second["index"] == rn.MISS).all()
        assert e._L.vc_fetch_render(e._ctx, 1, again.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, None, None) == -1


def test_render_views_after_configure(built, cams, masks, frames):
    from voxcarve import assignment
    H, W = masks[0].shape
    saved = dict(assignment._settings)                   # configure() keeps its settings: put them back afterwards
    assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]),
                         data_path=fx.GOLDEN + "/data", hull="photo", min_component_voxels=20)
    try:
        assignment.set_voxel_positions(64, 32, 64)
        e = assignment._engine
        got = assignment.render_views()
        want = e.render(e.cameras, H, W)
        for k in ("index", "depth", "face", "rgb"):
            assert np.array_equal(got[k], want[k])
        occ, idx, rgb = _state(e)
        ref = rn.render(occ, idx, rgb, e.grid, e.bounds, [rn.view_params(v) for v in e.cameras], H, W, block=8)
        assert np.array_equal(got["index"].reshape(4, -1), ref["index"])
        orb = _orbit(2)
        assert np.array_equal(assignment.render_views(orb, 320, 240)["rgb"], e.render(orb, 240, 320)["rgb"])
    finally:
        assignment.configure(frame_source=None, **saved)


def test_silhouette_agreement(reng, cams, masks, frames):
    _setup(reng, (128, 128, 128), cams, masks, frames)
    reng.carve()
    got = reng.silhouette_agreement()
    H, W = masks[0].shape
    idx = reng.render(cams, H, W)["index"]
    assert len(got) == 4
    for c in range(4):
        m = reng.fetch_mask(c) > 0
        h = idx[c] != rn.MISS
        b = int((m & h).sum())
        assert got[c] == {"mask_px": int(m.sum()), "hull_px": int(h.sum()), "both": b,
                          "iou": b / (int(m.sum()) + int(h.sum()) - b)}
        assert 0.5 < got[c]["iou"] <= 1.0
