"""The lit pass on the device (vc_light_render, vc_fetch_lit; csrc/vc_light.h) against the restatement (tests/light_np.py): rgb,
depth (as bits), kind, shadow, ao and the contract's counts, bit for bit.  The restatement is given the device's own render
(tests/test_gpu_render.py holds that one to render_np) and the device's records and normals.  Views are 64 x 48 and compared
whole; the four calibrated views at 486 x 644 are compared on a sample of their pixels (every pixel costs the restatement 17
walks), their counts against the device's own images."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures_util as fx
import light_np as ln
import render_np as rn
from voxcarve import _lib, camera, lighting, synthetic

pytestmark = pytest.mark.gpu

SHADE = (200, 190, 225, 215, 255, 150, 240)
BG = (9, 8, 7)
H0, W0 = 48, 64
CTR = np.array(synthetic.VOLUME_CENTRE)
KEYS = ("rgb", "depth", "kind", "shadow", "ao")
COUNTS = ("pixels", "hull_pixels", "floor_pixels", "shadowed", "facing_away", "rays_walked")
POINT = (900.0, -1400.0, -2600.0, 1.0)
SUN = (0.35, -0.5, -1.0, 0.0)


@pytest.fixture(scope="module")
def leng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _setup(e, grid, cams, masks, frames, bounds=None):
    H, W = masks[0].shape
    e.set_grid(*grid) if bounds is None else e.set_grid(*grid, bounds=bounds)
    e.set_cameras(cams, H, W)
    e.upload_masks(masks)
    for c, f in enumerate(frames):
        e.upload_frame(c, f)


def _orbit(n=3, radius=3200.0, el=25.0, centre=synthetic.VOLUME_CENTRE):
    return camera.orbit(n, radius, el, 0.9 * W0, H0, W0, centre=centre)


def _state(e):
    rec = e.fetch_records() if e.count else np.zeros(0, np.uint64)
    idx = (rec & np.uint64(0xffffffff)).astype(np.uint32)
    rgb = np.stack([(rec >> np.uint64(s)) & np.uint64(255) for s in (32, 40, 48)], 1).astype(np.uint8) if rec.size else \
        np.zeros((0, 3), np.uint8)
    return e.fetch_occupancy(), idx, rgb


def _floor(e, z=None):
    fl = lighting.auto_floor(e.grid, e.bounds)
    return dict(fl, z=fl["z"] if z is None else z, cell_mm=170.0, rgb=((70, 80, 90), (210, 200, 190)))


def _check(e, views, H, W, pos, smooth=0, floor=None, ambient=64, ao_reach=4.0, sample=None):
    """render + light_render on the device against light_np on the device's render; returns (device output, restatement)."""
    ren = e.render(views, H, W, shade=SHADE, background=BG)
    n4 = None
    if smooth:
        if not e.normals_valid():
            e.hull_normals()
        n4 = e.fetch_record_normals()
    got = e.light_render(pos, ambient=ambient, smooth=bool(smooth), ao_reach=ao_reach, floor=floor)
    occ, idx, rgb = _state(e)
    V = len(views)
    flat = lambda a: a.reshape(V, H * W, *a.shape[3:])
    pixels = None
    if sample is not None:                                   # hits and misses alike, the same pixels in every view
        rng = np.random.default_rng(sample)
        hit = np.flatnonzero((flat(ren["index"]) != rn.MISS).any(axis=0))
        pixels = np.unique(np.concatenate([rng.choice(hit, min(4000, hit.size), replace=False), rng.integers(0, H * W, 4000),
                                            np.arange(H * W - 256, H * W)]))      # (the tail of the last block of pixels too)
    sel = flat if pixels is None else (lambda a: flat(a)[:, pixels])
    lt = {"pos": pos, "ambient": ambient, "smooth": smooth, "ao_reach": ao_reach, "floor": floor}
    want = ln.light(occ, idx, rgb, n4, e.grid, e.bounds, [rn.view_params(v) for v in views], H, W,
                    {k: sel(ren[k]) for k in ("index", "depth", "face", "rgb")}, lt, pixels=pixels)
    for k in KEYS:
        a, b = sel(got[k]), want[k]
        if k == "depth":
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), (k, int((a != b).sum()), a.size)
    st = got["stats"]
    if pixels is None:
        assert {k: st[k] for k in COUNTS} == want["stats"], (st, want["stats"])
    cast = (got["kind"] == 2) | ((got["kind"] == 1) & (ren["face"] != 6))
    assert st["pixels"] == V * H * W and st["hull_pixels"] == int((got["kind"] == 1).sum())
    assert st["floor_pixels"] == int((got["kind"] == 2).sum())
    assert st["shadowed"] == int((got["shadow"] == 1).sum()) and st["facing_away"] == int((got["shadow"] == 2).sum())
    assert st["rays_walked"] == int((cast & (got["shadow"] != 2)).sum()) + (16 * int(cast.sum()) if ao_reach > 0 else 0)
    again = np.empty((H, W), np.uint32)                      # the render's images are left alone
    e._check(e._L.vc_fetch_render(e._ctx, 0, again.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, None, None), "vc_fetch_render")
    assert np.array_equal(again, ren["index"][0])
    return got, want


_carved = {}


def _carve64(e, cams, masks, frames, mode):
    """The 64^3 hull of the real cameras in `mode`, carved once per mode for the cases below."""
    if _carved.get("mode") != mode:
        _setup(e, (64, 64, 64), cams, masks, frames)
        if mode == "lut":
            e.build_lut()
        assert e.carve(mode=mode) > 0
        _carved["mode"] = mode


@pytest.mark.parametrize("pos,smooth,floor", [(POINT, 0, True), (SUN, 1, False), (POINT, 1, False), (SUN, 0, True)],
                         ids=["point-flat-floor", "sun-smooth", "point-smooth", "sun-flat-floor"])
@pytest.mark.parametrize("mode", ["fused", "lut"])
def test_real_cameras_orbit_views(leng, cams, masks, frames, mode, pos, smooth, floor):
    _carve64(leng, cams, masks, frames, mode)
    got, _ = _check(leng, _orbit(), H0, W0, pos, smooth=smooth, floor=_floor(leng) if floor else None)
    st = got["stats"]
    assert st["hull_pixels"] > 100 and st["shadowed"] > 0 and st["facing_away"] > 0 and (got["ao"] < 16).any()
    assert (st["floor_pixels"] > 1000) == bool(floor)
    assert st["cells_visited"] > 0 and st["blocks_skipped"] > 0


@pytest.mark.parametrize("mode", ["fused", "lut"])
def test_real_cameras_calibrated_views_sampled(leng, cams, masks, frames, mode):
    _carve64(leng, cams, masks, frames, mode)
    H, W = masks[0].shape
    got, _ = _check(leng, cams, H, W, POINT, smooth=1, floor=_floor(leng), sample=17)
    assert got["stats"]["hull_pixels"] > 0.01 * got["stats"]["pixels"] and got["stats"]["floor_pixels"] > 0


@pytest.mark.parametrize("grid", [(33, 97, 18), (8, 130, 9)])
def test_grids_whose_strides_and_blocks_do_not_line_up(leng, cams, masks, frames, grid):
    _carved.clear()
    _setup(leng, grid, cams, masks, frames)
    assert leng.carve() > 0
    got, _ = _check(leng, _orbit(), H0, W0, POINT, floor=_floor(leng), ao_reach=6.0)
    assert got["stats"]["hull_pixels"] > 50 and (got["ao"] < 16).any()
    leng.hull_normals(radius_mm=14.0 * min(rn.grid_params(leng.grid, leng.bounds)[1]))         # (the default ball is too long for y)
    _check(leng, _orbit(2, el=60.0), H0, W0, SUN, smooth=1)
    # 2 x 61 x 83 pixels are no multiple of a block of 256, of a wave or of a group of 16 listed pixels: whole, counts included
    _check(leng, camera.orbit(2, 3200.0, 25.0, 75.0, 61, 83, centre=synthetic.VOLUME_CENTRE), 61, 83, POINT, floor=_floor(leng))


def test_floor_planes_cameras_and_lights(leng, cams, masks, frames):
    """A floor outside the grid and one cutting through it, a camera below the floor, one inside the grid and one inside a survivor, lights
    inside the grid -- between a surface and what shadows it (the t < 1 rule), and one voxel off the surface --, lights with direction components of exactly 0."""
    e = leng
    _carve64(e, cams, masks, frames, "fused")
    zmax = lighting.auto_floor(e.grid, e.bounds)["z"]
    views = _orbit()
    got, _ = _check(e, views, H0, W0, POINT, floor=_floor(e, z=zmax + 400.0))                   # outside, under the grid
    assert got["stats"]["floor_pixels"] > 500
    got, _ = _check(e, views, H0, W0, SUN, floor=_floor(e, z=float(CTR[2])))                    # through the hull
    assert got["stats"]["floor_pixels"] > 500 and ((got["kind"] == 2) & (got["shadow"] == 1) & (got["ao"] == 0)).any()
    below = camera.look_at(CTR + (1500.0, 900.0, 3500.0), CTR, 0.9 * W0, H0, W0)              # under the floor, looking up
    got, _ = _check(e, [below], H0, W0, (0.2, 0.1, 1.0, 0.0), floor=_floor(e))
    assert got["stats"]["floor_pixels"] > 200 and (got["shadow"][got["kind"] == 2] != 2).all()
    inside = camera.look_at((900.0, 800.0, -900.0), CTR, 30.0, H0, W0)                          # in the grid's empty space
    got, _ = _check(e, [inside], H0, W0, POINT, floor=_floor(e))
    assert got["stats"]["hull_pixels"] > 100 and got["stats"]["rays_walked"] > 0
    buried = camera.look_at(CTR + (0.0, 0.0, 300.0), CTR + (900.0, 300.0, 200.0), 30.0, H0, W0) # in a survivor: face 6
    got, _ = _check(e, [buried], H0, W0, POINT, floor=_floor(e))
    assert (got["kind"] == 1).all() and got["stats"]["rays_walked"] == 0 and (got["ao"] == 16).all()
    # a point light between a surface point and what shadows it under the sun: the walk hits beyond the light, t >= 1
    n, step, _ = rn.grid_params(e.grid, e.bounds)
    occ = e.fetch_occupancy()
    o, d = rn.pixel_rays(rn.view_params(views[0]), H0, W0)
    sun = np.array(SUN[:3])

    def starts(ren, pix):
        """Points and start cells (items 1 and 2) of hull pixels of view 0."""
        Q = o[None, :] + ren["depth"][0].reshape(-1)[pix, None].astype(np.float64) * d[pix]
        i = ren["index"][0].reshape(-1)[pix].astype(np.int64)
        c0 = np.stack([(i // n[1]) % n[0], i % n[1], i // (n[0] * n[1])], axis=1)
        f = ren["face"][0].reshape(-1)[pix].astype(np.int64)
        c0[np.arange(pix.size), f // 2] += np.where(f % 2 == 0, -1, 1)
        return Q, c0

    ren = e.render(views, H0, W0, shade=SHADE, background=BG)
    _, want = _check(e, views, H0, W0, SUN, ao_reach=0.0)
    dark = np.flatnonzero((want["kind"][0] == 1) & (want["shadow"][0] == 1))
    Q, c0 = starts(ren, dark)
    hit, t = ln.secondary(occ, e.grid, e.bounds, Q, np.broadcast_to(sun, Q.shape), c0)
    assert hit.all()
    k = int(np.argmax(t))
    near = tuple(float(v) for v in Q[k] + 0.5 * t[k] * sun) + (1.0,)
    f = int(ren["face"][0].reshape(-1)[dark[k]])
    off = np.zeros(3)
    off[f // 2] = (-1.0 if f % 2 == 0 else 1.0) * step[f // 2]
    _check(e, views, H0, W0, tuple(float(v) for v in Q[k] + off) + (1.0,), ao_reach=2.0)       # one voxel off the surface
    _, want = _check(e, views, H0, W0, near, ao_reach=0.0)
    lit = np.flatnonzero((want["kind"][0] == 1) & (want["shadow"][0] == 0))
    assert dark[k] in lit
    Q, c0 = starts(ren, lit)
    hit, t = ln.secondary(occ, e.grid, e.bounds, Q, np.array(near[:3])[None, :] - Q, c0)
    assert (hit & (t >= 1.0)).any()                                                            # lit although the walk hits
    for zero in ((0.0, 0.5, -1.0, 0.0), (0.0, 0.0, -1.0, 0.0), (1.0, 0.0, 0.0, 0.0)):
        _check(e, views[:2], H0, W0, zero, floor=_floor(e))


def test_empty_and_solid_hull_and_a_camera_inside_a_survivor(leng, cams, masks, frames):
    e = leng
    _carved.clear()
    H, W = masks[0].shape
    _setup(e, (48, 48, 48), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert e.carve() == 0
    got, _ = _check(e, _orbit(2), H0, W0, POINT, floor=_floor(e))
    assert got["stats"]["hull_pixels"] == 0 and got["stats"]["shadowed"] == 0 and got["stats"]["floor_pixels"] > 0
    got, _ = _check(e, _orbit(2), H0, W0, SUN)
    assert (got["rgb"] == BG).all() and got["stats"]["rays_walked"] == 0
    lo, hi = CTR - 400.0, CTR + 400.0
    _setup(e, (24, 24, 24), cams, [np.full((H, W), 255, np.uint8)] * 4, frames, bounds=(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))
    assert e.carve() == 24 ** 3
    views = _orbit(2, centre=tuple(CTR)) + [camera.look_at(CTR, CTR + (1.0, 2.0, 3.0), 40.0, H0, W0)]
    got, _ = _check(e, views, H0, W0, POINT, floor=_floor(e))
    assert (got["ao"][got["kind"] == 1] == 16).all()                                            # every start cell is outside
    assert (got["kind"][2] == 1).all() and (got["shadow"][2] == 0).all() and (got["ao"][2] == 16).all()   # face 6
    assert np.array_equal(got["rgb"][2], e.render(views, H0, W0, shade=SHADE, background=BG)["rgb"][2])


def test_after_color_visible_and_filter_components(leng, cams, masks, frames):
    e = leng
    _carve64(e, cams, masks, frames, "fused")
    _carved.clear()
    views = _orbit(2)
    before, _ = _check(e, views, H0, W0, SUN)
    e.color_visible()
    after, _ = _check(e, views, H0, W0, SUN)                                                    # the colours follow the records
    assert not np.array_equal(before["rgb"], after["rgb"]) and np.array_equal(before["shadow"], after["shadow"])
    st = e.filter_components(min_voxels=50)
    assert st["survivors_after"] < st["survivors_before"]
    _check(e, views, H0, W0, POINT, smooth=1, floor=_floor(e))


def test_block_skipping_off_gives_the_same_images(leng, cams, masks, frames):
    e = leng
    _carve64(e, cams, masks, frames, "fused")
    views = _orbit(2)
    a, _ = _check(e, views, H0, W0, POINT, floor=_floor(e), ao_reach=30.0)
    e.set_option("render_blocks", 0)
    try:
        b, _ = _check(e, views, H0, W0, POINT, floor=_floor(e), ao_reach=30.0)
        e.set_option("render_blocks", 1)
        c = e.light_render(POINT, floor=_floor(e), ao_reach=30.0)          # on a render made without the map: built here
    finally:
        e.set_option("render_blocks", 1)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert b["stats"]["blocks_skipped"] == 0 and a["stats"]["blocks_skipped"] > 0 and c["stats"]["blocks_skipped"] > 0
    assert b["stats"]["cells_visited"] > a["stats"]["cells_visited"] == c["stats"]["cells_visited"]


def test_refusals_fetch_rules_and_lifetime(built, cams, masks, frames):
    import voxcarve
    L = _lib.load()
    orbit = _orbit(2)
    n = H0 * W0

    def raw(e, stats=True, flags=0, light=True, pos=POINT, smooth=0, ao_reach=4.0, floor=None):
        lt = lighting.light_struct(pos, 64, smooth, ao_reach, floor, e.grid, e.bounds)
        st = lighting.LightStats()
        return L.vc_light_render(e._ctx, ctypes.byref(lt) if light else None, flags, ctypes.byref(st) if stats else None)

    def fetch(e, view=1):
        rgb, depth, kind, sh, ao = (np.empty(n * 3, np.uint8), np.empty(n, np.float32), np.empty(n, np.uint8), np.empty(n, np.uint8),
                                    np.empty(n, np.uint8))
        u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        rc = L.vc_fetch_lit(e._ctx, view, u8(rgb), depth.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), u8(kind), u8(sh), u8(ao))
        return rc, tuple(a.tobytes() for a in (rgb, depth, kind, sh, ao))

    def refused(e, before, what, **kw):
        assert raw(e, **kw) == -1, kw
        assert what in L.vc_last_error(e._ctx).decode(), (kw, L.vc_last_error(e._ctx).decode())
        if before is not None:
            assert fetch(e) == (0, before), kw

    with voxcarve.CarveEngine(0) as e:
        assert L.vc_fetch_lit(e._ctx, 0, None, None, None, None, None) == -1
        _setup(e, (32, 32, 32), cams, masks, frames)
        refused(e, None, "no carve result")
        e.carve()
        refused(e, None, "vc_render")                                                # no render yet
        e.render(orbit, H0, W0)
        assert L.vc_fetch_lit(e._ctx, 0, None, None, None, None, None) == -1        # before the first call
        refused(e, None, "normals", smooth=1)                                        # no normals at all
        floor = _floor(e)
        assert raw(e, floor=floor) == 0
        assert L.vc_fetch_lit(e._ctx, 0, None, None, None, None, None) == 0
        assert L.vc_fetch_lit(e._ctx, 2, None, None, None, None, None) == -1
        s = fetch(e)[1]
        refused(e, s, "stats", stats=False)
        refused(e, s, "no light", light=False)
        refused(e, s, "flags", flags=1)
        for bad in (float("nan"), float("inf")):
            refused(e, s, "not finite", pos=(bad, 0.0, 0.0, 1.0))
            refused(e, s, "ao_reach", ao_reach=bad)
            refused(e, s, "floor_z", floor=dict(floor, z=bad))
            refused(e, s, "rectangle", floor=dict(floor, rect=(0.0, bad, 0.0, 1.0)))
            refused(e, s, "cells", floor=dict(floor, cell_mm=bad))
        refused(e, s, "pos[3]", pos=(0.0, 0.0, 0.0, 0.5))
        refused(e, s, "squared length", pos=(0.0, 0.0, 0.0, 0.0))
        refused(e, s, "ao_reach", ao_reach=-1.0)
        refused(e, s, "empty", floor=dict(floor, rect=(5.0, 4.0, 0.0, 1.0)))
        refused(e, s, "cells", floor=dict(floor, cell_mm=0.0))
        refused(e, s, "cells", floor=dict(floor, cell_mm=1e-300))
        for k, v in (("ambient", 256), ("smooth", 2), ("floor", 2)):           # (what light_struct itself would not pass on)
            lt = lighting.light_struct(POINT, 64, 0, 4.0, None)
            setattr(lt, k, v)
            st = lighting.LightStats()
            assert L.vc_light_render(e._ctx, ctypes.byref(lt), 0, ctypes.byref(st)) == -1 and k in L.vc_last_error(e._ctx).decode()
            assert fetch(e) == (0, s)
        e.hull_normals()
        assert raw(e, smooth=1, floor=floor) == 0
        s = fetch(e)[1]
        e.carve_begin()
        refused(e, None, "in flight")
        e.carve_end()
        refused(e, None, "vc_render")                                                # a new result: the render is stale
        assert fetch(e) == (0, s)                                                    # (the lit images stay)
        e.render(orbit, H0, W0)
        assert L.vc_fetch_lit(e._ctx, 0, None, None, None, None, None) == -1        # the new render dropped them
        refused(e, None, "normals", smooth=1)                                        # stale normals
        assert raw(e) == 0
        e.carve(records=False)
        refused(e, None, "VC_FLAG_NO_RECORDS")
        e.set_slab(0, 16)
        e.carve()
        refused(e, None, "slab")
    with pytest.raises(ValueError, match="ambient"):
        lighting.light_struct(POINT, 256, 0, 4.0, None)
    with pytest.raises(ValueError, match="floor"):
        lighting.light_struct(POINT, 64, 0, 4.0, "grid")


def test_assignment_and_demo_end_to_end(built, cams, masks, frames, tmp_path):
    from voxcarve import assignment
    saved = dict(assignment._settings)
    assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=fx.GOLDEN + "/data")
    try:
        assignment.set_voxel_positions(64, 32, 64)
        e = assignment._engine
        orbit = _orbit(2)
        rec = e.fetch_records().copy()
        got = assignment.render_views(orbit, W0, H0, lit=True)
        want = e.render_lit(orbit, H0, W0)
        for k in KEYS + ("rgb_flat", "depth_hull", "index", "face"):
            assert np.array_equal(got[k], want[k]), k
        auto = e.light_render(lighting.light_above(orbit[0]), floor="auto")
        assert np.array_equal(auto["rgb"], got["rgb"]) and got["light_stats"]["floor_pixels"] > 0
        assert not np.array_equal(got["rgb"], got["rgb_flat"]) and np.array_equal(got["rgb_flat"], e.render(orbit, H0, W0)["rgb"])
        assert np.array_equal(e.fetch_records(), rec)
        smooth = assignment.render_views(orbit, W0, H0, lit=True, smooth=True, light=SUN, floor=None)
        assert smooth["light_stats"]["floor_pixels"] == 0 and e.normals_valid()
        with pytest.raises(ValueError, match="textured"):
            assignment.render_views(orbit, W0, H0, lit=True, textured=True)
        with pytest.raises(ValueError, match="shade"):
            assignment.render_views(orbit, W0, H0, lit=True, shade=SHADE)
    finally:
        assignment.configure(frame_source=None, **saved)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "views"
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "demo.py"), "64", "-", "--render", str(out), "--lit"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "lit:" in r.stdout and len(os.listdir(out)) == 12
    assert all(os.path.getsize(os.path.join(out, f)) > 1000 for f in os.listdir(out))
