"""The hull's surface normals on the device (vc_hull_normals, vc_fetch_record_normals; csrc/vc_normals.h) against the restatement
(tests/normals_np.py), bit for bit on every int16 quadruple and on the stats: the real cameras at 64^3 and 128^3 in both carve
modes at 2 x and 3 x the largest step, the ball at its cap of 15 cells, random scenes whose hulls touch the grid faces on grids
whose y lines straddle occupancy words, the solid grid, the empty hull, a single voxel; after the passes that change the hull;
every refusal; 1024^3 on crops.  The consumers: vc_shade_render against the restatement's float64 shading, vc_surface_normals
against the ON elements of tests/surface_np.py, write_ply with normals, assignment.render_views(smooth=True),
assignment.surface_mesh(normals=True) and demo.py --smooth / --normals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import normals_np as nn
import surface_np as sn

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def neng(built):
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
        e.upload_frame(1, frames[1])


def _hull(e):
    rec = e.fetch_records().copy()
    idx = (rec & LOW).astype(np.uint32)
    return rec, idx, dn.volume(idx, e.grid), dn.steps_um(e.grid, e.bounds)


def _rgb(rec):
    return np.stack([(rec >> np.uint64(s)) & np.uint64(255) for s in (32, 40, 48)], 1).astype(np.uint8)


def _check_normals(e, radius_mm=None):
    """hull_normals over the current result: every quadruple and the stats against the restatement; the result is left alone."""
    rec, idx, occ, q = _hull(e)
    r2 = nn.default_r2(q) if radius_mm is None else dn.radius_r2(radius_mm)
    st = e.hull_normals(radius_mm)
    want, ws = nn.normals(occ, q, r2)
    got = e.fetch_record_normals()
    assert got.dtype == np.int16 and got.shape == (idx.size, 4)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%d of %d quadruples differ, first at record %d: %r, want %r" % (bad.size, idx.size, bad[0], got[bad[0]], want[bad[0]])
    for k in ("survivors", "surface", "zero", "offsets", "ext", "q"):
        assert st[k] == ws[k], k
    assert np.array_equal(e.fetch_records(), rec), "the pass leaves the result alone"
    assert np.array_equal(e.record_normals_unit(), nn.unit(want))
    return got, st


@pytest.mark.parametrize("mode", ["fused", "lut"])
@pytest.mark.parametrize("n", [64, 128])
def test_real_cameras_equal_restatement(neng, cams, masks, frames, n, mode):
    _setup(neng, (n, n, n), cams, masks, frames)
    if mode == "lut":
        neng.build_lut()
    S = neng.carve(mode=mode)
    assert np.array_equal(neng.fetch()[0], fx.expected(n)[0])
    big = max(dn.steps_um((n, n, n), neng.bounds))
    _, st3 = _check_normals(neng)                                # the default: 3 x the largest step
    assert st3["surface"] == {64: 2703, 128: 12462}[n] and st3["zero"] == 0 and st3["survivors"] == S
    if n == 128:
        assert st3["ext"] == (5, 3, 3) and st3["offsets"] == 222
    _, st2 = _check_normals(neng, 2 * big / 1000.0)
    assert st2["surface"] == st3["surface"] and st2["zero"] == {64: 1, 128: 2}[n]


def test_ball_at_the_cap(neng, cams, masks, frames):
    _setup(neng, (64, 64, 64), cams, masks, frames)
    neng.carve()
    _, st = _check_normals(neng, 366.0)
    assert st["ext"][0] == 15


@pytest.mark.parametrize("grid,seed,mv", [((37, 53, 29), 3, 1), ((37, 53, 29), 4, 2), ((20, 70, 33), 5, 1), ((9, 130, 12), 6, 1),
                                          ((12, 64, 10), 7, 2)])
def test_random_scenes_on_grids_that_straddle_words(neng, grid, seed, mv):
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    _setup(neng, grid, cams3, masks3, frames3)
    assert neng.carve(min_views=mv) > 0
    occ = neng.fetch_occupancy().reshape(grid[2], grid[0], grid[1])
    assert occ[0].any() or occ[-1].any() or occ[:, 0].any() or occ[:, -1].any() or occ[:, :, 0].any() or occ[:, :, -1].any()
    from voxcarve._lib import VoxcarveError
    q = dn.steps_um(grid, neng.bounds)
    checked = 0
    for mm in (None, 100, 250, 400):                             # (the steps of these grids are 16 to 290 mm)
        try:
            nn.ball(q, nn.default_r2(q) if mm is None else dn.radius_r2(mm))
        except ValueError:                                       # more than 15 cells along the fine axis: the device refuses it too
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*more than 15"):
                neng.hull_normals(mm)
            continue
        _check_normals(neng, mm)
        checked += 1
    assert checked >= 2


def test_solid_grid_empty_hull_single_voxel(neng, cams, masks, frames):
    H, W = masks[0].shape
    full = [np.full((H, W), 255, np.uint8)] * 4
    # a box that every camera sees whole (full masks alone do not fill a grid: a voxel outside an image does not survive)
    _setup(neng, (32, 48, 40), cams, full, frames, bounds=(0.0, 620.0, -470.0, 470.0, -1560.0, -780.0))
    assert neng.carve() == 32 * 48 * 40
    got, st = _check_normals(neng)
    assert st["surface"] == 32 * 48 * 40 - 30 * 46 * 38
    _check_normals(neng, 90)
    _setup(neng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert neng.carve() == 0
    got, st = _check_normals(neng)
    assert got.shape == (0, 4) and st["survivors"] == st["surface"] == st["zero"] == 0 and st["offsets"] > 0
    # a single voxel: in every camera's mask only the pixel under the centre of voxel 292 of an 8^3 grid is foreground
    from oracle import carve_np as cn
    pts = cn.points_of_indices(np.array([292]), 8, 8, 8)
    one = [np.zeros((H, W), np.uint8) for _ in cams]
    for c, cam in enumerate(cams):
        off = int(cn.pixel_offsets(cn.project_points(pts, cam.R, cam.tvec, cam.K, cam.dist), H, W)[0])
        assert off >= 0
        one[c].reshape(-1)[off] = 255
    _setup(neng, (8, 8, 8), cams, one, frames)
    assert neng.carve() == 1 and int(neng.fetch()[0][0]) == 292
    got, st = _check_normals(neng)
    assert got.tolist() == [[0, 0, 0, 1]] and st["surface"] == st["zero"] == 1


def test_after_the_passes_that_change_the_hull(neng, cams, masks, frames):
    from voxcarve._lib import VoxcarveError
    n = 128
    _setup(neng, (n, n, n), cams, masks, frames)
    for c in range(4):
        neng.upload_frame(c, frames[c])
    S = neng.carve()

    def stale():
        assert not neng.normals_valid()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no normals"):
            neng.fetch_record_normals()

    stale()
    before, _ = _check_normals(neng)
    assert neng.normals_valid()
    neng.color_visible()                                         # colours only: the normals stay
    assert neng.normals_valid() and np.array_equal(neng.fetch_record_normals(), before)
    neng.hull_distance()                                         # leaves the result alone
    assert np.array_equal(neng.fetch_record_normals(), before)
    assert neng.close_hull(0.0)["added"] == 0                    # a grow that adds nothing
    assert np.array_equal(neng.fetch_record_normals(), before)
    assert neng.photo_carve(max_rounds=2)["survivors_after"] < S
    stale()
    _check_normals(neng)
    neng.carve()
    stale()
    neng.hull_normals()
    assert neng.filter_components(keep_largest=1)["survivors_after"] < S
    stale()
    _check_normals(neng)
    neng.carve()
    neng.hull_normals()
    assert neng.open_hull(25)["survivors_after"] < S
    stale()
    _check_normals(neng)
    neng.carve()
    neng.hull_normals()
    assert neng.close_hull(40)["added"] > 0
    stale()
    _check_normals(neng)
    neng.hull_normals()
    neng.erode_hull(15)
    stale()
    neng.hull_normals()
    neng.dilate_hull(15)
    stale()


def test_refusals(built, cams, masks, frames):
    """Every refusal of the contract but one: a communicator of more than one rank needs two processes with a device each, and
    the message comes from the check the other post-carve passes share."""
    import voxcarve
    from voxcarve import camera
    from voxcarve._lib import VoxcarveError, VcNormalsStats
    H, W = masks[0].shape
    with voxcarve.CarveEngine(0) as e:
        e.set_grid(64, 64, 64)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.hull_normals()
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        S = e.carve()
        st = VcNormalsStats()
        L = e._L
        err = lambda: L.vc_last_error(e._ctx).decode()
        r2 = e.normals_r2()
        assert L.vc_hull_normals(e._ctx, r2, 1, ctypes.byref(st)) == -1 and "flags" in err()
        assert L.vc_hull_normals(e._ctx, r2, 0, None) == -1 and "stats" in err()
        q = dn.steps_um(e.grid, e.bounds)
        assert L.vc_hull_normals(e._ctx, (min(q) - 1) ** 2, 0, ctypes.byref(st)) == -1 and "no voxel offset" in err()
        assert L.vc_hull_normals(e._ctx, 0, 0, ctypes.byref(st)) == -1 and "no voxel offset" in err()
        assert L.vc_hull_normals(e._ctx, (16 * q[0]) ** 2, 0, ctypes.byref(st)) == -1 and "along x" in err()
        assert L.vc_hull_normals(e._ctx, (16 * q[0]) ** 2 - 1, 0, ctypes.byref(st)) == 0 and tuple(st.ext)[0] == 15
        assert L.vc_hull_normals(e._ctx, min(q) ** 2, 0, ctypes.byref(st)) == 0 and tuple(st.ext) == (1, 0, 0) and st.offsets == 2
        assert e.count == S and e.fetch_records().size == S
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                e.hull_normals(bad)
        # the consumers
        view = camera.orbit(1, 4000.0, 25.0, 100.0, 30, 40)
        light = np.array([[0.0, 0.0, -1.0]])
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no normals"):
            e.surface_normals()
        e.render(view, 30, 40)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no normals"):
            e.shade_render(light)
        e.hull_normals()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no mesh"):
            e.surface_normals()
        assert e.shade_render(light).shape == (1, 30, 40, 3)
        lp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert L.vc_shade_render(e._ctx, lp([0, 0, -1]), 256, 0) == -1 and "ambient" in err()
        assert L.vc_shade_render(e._ctx, lp([0, 0, -1]), 64, 1) == -1 and "flags" in err()
        assert L.vc_shade_render(e._ctx, None, 64, 0) == -1
        for bad in ([0, 0, float("nan")], [float("inf"), 0, 0], [0, 0, 0], [1e-170, 0, 0], [1e200, 0, 0]):
            assert L.vc_shade_render(e._ctx, lp(bad), 64, 0) == -1, bad
        with pytest.raises(ValueError):
            e.shade_render(np.zeros((2, 3)))
        with pytest.raises(ValueError):
            e.shade_render(light, ambient=300)
        rgb = np.empty((30, 40, 3), np.uint8)
        assert L.vc_fetch_shaded(e._ctx, 1, rgb.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == -1 and "view" in err()
        # a render or a mesh made before the hull changed is refused, with fresh normals too
        e.surface_mesh(2)
        assert e.surface_normals().shape[1] == 4
        e.open_hull(25)
        e.hull_normals()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no images of the current"):
            e.shade_render(light)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no mesh of the current"):
            e.surface_normals()
        assert e.render(view, 30, 40)["rgb"].shape == (1, 30, 40, 3)          # vc_fetch_render is untouched by all this
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no shaded images"):
            L_rgb = np.empty((1, 30, 40, 3), np.uint8)
            e._check(L.vc_fetch_shaded(e._ctx, 0, L_rgb.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "vc_fetch_shaded")
        e.carve()
        e.hull_normals()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no images of the current"):
            e.shade_render(light)
        # the refusals every pass over the result shares, and the metric's
        e.set_grid(64, 64, 64, bounds=(0, 63 * 1100.0, 0, 1, 0, 1))
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis x"):
            e.hull_normals()
        e.set_grid(64, 64, 1, bounds=(0, 100, 0, 100, 5, 5))
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis z"):
            e.hull_normals()
        e.set_grid(64, 64, 64)
        e.carve(records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.hull_normals()
        e.set_slab(0, 32)
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.hull_normals()
        e.set_slab(0, 64)
        e.carve_begin()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
            e.hull_normals()
        e.carve_end()
        assert e.hull_normals()["surface"] == 2703


CROP = 64


def test_bench_workload_1024_on_crops(neng, cams, masks, frames):
    """At 1024^3 the restatement runs on 8 crops of 64^3 cells around seeded survivors.  A normal depends on the ball's
    neighbourhood alone, so the crop's value is exact for every record whose ball lies inside the crop (or is cut by a face the
    crop shares with the grid); all of those are compared, and they must be at least half of the crops' surface records."""
    n = 1024
    _setup(neng, (n, n, n), cams, masks, frames)
    S = neng.carve()
    rec = neng.fetch_records()
    idx = (rec & LOW).astype(np.int64)
    q = dn.steps_um((n, n, n), neng.bounds)
    st = neng.hull_normals()
    dev = neng.fetch_record_normals()
    assert st["survivors"] == S and st["surface"] == int((dev[:, 3] == 1).sum()) > 0
    assert st["zero"] == int(((dev[:, 3] == 1) & ~dev[:, :3].any(axis=1)).sum())
    ext = st["ext"]
    assert ext == nn.ball(q, nn.default_r2(q))[0]
    iy, t = idx % n, idx // n
    ix, iz = t % n, t // n
    coords = (iz, ix, iy)
    reach = (ext[2], ext[0], ext[1])                             # the volume's axes: z, x, y
    rng = np.random.default_rng(1024)
    surface = covered = 0
    for s in rng.choice(S, 8, replace=False):
        c = (int(iz[s]), int(ix[s]), int(iy[s]))
        lo = [min(max(v - CROP // 2, 0), n - CROP) for v in c]
        hi = [l + CROP for l in lo]
        inside = np.ones(S, dtype=bool)
        for a in range(3):
            inside &= (coords[a] >= lo[a]) & (coords[a] < hi[a])
        rs = np.flatnonzero(inside)                              # ascending record order = ascending index inside the crop too
        loc = [coords[a][rs] - lo[a] for a in range(3)]
        occ = np.zeros((CROP, CROP, CROP), dtype=bool)
        occ[loc[0], loc[1], loc[2]] = True
        order = np.argsort(np.ravel_multi_index(loc, occ.shape), kind="stable")
        want, _ = nn.normals(occ, q, nn.default_r2(q))
        exact = np.ones(rs.size, dtype=bool)
        for a in range(3):
            exact &= ((loc[a] >= reach[a]) | (lo[a] == 0)) & ((loc[a] < CROP - reach[a]) | (hi[a] == n))
        got = dev[rs][order]                                     # in the crop's own index order, as `want` is
        ex = exact[order]
        assert np.array_equal(got[ex], want[ex])
        surface += int((got[:, 3] == 1).sum())
        covered += int((got[ex][:, 3] == 1).sum())
    print("1024^3 crops: %d surface records, %d checked exactly" % (surface, covered))
    assert surface > 0 and 2 * covered >= surface


# ---- shading ---------------------------------------------------------------------------------------------------------------------
def _orbit(n=6, H=120, W=160, radius=4000.0):
    from voxcarve import camera
    return camera.orbit(n, radius, 25.0, 0.9 * W, H, W)


def _headlights(views):
    return np.array([-np.asarray(v.R, dtype=np.float64).reshape(3, 3)[2, :] for v in views])


def _check_shaded(e, views, H, W, light=None, ambient=64, background=(0, 0, 0)):
    rec, idx, _, _ = _hull(e)
    n4 = e.fetch_record_normals()
    got = e.render_shaded(views, H, W, ambient=ambient, light=light, background=background)
    L = _headlights(views) if light is None else np.asarray(light, dtype=np.float64)
    flat = e.render(views, H, W, background=background)
    assert np.array_equal(got["rgb_flat"], flat["rgb"]) and np.array_equal(got["index"], flat["index"])
    for v in range(len(views)):
        want = nn.shade(flat["index"][v], flat["rgb"][v], idx, _rgb(rec), n4, L[v], ambient)
        bad = np.argwhere((got["rgb"][v] != want).any(axis=2))
        assert bad.size == 0, "view %d: %d pixels differ, first at %r: %r, want %r" % (v, len(bad), tuple(bad[0]), got["rgb"][v][tuple(bad[0])],
                                                                                  want[tuple(bad[0])])
    return got, flat, n4, idx


@pytest.mark.parametrize("n", [64, 128])
def test_shaded_images_equal_restatement(neng, cams, masks, frames, n):
    H, W = masks[0].shape
    _setup(neng, (n, n, n), cams, masks, frames)
    neng.carve()
    neng.hull_normals()
    got, flat, n4, idx = _check_shaded(neng, cams, H, W, background=(9, 8, 7))
    hit = flat["index"] != MISS
    assert hit.any() and (got["rgb"][~hit] == np.array([9, 8, 7], np.uint8)).all()
    assert (got["rgb"][hit] != flat["rgb"][hit]).any()
    views = _orbit()
    for ambient in (0, 64, 255):
        got, flat, n4, idx = _check_shaded(neng, views, 120, 160, ambient=ambient)
        if ambient == 255:                                       # s = 255 wherever a normal exists: the unshaded render
            assert np.array_equal(got["rgb"], flat["rgb"])
    # lights that are no headlights: from above, from one side, and facing away from every surface a view can see
    _check_shaded(neng, views, 120, 160, light=np.tile([0.3, -0.2, -1.0], (6, 1)))
    away = -_headlights(views)
    got, flat, n4, idx = _check_shaded(neng, views, 120, 160, light=away, ambient=40)
    # (a surface the camera sees mostly faces it; where its normal has no part towards the reversed light, c = 0 and s = ambient)
    pos = np.searchsorted(idx, flat["index"][0][flat["index"][0] != MISS])
    nrm = n4[pos][:, :3].astype(np.float64)
    dark = (nrm @ away[0] <= 0) & (n4[pos][:, 3] == 1) & n4[pos][:, :3].any(axis=1)
    assert dark.sum() > 100
    rec = neng.fetch_records()
    want = ((_rgb(rec)[pos][dark].astype(np.int64) * 40 + 127) // 255).astype(np.uint8)
    assert np.array_equal(got["rgb"][0][flat["index"][0] != MISS][dark], want)


def test_camera_inside_the_hull_keeps_the_render(neng, cams, masks, frames):
    from voxcarve import camera
    n = 64
    _setup(neng, (n, n, n), cams, masks, frames)
    neng.carve()
    neng.hull_distance()
    deep = int(np.argmax(neng.fetch_record_distance()))
    got4, _ = _check_normals(neng)
    assert not got4[deep].any()                                  # the deepest survivor is no surface record
    i = int(neng.fetch_records()[deep] & LOW)
    xs, ys, zs = neng.axes()
    eye = np.array([xs[(i // n) % n], ys[i % n], zs[i // (n * n)]])
    view = camera.look_at(eye, eye + (300.0, 200.0, -100.0), 60.0, 24, 32)
    got, flat, _, _ = _check_shaded(neng, [view], 24, 32, ambient=10)
    assert (flat["face"] == 6).all() and (flat["index"] == i).all()
    assert np.array_equal(got["rgb"], flat["rgb"])


# ---- mesh normals ----------------------------------------------------------------------------------------------------------------
def _check_mesh_normals(e):
    rec, idx, occ, q = _hull(e)
    n4 = e.fetch_record_normals()
    mesh = e.surface_mesh(4)
    got = e.surface_normals()
    el, axis, on_low = sn.mesh_edges(occ, e.grid)
    nx, ny, _ = e.grid
    on = np.where(on_low, el, el + np.array([nx * ny, ny, 1], dtype=np.int64)[axis])
    pos = np.searchsorted(idx.astype(np.int64), on)
    assert np.array_equal(idx[pos], on)
    assert got.shape == (mesh["stats"]["n_verts"], 4) and np.array_equal(got, n4[pos])
    assert (got[:, 3] == 1).all()                                # a voxel with a mesh vertex has an OFF face neighbour
    return mesh, got


@pytest.mark.parametrize("n", [64, 128])
def test_mesh_normals_equal_on_elements(neng, cams, masks, frames, n):
    _setup(neng, (n, n, n), cams, masks, frames)
    S = neng.carve()
    neng.hull_normals()
    _check_mesh_normals(neng)
    assert neng.filter_components(keep_largest=1)["survivors_after"] < S
    neng.hull_normals()
    _check_mesh_normals(neng)


def _read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in head if l.startswith("element face")][0].split()[-1])
    props = [l.split()[1:] for l in head if l.startswith("property") and "list" not in l]
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[kind]) for kind, name in props])
    v = np.frombuffer(raw, dtype=dt, count=nv, offset=end)
    f = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("v", "<u4", (3,))]), count=nf, offset=end + nv * dt.itemsize)
    assert end + nv * dt.itemsize + nf * 13 == len(raw)
    return v, f["v"], [name for _, name in props]


def test_ply_with_and_without_normals(neng, cams, masks, frames, tmp_path):
    from voxcarve.voxel_reconstruction import write_ply
    _setup(neng, (64, 64, 64), cams, masks, frames)
    neng.carve()
    neng.hull_normals()
    mesh, n4 = _check_mesh_normals(neng)
    unit = nn.unit(n4)
    p = write_ply(str(tmp_path / "n.ply"), mesh["verts"], mesh["faces"], mesh["rgb"], normals=unit)
    v, f, names = _read_ply(p)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), unit.astype(np.float32))
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), mesh["verts"].astype(np.float32))
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), mesh["rgb"]) and np.array_equal(f, mesh["faces"])
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "bad.ply"), mesh["verts"], mesh["faces"], normals=unit[:-1])
    # without normals: the bytes of the writer as it was -- header, float32 x y z (+ u8 colours), 13-byte faces
    for rgb in (mesh["rgb"], None):
        p = write_ply(str(tmp_path / "plain.ply"), mesh["verts"], mesh["faces"], rgb)
        V, F = mesh["verts"].shape[0], mesh["faces"].shape[0]
        head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % V
        if rgb is not None:
            head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        head += "element face %d\nproperty list uchar uint vertex_indices\nend_header\n" % F
        vrec = np.empty(V, dtype=[("p", "<f4", (3,))] + ([("c", "u1", (3,))] if rgb is not None else []))
        vrec["p"] = mesh["verts"]
        if rgb is not None:
            vrec["c"] = rgb
        frec = np.empty(F, dtype=[("n", "u1"), ("v", "<u4", (3,))])
        frec["n"], frec["v"] = 3, mesh["faces"]
        assert open(p, "rb").read() == head.encode("ascii") + vrec.tobytes() + frec.tobytes()


# ---- the drop-in layer and the demo ----------------------------------------------------------------------------------------------
def test_assignment_and_demo_end_to_end(built, cams, masks, frames, tmp_path):
    from voxcarve import assignment
    H, W = masks[0].shape
    saved = dict(assignment._settings)
    try:
        with pytest.raises(ValueError):
            assignment.configure(normal_radius_mm=-1.0)
        for radius in (None, 90.0):
            assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=fx.GOLDEN + "/data",
                                 normal_radius_mm=radius)
            assignment.set_voxel_positions(64, 32, 64)
            e = assignment._engine
            got = assignment.render_views(smooth=True, ambient=32)
            st = e.hull_normals(radius)
            want = e.render_shaded(e.cameras, H, W, ambient=32)
            assert np.array_equal(got["rgb"], want["rgb"]) and np.array_equal(got["rgb_flat"], want["rgb_flat"])
            assert (got["rgb"] != got["rgb_flat"]).any() and st["surface"] == 2703
            rec, idx, occ, q = _hull(e)
            n4, _ = nn.normals(occ, q, nn.default_r2(q) if radius is None else dn.radius_r2(radius))
            assert np.array_equal(e.fetch_record_normals(), n4)
            flat = assignment.render_views()
            assert "rgb_flat" not in flat and np.array_equal(flat["rgb"], e.render(e.cameras, H, W)["rgb"])
            with pytest.raises(ValueError):
                assignment.render_views(smooth=True, shade=(255,) * 7)
            mesh = assignment.surface_mesh(4, normals=True)
            assert np.array_equal(mesh["normals"], nn.unit(e.surface_normals()))
            assert np.allclose(np.sqrt((mesh["normals"] ** 2).sum(axis=1)), 1.0)
            assert "normals" not in assignment.surface_mesh(4)
    finally:
        assignment.configure(frame_source=None, **saved)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path, rdir = str(tmp_path / "hull_mesh.ply"), str(tmp_path / "views")
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "demo.py"), "64", "-", "--render", rdir, "--smooth", "--mesh", path,
                        "--normals"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    v, f, names = _read_ply(path)
    assert names[3:6] == ["nx", "ny", "nz"] and v.shape[0] > 0 and f.max() < v.shape[0]
    length = np.sqrt(v["nx"].astype(np.float64) ** 2 + v["ny"].astype(np.float64) ** 2 + v["nz"].astype(np.float64) ** 2)
    assert np.allclose(length[length > 0], 1.0, atol=1e-6) and (length > 0).mean() > 0.99
    assert len(os.listdir(rdir)) == 12 and "mesh:" in r.stdout
