"""The silhouette-refined surface mesh on the device (vc_surface_mesh, vc_fetch_surface_mesh; csrc/vc_surface.h) against the
restatement (tests/surface_np.py): vertices (float64 bits), faces, colours, refined flags and counts bit for bit -- the real
cameras at 64^3 and 128^3 in both carve modes at four step counts and two thresholds, after color_visible, filter_components and
photo_carve, 16 cameras at 1080p, grids whose rows straddle occupancy words and a grid one voxel thick, the empty and the solid
hull, 1024^3 (the bench's workload); the topology against marching_cubes(axes="grid"), vc_fetch_mesh left alone, every refusal,
assignment.surface_mesh and demo.py --mesh."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures_util as fx
import surface_np as sn
from oracle import marching_np
from test_surface_restatement import read_ply
from voxcarve import _lib, synthetic

pytestmark = pytest.mark.gpu

REAL_PIT = dict(centre=(360.0, 40.0, -300.0), half=(350.0, 350.0, 300.0), opening=(200.0, 200.0), depth=150.0)


@pytest.fixture(scope="module")
def seng(built):
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


def _records(e):
    rec = e.fetch_records() if e.count else np.zeros(0, np.uint64)
    idx = (rec & np.uint64(0xffffffff)).astype(np.int64)
    rgb = np.stack([(rec >> np.uint64(s)) & np.uint64(255) for s in (32, 40, 48)], 1).astype(np.uint8) if rec.size else \
        np.zeros((0, 3), np.uint8)
    return idx, rgb


def _check(e, cams, m, steps, edges=None, faces="device"):
    """Device mesh of the current result against the restatement; returns the device output."""
    got = e.surface_mesh(steps)
    occ = e.fetch_occupancy() if edges is None else None
    idx, rgb = _records(e)
    bm = np.stack([e.fetch_mask(c) > 0 for c in range(len(cams))])          # what the carve read (post-filtered)
    want = sn.refine(occ, e.grid, e.bounds, fx.oracle_cams(cams), bm, m, steps, edges=edges)
    V = want["verts"].shape[0]
    assert got["verts"].shape == (V, 3)
    assert np.array_equal(got["verts"].view(np.uint64), want["verts"].view(np.uint64))
    assert np.array_equal(got["refined"], want["refined"])
    assert np.array_equal(got["rgb"], sn.colours(idx, rgb, want["e"], want["axis"], want["on_low"], e.grid) if V else
                          np.zeros((0, 3), np.uint8))
    st = got["stats"]
    assert (st["n_verts"], st["refined"], st["unrefined"]) == (V, int(want["refined"].sum()), V - int(want["refined"].sum()))
    assert st["n_faces"] == got["faces"].shape[0]
    if faces == "device":
        mv, mf = e.marching_cubes(axes="grid", level=0.25)
        lo3, axis, on_low = sn.edges_from_grid_verts(mv)
        assert np.array_equal(axis, want["axis"]) and np.array_equal(on_low, want["on_low"])
        nx, ny, _ = e.grid
        assert np.array_equal((lo3[:, 0] * nx + lo3[:, 1]) * ny + lo3[:, 2], want["e"])
        assert np.array_equal(got["faces"], mf)
    if V and st["refined"] and steps:
        assert st["point_tests"] > 0
    return got


@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("mode", ["fused", "lut"])
def test_real_cameras_equal_restatement(seng, cams, masks, frames, n, mode):
    _setup(seng, (n, n, n), cams, masks, frames)
    if mode == "lut":
        seng.build_lut()
    for m in (4, 3):
        seng.carve(mode=mode, min_views=m)
        for steps in (0, 1, 8, 24):
            got = _check(seng, cams, m, steps, faces="device" if steps == 8 else None)
            if steps == 0:
                assert got["stats"]["n_verts"] > 0
    closed, oriented, _, vol = marching_np.mesh_invariants(got["verts"], got["faces"])
    assert oriented and vol > 0


def test_colour_passes_change_colours_not_geometry(seng, cams, masks, frames):
    _setup(seng, (64, 64, 64), cams, masks, frames)
    seng.carve()
    a = _check(seng, cams, 4, 8)
    seng.color_visible()
    b = _check(seng, cams, 4, 8)
    assert np.array_equal(a["verts"].view(np.uint64), b["verts"].view(np.uint64)) and np.array_equal(a["faces"], b["faces"])
    assert not np.array_equal(a["rgb"], b["rgb"])
    seng.filter_components(keep_largest=1)
    c = _check(seng, cams, 4, 8)
    assert c["stats"]["unrefined"] == 0 and c["stats"]["n_verts"] > 0


def test_photo_carve_leaves_unrefined_vertices(seng, cams):
    H, W = 486, 644
    masks, frames = synthetic.textured_scene(cams, H, W, **REAL_PIT)
    _setup(seng, (64, 64, 64), cams, masks, frames)
    seng.carve()
    seng.photo_carve()
    got = _check(seng, cams, 4, 8)
    assert got["stats"]["unrefined"] > 0


def test_sixteen_cameras_1080p(seng):
    H, W = 1080, 1920
    cams = synthetic.ring_cameras(16, H, W)
    masks = synthetic.ellipsoid_masks(cams, H, W)
    _setup(seng, (48, 48, 48), cams, masks)
    for m in (16, 13):
        seng.carve(min_views=m)
        _check(seng, cams, m, 8)


def test_odd_grids_thin_grid_empty_and_solid_hull(seng, cams, masks, frames):
    H, W = masks[0].shape
    for grid in ((40, 72, 24), (8, 130, 9), (40, 40, 1), (1, 40, 40)):
        _setup(seng, grid, cams, masks)
        seng.carve()
        _check(seng, cams, 4, 8)
    _setup(seng, (16, 16, 16), cams, [np.zeros((H, W), np.uint8)] * 4)
    seng.carve()
    got = _check(seng, cams, 4, 8)
    assert got["stats"]["n_verts"] == 0 and got["stats"]["n_faces"] == 0
    # a solid hull: a small box around the centroid of the real hull, every mask full
    _setup(seng, (64, 64, 64), cams, masks)
    seng.carve()
    idx, _ = _records(seng)
    xs, ys, zs = seng.axes()
    c = np.array([xs[(idx // 64) % 64].mean(), ys[idx % 64].mean(), zs[idx // 4096].mean()])
    _setup(seng, (16, 16, 16), cams, [np.full((H, W), 255, np.uint8)] * 4,
           bounds=(c[0] - 30, c[0] + 30, c[1] - 30, c[1] + 30, c[2] - 30, c[2] + 30))
    assert seng.carve() == 16 ** 3
    got = _check(seng, cams, 4, 8)
    assert got["stats"]["n_verts"] == 0


def test_faces_match_the_oracle_and_fetch_mesh_is_left_alone(seng, cams, masks, frames):
    _setup(seng, (24, 20, 28), cams, masks, frames)
    seng.carve()
    got = _check(seng, cams, 4, 8)
    occ = seng.fetch_occupancy()
    assert np.array_equal(got["faces"], marching_np.extract(occ.reshape(28, 24, 20))[1])
    gv, gf = seng.marching_cubes(axes="grid", level=0.25)
    seng.surface_mesh(3)
    v2, f2 = np.empty_like(gv), np.empty_like(gf)
    seng._check(seng._L.vc_fetch_mesh(seng._ctx, v2.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                      f2.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), "vc_fetch_mesh")
    assert np.array_equal(v2, gv) and np.array_equal(f2, gf)
    # the next carve's result gives its own mesh; the old one stays until then
    before = seng.surface_mesh(8)
    seng.carve(min_views=3)
    again = np.empty_like(before["verts"])
    seng._check(seng._L.vc_fetch_surface_mesh(seng._ctx, again.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None),
                "vc_fetch_surface_mesh")
    assert np.array_equal(again.view(np.uint64), before["verts"].view(np.uint64))
    after = _check(seng, cams, 3, 8)
    assert after["verts"].shape != before["verts"].shape or not np.array_equal(after["verts"], before["verts"])


def test_1024_cubed_against_marching_cubes_edges(seng, cams, masks, frames):
    _setup(seng, (1024, 1024, 1024), cams, masks, frames)
    seng.carve()
    mv, mf = seng.marching_cubes(axes="grid", level=0.25)
    lo3, axis, on_low = sn.edges_from_grid_verts(mv)
    e = (lo3[:, 0] * 1024 + lo3[:, 1]) * 1024 + lo3[:, 2]
    got = _check(seng, cams, 4, 8, edges=(e, axis, on_low), faces=None)
    assert np.array_equal(got["faces"], mf)
    st = got["stats"]
    print("1024^3: %d vertices, %d faces, %d refined, %d point tests, %.3f ms" % (st["n_verts"], st["n_faces"], st["refined"],
                                                                                 st["point_tests"], st["surface_ms"]))


def test_refusals(built, cams, masks, frames):
    import voxcarve
    H, W = masks[0].shape

    def raw(e, steps=8, flags=0, stats=True):
        st = _lib.VcSurfaceStats()
        return e._L.vc_surface_mesh(e._ctx, steps, flags, ctypes.byref(st) if stats else None)

    with voxcarve.CarveEngine(0) as e:
        assert e._L.vc_fetch_surface_mesh(e._ctx, None, None, None, None) == -1
        assert raw(e) == -1                                                          # no carve result
        _setup(e, (32, 32, 32), cams, masks, frames)
        assert raw(e) == -1
        e.carve(records=False)
        assert raw(e) == -1                                                          # VC_FLAG_NO_RECORDS
        e.carve()
        e.carve_begin()
        assert raw(e) == -1                                                          # a step in flight
        e.carve_end()
        assert raw(e) == 0 and raw(e, steps=24) == 0
        assert raw(e, steps=25) == -1
        assert raw(e, flags=1) == -1
        assert raw(e, stats=False) == -1
        assert e._L.vc_fetch_surface_mesh(e._ctx, None, None, None, None) == -1    # a refused call leaves no mesh
        assert raw(e) == 0
        e.touch_masks(0)
        e.fetch_mask(0)                                                              # the frame set is prepared again
        assert raw(e) == -1
        e.carve()
        assert raw(e) == 0
        e.upload_masks([np.zeros((H, W), np.uint8)] * 4)                             # staged, not yet prepared: the masks read
        assert raw(e) == 0                                                           # are still the carve's
        e.carve()
        assert raw(e) == 0
        e.set_slab(0, 16)
        e.carve()
        assert raw(e) == -1                                                          # slab narrower than the grid
        msg = _lib.load().vc_last_error(e._ctx).decode()
        assert "slab" in msg


def test_assignment_and_demo_end_to_end(built, cams, masks, frames, tmp_path):
    from voxcarve import assignment
    saved = dict(assignment._settings)
    assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=fx.GOLDEN + "/data")
    try:
        assignment.set_voxel_positions(64, 32, 64)
        e = assignment._engine
        got = assignment.surface_mesh(8)
        want = e.surface_mesh(8)
        for k in ("verts", "faces", "rgb", "refined"):
            assert np.array_equal(got[k], want[k])
        assert got["stats"]["n_verts"] > 0
    finally:
        assignment.configure(frame_source=None, **saved)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "hull_mesh.ply")
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "demo.py"), "64", "-", "--mesh", path], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    v, f, c = read_ply(path)
    assert v.shape[0] > 0 and f.shape[0] > 0 and c is not None and f.max() < v.shape[0]
    assert "mesh:" in r.stdout
