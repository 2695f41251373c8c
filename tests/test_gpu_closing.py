"""Dilation and closing of the hull on the device (vc_hull_grow, vc_fetch_grown; csrc/vc_grow.h) against the restatement
(tests/closing_np.py), bit for bit: indices, order, all 8 bytes of every record, the `added` bytes, the occupancy words and the
stats.  Real cameras at 64^3 and 128^3 in both carve modes at 15 / 25 / 40 mm and r2 = 0, random frames, no colour camera, random
scenes whose hulls touch the grid's faces, a solid grid, the empty hull, a single voxel, a radius that makes the box the grid; after
photo_carve, filter_components and open_hull, twice in a row; the readers of the closed hull, each against its own restatement;
the next carve; a punched mask end to end; configure(hull_close_mm=...); every refusal; 256^3 against scipy; 1024^3 on crops."""
import ctypes
import os

import numpy as np
import pytest

import closing_np as cl
import distance_np as dn
import fixtures_util as fx

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)


@pytest.fixture(scope="module")
def geng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _setup(e, grid, cams, masks, frames=None, bounds=None, cc=1):
    H, W = masks[0].shape
    if bounds is None:
        e.set_grid(*grid)
    else:
        e.set_grid(*grid, bounds=bounds)
    e.set_cameras(cams, H, W)
    e.upload_masks(masks)
    if frames is not None:
        e.upload_frame(cc, frames[cc])


def _words(e):
    raw = np.empty((e.n_voxels + 63) // 64, dtype=np.uint64)
    e._check(e._L.vc_fetch_occupancy(e._ctx, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "vc_fetch_occupancy")
    return raw


def _want_words(idx, n):
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    i = np.asarray(idx, dtype=np.uint64)
    np.bitwise_or.at(w, (i >> np.uint64(6)).astype(np.int64), np.uint64(1) << (i & np.uint64(63)))
    return w


def _hull(e):
    rec = e.fetch_records().copy()
    idx = (rec & LOW).astype(np.uint32)
    return rec, idx, dn.volume(idx, e.grid), dn.steps_um(e.grid, e.bounds)


def _check_grow(e, op, cams, frames, mm=None, r2=None, cc=1):
    """dilate_hull / close_hull over the current result: records (order, all 8 bytes), added bytes, occupancy words, stats.
    cc: the colour camera the carve ran with (None: none); frames: the images it had (None: none uploaded)."""
    from voxcarve import _lib
    rec, idx, occ, q = _hull(e)
    if r2 is None:
        r2 = dn.radius_r2(mm)
    H, W = e.image_size
    new_occ, dilated, cells = cl.grow(occ, q, r2, op)
    cam = None if cc is None else fx.oracle_cams(cams)[cc]
    want, want_added = cl.records_after(rec, new_occ, e.grid, e.bounds, cam, None if frames is None or cc is None else frames[cc], H, W)
    if mm is not None:
        st = (e.close_hull if op == "close" else e.dilate_hull)(mm)
    else:
        st = e._grow(_lib.VC_GROW_CLOSE if op == "close" else _lib.VC_GROW_DILATE, r2)
    assert st["survivors_before"] == idx.size and st["survivors_after"] == want.size == e.count
    assert st["added"] == want.size - idx.size == int(want_added.sum())
    assert st["dilated"] == dilated and st["box_cells"] == cells and st["q"] == q
    assert st["grow_ms"] > 0 or idx.size == 0
    got = e.fetch_records()
    assert np.array_equal(got & LOW, want & LOW), "indices and order"
    assert np.array_equal(got, want), "records"
    assert np.array_equal(e.fetch_added(), want_added), "added bytes"
    assert np.array_equal(_words(e), _want_words(want & LOW, e.n_voxels)), "occupancy words"
    return st, want, want_added


@pytest.mark.parametrize("mode", ["fused", "lut"])
@pytest.mark.parametrize("n", [64, 128])
def test_golden_cameras_equal_restatement(geng, cams, masks, frames, n, mode):
    _setup(geng, (n, n, n), cams, masks, frames)
    if mode == "lut":
        geng.build_lut()
    table = {64: {15: 0, 25: 141, 40: 160}, 128: {15: 341, 25: 1168, 40: 3460}}[n]
    S = geng.carve(mode=mode)
    hull = geng.fetch_records().copy()
    assert np.array_equal(geng.fetch()[0], fx.expected(n)[0])
    for mm in (0, 15, 25, 40):
        for op in ("dilate", "close"):
            assert geng.carve(mode=mode) == S
            st, want, added = _check_grow(geng, op, cams, frames, mm=mm)
            if mm == 0:
                assert st["added"] == 0 and np.array_equal(geng.fetch_records(), hull)
            elif op == "close":
                assert st["added"] == table[mm]
                assert ((want[added == 1] >> np.uint64(56)) == 1).all()          # the real cameras see the whole volume
            else:
                assert st["added"] >= table[mm] and st["dilated"] == st["survivors_after"]
                assert (st["added"] > table[mm]) == any(cl.reach(st["q"], dn.radius_r2(mm)))
    # twice in a row: the closing is idempotent, the dilation keeps growing
    geng.carve(mode=mode)
    st1, _, _ = _check_grow(geng, "close", cams, frames, mm=25)
    st2, _, added = _check_grow(geng, "close", cams, frames, mm=25)
    assert st2["added"] == 0 and st2["survivors_after"] == st1["survivors_after"] and not added.any()
    st3, _, _ = _check_grow(geng, "dilate", cams, frames, mm=25)
    st4, _, _ = _check_grow(geng, "dilate", cams, frames, mm=25)
    assert st4["survivors_after"] > st3["survivors_after"] > st1["survivors_after"]
    # the next carve restores the golden hull
    assert geng.carve(mode=mode) == S and np.array_equal(geng.fetch_records(), hull)


def test_no_colour_camera_and_no_image(geng, cams, masks, frames):
    import voxcarve
    n = 64
    _setup(geng, (n, n, n), cams, masks, frames)
    S = geng.carve(color_cam=None)
    assert ((geng.fetch_records() >> np.uint64(32)) == 0).all()
    st, want, added = _check_grow(geng, "close", cams, frames, mm=40, cc=None)
    assert st["added"] == 160 and ((want[added == 1] >> np.uint64(32)) == 0).all()
    assert geng.carve(color_cam=None) == S
    _check_grow(geng, "dilate", cams, frames, mm=25, cc=None)
    # a colour camera without an image: seen = 1, colour 0 (what the carve's own records carry)
    with voxcarve.CarveEngine(0) as e:
        _setup(e, (n, n, n), cams, masks)
        e.carve(color_cam=2)
        st, want, added = _check_grow(e, "close", cams, None, mm=40, cc=2)
        assert ((want[added == 1] >> np.uint64(32)) == (1 << 24)).all()
        # another colour camera, with its image
        e.upload_frame(0, frames[0])
        e.carve(color_cam=0)
        _check_grow(e, "dilate", cams, frames, mm=25, cc=0)


@pytest.mark.parametrize("grid,seed,mv", [((37, 53, 29), 3, 1), ((37, 53, 29), 4, 2), ((20, 70, 33), 5, 1), ((9, 130, 12), 6, 1),
                                          ((12, 64, 10), 7, 2)])
def test_random_scenes_touching_the_faces(geng, grid, seed, mv):
    """Random cameras, masks and frames: hulls that touch the grid's faces on grids whose columns straddle occupancy words; the
    added voxels carry real colours, and some lie outside the colour camera's image (seen = 0)."""
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    _setup(geng, grid, cams3, masks3, frames3)
    S = geng.carve(min_views=mv)
    assert S > 0
    occ = _hull(geng)[2]
    assert occ[0].any() or occ[-1].any() or occ[:, 0].any() or occ[:, -1].any() or occ[:, :, 0].any() or occ[:, :, -1].any()
    coloured = 0
    for op in ("dilate", "close"):
        for mm in (0, 45, 100, 250, 700):                        # (the steps of these grids are 30 to 190 mm)
            assert geng.carve(min_views=mv) == S
            st, want, added = _check_grow(geng, op, cams3, frames3, mm=mm)
            coloured += int((((want[added == 1] >> np.uint64(32)) & np.uint64(0xffffff)) != 0).sum())
    assert coloured > 0
    # a radius large enough that the box is the whole grid, and one beyond the grid
    assert geng.carve(min_views=mv) == S
    st, _, _ = _check_grow(geng, "close", cams3, frames3, mm=3000)
    assert st["box_cells"] == geng.n_voxels
    assert geng.carve(min_views=mv) == S
    st, _, _ = _check_grow(geng, "dilate", cams3, frames3, mm=20000)
    assert st["survivors_after"] == geng.n_voxels == st["box_cells"]
    assert geng.carve(min_views=mv) == S
    st, _, _ = _check_grow(geng, "close", cams3, frames3, r2=2 ** 64 - 1)
    assert st["survivors_after"] == geng.n_voxels == st["dilated"]


def test_solid_grid_empty_hull_and_single_voxel(geng, cams, masks, frames):
    from voxcarve import synthetic
    H, W = masks[0].shape
    full = [np.full((H, W), 255, np.uint8)] * 4
    # a 600 mm cube around the figure: every real camera has all of it in its image (the default volume they do not)
    _setup(geng, (32, 48, 40), cams, full, frames, bounds=(60.0, 660.0, -253.0, 347.0, -901.0, -301.0))
    S = geng.carve()
    assert S == 32 * 48 * 40
    for op in ("dilate", "close"):
        for mm in (0, 30):
            st, _, _ = _check_grow(geng, op, cams, frames, mm=mm)
            assert st["added"] == 0 and st["survivors_after"] == S
    _setup(geng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert geng.carve() == 0
    for op in ("dilate", "close"):
        st, _, _ = _check_grow(geng, op, cams, frames, mm=25)
        assert st["survivors_before"] == st["dilated"] == st["survivors_after"] == st["added"] == st["box_cells"] == 0
        assert geng.fetch_added().size == 0 and geng.fetch_records().size == 0
    # one voxel: a grid around the volume's centre of which the masks leave the centre cell alone
    ring = synthetic.ring_cameras(4, 120, 160)
    x, y, z = synthetic.VOLUME_CENTRE
    grid, bounds = (9, 11, 7), (x - 400, x + 400, y - 500, y + 500, z - 300, z + 300)
    geng.set_grid(*grid, bounds=bounds)
    geng.set_cameras(ring, 120, 160)
    from oracle import carve_np
    pts = carve_np.points_of_indices(np.array([(3 * 9 + 4) * 11 + 5]), *grid, bounds)
    dots = []
    for c in ring:
        off = carve_np.pixel_offsets(carve_np.project_points(pts, c.R, c.tvec, c.K, c.dist), 120, 160)
        m = np.zeros(120 * 160, np.uint8)
        m[off[0]] = 255
        dots.append(m.reshape(120, 160))
    geng.upload_masks(dots)
    fr = fx.synthetic_frames(4, 120, 160)
    geng.upload_frame(1, fr[1])
    if geng.carve() == 1:
        for op, mm in (("dilate", 100), ("close", 100), ("dilate", 250), ("close", 1000)):
            assert geng.carve() == 1
            _check_grow(geng, op, ring, fr, mm=mm)
    else:
        pytest.fail("the single-voxel scene holds %d voxels" % geng.count)


def test_after_photo_carve_filter_components_and_open_hull(geng, cams, masks, frames):
    n = 128
    _setup(geng, (n, n, n), cams, masks, frames)
    for c in range(4):
        geng.upload_frame(c, frames[c])
    S = geng.carve()
    ph = geng.photo_carve(max_rounds=2)
    assert ph["survivors_after"] < S
    st, _, _ = _check_grow(geng, "close", cams, frames, mm=25)       # (old records keep the photo carve's colours)
    assert st["added"] > 0
    geng.carve()
    cc = geng.filter_components(keep_largest=1)
    assert cc["survivors_after"] < S
    _check_grow(geng, "dilate", cams, frames, mm=15)
    geng.carve()
    op = geng.open_hull(25)
    assert op["survivors_after"] == 54466
    st, _, _ = _check_grow(geng, "close", cams, frames, mm=25)
    assert st["survivors_before"] == 54466 and st["added"] > 0
    st2, _, _ = _check_grow(geng, "close", cams, frames, mm=25)
    assert st2["added"] == 0


def test_readers_see_the_closed_hull(geng, cams, masks, frames):
    """Every reader of the step after a closing, each against its own restatement fed with the closed hull's records and
    occupancy: fetch*, fetch_occupancy, filter_components, color_visible, photo_carve, render, marching_cubes(volume=None),
    surface_mesh, pack_entries / expand_entries, hull_distance, erode_hull / open_hull; what the pass invalidates."""
    import photo_np as pn
    import visible_np as vn
    from test_gpu_components import _check as check_components
    from test_gpu_distance import _check_field, _check_morph
    from test_gpu_render import _check as check_render
    from test_gpu_surface import _check as check_surface
    from voxcarve._lib import VoxcarveError
    n = 128
    H, W = masks[0].shape
    oc = fx.oracle_cams(cams)
    _setup(geng, (n, n, n), cams, masks, frames)
    for c in range(4):
        geng.upload_frame(c, frames[c])

    def closed():
        geng.carve()
        st, want, added = _check_grow(geng, "close", cams, frames, mm=25)
        assert st["survivors_after"] == 58216
        return want

    want = closed()
    idx, rgb, seen = geng.fetch()
    assert np.array_equal(idx, (want & LOW).astype(np.uint32)) and seen.all()
    assert np.array_equal(rgb, np.stack([(want >> np.uint64(k)) & np.uint64(0xff) for k in (32, 40, 48)], axis=1).astype(np.uint8))
    occ = geng.fetch_occupancy()
    assert int(occ.sum()) == 58216 and np.array_equal(np.flatnonzero(occ), idx)
    w, cst = check_components(geng, 26, 0, 0)
    assert cst["components"] == 1                                # the closing at 25 mm joins the two components of the hull
    closed()
    v, f = geng.marching_cubes(volume=None)
    v2, f2 = geng.marching_cubes(volume=geng.fetch_occupancy().reshape(n, n, n))
    assert np.array_equal(v, v2) and np.array_equal(f, f2) and f.size > 0
    check_render(geng, cams[:2], H, W)
    got = check_surface(geng, cams, 4, 8)
    assert got["stats"]["unrefined"] > 0 and got["stats"]["refined"] > 0         # edges at added voxels stay at the midpoint
    rec = geng.fetch_records().copy()
    ent = geng.pack_entries()
    assert int(np.bitwise_count(ent[:, 0]).sum()) == rec.size
    assert geng.expand_entries(ent) == rec.size
    assert np.array_equal(geng.fetch_gathered() & LOW, rec & LOW)
    # colour by visibility, then the photo carve, of the closed hull
    rec0 = closed()
    geng.color_visible()
    i0 = (rec0 & LOW).astype(np.uint32)
    rgb0 = np.stack([(rec0 >> np.uint64(k)) & np.uint64(0xff) for k in (32, 40, 48)], axis=1).astype(np.uint8)
    zmaps, vis, rgb1 = vn.color_visible(i0, rgb0, geng.grid, geng.bounds, oc, frames, H, W, None)
    wrec = (rec0 & np.uint64(0xff000000ffffffff)) | (rgb1[:, 0].astype(np.uint64) << np.uint64(32)) | \
        (rgb1[:, 1].astype(np.uint64) << np.uint64(40)) | (rgb1[:, 2].astype(np.uint64) << np.uint64(48))
    assert np.array_equal(geng.fetch_visibility(), vis) and np.array_equal(geng.fetch_records(), wrec)
    assert int(geng.fetch_added().sum()) == 1168                 # (a recolouring leaves the set of survivors alone)
    rec0 = closed()
    st = geng.photo_carve(max_rounds=2)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no added flags"):
        geng.fetch_added()
    wp = pn.photo_carve(i0, rgb0, geng.grid, geng.bounds, oc, frames, H, W, max_rounds=2)
    assert st["survivors_before"] == rec0.size and st["survivors_after"] == wp["idx"].size
    assert np.array_equal(geng.fetch()[0], wp["idx"]) and np.array_equal(geng.fetch()[1], wp["rgb"])
    # the distance field and the shrinking half on the closed hull
    closed()
    _check_field(geng, "open", outside=True)
    _check_morph(geng, "erode", 25)
    closed()
    st, _ = _check_morph(geng, "open", 25)
    assert st["survivors_before"] == 58216
    # what the pass invalidates
    geng.carve()
    geng.filter_components()
    geng.hull_distance()
    geng.color_visible()
    geng.close_hull(25)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no component labels"):
        geng.fetch_component_labels()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no distance field"):
        geng.fetch_record_distance()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG"):
        geng.fetch_visibility()
    assert geng.fetch_added().sum() == 1168
    geng.carve()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no added flags"):
        geng.fetch_added()


def test_a_call_that_adds_nothing_keeps_what_the_result_carries(geng, cams, masks, frames):
    """r2 = 0 and a second closing leave records and occupancy alone, so visibility and component labels stay valid; the stored
    distance field goes, since the transforms use its buffer; the added bytes are the call's own (all 0)."""
    from voxcarve._lib import VoxcarveError
    _setup(geng, (64, 64, 64), cams, masks, frames)
    for c in range(4):
        geng.upload_frame(c, frames[c])
    geng.carve()
    assert geng.close_hull(40)["added"] == 160
    geng.filter_components(min_voxels=1)
    geng.color_visible()
    geng.hull_distance()
    vis, lab, rec = geng.fetch_visibility().copy(), geng.fetch_component_labels().copy(), geng.fetch_records().copy()
    geng.fetch_record_distance()
    for call in (lambda: geng.close_hull(40), lambda: geng.dilate_hull(0)):
        assert call()["added"] == 0
        assert np.array_equal(geng.fetch_visibility(), vis) and np.array_equal(geng.fetch_component_labels(), lab)
        assert np.array_equal(geng.fetch_records(), rec) and not geng.fetch_added().any()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no distance field"):
            geng.fetch_record_distance()


def test_one_rank_allgather_of_the_closed_hull(built, cams, masks, frames):
    import voxcarve
    with voxcarve.CarveEngine(0) as e:
        _setup(e, (64, 64, 64), cams, masks, frames)
        e.comm_init(1, 0, voxcarve.CarveEngine.comm_unique_id())
        for compact in (1, 0):
            e.set_option("gather_compact", compact)
            e.carve()
            st, want, _ = _check_grow(e, "close", cams, frames, mm=40)
            counts, total = e.allgather()
            assert counts.tolist() == [want.size] and total == want.size == 6981 + 160
            got = e.fetch_gathered()
            assert np.array_equal(got & LOW, want & LOW)
            if not compact:
                assert np.array_equal(got, want)


def test_punched_mask_end_to_end(geng, cams, masks, frames):
    """A hole of 2 px in camera 1's mask carves 130 voxels out of the 128^3 hull; the closing by 25 mm on the device returns 128
    of them and adds nothing outside the closing of the intact hull."""
    from test_closing_restatement import punched_masks
    n = 128
    grid = (n, n, n)
    pm, was_fg = punched_masks(masks, 1, 2)
    assert was_fg
    _setup(geng, grid, cams, pm, frames)
    idx, _, _ = fx.expected(n)
    occ = dn.volume(idx, grid)
    S = geng.carve()
    hull = dn.volume(geng.fetch()[0], grid)
    lost = occ & ~hull
    assert S == idx.size - 130 and int(lost.sum()) == 130 and not (hull & ~occ).any()
    st, want, added = _check_grow(geng, "close", cams, frames, mm=25)
    c = dn.volume((want & LOW).astype(np.uint32), grid)
    assert int((c & lost).sum()) == 128
    assert not (c & ~cl.close_box(occ, dn.steps_um(grid, geng.bounds), dn.radius_r2(25))[0]).any()


def test_configure_hull_close_mm(built, cams, masks):
    import components_np as cn
    from voxcarve import assignment
    from voxcarve.engine import viewer_positions, voxel_keys
    frames = [np.dstack([m // 2 + 60, m // 3 + 40, 255 - m // 2]).astype(np.uint8) for m in masks]
    data = os.path.join(fx.GOLDEN, "data")
    grid = (128, 128, 128)
    try:
        with pytest.raises(ValueError):
            assignment.configure(hull_close_mm=-1.0)
        with pytest.raises(ValueError):
            assignment.configure(hull_close_mm=float("nan"))
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=data, hull_close_mm=25)
        p1, c1 = assignment.set_voxel_positions(128, 64, 128)
        assert len(p1) == 58216 and len(c1) == 58216
        e = assignment._engine
        rec1 = e.fetch_records().copy()
        q = dn.steps_um(grid, e.bounds)
        idx, _, _ = fx.expected(128)
        c = cl.close_box(dn.volume(idx, grid), q, dn.radius_r2(25))[0]
        assert np.array_equal(p1, viewer_positions(voxel_keys(dn.indices(c), grid, e.axes())))
        assert np.array_equal(assignment.voxels_status().reshape(-1), c.reshape(-1))
        assert cn.components(dn.indices(c), grid, 26, 0, 0)["label"].size == 1
        # equal to carve + close by hand
        e.carve(slot=0, min_views=4, color_cam=assignment._settings["color_camera"])
        assert e.close_hull(25)["added"] == 1168 and np.array_equal(e.fetch_records(), rec1)
        # close, then open: the opening sees the closed hull
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=data, hull_close_mm=25,
                             hull_open_mm=25)
        p2, _ = assignment.set_voxel_positions(128, 64, 128)
        o, _ = dn.open_(c, q, dn.radius_r2(25))
        assert len(p2) == int(o.sum()) and np.array_equal(assignment.voxels_status().reshape(-1), o.reshape(-1))
    finally:
        assignment.configure(frame_source=None, hull_close_mm=0.0, hull_open_mm=0.0)


def test_refusals(built, cams, masks, frames):
    """Every refusal of the contract but one: a communicator of more than one rank needs two processes with a device each, and the
    message comes from the check every post-carve pass shares."""
    import voxcarve
    from voxcarve._lib import VoxcarveError, VcGrowStats
    H, W = masks[0].shape
    calls = (lambda e: e.dilate_hull(10), lambda e: e.close_hull(10))
    with voxcarve.CarveEngine(0) as e:
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
                call(e)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no added flags"):
            e.fetch_added()
        e.set_grid(64, 64, 64)
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        S = e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no added flags"):
            e.fetch_added()
        gs = VcGrowStats()
        assert e._L.vc_hull_grow(e._ctx, 2, 0, 0, ctypes.byref(gs)) == -1 and "op" in e._L.vc_last_error(e._ctx).decode()
        assert e._L.vc_hull_grow(e._ctx, 1, 0, 1, ctypes.byref(gs)) == -1 and "flags" in e._L.vc_last_error(e._ctx).decode()
        assert e._L.vc_hull_grow(e._ctx, 1, 0, 0, None) == -1 and "stats" in e._L.vc_last_error(e._ctx).decode()
        assert e._L.vc_fetch_grown(e._ctx, None) == -1
        assert e.count == S and e.fetch_records().size == S      # a refused call leaves the result alone
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                e.close_hull(bad)
            with pytest.raises(ValueError):
                e.dilate_hull(bad)
        # a slot prepared again since the carve: its images are not the ones the colours came from
        hull = e.fetch_records().copy()
        e.touch_masks(0)
        e.fetch_mask(0)                                          # the frame set is prepared again
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*prepared again"):
                call(e)
        assert np.array_equal(e.fetch_records(), hull)
        # the metric's limits
        e.set_grid(64, 64, 64, bounds=(0, 63 * 1100.0, 0, 1, 0, 1))
        e.carve()
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis x"):
                call(e)
        e.set_grid(64, 64, 1, bounds=(0, 100, 0, 100, 5, 5))
        e.carve()
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis z"):
                call(e)
        e.set_grid(4097, 2, 2)                                   # an axis longer than the kernels' lines
        e.carve()
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis x has 4097 cells"):
                call(e)
        e.set_grid(64, 64, 64)
        e.carve(records=False)
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
                call(e)
        e.set_slab(0, 32)
        e.carve()
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
                call(e)
        e.set_slab(0, 64)
        e.carve_begin()
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
                call(e)
        e.carve_end()
        assert e.close_hull(40)["added"] == 160


def test_timing_reports_the_kernels(built, cams, masks, frames):
    import voxcarve
    with voxcarve.CarveEngine(0) as e:
        _setup(e, (128, 128, 128), cams, masks, frames)
        e.set_option("timing_detail", 1)
        e.carve()
        e.timing(reset=True)
        st = e.dilate_hull(25)
        t = e.timing()
        k = t["kernels"]
        assert k["k_dist_box"]["launches"] == 1 and k["k_dist_y"]["launches"] == 1 and k["k_dist_env"]["launches"] == 2
        assert k["k_grow_mark"]["launches"] == 1 and k["grow_rank"]["launches"] == 4 and k["grow_merge"]["launches"] == 2
        assert all(k[name]["ms_sum"] > 0 for name in ("k_grow_mark", "grow_rank", "grow_merge"))
        assert t["work"]["dist_cells"] == st["box_cells"]
        e.carve()
        e.timing(reset=True)
        st = e.close_hull(25)
        t = e.timing()
        k = t["kernels"]
        assert k["k_dist_y"]["launches"] == 2 and k["k_dist_env"]["launches"] == 4 and k["k_grow_mark"]["launches"] == 2
        assert t["work"]["dist_cells"] == 2 * st["box_cells"]
        e.timing(reset=True)
        assert e.close_hull(25)["added"] == 0                    # nothing to merge: no rank, no merge
        k = e.timing()["kernels"]
        assert "grow_rank" not in k and "grow_merge" not in k and k["k_grow_mark"]["launches"] == 2


def test_real_256_against_scipy(geng, cams, masks, frames):
    """The sets against the restatement; then scipy.ndimage.distance_transform_edt as an independent referee of Dl (that last
    part alone needs scipy)."""
    n = 256
    _setup(geng, (n, n, n), cams, masks, frames)
    S = geng.carve()
    for op in ("dilate", "close"):
        for mm in (15, 25):
            assert geng.carve() == S
            st, _, _ = _check_grow(geng, op, cams, frames, mm=mm)
            assert st["added"] > 0
    assert geng.carve() == S
    rec, idx, occ, q = _hull(geng)
    r2 = dn.radius_r2(25)
    geng.dilate_hull(25)
    got = dn.volume(geng.fetch()[0], geng.grid)
    ndimage = pytest.importorskip("scipy.ndimage")
    edt = ndimage.distance_transform_edt(~occ, sampling=(q[2], q[0], q[1]))
    assert np.array_equal(np.rint(edt ** 2).astype(np.uint64) <= np.uint64(r2), got)


CROP = 144          # cells per side of a crop of the 1024^3 check; its core is the inner CROP / 2 cells per side


def test_bench_workload_1024_on_crops(geng, cams, masks, frames):
    """At 1024^3 the whole restatement is too slow.  The invariants of the contract's item 2 hold on the whole result: hull <= C
    <= Dl, a second closing adds nothing, `added` sums to the stats.  The sets themselves are compared on 6 crops of CROP^3 cells
    centred on seeded survivors that have an OFF neighbour along y, each closed by the restatement as a grid of its own.  The
    crop's dilation equals the grid's wherever the margin to the crop's faces exceeds g_a + 1 cells (every survivor within reach
    is in the crop), and its closing wherever the margin exceeds 2 (g_a + 1) (every cell within reach has its right dilation).
    Condition, decided by the steps and the radius alone: 2 (g_a + 1) < CROP / 4 on every axis, so the comparison covers EVERY
    voxel of every core (the inner CROP / 2 cells per side); and the cores must hold voxels the closing adds."""
    n = 1024
    mm = 25
    _setup(geng, (n, n, n), cams, masks, frames)
    S = geng.carve()
    rec = geng.fetch_records().copy()
    idx = (rec & LOW).astype(np.int64)
    q = dn.steps_um((n, n, n), geng.bounds)
    r2 = dn.radius_r2(mm)
    g = cl.reach(q, r2)
    assert all(2 * (ga + 1) < CROP // 4 for ga in g)
    st = geng.close_hull(mm)
    crec = geng.fetch_records().copy()
    added = geng.fetch_added()
    cidx = (crec & LOW).astype(np.int64)
    assert st["survivors_before"] == S and st["survivors_after"] == crec.size == geng.count and st["added"] == crec.size - S > 0
    assert int(added.sum()) == st["added"] and (np.diff(cidx) > 0).all()
    assert np.array_equal(crec[added == 0], rec)                                  # hull <= C, the old records byte for byte
    assert st["dilated"] > crec.size
    geng.carve()
    dst = geng.dilate_hull(mm)
    didx = (geng.fetch_records() & LOW).astype(np.int64)
    assert dst["survivors_after"] == st["dilated"] == didx.size
    assert np.isin(cidx, didx, assume_unique=True).all()                          # C <= Dl
    iy, t = idx % n, idx // n
    ix, iz = t % n, t // n
    edge = np.flatnonzero(np.diff(idx, append=idx[-1] + 2) != 1)                  # survivors whose +y neighbour is not one
    rng = np.random.default_rng(1024)
    in_core = fresh = 0
    dl_of = lambda a: (a // n // n, a // n % n, a % n)
    for s in rng.choice(edge, 6, replace=False):
        c = (int(iz[s]), int(ix[s]), int(iy[s]))                 # the volume's axes: z, x, y
        lo = [min(max(v - CROP // 2, 0), n - CROP) for v in c]
        vols = []
        for lin in (idx, cidx, didx):
            z, x, y = dl_of(lin)
            inside = (z >= lo[0]) & (z < lo[0] + CROP) & (x >= lo[1]) & (x < lo[1] + CROP) & (y >= lo[2]) & (y < lo[2] + CROP)
            v = np.zeros((CROP, CROP, CROP), dtype=bool)
            v[z[inside] - lo[0], x[inside] - lo[1], y[inside] - lo[2]] = True
            vols.append(v)
        occ, dev_c, dev_dl = vols
        want_c, want_dl = cl.close_(occ, q, r2)
        core = (slice(CROP // 4, CROP - CROP // 4),) * 3
        assert np.array_equal(dev_dl[core], want_dl[core]) and np.array_equal(dev_c[core], want_c[core])
        in_core += int(occ[core].sum())
        fresh += int((want_c[core] & ~occ[core]).sum())
    print("1024^3 crops: %d survivors in the cores, %d voxels added there" % (in_core, fresh))
    assert in_core > 0 and fresh > 0
    # a second closing adds nothing
    geng.carve()
    geng.close_hull(mm)
    st2 = geng.close_hull(mm)
    assert st2["added"] == 0 and st2["survivors_before"] == st2["survivors_after"] == crec.size
    assert np.array_equal(geng.fetch_records(), crec) and not geng.fetch_added().any()
