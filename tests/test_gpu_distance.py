"""The distance field of the hull, erosion and opening on the device (vc_hull_distance, vc_fetch_record_distance,
vc_fetch_distance, vc_hull_morphology; csrc/vc_distance.h) against the restatement (tests/distance_np.py), bit for bit: the dense
inside and outside fields and the record distances with the real cameras at 64^3 and 128^3, random scenes whose hulls touch the
grid faces on grids whose columns straddle occupancy words in both border modes, the empty hull; erode and open (index list,
colours, seen bytes, occupancy, stats) at 15 / 25 / 40 mm and r2 = 0, after photo_carve and filter_components, twice in a row;
the readers after the pass and the next carve; configure(hull_open_mm=...); every refusal and the stale fetches; 256^3 against
scipy; 1024^3 (the bench's workload) on crops."""
import ctypes
import os

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)


@pytest.fixture(scope="module")
def deng(built):
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


def _check_field(e, border="open", outside=False, dense=True):
    """hull_distance over the current result; stats, record distances and the dense fields against the restatement."""
    rec, idx, occ, q = _hull(e)
    st = e.hull_distance(border=border, outside=outside)
    want = dn.inside_box(occ, q, border)
    wrec = want.reshape(-1)[idx]
    assert st["survivors"] == idx.size == e.count and st["q"] == q
    assert st["max_d2"] == (int(wrec.max()) if idx.size else 0)
    assert st["distance_ms"] > 0 or idx.size == 0
    got = e.fetch_record_distance()
    assert got.dtype == np.uint64 and np.array_equal(got, wrec), "record distances"
    assert np.array_equal(e.fetch_record_depth(), np.sqrt(wrec.astype(np.float64)) / 1000)
    if dense:
        assert np.array_equal(e.fetch_distance_raw("inside"), want), "dense inside field"
    if outside:
        assert np.array_equal(e.fetch_distance_raw("outside"), dn.outside(occ, q)), "dense outside field"
    assert np.array_equal(e.fetch_records(), rec), "the pass leaves the result alone"
    return want, st


def _check_morph(e, op, mm, border="open"):
    """erode_hull / open_hull over the current result: records (order, colour, seen byte), occupancy words and stats."""
    rec, idx, occ, q = _hull(e)
    r2 = dn.radius_r2(mm)
    o, er = dn.open_(occ, q, r2, border)
    keep = (o if op == "open" else er).reshape(-1)[idx]
    d_in = dn.inside_box(occ, q, border).reshape(-1)[idx]
    st = (e.open_hull if op == "open" else e.erode_hull)(mm, border=border)
    assert st["survivors_before"] == idx.size and st["eroded"] == int(er.sum()) == int((d_in > np.uint64(r2)).sum())
    assert st["survivors_after"] == int(keep.sum()) == e.count and st["q"] == q
    assert st["max_d2"] == (int(d_in.max()) if idx.size else 0)
    assert np.array_equal(e.fetch_records(), rec[keep]), "records"
    assert np.array_equal(_words(e), _want_words(idx[keep], e.n_voxels)), "occupancy words"
    return st, keep


@pytest.mark.parametrize("n", [64, 128])
def test_golden_cameras_fields_equal_restatement(deng, cams, masks, frames, n):
    _setup(deng, (n, n, n), cams, masks, frames)
    S = deng.carve()
    idx, _, _ = fx.expected(n)
    assert np.array_equal(deng.fetch()[0], idx)
    want, st = _check_field(deng, "open", outside=True)
    assert st["max_d2"] == {64: 44912727720, 128: 39784228900}[n]
    assert 0 < st["sites_inside_box"] < n ** 3 - S
    _check_field(deng, "off", outside=False)
    deng.hull_distance(outside=True)
    signed = deng.fetch_distance_field("signed")
    occ = dn.volume(idx, (n, n, n))
    assert signed.shape == (n, n, n) and (signed[occ] < 0).all() and (signed[~occ] > 0).all()
    assert deng.fetch_distance_field("inside").max() == np.sqrt(float(st["max_d2"])) / 1000


@pytest.mark.parametrize("grid,seed,mv", [((37, 53, 29), 3, 1), ((37, 53, 29), 4, 2), ((20, 70, 33), 5, 1), ((9, 130, 12), 6, 1),
                                          ((12, 64, 10), 7, 2)])
def test_random_scenes_both_borders(deng, grid, seed, mv):
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    _setup(deng, grid, cams3, masks3, frames3)
    S = deng.carve(min_views=mv)
    assert S > 0
    for border in dn.BORDERS:
        _check_field(deng, border, outside=True)
    for border in dn.BORDERS:
        for op in ("erode", "open"):
            for mm in (0, 45, 100, 250):                         # (the steps of these grids are 30 to 190 mm)
                assert deng.carve(min_views=mv) == S
                _check_morph(deng, op, mm, border)


def test_solid_grid_and_empty_hull(deng, cams, masks, frames):
    H, W = masks[0].shape
    full = [np.full((H, W), 255, np.uint8)] * 4
    _setup(deng, (32, 48, 40), cams, full, frames)
    S = deng.carve()
    for border in dn.BORDERS:                                    # (a full grid with the border open has no site at all)
        want, st = _check_field(deng, border, outside=True)
        for op in ("erode", "open"):
            for mm in (0, 30):
                assert deng.carve() == S
                _check_morph(deng, op, mm, border)
    _setup(deng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert deng.carve() == 0
    want, st = _check_field(deng, "open", outside=True)
    assert st["survivors"] == 0 and st["sites_inside_box"] == 0 and st["max_d2"] == 0
    assert (deng.fetch_distance_raw("outside") == dn.NONE).all() and deng.fetch_record_distance().size == 0
    for op in ("erode", "open"):
        st, _ = _check_morph(deng, op, 25, "off")
        assert st["survivors_before"] == st["eroded"] == st["survivors_after"] == 0


@pytest.mark.parametrize("n", [64, 128])
def test_erode_and_open_golden(deng, cams, masks, frames, n):
    _setup(deng, (n, n, n), cams, masks, frames)
    table = {64: {15: (6981, 6981), 25: (5531, 6675), 40: (4852, 6599)}, 128: {15: (50811, 56387), 25: (39714, 54466), 40: (30357, 52773)}}[n]
    S = deng.carve()
    hull = deng.fetch_records().copy()
    for mm in (0, 15, 25, 40):
        for op in ("erode", "open"):
            assert deng.carve() == S
            st, keep = _check_morph(deng, op, mm)
            if mm:
                assert (st["eroded"], st["survivors_after"]) == (table[mm][0], table[mm][0] if op == "erode" else table[mm][1])
            else:
                assert st["survivors_after"] == S and np.array_equal(deng.fetch_records(), hull)
    # twice in a row: the opening is idempotent, the erosion keeps shrinking
    deng.carve()
    st1, _ = _check_morph(deng, "open", 25)
    st2, _ = _check_morph(deng, "open", 25)
    assert st2["survivors_before"] == st2["survivors_after"] == st1["survivors_after"]
    st3, _ = _check_morph(deng, "erode", 25)
    st4, _ = _check_morph(deng, "erode", 25)
    assert st4["survivors_after"] < st3["survivors_after"] < st1["survivors_after"]
    _check_field(deng, "off", outside=True)                      # the field of an eroded hull
    # the next carve restores the hull
    assert deng.carve() == S and np.array_equal(deng.fetch_records(), hull)


def test_after_photo_carve_and_filter_components(deng, cams, masks, frames):
    n = 128
    _setup(deng, (n, n, n), cams, masks, frames)
    for c in range(4):
        deng.upload_frame(c, frames[c])
    S = deng.carve()
    ph = deng.photo_carve(max_rounds=2)
    assert ph["survivors_after"] < S
    _check_field(deng, "open", outside=True)
    _check_morph(deng, "open", 25)
    deng.carve()
    cc = deng.filter_components(keep_largest=1)
    assert cc["survivors_after"] < S
    _check_field(deng, "open")
    st, _ = _check_morph(deng, "open", 25)
    assert 0 < st["survivors_after"] < cc["survivors_after"]


def test_readers_see_the_opened_hull(deng, cams, masks, frames):
    """filter_components, render, surface_mesh and marching_cubes after an opening: each equals its own restatement
    (tests/components_np.py, render_np.py, surface_np.py) fed with the opened hull's records and occupancy."""
    import components_np as cn
    import render_np as rn
    import surface_np as sn
    from voxcarve._lib import VoxcarveError
    n = 128
    H, W = masks[0].shape
    _setup(deng, (n, n, n), cams, masks, frames)
    deng.carve()
    st, keep = _check_morph(deng, "open", 15)
    occ = deng.fetch_occupancy()
    assert int(occ.sum()) == st["survivors_after"] == 56387
    rec, idx, _, _ = _hull(deng)
    cst = deng.filter_components(connectivity=26, min_voxels=3)
    want = cn.components(idx, deng.grid, 26, 3, 0)
    assert cst["components"] == want["label"].size == 9 and cst["survivors_before"] == 56387
    assert np.array_equal(deng.fetch_component_labels(), want["labels"]) and np.array_equal(deng.fetch_records(), rec[want["keep"]])
    deng.carve()
    _check_morph(deng, "open", 25)
    rec, idx, _, _ = _hull(deng)
    rgb = np.stack([(rec >> np.uint64(s)) & np.uint64(255) for s in (32, 40, 48)], 1).astype(np.uint8)
    occ = deng.fetch_occupancy()
    # render
    shade, bg, views = (200, 190, 225, 215, 255, 150, 240), (9, 8, 7), cams[:2]
    got = deng.render(views, H, W, shade=shade, background=bg)
    wr = rn.render(occ, idx, rgb, deng.grid, deng.bounds, [rn.view_params(v) for v in views], H, W, shade=shade, background=bg,
                   pixels=None, block=8)
    flat = lambda a: a.reshape(len(views), H * W, *a.shape[3:])
    assert np.array_equal(flat(got["index"]), wr["index"]) and np.array_equal(flat(got["rgb"]), wr["rgb"])
    assert np.array_equal(flat(got["depth"]).view(np.uint32), wr["depth"].view(np.uint32)) and np.array_equal(flat(got["face"]), wr["face"])
    assert got["stats"]["hits"] == int((wr["index"] != rn.MISS).sum()) > 0
    # surface mesh
    got = deng.surface_mesh(8)
    bm = np.stack([deng.fetch_mask(c) > 0 for c in range(len(cams))])
    ws = sn.refine(occ, deng.grid, deng.bounds, fx.oracle_cams(cams), bm, 4, 8)
    assert got["stats"]["n_verts"] == ws["verts"].shape[0] > 0
    assert np.array_equal(got["verts"].view(np.uint64), ws["verts"].view(np.uint64)) and np.array_equal(got["refined"], ws["refined"])
    assert np.array_equal(got["rgb"], sn.colours(idx, rgb, ws["e"], ws["axis"], ws["on_low"], deng.grid))
    assert np.array_equal(got["faces"], deng.marching_cubes(axes="grid", level=0.25)[1])
    v, f = deng.marching_cubes(volume=None)
    v2, f2 = deng.marching_cubes(volume=deng.fetch_occupancy().reshape(n, n, n))
    assert np.array_equal(v, v2) and np.array_equal(f, f2) and f.size > 0
    # what the pass invalidates
    deng.carve()
    deng.filter_components()
    deng.hull_distance()
    deng.open_hull(25)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no component labels"):
        deng.fetch_component_labels()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no distance field"):
        deng.fetch_record_distance()


def test_configure_hull_open_mm(built, cams, masks):
    from voxcarve import assignment
    from voxcarve.engine import viewer_positions, voxel_keys
    frames = [np.dstack([m // 2 + 60, m // 3 + 40, 255 - m // 2]).astype(np.uint8) for m in masks]
    data = os.path.join(fx.GOLDEN, "data")
    try:
        with pytest.raises(ValueError):
            assignment.configure(hull_open_mm=-1.0)
        with pytest.raises(ValueError):
            assignment.configure(hull_open_mm=float("nan"))
        with pytest.raises(ValueError):
            assignment.configure(hull_border="closed")
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=data)
        p0, c0 = assignment.set_voxel_positions(128, 64, 128)
        assert len(p0) == 57048
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=data, hull_open_mm=25)
        p1, c1 = assignment.set_voxel_positions(128, 64, 128)
        assert len(p1) == 54466 and len(c1) == 54466
        idx, _, _ = fx.expected(128)
        grid = (128, 128, 128)
        o, _ = dn.open_(dn.volume(idx, grid), dn.steps_um(grid, assignment._engine.bounds), dn.radius_r2(25))
        assert np.array_equal(p1, viewer_positions(voxel_keys(dn.indices(o), grid, assignment._engine.axes())))
        assert np.array_equal(assignment.voxels_status().reshape(-1), o.reshape(-1))
        # before the component filter: the opening at 15 mm splits fragments off, the filter then drops them
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=data, hull_open_mm=15,
                             keep_components=1)
        p2, _ = assignment.set_voxel_positions(128, 64, 128)
        assert 0 < len(p2) < 56387
    finally:
        assignment.configure(frame_source=None, hull_open_mm=0.0, hull_border="open", keep_components=0)


def test_refusals_and_stale_fetches(built, cams, masks, frames):
    """Every refusal of the contract but one: a communicator of more than one rank needs two processes with a device each, and
    the message comes from the check the other post-carve passes share (result_refusals), which has no test of that case
    either."""
    import voxcarve
    from voxcarve._lib import VoxcarveError, VcDistanceStats, VcMorphStats
    H, W = masks[0].shape
    calls = (lambda e: e.hull_distance(), lambda e: e.erode_hull(10), lambda e: e.open_hull(10))
    with voxcarve.CarveEngine(0) as e:
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
                call(e)
        e.set_grid(64, 64, 64)
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        S = e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no distance field"):
            e.fetch_record_distance()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no distance field"):
            e.fetch_distance_raw("inside")
        ds, ms = VcDistanceStats(), VcMorphStats()
        assert e._L.vc_hull_distance(e._ctx, 4, ctypes.byref(ds)) == -1 and "flags" in e._L.vc_last_error(e._ctx).decode()
        assert e._L.vc_hull_distance(e._ctx, 0, None) == -1 and "stats" in e._L.vc_last_error(e._ctx).decode()
        assert e._L.vc_hull_morphology(e._ctx, 2, 0, 0, ctypes.byref(ms)) == -1 and "op" in e._L.vc_last_error(e._ctx).decode()
        assert e._L.vc_hull_morphology(e._ctx, 1, 0, 2, ctypes.byref(ms)) == -1 and "flags" in e._L.vc_last_error(e._ctx).decode()
        assert e._L.vc_hull_morphology(e._ctx, 1, 0, 0, None) == -1 and "stats" in e._L.vc_last_error(e._ctx).decode()
        assert e.count == S and e.fetch_records().size == S      # a refused call leaves the result alone
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                e.open_hull(bad)
            with pytest.raises(ValueError):
                e.erode_hull(bad)
        with pytest.raises(ValueError):
            e.hull_distance(border="closed")
        with pytest.raises(ValueError):
            e.fetch_distance_field("between")
        # the outside field needs VC_DIST_OUTSIDE; anything that changes the result makes the fetches fail again
        e.hull_distance()
        assert e.fetch_record_distance().size == S
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no outside field"):
            e.fetch_distance_raw("outside")
        e.hull_distance(outside=True)
        assert e.fetch_distance_raw("outside").shape == (64, 64, 64)
        e.filter_components(keep_largest=1)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no distance field"):
            e.fetch_distance_raw("outside")
        e.hull_distance()
        e.erode_hull(10)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no distance field"):
            e.fetch_record_distance()
        e.hull_distance()
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no distance field"):
            e.fetch_record_distance()
        for c in range(4):
            e.upload_frame(c, frames[c])
        e.carve()
        e.hull_distance()
        e.photo_carve(max_rounds=1)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no distance field"):
            e.fetch_record_distance()
        # the metric's limits
        e.set_grid(64, 64, 64, bounds=(0, 63 * 1100.0, 0, 1, 0, 1))
        e.carve()
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis x"):
                call(e)
        e.set_grid(64, 64, 64, bounds=(0, 1, 0, 1e-5, 0, 1))
        e.carve()
        for call in calls:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis y"):
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
        assert e.open_hull(25)["survivors_after"] == 6675


def test_timing_reports_the_kernels(built, cams, masks, frames):
    import voxcarve
    with voxcarve.CarveEngine(0) as e:
        _setup(e, (128, 128, 128), cams, masks, frames)
        e.set_option("timing_detail", 1)
        e.carve()
        e.timing(reset=True)
        st = e.hull_distance(outside=True)
        t = e.timing()
        k, w = t["kernels"], t["work"]
        assert k["k_dist_box"]["launches"] == 1 and k["k_dist_y"]["launches"] == 2 and k["k_dist_env"]["launches"] == 4
        assert k["k_dist_records"]["launches"] == 1
        assert all(k[name]["ms_sum"] > 0 for name in ("k_dist_box", "k_dist_y", "k_dist_env", "k_dist_records"))
        assert w["dist_cells"] == st["sites_inside_box"] + st["survivors"] + 128 ** 3
        assert w["dist_lines"] > 3 * 128 * 128
        e.timing(reset=True)
        e.open_hull(25)
        t = e.timing()
        assert t["kernels"]["k_dist_y"]["launches"] == 2 and t["kernels"]["k_dist_env"]["launches"] == 4
        assert t["kernels"]["k_dist_records"]["launches"] == 2
        assert t["work"]["dist_cells"] == 2 * (st["sites_inside_box"] + st["survivors"])


def test_real_256_against_scipy(deng, cams, masks, frames):
    """The sets and the field against the restatement; then scipy.ndimage.distance_transform_edt as an independent referee of
    the field (that last part alone needs scipy)."""
    n = 256
    _setup(deng, (n, n, n), cams, masks, frames)
    S = deng.carve()
    for op in ("erode", "open"):
        for mm in (15, 25):
            assert deng.carve() == S
            st, _ = _check_morph(deng, op, mm)
            assert 0 < st["survivors_after"] < S
    assert deng.carve() == S
    _check_field(deng, "off")
    rec, idx, occ, q = _hull(deng)
    deng.hull_distance()
    got = deng.fetch_distance_raw("inside")
    assert np.array_equal(deng.fetch_record_distance(), got.reshape(-1)[idx]) and (got[~occ] == 0).all()
    ndimage = pytest.importorskip("scipy.ndimage")
    edt = ndimage.distance_transform_edt(occ, sampling=(q[2], q[0], q[1]))
    assert np.array_equal(np.rint(edt[occ] ** 2).astype(np.uint64), got[occ])


CROP = 128          # cells per side of a crop of the 1024^3 check; its core is the inner CROP / 2 cells per side


def test_bench_workload_1024_on_crops(deng, cams, masks, frames):
    """At 1024^3 the restatement runs on 8 crops of CROP^3 cells centred on seeded survivors, border open.  A crop's sites are a
    subset of the grid's, so the device's value is <= the crop's value c at every record of the crop; and where c <= m^2, m the
    distance to the nearest cell outside the crop, the nearest site lies inside the crop and the device's value equals c.  The
    restatement alone decides which records are covered: at least half of those in the crops' cores must be."""
    n = 1024
    _setup(deng, (n, n, n), cams, masks, frames)
    S = deng.carve()
    rec = deng.fetch_records().copy()
    idx = (rec & LOW).astype(np.int64)
    q = dn.steps_um((n, n, n), deng.bounds)
    st = deng.hull_distance()
    dev = deng.fetch_record_distance()
    assert st["survivors"] == S and st["max_d2"] == int(dev.max()) and dev.min() > 0
    iy, t = idx % n, idx // n
    ix, iz = t % n, t // n
    rng = np.random.default_rng(1024)
    core = covered = 0
    for s in rng.choice(S, 8, replace=False):
        c = (int(iz[s]), int(ix[s]), int(iy[s]))                 # the volume's axes: z, x, y
        lo = [max(v - CROP // 2, 0) for v in c]
        hi = [min(v + CROP // 2, n) for v in c]
        coords = (iz, ix, iy)
        inside = np.ones(S, dtype=bool)
        for a in range(3):
            inside &= (coords[a] >= lo[a]) & (coords[a] < hi[a])
        rs = np.flatnonzero(inside)
        loc = [coords[a][rs] - lo[a] for a in range(3)]
        occ = np.zeros(tuple(h - l for l, h in zip(lo, hi)), dtype=bool)
        occ[loc[0], loc[1], loc[2]] = True
        cval = dn.inside_box(occ, q, "open")[loc[0], loc[1], loc[2]]
        qa = (q[2], q[0], q[1])
        m = np.min([np.minimum(loc[a] + 1, occ.shape[a] - loc[a]) * qa[a] for a in range(3)], axis=0).astype(np.uint64)
        exact = cval <= m * m
        assert (dev[rs] <= cval).all()
        assert np.array_equal(dev[rs][exact], cval[exact])
        in_core = np.ones(rs.size, dtype=bool)
        for a in range(3):
            in_core &= np.abs(coords[a][rs] - c[a] + 0.5) < CROP // 4
        core += int(in_core.sum())
        covered += int((in_core & exact).sum())
    print("1024^3 crops: %d records in the cores, %d checked exactly" % (core, covered))
    assert core > 0 and 2 * covered >= core
    # open at 25 mm: invariants
    r2 = dn.radius_r2(25)
    st = deng.open_hull(25)
    kept = deng.fetch_records().copy()
    assert st["survivors_before"] == S and st["survivors_after"] == kept.size == deng.count
    assert st["eroded"] == int((dev > np.uint64(r2)).sum()) and st["max_d2"] == int(dev.max())
    assert 0 < kept.size < S and np.isin(kept, rec).all() and (np.diff((kept & LOW).astype(np.int64)) > 0).all()
    st2 = deng.open_hull(25)
    assert st2["survivors_before"] == st2["survivors_after"] == kept.size and np.array_equal(deng.fetch_records(), kept)
