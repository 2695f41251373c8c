"""Random chains of carves and post-carve passes on the device against tests/chain_model.py: how the passes COMBINE.

Every pass is held to its restatement by its own test, always behind a synchronous carve of slot 0.  Here 24 chains of 10 drawn
operations (chain_model.SEEDS; tests/test_chain_model.py asserts what they cover) run on three frame sets with different hulls and
colours, through synchronous, footprint and pipelined carves, with up to nine passes behind one carve.  After EVERY operation the
device is compared with the model: the call's stats, all 8 bytes of every record, the occupancy, the packed words' popcount, what
the operation itself produces, and every product of every pass -- its fetch returns the model's bytes or refuses with its own
message.  At the end of a chain the exchange form, the marching cubes of the occupancy and one run of every quiet pass are compared
on the final hull.  The two geodesic routes and the two floor-map routes alternate by step parity.

test_chain_c walks family C the same way (chain_model.SEEDS_C: 16 chains of 12 operations, family A's kinds and keep, upload, release,
combine, compare, motion, warp, paint_motion): behind pipelined and footprint carves, on every slot, with and without a colour
camera.  After every operation it compares, besides all of the above, the combine's added bytes and the motion field (the model's
bytes or the refusal by name) and all four hull registers (count, has_records, words, records, or "register r is empty").

test_chain_d walks family D (chain_model.SEEDS_D: 16 chains of 12 operations, family A's kinds and shade, texture, light,
surface_normals and the feed of the carve's frame set).  After every operation it compares, besides what test_chain checks, every
pixel of every view (chain_model.HW_D, 24 x 32: 3 x 4 tiles of the kernels) of the shaded, the textured and the lit images (the model's bytes, depths as their bits, or the refusal by
name; a view index of n_views is refused too) and of the last render, which like them outlives the result it was made of.  A call
that the model refuses must raise with the model's words, and the whole comparison then holds as before: nothing moved.

test_chain_e walks family E (chain_model.SEEDS_E: 12 chains of 12 operations, family C's kinds, the aligned vote and
temporal_reset, every motion estimate with 0 to 3 coarser levels).  After every operation it compares, besides what test_chain_c
checks, every level of a current motion field (rows, scalars, the level words of A and B; the level behind the coarsest is
refused; every level's fetch refuses once the field is stale), the votes, the vote's own field (chain_model.REFUSAL_E) and the
ring.  "One push per result" is drawn: the call must raise with the model's words, and nothing may have moved.

Family B (the plain vote, the measurements, the skeleton, the shell) is not walked here: DESIGN.md, "The abort at exit".

A failure names (seed, step, operation, parameters); chain_model.replay(seed, upto=step) rebuilds the model in front of it."""
import contextlib
import ctypes
import re

import numpy as np
import pytest

import chain_model as cm
import motion_np
from test_gpu_light import COUNTS as LIGHT_COUNTS
from test_gpu_motion import STAT_KEYS
from test_gpu_result_generation import REFUSAL, RENDER_HW, _fetches, _light, _render_images, _surface_mesh

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)


@pytest.fixture(scope="module")
def eng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _setup(e, sc, cams, masks, frames):
    """The scene's three frame sets; slot 0 is the suite's own fixtures."""
    assert all(np.array_equal(a, b) for a, b in zip(masks, sc.masks[0])) and all(np.array_equal(a, b) for a, b in zip(frames, sc.frames[0]))
    e.set_grid(*sc.grid, bounds=sc.bounds)
    e.set_cameras(cams, sc.H, sc.W)
    for slot in range(len(sc.masks)):
        e.upload_masks(masks if slot == 0 else sc.masks[slot], slot=slot)
        for c in cm.SLOT_IMAGES[slot]:
            e.upload_frame(c, (frames if slot == 0 else sc.frames[slot])[c], slot=slot)
    e.build_lut()


@contextlib.contextmanager
def _at(seed, step, op):
    try:
        yield
    except AssertionError as err:
        raise AssertionError("chain seed=%d, step=%s, %s: %s" % (seed, step, cm.describe_op(op), err)) from err


def _same(got, want, keys):
    for k in keys:
        assert got[k] == want[k], (k, got[k], want[k])


def _depth_maps(e, zmaps):
    for c in range(e.n_cameras):
        assert np.array_equal(e.fetch_depth(c).view(np.uint32).reshape(-1), zmaps[c]), ("depth map", c)


def _carve(e, op, out):
    if op["first"] is None:
        n = e.carve(slot=op["slot"], min_views=op["min_views"], color_cam=op["color_cam"], mode=op["mode"], footprint=op["footprint"])
    else:                                        # two steps in flight on two slots; the older one is collected and read first
        f = op["first"]
        begun = 0                                # both steps are collected before anything is asserted, whatever happens: a
        try:                                     # mismatch must not leave the engine, which every later chain uses, in flight
            e.carve_begin(slot=f["slot"], min_views=f["min_views"], color_cam=f["color_cam"], mode=f["mode"])
            begun += 1
            e.carve_begin(slot=op["slot"], min_views=op["min_views"], color_cam=op["color_cam"], mode=op["mode"])
            begun += 1
            n_first = e.carve_end()
            begun -= 1
            first = e.fetch_records()
            n = e.carve_end()
            begun -= 1
        finally:
            for _ in range(begun):
                e.carve_end()
        assert n_first == out["first_records"].size, "the first step's count"
        assert np.array_equal(first, out["first_records"]), "the first step's records"
    assert n == out["count"]


def _grow(e, op, out):
    st = (e.close_hull if op["op"] == "close" else e.dilate_hull)(op["radius_mm"])
    _same(st, out["stats"], ("survivors_before", "dilated", "survivors_after", "added", "box_cells", "q"))


def _shrink(e, op, out):
    st = (e.open_hull if op["op"] == "open" else e.erode_hull)(op["radius_mm"], border=op["border"])
    _same(st, out["stats"], ("survivors_before", "eroded", "survivors_after", "max_d2", "q"))


def _filter_components(e, op, out):
    st = e.filter_components(connectivity=op["connectivity"], min_voxels=op["min_voxels"], keep_largest=op["keep_largest"])
    _same(st, out["stats"], ("components", "components_kept", "survivors_before", "survivors_after", "largest"))
    got = e.fetch_components()
    for k in ("label", "size", "lo", "hi", "kept"):
        assert np.array_equal(got[k], out["components"][k]), k


def _photo_carve(e, op, out):
    st = e.photo_carve(slot=op["slot"], max_rounds=op["max_rounds"])
    _same(st, out["stats"], ("rounds", "converged", "survivors_before", "survivors_after"))
    _depth_maps(e, out["zmaps"])


def _color_visible(e, op, out):
    e.color_visible(slot=op["slot"])
    _depth_maps(e, out["zmaps"])


def _clusters(e, op, out, step):
    e.set_option("cluster_floor_records", step & 1)
    try:
        st = e.cluster_hull(op["k"], max_iters=op["max_iters"], min_column=op["min_column"])
    finally:
        e.set_option("cluster_floor_records", 1)
    w, d = out["clusters"], out["describe"]
    _same(st, out["stats"], ("survivors", "columns", "weight", "iterations", "q"))
    assert st["converged"] == out["converged"] and st["k"] == op["k"]
    cl = e.fetch_clusters()
    assert np.array_equal(cl["centre_um"], w["centres"])
    assert np.array_equal(e.fetch_floor_map().reshape(-1), w["floor_map"]), "floor map"
    assert np.array_equal(e.fetch_floor_labels().reshape(-1), w["floor_labels"]), "floor labels"
    for k in ("voxels", "weight", "columns", "lo", "hi"):
        assert np.array_equal(cl[k], d[k]), k
    assert np.array_equal(e.fetch_cluster_histograms(), d["histograms"]), "histograms"
    e.paint_clusters(op["palette"])


def _geodesic(e, op, out, step):
    e.set_option("geodesic_tiles", step & 1)
    try:
        st = e.hull_geodesic(seeds=op["seeds"], layers=op["layers"], extrema=op["extrema"], connectivity=op["connectivity"])
    finally:
        e.set_option("geodesic_tiles", 1)
    _same(st, out["stats"], ("survivors", "seeds", "reached", "unreached", "max_d", "extremities", "edge_um", "q"))
    assert np.array_equal(e.fetch_geodesic_labels(), out["labels"]), "labels"
    ex = e.fetch_extrema()
    rows = [(int(ex["label"][k]), int(ex["voxel"][k]), int(ex["record"][k]), int(ex["d"][k])) + tuple(int(v) for v in ex["index"][k])
            for k in range(ex["label"].size)]
    assert rows == out["extrema"], "extremities"
    e.paint_geodesic(op["paint"], op["palette"])


def _hull_distance(e, op, out):
    st = e.hull_distance(border=op["border"], outside=op["outside"])
    _same(st, out["stats"], ("survivors", "max_d2", "q"))
    assert np.array_equal(e.fetch_record_distance(), out["records"]), "record distances"
    if op["outside"]:
        assert np.array_equal(e.fetch_distance_raw("outside"), out["outside"]), "outside field"


def _hull_normals(e, op, out):
    st = e.hull_normals(op["radius_mm"])
    _same(st, out["stats"], ("survivors", "surface", "zero", "offsets", "ext", "q"))


def _render(e, op, out, sc, views=None, hw=RENDER_HW):
    got = e.render(sc.views if views is None else views, *hw)
    assert np.array_equal(got["index"], out["index"]), "index"
    assert np.array_equal(got["depth"].view(np.uint32), out["depth"].view(np.uint32)), "depth"
    assert np.array_equal(got["face"], out["face"]) and np.array_equal(got["rgb"], out["rgb"]), "face, rgb"
    _same(got["stats"], out["stats"], ("pixels", "hits"))


def _surface_mesh_op(e, op, out):
    got, want = e.surface_mesh(op["refine_steps"]), out["mesh"]
    assert got["verts"].shape == want["verts"].shape and np.array_equal(got["verts"].view(np.uint64), want["verts"].view(np.uint64)), "vertices"
    assert np.array_equal(got["faces"], want["faces"]), "faces"
    assert np.array_equal(got["rgb"], want["rgb"].reshape(-1, 3)) and np.array_equal(got["refined"], want["refined"]), "colours, refined"
    _same(got["stats"], out["stats"], ("n_verts", "n_faces", "refined", "unrefined"))


def _keep(e, op, out):
    e.keep_hull(op["reg"])


def _upload(e, op, out):
    e.upload_hull(out["occ"].reshape(-1) if op["form"] == "bits" else out["records"], op["reg"])


def _release(e, op, out):
    e.release_hull(op["reg"])


def _timed(st, key):
    """The call's stats without its time, which is positive."""
    assert st.pop(key) > 0, key
    return st


def _combine(e, op, out):
    st = _timed(e.combine_hull(op["setop"], op["reg"]), "setop_ms")
    assert sorted(st) == sorted(out["stats"])                    # (every field of VcSetopStats but the time)
    _same(st, out["stats"], sorted(st))


def _compare(e, op, out):
    st = _timed(e.compare_hull(op["reg"], distance=op["distance"]), "compare_ms")
    derived = {k: st.pop(k) for k in ("iou", "dice", "hausdorff_mm")}
    assert sorted(st) == sorted(out["stats"])
    _same(st, out["stats"], sorted(st))
    _same(derived, out["derived"], sorted(derived))


def _motion(e, op, out):
    st = _timed(e.hull_motion(op["reg"], op["block"], op["apron"], op["search"]), "motion_ms")
    assert sorted(st) == sorted(STAT_KEYS)
    _same(st, out["stats"], STAT_KEYS)


def _warp(e, op, out):
    st = _timed(e.warp_hull(op["src"], op["dst"]), "warp_ms")
    assert st.pop("predicted_iou") == out["predicted_iou"], "predicted_iou"
    assert sorted(st) == sorted(out["stats"])
    _same(st, out["stats"], sorted(st))


def _paint_motion(e, op, out):
    e.paint_motion()


def _run(e, sc, step, op, out):
    kind = op["op"]
    if kind in cm.REGISTER_KINDS:
        {"keep": _keep, "upload": _upload, "release": _release, "combine": _combine, "compare": _compare, "motion": _motion,
         "warp": _warp, "paint_motion": _paint_motion}[kind](e, op, out)
    elif kind == "carve":
        _carve(e, op, out)
    elif kind in ("close", "dilate"):
        _grow(e, op, out)
    elif kind in ("erode", "open"):
        _shrink(e, op, out)
    elif kind == "clusters":
        _clusters(e, op, out, step)
    elif kind == "geodesic":
        _geodesic(e, op, out, step)
    elif kind == "render":
        _render(e, op, out, sc)
    elif kind == "surface_mesh":
        _surface_mesh_op(e, op, out)
    else:
        {"filter_components": _filter_components, "photo_carve": _photo_carve, "color_visible": _color_visible,
         "hull_distance": _hull_distance, "hull_normals": _hull_normals}[kind](e, op, out)


def _result_equals_model(e, m):
    """Records, occupancy, packed words and every product: the model's bytes, or the product's own refusal."""
    from voxcarve._lib import VoxcarveError
    assert e.count == m.S, ("count", e.count, m.S)
    got = e.fetch_records()
    assert np.array_equal(got & LOW, m.records & LOW), "indices and order"
    bad = np.flatnonzero(got != m.records)
    assert bad.size == 0, "%d of %d records differ, first at %d: %#018x, want %#018x" % (bad.size, m.S, bad[0], int(got[bad[0]]), int(m.records[bad[0]]))
    assert np.array_equal(e.fetch_occupancy(), m.occ().reshape(-1)), "occupancy"
    assert int(np.bitwise_count(e.pack_entries()[:, 0]).sum()) == m.S, "popcount of the packed words"
    for name, fetch in _fetches(e).items():
        if name in m.products:
            assert fetch().tobytes() == m.products[name], "product %s differs from the model" % name
        else:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*" + REFUSAL[name]):
                fetch()
    if "normals" in m.products:                  # (the calls that read the images and the mesh look at the normals first)
        if "render" in m.products:
            e.shade_render(_light(e))
            assert _render_images(e) == m.products["render"], "product render differs from the model"
        else:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no images of the current"):
                e.shade_render(_light(e))
        if "surface" in m.products:
            e.surface_normals()
            assert _surface_mesh(e, m.mesh_shape) == m.products["surface"], "product surface differs from the model"
        else:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no mesh of the current"):
                e.surface_normals()


def _registers_equal_model(e, m):
    """What outlives a result: the combine's added bytes and the motion field -- the model's bytes, or the refusal by name -- and
    the four hull registers."""
    from voxcarve._lib import VoxcarveError
    if "combined" in m.products:
        assert e.fetch_combined().tobytes() == m.products["combined"], "product combined differs from the model"
    else:
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*" + cm.REFUSAL_C["combined"]):
            e.fetch_combined()
    if "motion" in m.products:
        got, f = e.fetch_motion(), m.field
        for key in cm.MOTION_ROW_KEYS:
            assert np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(f["rows"][key]).astype(np.int64)), ("motion field", key)
        assert sorted(got) == sorted(cm.MOTION_ROW_KEYS + ("grid", "edge", "apron", "search") + (("levels", "refine", "reach") if f.get("levels") else ()))
        assert (got["grid"], got["edge"], got["apron"], got["search"]) == (m.grid, f["b"], f["a"], f["s"]), "the field's scalars"
    else:
        for call in (e.fetch_motion, e.paint_motion):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*" + cm.REFUSAL_C["motion"]):
                call()
    for reg, want in enumerate(m.registers):
        if want is None:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*register %d is empty" % reg):
                e.fetch_kept(reg)
            continue
        got = e.fetch_kept(reg)
        assert got["count"] == int(want["occ"].sum()), ("register", reg, "count", got["count"])
        assert got["has_records"] == (want["records"] is not None), ("register", reg, "has_records")
        assert np.array_equal(got["words"], motion_np.words(want["occ"])), ("register", reg, "words")
        if want["records"] is None:
            assert got["records"] is None, ("register", reg, "records")
        else:
            assert np.array_equal(got["records"], want["records"]), ("register", reg, "records")


def _end_of_chain(e, sc, m, seed, after=lambda: None, run=None):
    """The final hull: the exchange form, the marching cubes of the occupancy, one run of every quiet pass."""
    with _at(seed, "end", {"op": "expand_entries(pack_entries())"}):
        assert e.expand_entries(e.pack_entries()) == m.S
        assert np.array_equal(e.fetch_gathered() & LOW, m.records & LOW)
    with _at(seed, "end", {"op": "marching_cubes"}):
        verts, faces = e.marching_cubes(volume=None)
        want_v, want_f = m.marching_cubes()
        assert np.array_equal(verts, want_v) and np.array_equal(faces, want_f)
    for k, op in enumerate(cm.final_ops(sc)):
        out = m.apply(op)
        with _at(seed, "end + %d" % k, op):
            (run or _run)(e, sc, k, op, out)
            _result_equals_model(e, m)
            after()


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_chain(eng, cams, masks, frames, seed):
    e = eng
    sc, ops = cm.draw_chain(seed)
    _setup(e, sc, cams, masks, frames)
    m = cm.Model(sc)
    for step, op in enumerate(ops):
        out = m.apply(op)
        with _at(seed, step, op):
            _run(e, sc, step, op, out)
            _result_equals_model(e, m)
    # the final hull: the exchange form, the marching cubes of the occupancy, one run of every quiet pass
    with _at(seed, "end", {"op": "expand_entries(pack_entries())"}):
        assert e.expand_entries(e.pack_entries()) == m.S
        assert np.array_equal(e.fetch_gathered() & LOW, m.records & LOW)
    with _at(seed, "end", {"op": "marching_cubes"}):
        verts, faces = e.marching_cubes(volume=None)
        want_v, want_f = m.marching_cubes()
        assert np.array_equal(verts, want_v) and np.array_equal(faces, want_f)
    for k, op in enumerate(cm.final_ops(sc)):
        out = m.apply(op)
        with _at(seed, "end + %d" % k, op):
            _run(e, sc, k, op, out)
            _result_equals_model(e, m)


@pytest.mark.parametrize("seed", cm.SEEDS_C)
def test_chain_c(eng, cams, masks, frames, seed):
    """Family C: the hull registers and the motion field behind every kind of carve.  The engine is the one the chains before
    have used: set_cameras empties the registers."""
    from voxcarve._lib import VoxcarveError
    e = eng
    sc, ops = cm.draw_chain(seed)
    _setup(e, sc, cams, masks, frames)
    for reg in range(cm.REGISTERS):
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*register %d is empty" % reg):
            e.fetch_kept(reg)
    m = cm.Model(sc)
    for step, op in enumerate(ops):
        out = m.apply(op)
        with _at(seed, step, op):
            _run(e, sc, step, op, out)
            _result_equals_model(e, m)
            _registers_equal_model(e, m)
    _end_of_chain(e, sc, m, seed, after=lambda: _registers_equal_model(e, m))


# ---- the vote's state, for family E ---------------------------------------------------------------------------------------------------
def _refuses_b(name):
    from voxcarve._lib import VoxcarveError
    return pytest.raises(VoxcarveError, match="VC_ERR_ARG.*" + cm.REFUSAL_B[name])


def _ring_equals_model(e, m):
    """Every hull of the vote's ring, newest first, and the refusal of the age behind the oldest."""
    from voxcarve._lib import VoxcarveError
    ring = m.ring()                              # (newest last; the aligned vote's ring holds the aligned hulls)
    held = len(ring)
    for age in range(held):
        assert np.array_equal(e.temporal_history(age), motion_np.words(ring[held - 1 - age])), ("the ring's hull of age", age)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*the ring holds %d hulls" % held):
        e.temporal_history(held)


# ---- family D: the passes over a render's images -------------------------------------------------------------------------------------
TEXTURE_COUNTS = ("pixels", "hits", "refined", "textured", "fallback")


def _image_call(e, op):
    """One of the three passes over the render's images, as the operation says; returns the call's stats (None: it has none)."""
    if op["op"] == "shade":
        e.shade_render(op["light"], op["ambient"])
        return None
    if op["op"] == "texture":
        return e.texture_render(op["slot"], op["steps"], op["reach_mm"], op["depth_tolerance"], op["best"], op["sharpen"], op["filter"])["stats"]
    return e.light_render(op["pos"], ambient=op["ambient"], smooth=op["smooth"], ao_reach=op["ao_reach"], floor=op["floor"])["stats"]


def _refuses(out):
    from voxcarve._lib import VoxcarveError
    return pytest.raises(VoxcarveError, match="VC_ERR_ARG.*" + re.escape(out["refusal"]))


def _carve_probed(e, op, out):
    """A carve with an image pass tried where every pass must refuse: while the carve's step is in flight, or behind the same
    carve without records.  Whatever happens, no step is left in flight."""
    probe = op["probe"]
    assert out["refused"] == probe["how"]
    kw = dict(slot=op["slot"], min_views=op["min_views"], color_cam=op["color_cam"], mode=op["mode"])
    if probe["how"] == "in_flight":
        e.carve_begin(**kw)
        try:
            with _refuses(out):
                _image_call(e, probe["op"])
        finally:
            n = e.carve_end()
        assert n == out["count"]
    else:
        assert e.carve(records=False, footprint=op["footprint"], **kw) == out["count"]
        with _refuses(out):
            _image_call(e, probe["op"])
        _carve(e, op, out)


def _run_d(e, sc, step, op, out):
    kind = op["op"]
    if kind == "carve" and op.get("probe") is not None:
        _carve_probed(e, op, out)
    elif kind == "render":                       # (family D's views are smaller than the other families')
        _render(e, op, out, sc, sc.views_at(cm.HW_D), cm.HW_D)
    elif kind == "feed":
        if op["how"] == "touch":
            e.touch_masks(op["slot"])
        else:
            e.upload_masks(sc.masks[op["slot"]], slot=op["slot"])
    elif kind not in cm.IMAGE_KINDS:
        _run(e, sc, step, op, out)
    elif out.get("refused"):
        with _refuses(out):
            e.surface_normals() if kind == "surface_normals" else _image_call(e, op)
    elif kind == "surface_normals":
        assert np.array_equal(e.surface_normals(), out["n4"]), "the mesh's normals"
    else:
        st = _image_call(e, op)
        if kind == "texture":
            _same(st, out["stats"], TEXTURE_COUNTS)
        elif kind == "light":
            _same(st, out["stats"], LIGHT_COUNTS)


def _fetch_picture(e, name, view):
    """One view of a pass's images through the library's fetch, every plane of it."""
    from voxcarve.engine import _ptr
    H, W = cm.HW_D
    got = {k: np.empty((H, W, 3) if k == "rgb" else (H, W), dtype=np.float32 if k == "depth" else np.uint8) for k in cm.PICTURE_KEYS[name]}
    ptrs = [_ptr(got[k], ctypes.c_float if k == "depth" else ctypes.c_uint8) for k in cm.PICTURE_KEYS[name]]
    call = {"shaded": e._L.vc_fetch_shaded, "textured": e._L.vc_fetch_textured, "lit": e._L.vc_fetch_lit}[name]
    e._check(call(e._ctx, view, *ptrs), "vc_fetch_" + name)
    return got


def _pictures_equal_model(e, m):
    """The images that outlive a result: the last render's, and the shaded, textured and lit ones -- every pixel of every view is
    the model's (depths as their bits), or the fetch refuses by name; a view index of n_views is refused as well."""
    from voxcarve._lib import VoxcarveError
    from voxcarve.engine import _ptr
    V, (H, W) = len(m.views), m.hw
    if m.images is not None:
        for v in range(V):
            got = {"index": np.empty((H, W), np.uint32), "depth": np.empty((H, W), np.float32), "rgb": np.empty((H, W, 3), np.uint8),
                   "face": np.empty((H, W), np.uint8)}
            e._check(e._L.vc_fetch_render(e._ctx, v, _ptr(got["index"], ctypes.c_uint32), _ptr(got["depth"], ctypes.c_float),
                                          _ptr(got["rgb"], ctypes.c_uint8), _ptr(got["face"], ctypes.c_uint8)), "vc_fetch_render")
            for k, a in got.items():
                assert a.tobytes() == m.images[k][v].tobytes(), ("the last render", k, "view", v)
    for name in cm.REFUSAL_D:
        if name not in m.pictures:
            for v in (0, V):
                with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*" + cm.REFUSAL_D[name]):
                    _fetch_picture(e, name, v)
            continue
        for v in range(V):
            got = _fetch_picture(e, name, v)
            for k in cm.PICTURE_KEYS[name]:
                want = m.pictures[name][k][v]
                a = (got[k] != 0).astype(np.uint8) if k == "refined" else got[k]
                bad = np.flatnonzero((a.view(np.uint32) if k == "depth" else a).reshape(-1) != (want.view(np.uint32) if k == "depth" else want).reshape(-1))
                assert bad.size == 0, "%s, %s of view %d: %d values differ from the model, first at %d" % (name, k, v, bad.size, bad[0])
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*view %d not in" % V):
            _fetch_picture(e, name, V)


def _told_of_the_probe(e, m):
    """_result_equals_model asks vc_shade_render whether the render is of the current result, and where it is, that call has made
    shaded images of its own light: the model is told."""
    if "normals" in m.products and "render" in m.products:
        assert not m.apply({"op": "shade", "light": _light(e), "ambient": 64}).get("refused")


@pytest.mark.parametrize("seed", cm.SEEDS_D)
def test_chain_d(eng, cams, masks, frames, seed):
    """Family D: the passes over a render's images behind every kind of carve, with the refusals the model expects.  The engine is
    the one the chains before have used, and images outlive set_grid and set_cameras: a carve and a render in front of the chain
    drop whatever an earlier chain left, so that the chain starts without shaded, textured or lit images, as the model does."""
    e = eng
    sc, ops = cm.draw_chain(seed)
    _setup(e, sc, cams, masks, frames)
    e.carve()
    e.render(sc.views_at(cm.HW_D), *cm.HW_D)
    m = cm.model_of(seed)
    assert m.hw == cm.HW_D
    for step, op in enumerate(ops):
        out = m.apply(op)
        with _at(seed, step, op):
            _run_d(e, sc, step, op, out)
            _pictures_equal_model(e, m)              # (in front of the probe below, which shades)
            _result_equals_model(e, m)
            _told_of_the_probe(e, m)

    def after():
        _told_of_the_probe(e, m)
        _pictures_equal_model(e, m)
    _end_of_chain(e, sc, m, seed, after=after, run=_run_d)


# ---- family E: the aligned vote and the motion pyramid ------------------------------------------------------------------------------------
def _temporal_motion(e, op, out):
    call = lambda: e.temporal_filter(op["window"], op["keep"], op["keep_off"], motion=(op["block"], op["apron"], op["search"]))
    if out.get("refused"):
        with _refuses(out):
            call()
        return
    st = call()
    assert st.pop("temporal_ms") > 0
    assert sorted(st) == sorted(out["stats"])                    # (every field of the stats but the time)
    _same(st, out["stats"], sorted(st))


def _motion_e(e, op, out):
    if not op["levels"]:
        return _motion(e, op, out)
    st = _timed(e.hull_motion(op["reg"], op["block"], op["apron"], op["search"], levels=op["levels"], refine=op["refine"]), "motion_ms")
    assert st == out["stats"], (st, out["stats"])


def _run_e(e, sc, step, op, out):
    kind = op["op"]
    if kind == "temporal_motion":
        _temporal_motion(e, op, out)
    elif kind == "temporal_reset":
        e.temporal_reset()
    elif kind == "motion":
        _motion_e(e, op, out)
    else:
        _run(e, sc, step, op, out)


def _same_rows(got, want, what):
    for key in cm.MOTION_ROW_KEYS:
        assert np.array_equal(np.asarray(got[key]).astype(np.int64).reshape(-1), np.asarray(want[key]).astype(np.int64).reshape(-1)), (what, key)


def _votes_and_levels_equal_model(e, m):
    """Every level of a current motion field (rows, scalars, the level words of A and B; the level behind the coarsest one is
    refused), or the refusal of every level's fetches; the votes, the aligned vote's field (the model's rows and scalars, or the
    refusal by name) and the ring."""
    from voxcarve._lib import VoxcarveError
    import motion_pyramid_np as mp
    if "motion" in m.products:
        f = m.field
        L = f["levels"]
        for l in range(L + 1):
            rows = e.fetch_motion_level(l)
            _same_rows(rows, f["res"]["rows"][l] if L else f["rows"], "level %d" % l)
            assert rows["grid"] == mp.level_grid(m.grid, l) and (rows["edge"], rows["apron"], rows["search"]) == (f["b"], f["a"], f["s"]), l
            assert (rows["levels"], rows["reach"]) == (L, f["reach"]) and (not L or rows["refine"] == f["refine"]), l
            a, b = (f["res"]["a"][l], f["res"]["b"][l]) if L else (m.occ(), m.registers[f["reg"]]["occ"])
            assert np.array_equal(e.fetch_motion_occupancy(l, 0), motion_np.words(a)), ("the words of A, level", l)
            assert np.array_equal(e.fetch_motion_occupancy(l, 1), motion_np.words(b)), ("the words of B, level", l)
        for call in (lambda: e.fetch_motion_level(L + 1), lambda: e.fetch_motion_occupancy(L + 1, 0)):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*the field has the levels 0..%d" % L):
                call()
    else:
        for call in (lambda: e.fetch_motion_level(0), lambda: e.fetch_motion_level(1), lambda: e.fetch_motion_occupancy(0, 0),
                     lambda: e.fetch_motion_occupancy(1, 1)):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*" + cm.REFUSAL_C["motion"]):
                call()
    if "temporal" in m.products:
        votes, added = e.fetch_temporal()
        assert votes.tobytes() + added.tobytes() == m.products["temporal"], "product temporal differs from the model"
    else:
        with _refuses_b("temporal"):
            e.fetch_temporal()
    if "temporal_field" in m.products:
        got = e.fetch_temporal_motion()
        _same_rows(got, m.avote.rows, "the vote's field")
        assert (got["grid"], got["edge"], got["apron"], got["search"]) == ((m.grid,) + m.vote_params), "the scalars of the vote's field"
    else:
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*" + cm.REFUSAL_E["temporal_field"]):
            e.fetch_temporal_motion()
    _ring_equals_model(e, m)


@pytest.mark.parametrize("seed", cm.SEEDS_E)
def test_chain_e(eng, cams, masks, frames, seed):
    """Family E: test_chain_c's loop with the aligned vote (vc_hull_temporal_motion) and the motion pyramid
    (vc_hull_motion_pyramid) among the operations.  After every operation also every level of the motion field, the votes, the
    vote's field and the ring; a refusal the model draws must raise with the model's words, and the whole comparison then holds
    as before.  The engine is the one the chains before have used: set_cameras empties the registers and the ring."""
    e = eng
    sc, ops = cm.draw_chain(seed)
    _setup(e, sc, cams, masks, frames)
    m = cm.model_of(seed)
    with _at(seed, "start", {"op": "nothing"}):
        assert not m.ring() and not set(m.products)
        _registers_equal_model(e, m)
        _votes_and_levels_equal_model(e, m)
    for step, op in enumerate(ops):
        out = m.apply(op)
        with _at(seed, step, op):
            _run_e(e, sc, step, op, out)
            _result_equals_model(e, m)
            _registers_equal_model(e, m)
            _votes_and_levels_equal_model(e, m)

    def after():
        _registers_equal_model(e, m)
        _votes_and_levels_equal_model(e, m)
    _end_of_chain(e, sc, m, seed, after=after, run=_run_e)
