"""What invalidates what among the passes over a carve result, in one table (include/voxcarve.h gives each pass's own rule).

Every product is built once on the 64^3 hull of the four golden cameras.  After each call that changes the result every product's
fetch refuses with its own message, except what that call itself produces; a pass that leaves the hull alone leaves every other
product valid and byte-identical.  The per-pass test_stale_* tests know the passes that existed when they were written; this one
knows the passes that existed before the vote.  It does not know vc_hull_temporal, vc_hull_measure, vc_hull_thin, vc_hull_shell, the
hull registers (vc_hull_keep, vc_hull_combine, vc_hull_compare), vc_hull_motion and vc_hull_warp, nor what vc_texture_render and
vc_light_render make: tests/test_gpu_chain.py covers the registers and the motion field (family C of tests/chain_model.py) and the
passes over a render's images (family D) in random chains, after every step."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID = (64, 64, 64)
RENDER_HW = (48, 64)

# product -> the refusal of its fetch once the result is another
REFUSAL = {
    "visibility": "no visibility",
    "photo_rounds": "no photo rounds",
    "component_labels": "no component labels",
    "distance": "no distance field",
    "grown": "no added flags",
    "normals": "no normals",
    "clusters": "no clusters",
    "geodesic": "no geodesic distances",
}
# what the passes that leave the hull alone build; render and surface mesh are read through vc_fetch_render / vc_fetch_surface_mesh
# and are "of the current result" while vc_shade_render / vc_surface_normals accept them
BUILT = {"visibility", "distance", "normals", "clusters", "geodesic", "render", "surface"}


@pytest.fixture(scope="module")
def eng(built, cams, masks, frames):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    e.set_grid(*GRID)
    e.set_cameras(cams, *masks[0].shape)
    e.upload_masks(masks)
    for c in range(4):                                           # (color_visible and photo_carve look through every camera)
        e.upload_frame(c, frames[c])
    yield e
    e.close()


def _fetches(e):
    return {"visibility": e.fetch_visibility, "photo_rounds": e.fetch_photo_rounds, "component_labels": e.fetch_component_labels,
            "distance": e.fetch_distance_raw, "grown": e.fetch_added, "normals": e.fetch_record_normals,
            "clusters": e.fetch_cluster_labels, "geodesic": e.fetch_geodesic}


def _views(e):
    """Two small views of the grid's centre from outside it."""
    from voxcarve import camera
    b = e.bounds
    ctr = np.array([(b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2])
    H, W = RENDER_HW
    return [camera.look_at(ctr + eye, ctr, 60.0, H, W) for eye in ((2500.0, 1500.0, -2000.0), (-1800.0, 2600.0, -900.0))]


def _light(e):
    return np.tile(np.array([0.0, 0.0, -1.0]), (e._render_shape[0], 1))


def _render_images(e):
    from voxcarve.engine import _ptr
    V, (H, W) = e._render_shape
    idx, depth = np.empty((V, H, W), dtype=np.uint32), np.empty((V, H, W), dtype=np.float32)
    for k in range(V):
        e._check(e._L.vc_fetch_render(e._ctx, k, _ptr(idx[k], ctypes.c_uint32), _ptr(depth[k], ctypes.c_float), None, None), "vc_fetch_render")
    return idx.tobytes() + depth.tobytes()


def _surface_mesh(e, shape):
    from voxcarve.engine import _ptr
    verts, faces = np.empty((shape[0], 3), dtype=np.float64), np.empty((shape[1], 3), dtype=np.uint32)
    e._check(e._L.vc_fetch_surface_mesh(e._ctx, _ptr(verts, ctypes.c_double), _ptr(faces, ctypes.c_uint32), None, None), "vc_fetch_surface_mesh")
    return verts.tobytes() + faces.tobytes()


def _build(e):
    """Every product of the passes that leave the hull alone, once.  Returns the mesh's (V, F)."""
    e.color_visible()
    e.hull_distance(outside=True)
    e.hull_normals()
    e.cluster_hull(2)
    e.hull_geodesic(extrema=2)
    e.render(_views(e), *RENDER_HW)
    st = e.surface_mesh()["stats"]
    return st["n_verts"], st["n_faces"]


def _snapshot(e, mesh_shape):
    """product -> its bytes, for every product that is valid now (render and surface need valid normals to be asked)."""
    from voxcarve._lib import VoxcarveError
    snap = {}
    for name, fetch in _fetches(e).items():
        try:
            snap[name] = fetch().tobytes()
        except VoxcarveError as err:
            assert "VC_ERR_ARG" in str(err) and REFUSAL[name] in str(err), (name, str(err))
    try:
        e.shade_render(_light(e))
        snap["render"] = _render_images(e)
    except VoxcarveError as err:
        assert "no images of the current" in str(err), str(err)
    try:
        e.surface_normals()
        snap["surface"] = _surface_mesh(e, mesh_shape)
    except VoxcarveError as err:
        assert "no mesh of the current" in str(err), str(err)
    return snap


def _fetches_refuse(e, own=()):
    """Every fetch refuses with its message, except those of the products in `own`."""
    from voxcarve._lib import VoxcarveError
    for name, fetch in _fetches(e).items():
        if name in own:
            fetch()
            continue
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*" + REFUSAL[name]):
            fetch()


def _all_stale_but(e, own=()):
    """After a call that changed the result: every product is stale, except what the call itself made."""
    from voxcarve._lib import VoxcarveError
    _fetches_refuse(e, own)
    # the images and the mesh of the hull that is gone: the calls that read them look at the normals first
    e.hull_normals()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no images of the current"):
        e.shade_render(_light(e))
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no mesh of the current"):
        e.surface_normals()


def _passes_that_leave_the_hull_alone(e):
    return [("color_visible", e.color_visible, "visibility"),
            ("hull_distance", lambda: e.hull_distance(outside=True), "distance"),
            ("hull_normals", e.hull_normals, "normals"),
            ("cluster_hull", lambda: e.cluster_hull(2), "clusters"),
            ("hull_geodesic", lambda: e.hull_geodesic(extrema=2), "geodesic"),
            ("render", lambda: e.render(_views(e), *RENDER_HW), "render"),
            ("surface_mesh", e.surface_mesh, "surface"),
            ("shade_render", lambda: e.shade_render(_light(e)), None),
            ("paint_clusters", e.paint_clusters, None),
            ("paint_geodesic", e.paint_geodesic, None)]


def _others_survive(e, own):
    """On the current result, with `own` the products of the call that made it: builds the rest, then runs every pass that leaves
    the hull alone and finds every other product still valid and byte-identical."""
    mesh_shape = _build(e)
    before = _snapshot(e, mesh_shape)
    assert set(before) == BUILT | set(own)
    for what, run, product in _passes_that_leave_the_hull_alone(e):
        run()
        after = _snapshot(e, mesh_shape)
        assert set(after) == set(before), what
        for name in before:
            if name != product:
                assert after[name] == before[name], (what, name)
        before = after


def test_what_each_call_invalidates(eng):
    e = eng
    S = e.carve()
    assert S > 0
    _fetches_refuse(e)                                           # a fresh carve: nothing has been made
    assert e.filter_components()["survivors_after"] == S         # (drops nothing; the sizes pick a min_voxels that does)
    sizes = np.sort(e.fetch_components()["size"])
    assert sizes.size >= 2 and sizes[0] < sizes[-1], "the hull has a fragment that min_voxels can drop"
    largest = int(sizes[-1])

    changes = [("carve", e.carve, lambda st: st == S, ()),
               ("photo_carve", lambda: e.photo_carve(max_rounds=2), lambda st: st["survivors_before"] == S, ("visibility", "photo_rounds")),
               ("filter_components", lambda: e.filter_components(min_voxels=largest), lambda st: st["survivors_after"] < S, ("component_labels",)),
               ("erode_hull", lambda: e.erode_hull(25), lambda st: st["survivors_after"] < S, ()),
               ("close_hull", lambda: e.close_hull(40), lambda st: st["added"] > 0, ("grown",))]
    for what, change, changed, own in changes:
        e.carve()
        mesh_shape = _build(e)
        assert set(_snapshot(e, mesh_shape)) == BUILT, what
        assert changed(change()), what
        _all_stale_but(e, own)
        if own:
            _others_survive(e, own)

    # a grow that adds nothing (the radius is below every grid step) hands the distance field's buffer to its transforms and
    # makes its own flags; everything else stays
    e.carve()
    mesh_shape = _build(e)
    before = _snapshot(e, mesh_shape)
    assert min(e.grid_steps_um()) > 1000
    assert e.dilate_hull(1.0)["added"] == 0
    after = _snapshot(e, mesh_shape)
    assert set(after) == (BUILT - {"distance"}) | {"grown"}
    assert not np.frombuffer(after["grown"], dtype=np.uint8).any()
    for name in BUILT - {"distance"}:
        assert after[name] == before[name], name
