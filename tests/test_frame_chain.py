"""The order in which set_voxel_positions runs a frame's passes, pinned without a device: CarveEngine is replaced by a fake
that records every method called on it.  The sequences are those of the ladder of ifs the drop-in had before its passes
became one table; a pass put at the wrong place in the chain still returns a hull, so only a recorded order can tell."""
import numpy as np
import pytest

from unittest.mock import MagicMock

from voxcarve import assignment, clusters, measure, skeleton
from voxcarve.engine import CarveEngine

SHELL_ARRAYS = (object(), object())


class _RecordingEngine:
    radius_r2 = staticmethod(CarveEngine.radius_r2)
    _dist_flags = staticmethod(CarveEngine._dist_flags)
    temporal_thresholds = staticmethod(CarveEngine.temporal_thresholds)
    grid = bounds = cameras = image_size = None

    def __init__(self, device=0):
        self.calls = [("create", (device,), {}, None)]

    def names(self):
        return [c[0] for c in self.calls]

    def _result(self, name, args, kwargs):
        if name == "component_ranks":
            raise ValueError("the filter removed something")
        if name == "set_grid":
            self.grid, self.bounds = tuple(args[:3]), tuple(args[3])
        if name == "set_cameras":
            self.cameras, self.image_size = list(args[0]), (args[1], args[2])
        if name == "fetch_shell_viewer":
            return SHELL_ARRAYS
        if name == "fetch":
            return np.zeros(0, np.uint32), np.zeros((0, 3), np.uint8), np.zeros(0, bool)
        if name == "axes":
            return tuple(np.arange(n, dtype=np.float64) for n in self.grid)
        return MagicMock(name=name)

    def __getattr__(self, name):
        if name.startswith("_"):                                 # nothing outside the engine keeps state on it
            raise AttributeError(name)

        def call(*args, **kwargs):
            self.calls.append((name, args, kwargs, None))
            out = self._result(name, args, kwargs)
            self.calls[-1] = (name, args, kwargs, out)
            return out
        return call


@pytest.fixture
def chain(monkeypatch):
    saved = dict(assignment._settings)
    monkeypatch.setattr(assignment, "CarveEngine", _RecordingEngine)
    monkeypatch.setattr(assignment, "load_cameras", lambda path, n: ["camera %d" % c for c in range(n)])
    monkeypatch.setattr(measure, "describe", lambda *a: MagicMock(name="measure.describe"))
    monkeypatch.setattr(skeleton, "describe", lambda *a: MagicMock(name="skeleton.describe"))
    monkeypatch.setattr(clusters, "match", lambda *a: MagicMock(name="clusters.match"))

    def run(frames=1, **settings):
        """configure(**settings) with a source of `frames` 4 x 6 frame sets for four cameras."""
        sets = [([np.zeros((4, 6, 3), np.uint8)] * 4, [np.zeros((4, 6), np.uint8)] * 4) for _ in range(frames)]
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), **dict(saved, **settings))
    try:
        yield run
    finally:
        assignment.configure(frame_source=None, **saved)


FULL = dict(mode="lut", hull_subtract=np.zeros(8 * 8 * 8, bool), hull_clip=np.ones(8 * 8 * 8, bool), temporal_window=3, hull_close_mm=1,
            hull_open_mm=1, min_component_voxels=2, hull="photo", clusters=2, cluster_paint=True, extremities=3, geodesic_paint="labels",
            measure="components", measure_profile=True, skeleton="curve", skeleton_anchors="extrema", output="shell", output_level=1)
SETUP = ["create", "set_grid", "set_cameras", "build_lut", "upload_hull", "upload_hull"]
FRAME = ["upload_masks"] + ["upload_frame"] * 4 + [
    "carve",
    "combine_hull", "combine_hull", "temporal_filter",
    "close_hull", "open_hull", "filter_components",
    "photo_carve",
    "cluster_hull", "fetch_clusters", "fetch_cluster_histograms", "paint_clusters",
    "hull_geodesic", "fetch_extrema", "stick_figure", "paint_geodesic",
    "component_ranks", "filter_components",
    "measure_hull", "fetch_measure", "fetch_measure_profile",
    "thin_hull", "fetch_skeleton",
    "hull_shell", "fetch_shell_viewer"]
ACCESSORS = [("hull_ops", "no hull operations: configure(hull_subtract=... or hull_clip=...) and set_voxel_positions have not run"),
             ("temporal", "no temporal vote: configure(temporal_window=T) and set_voxel_positions have not run"),
             ("clusters", "no clusters: configure(clusters=K) and set_voxel_positions have not run"),
             ("extremities", "no extremities: configure(extremities=K) and set_voxel_positions have not run"),
             ("measurements", "no measurements: configure(measure=...) and set_voxel_positions have not run"),
             ("skeleton", "no skeleton: configure(skeleton=...) and set_voxel_positions have not run"),
             ("shell", "no shell: configure(output=\"shell\") and set_voxel_positions have not run")]


def test_every_pass_in_order(chain):
    chain(frames=3, **FULL)
    assert assignment.set_voxel_positions(8, 4, 8) is SHELL_ARRAYS
    e = assignment._engine
    assert e.names() == SETUP + FRAME
    by_name = {}
    for name, args, kwargs, out in e.calls:
        by_name.setdefault(name, []).append((args, kwargs, out))
    assert by_name["set_grid"][0][0][:3] == (8, 8, 8) and by_name["set_cameras"][0][0] == (["camera %d" % c for c in range(4)], 4, 6)
    assert [c[0] for c in by_name["combine_hull"]] == [("andnot", 3), ("and", 2)]
    assert [c[0][1] for c in by_name["upload_hull"]] == [3, 2]
    assert by_name["upload_hull"][0][0][0] is FULL["hull_subtract"] and by_name["upload_hull"][1][0][0] is FULL["hull_clip"]
    assert by_name["filter_components"][0][1] == {"connectivity": 26, "min_voxels": 2, "keep_largest": 0}
    assert by_name["filter_components"][1][1] == {"connectivity": 26}
    assert by_name["hull_shell"][0][0] == (1,) and by_name["thin_hull"][0] [:2] == (("curve",), {"anchors": "extrema"})
    # what the accessors hand out is what the passes returned
    assert assignment.hull_ops() == {"subtract": by_name["combine_hull"][0][2], "clip": by_name["combine_hull"][1][2]}
    assert assignment.temporal() is by_name["temporal_filter"][0][2]
    assert assignment.clusters() is by_name["cluster_hull"][0][2]
    assert assignment.extremities() is by_name["hull_geodesic"][0][2]
    assert assignment.measurements() is by_name["measure_hull"][0][2]
    assert assignment.skeleton()["stats"] is by_name["thin_hull"][0][2] and assignment.skeleton()["skeleton"] is by_name["fetch_skeleton"][0][2]
    assert assignment.shell() is by_name["hull_shell"][0][2]
    assert by_name["cluster_hull"][0][1]["init_mm"] is None
    first = assignment.clusters()

    # the second frame sets nothing up again and starts the clusters from the first frame's centres
    del e.calls[:]
    assert assignment.set_voxel_positions(8, 4, 8) is SHELL_ARRAYS
    assert e.names() == FRAME
    assert [c for c in e.calls if c[0] == "cluster_hull"][0][2]["init_mm"] is first["centres_mm"]
    assert assignment.clusters() is not first and assignment.frame_count == 2

    # a refused configure() changes nothing: neither the settings nor the last results
    before = dict(assignment._settings)
    last = {name: getattr(assignment, name)() for name, _ in ACCESSORS}
    for bad, exc in (({"clusters": 99}, ValueError), ({"no_such_setting": 1}, TypeError), ({"measure": "clusters", "clusters": 0}, ValueError),
                     ({"extremities": 0}, ValueError), ({"output": "all"}, ValueError)):
        with pytest.raises(exc):
            assignment.configure(**bad)
    assert list(assignment._settings) == list(before) and all(assignment._settings[k] is before[k] for k in before)
    assert all(getattr(assignment, name)() is last[name] for name, _ in ACCESSORS) and assignment._engine is e
    del e.calls[:]
    assert assignment.set_voxel_positions(8, 4, 8) is SHELL_ARRAYS and e.names() == FRAME and assignment.frame_count == 3
    assert assignment.set_voxel_positions(8, 4, 8) == ([], [])                   # the end of the video


def test_visible_colouring_stands_where_the_photo_carve_did(chain):
    chain(color_mode="visible")
    pos, col = assignment.set_voxel_positions(8, 4, 8)
    assert assignment._engine.names() == ["create", "set_grid", "set_cameras", "upload_masks"] + ["upload_frame"] * 4 + [
        "carve", "color_visible", "fetch", "axes"]
    assert pos.shape == (0, 3) and pos.dtype == np.float32 and col.shape == (0, 3) and col.dtype == np.float32


def test_defaults_end_in_the_full_fetch(chain):
    chain()
    pos, col = assignment.set_voxel_positions(8, 4, 8)
    e = assignment._engine
    assert e.names() == ["create", "set_grid", "set_cameras", "upload_masks", "upload_frame", "carve", "fetch", "axes"]
    assert pos.shape == (0, 3) and pos.dtype == np.float32 and col.shape == (0, 3) and col.dtype == np.float32
    s = assignment._settings
    assert [c for c in e.calls if c[0] == "upload_frame"][0][1][0] == s["color_camera"]
    assert [c for c in e.calls if c[0] == "carve"][0][2] == {"slot": 0, "min_views": s["views_threshold"], "color_cam": s["color_camera"],
                                                             "mode": s["mode"], "footprint": s["footprint"]}


def test_accessors_refuse_after_configure(chain):
    chain(**FULL)
    for name, message in ACCESSORS:                              # before any frame
        with pytest.raises(RuntimeError) as exc:
            getattr(assignment, name)()
        assert str(exc.value) == message
    assignment.set_voxel_positions(8, 4, 8)
    chain(**FULL)                                                # ... and after a configure() that follows one
    assert assignment._engine is None and not assignment.initialized and assignment.frame_count == 0
    for name, message in ACCESSORS:
        with pytest.raises(RuntimeError) as exc:
            getattr(assignment, name)()
        assert str(exc.value) == message
    with pytest.raises(RuntimeError, match="set_voxel_positions has not run"):
        assignment.voxels_status()
    with pytest.raises(RuntimeError, match="set_voxel_positions has not run"):
        assignment.render_views()
    with pytest.raises(RuntimeError, match="set_voxel_positions has not run"):
        assignment.surface_mesh()
