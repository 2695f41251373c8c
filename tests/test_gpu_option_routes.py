"""The options of vc_set_option that no other test sets: surface_order, kernel_events, launch_events, event_scope, stream_priority
and reserve_cus.  The last four rebuild the streams and events that order overlapped carve steps, and the shipped defaults are the
aggressive settings; the conservative ones are the documented cross-check.

One workload on the 64^3 golden scene: two overlapped steps on slots 0 and 1 with different mask sets, both collected, then close ->
open -> filter_components -> color_visible -> surface_mesh on the current result.  The records of both steps equal oracle.carve_c;
everything behind them equals, byte for byte, the run under the default options -- under each setting, one at a time."""
import numpy as np
import pytest

import fixtures_util as fx

pytestmark = pytest.mark.gpu

GRID = (64, 64, 64)
ROLL = 9                                        # columns the masks of slot 1 are rolled by: another hull
DEFAULTS = {"launch_events": 1, "event_scope": 1, "stream_priority": 1, "reserve_cus": 0, "kernel_events": 0, "surface_order": 1,
            "timing_detail": 0}
STEP_KINDS = 14                                 # vc_kernel_kind below VC_K_DIST_BOX: the kernels of a carve step
IN_FLIGHT = "carve steps are in flight"


@pytest.fixture(scope="module")
def scene(built, cams, masks, frames):
    from oracle import carve_c
    sets = [masks, [np.ascontiguousarray(np.roll(m, ROLL, axis=1)) for m in masks]]
    want = []
    for s in sets:
        w = carve_c.carve(*GRID, fx.oracle_cams(cams), s, frames)
        bgr = w["bgr"].astype(np.uint64)
        want.append(w["idx"].astype(np.uint64) | (bgr[:, 2] << np.uint64(32)) | (bgr[:, 1] << np.uint64(40)) | (bgr[:, 0] << np.uint64(48)) |
                    (np.uint64(1) << np.uint64(56)))
    assert want[0].size > 1000 and want[1].size > 1000 and not np.array_equal(want[0], want[1])
    return sets, want


@pytest.fixture(scope="module")
def eng(built, cams, masks, frames, scene):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    e.set_grid(*GRID)
    e.set_cameras(cams, *masks[0].shape)
    for slot, s in enumerate(scene[0]):
        e.upload_masks(s, slot=slot)
        for c in range(4):                       # (the same images in both slots: the oracle's colours, color_visible's cameras)
            e.upload_frame(c, frames[c], slot=slot)
    yield e
    e.close()


def _workload(e, want):
    """Returns (what the passes behind the carves left, as a list of (name, bytes or stats), the mesh's point_tests)."""
    e.touch_masks(0)                             # every run pays for its own preparation: the same launches each time
    e.touch_masks(1)
    e.carve_begin(slot=0)
    e.carve_begin(slot=1)
    assert e.carve_end() == want[0].size
    assert np.array_equal(e.fetch_records(), want[0]), "records of the step on slot 0"
    assert e.carve_end() == want[1].size
    assert np.array_equal(e.fetch_records(), want[1]), "records of the step on slot 1"
    got = []

    def keep(name, st, drop):
        got.append((name + " stats", {k: v for k, v in st.items() if k not in drop}))
        got.append((name + " records", e.fetch_records().tobytes()))

    keep("close", e.close_hull(40), ("grow_ms",))
    got.append(("added", e.fetch_added().tobytes()))
    keep("open", e.open_hull(25), ("morph_ms",))
    keep("filter_components", e.filter_components(keep_largest=1), ("components_ms",))
    got.append(("component labels", e.fetch_component_labels().tobytes()))
    e.color_visible(slot=0)
    got.append(("color_visible records", e.fetch_records().tobytes()))
    got.append(("visibility", e.fetch_visibility().tobytes()))
    mesh = e.surface_mesh()
    for k in ("verts", "faces", "rgb", "refined"):
        got.append(("mesh " + k, np.ascontiguousarray(mesh[k]).tobytes()))
    got.append(("mesh stats", {k: mesh["stats"][k] for k in ("n_verts", "n_faces", "refined", "unrefined")}))
    got.append(("occupancy", e.fetch_occupancy().tobytes()))
    return got, mesh["stats"]["point_tests"]


@pytest.fixture(scope="module")
def baseline(eng, scene):
    for name, value in DEFAULTS.items():
        eng.set_option(name, value)
    got, point_tests = _workload(eng, scene[1])
    d = dict(got)
    assert d["close stats"]["added"] > 0 and d["open stats"]["survivors_after"] < d["open stats"]["survivors_before"]
    assert d["mesh stats"]["n_verts"] > 0 and d["mesh stats"]["refined"] > 0 and point_tests > 0
    return got


def _equal(got, want):
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert a == b, name


@pytest.mark.parametrize("name,value", [("launch_events", 0), ("event_scope", 0), ("event_scope", 2), ("stream_priority", 0),
                                        ("reserve_cus", 2), ("surface_order", 0)])
def test_setting_gives_the_bytes_of_the_defaults(eng, scene, baseline, name, value):
    """surface_order 0 included: the same vertices, faces, colours and refined flags; its point_tests statistic is a diagnostic
    of the order the cameras are tried in (include/voxcarve.h) and is not compared under any setting."""
    eng.set_option(name, value)
    try:
        got, _ = _workload(eng, scene[1])
    finally:
        eng.set_option(name, DEFAULTS[name])
    _equal(got, baseline)
    _equal(_workload(eng, scene[1])[0], baseline)                # (and the defaults, restored, still do)


def test_kernel_events(eng, scene, baseline):
    """kernel_events = 1 changes no byte and fills vc_timing_t::kernel_ms_sum / kernel_launches for the kernels of the carve steps,
    with the launch counts that a timing_detail run of the same workload gives them; the launches of the post-carve passes carry
    events under timing_detail alone."""
    from voxcarve import _lib
    runs = {}
    for name in ("kernel_events", "timing_detail"):
        eng.timing(reset=True)
        eng.set_option(name, 1)
        try:
            got, _ = _workload(eng, scene[1])
        finally:
            eng.set_option(name, 0)
        _equal(got, baseline)
        runs[name] = eng.timing(reset=True)
    step_kinds, pass_kinds = _lib.KERNEL_KINDS[:STEP_KINDS], _lib.KERNEL_KINDS[STEP_KINDS:]
    ke, td = runs["kernel_events"]["kernels"], runs["timing_detail"]["kernels"]
    assert ke and set(ke) <= set(step_kinds), sorted(ke)
    assert {k: v["launches"] for k, v in ke.items()} == {k: v["launches"] for k, v in td.items() if k in step_kinds}
    assert "k_emit" in ke and all(v["launches"] >= 1 and v["ms_sum"] >= 0.0 for v in ke.values())
    assert sum(v["ms_sum"] for v in ke.values()) > 0.0
    assert any(k in td for k in pass_kinds), sorted(td)          # (close and open ran: k_dist_*, k_grow_*)


def test_a_step_in_flight_refuses_what_rebuilds_streams_and_events(eng, scene, baseline):
    from voxcarve._lib import VoxcarveError
    eng.carve_begin(slot=0)
    try:
        for name, value in (("event_scope", 0), ("stream_priority", 0), ("reserve_cus", 2)):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*" + IN_FLIGHT):
                eng.set_option(name, value)
    finally:
        assert eng.carve_end() == scene[1][0].size
    assert np.array_equal(eng.fetch_records(), scene[1][0])
    _equal(_workload(eng, scene[1])[0], baseline)                # (nothing was rebuilt: the defaults' bytes)
