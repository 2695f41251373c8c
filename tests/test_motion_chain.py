"""The motion stage of the frame chain, pinned without a device on the recording engine of test_frame_chain.py: its place between
the skeleton and the output, its calls per frame, the first frame that only keeps, the accessor's message, the paint conflict and
a refused configure()."""
import pytest

from unittest.mock import MagicMock

from test_frame_chain import FULL, SHELL_ARRAYS, chain  # noqa: F401  (chain is a fixture)
from voxcarve import assignment, motion

MESSAGE = "no motion field: configure(motion_block=b) and set_voxel_positions have not run"
HEAD = ["upload_masks", "upload_frame", "carve"]
TAIL = ["fetch", "axes"]


@pytest.fixture
def mchain(chain, monkeypatch):
    monkeypatch.setattr(motion, "describe", lambda *a, **k: MagicMock(name="motion.describe"))
    return chain


def test_stage_sits_between_skeleton_and_output():
    names = [s.name for s in assignment.STAGES]
    assert names.index("motion") == names.index("skeleton") + 1 == names.index("output") - 1
    stage = assignment.STAGES[names.index("motion")]
    assert stage.defaults == {"motion_block": 0, "motion_apron": None, "motion_search": 4, "motion_paint": False}
    assert not stage.on(assignment._settings) and assignment.MOTION_REG == 1
    assert assignment.MOTION_REG not in (assignment.HULL_SUBTRACT_REG, assignment.HULL_CLIP_REG)
    assert "12. motion_block" in assignment.configure.__doc__ and "13. output" in assignment.configure.__doc__


def test_first_frame_keeps_and_later_frames_match(mchain):
    mchain(frames=3, motion_block=8, motion_paint=True)
    with pytest.raises(RuntimeError) as exc:                     # before any frame
        assignment.motion()
    assert str(exc.value) == MESSAGE
    assignment.set_voxel_positions(8, 4, 8)
    e = assignment._engine
    assert e.names() == ["create", "set_grid", "set_cameras"] + HEAD + ["keep_hull"] + TAIL
    assert [c[1] for c in e.calls if c[0] == "keep_hull"] == [(1,)]
    with pytest.raises(RuntimeError) as exc:                     # the first frame has no previous hull
        assignment.motion()
    assert str(exc.value) == MESSAGE
    for frame in (2, 3):
        del e.calls[:]
        assignment.set_voxel_positions(8, 4, 8)
        assert e.names() == HEAD + ["hull_motion", "fetch_motion", "paint_motion", "keep_hull"] + TAIL
        by_name = {c[0]: c for c in e.calls}
        assert by_name["hull_motion"][1] == (1, 8, None, 4) and by_name["keep_hull"][1] == (1,)
        m = assignment.motion()
        assert m["stats"] is by_name["hull_motion"][3] and m["rows"] is by_name["fetch_motion"][3] and set(m) == {"stats", "rows", "description"}
        assert assignment.frame_count == frame


def test_after_every_other_pass_and_without_paint(mchain):
    full = dict(FULL, cluster_paint=False, geodesic_paint=None, motion_block=16, motion_apron=8, motion_search=8)
    mchain(frames=2, **full)
    assignment.set_voxel_positions(8, 4, 8)
    e = assignment._engine
    assert e.names()[-5:] == ["thin_hull", "fetch_skeleton", "keep_hull", "hull_shell", "fetch_shell_viewer"]
    del e.calls[:]
    assert assignment.set_voxel_positions(8, 4, 8) is SHELL_ARRAYS
    assert e.names()[-7:] == ["thin_hull", "fetch_skeleton", "hull_motion", "fetch_motion", "keep_hull", "hull_shell", "fetch_shell_viewer"]
    assert [c[1] for c in e.calls if c[0] == "hull_motion"] == [(1, 16, 8, 8)]


def test_new_cameras_start_the_session_over(mchain):
    mchain(frames=2, motion_block=4)
    assignment.set_voxel_positions(8, 4, 8)
    assignment._sized = None                                     # as a frame set of another size does: set_cameras empties the registers
    e = assignment._engine
    del e.calls[:]
    assignment.set_voxel_positions(8, 4, 8)
    assert "hull_motion" not in e.names() and e.names().count("keep_hull") == 1


def test_paint_conflict_and_a_refused_configure(mchain):
    mchain(frames=2, motion_block=8)
    assignment.set_voxel_positions(8, 4, 8)
    assignment.set_voxel_positions(8, 4, 8)
    e, before, last = assignment._engine, dict(assignment._settings), assignment.motion()
    for bad in ({"motion_paint": True, "cluster_paint": True, "clusters": 2}, {"motion_paint": True, "geodesic_paint": "labels", "extremities": 2},
                {"motion_block": 5}, {"motion_block": True}, {"motion_apron": 17}, {"motion_search": 0}, {"motion_search": 9},
                {"motion_paint": 1}):
        with pytest.raises(ValueError):
            assignment.configure(**bad)
    with pytest.raises(TypeError):
        assignment.configure(motion_blocks=8)
    assert list(assignment._settings) == list(before) and all(assignment._settings[k] is before[k] for k in before)
    assert assignment._engine is e and assignment.motion() is last
