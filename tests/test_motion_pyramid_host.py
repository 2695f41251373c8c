"""The host side of vc_hull_motion_pyramid without a device: the header's struct and prototypes against voxcarve.motion and
_lib.SIGNATURES, motion.check_pyramid / reach / level_grid against the restatement, the keyword of CarveEngine.hull_motion, and the
motion stage of the frame chain with motion_levels on the recording engine of test_frame_chain.py."""
import ctypes
import inspect
import os
import re

import pytest

import fixtures_util as fx
import motion_pyramid_np as mp
from test_frame_chain import chain  # noqa: F401  (a fixture)
from voxcarve import _lib, assignment, engine, motion


def _header():
    return open(os.path.join(fx.ROOT, "include", "voxcarve.h")).read()


def test_stats_struct_is_the_headers():
    body = re.search(r"typedef struct \{([^}]*)\} vc_motion_pyramid_stats_t;", _header()).group(1)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S).strip()
        if decl:
            names += [re.sub(r"\[.*", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in motion.PyramidStats._fields_]
    nine = [f[0] for f in motion.MotionStats._fields_][:9]
    assert names[:9] == nine                                     # the nine integers of vc_motion_stats_t, in its order
    # 9 + 6 u64, 4 + 12 u32, a float and the tail's padding
    assert ctypes.sizeof(motion.PyramidStats) == 192 and motion.PyramidStats.listed_level.offset == 88
    assert motion.PyramidStats.dims_level.offset == 120 and motion.PyramidStats.evaluated.offset == 168
    assert motion.PyramidStats.motion_ms.offset == 184


def test_prototypes_and_signatures():
    header = _header()
    u32, ctx = ctypes.c_uint32, _lib.SIGNATURES["vc_hull_motion"][1][0]
    assert re.search(r"int vc_hull_motion_pyramid\(vc_ctx \*ctx(,\s+uint32_t \w+){7}\s*/\* must be 0 \*/,\s*vc_motion_pyramid_stats_t \*stats\);", header)
    assert _lib.SIGNATURES["vc_hull_motion_pyramid"] == (ctypes.c_int, [ctx] + [u32] * 7 + [ctypes.POINTER(motion.PyramidStats)])
    assert _lib.SIGNATURES["vc_fetch_motion_level"] == (ctypes.c_int, [ctx, u32, ctypes.c_void_p, _lib.c_u64p])
    assert _lib.SIGNATURES["vc_fetch_motion_occupancy"] == (ctypes.c_int, [ctx, u32, u32, _lib.c_u64p, _lib.c_u64p])
    assert _lib.SIGNATURES["vc_hull_motion"][1][-1]._type_ is motion.MotionStats       # (the old call keeps its struct)
    for name in ("VcPyramidStats", "VcMotionPyramidStats"):
        assert not hasattr(_lib, name)                           # the struct lives in voxcarve.motion


def test_check_pyramid():
    assert motion.check_pyramid(0, 1, 4) == (0, 1) and motion.check_pyramid(3, 8, 8) == (3, 8) and motion.MAX_LEVELS == 3
    for levels, refine, search in ((4, 1, 4), (-1, 1, 4), (1, 0, 4), (1, 5, 4), (0, 0, 4), (0, 5, 4), (True, 1, 4), (1, True, 4), (1.0, 1, 4),
                                   (None, 1, 4), (1, None, 4)):
        with pytest.raises(ValueError, match="motion: "):
            motion.check_pyramid(levels, refine, search)
    assert motion.check_params(8, None, 4) == (8, 4, 4)          # (as it was)
    for s, L, r in ((4, 0, 1), (4, 2, 1), (8, 3, 8), (1, 1, 1)):
        assert motion.reach(s, L, r) == mp.reach(s, L, r)
    assert motion.reach(8, 3, 8) == 120
    for grid in ((5, 7, 3), (24, 130, 20), (1, 1, 1)):
        for level in range(4):
            assert motion.level_grid(grid, level) == mp.level_grid(grid, level)
    assert (motion.FLAG_CLIPPED, motion.FLAG_BORROWED) == (mp.FLAG_CLIPPED, mp.FLAG_BORROWED)


def test_stats_dict():
    st = motion.PyramidStats()
    st.listed, st.levels, st.refine, st.reach, st.evaluated, st.borrowed, st.motion_ms = 7, 2, 1, 19, 99, 3, 0.5
    st.listed_level[0], st.listed_level[1] = 7, 2
    st.dims_level[1][2] = 16
    d = motion.pyramid_stats_dict(st)
    assert set(d) == {f[0] for f in motion.PyramidStats._fields_} - {"reserved"}
    assert d["listed_level"] == [7, 2, 0, 0] and d["dims_level"][1] == [0, 0, 16] and d["motion_ms"] == 0.5
    assert (d["listed"], d["levels"], d["refine"], d["reach"], d["evaluated"], d["borrowed"]) == (7, 2, 1, 19, 99, 3)


def test_engine_keywords():
    sig = inspect.signature(engine.CarveEngine.hull_motion)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("reg", 0), ("block", 8), ("apron", None), ("search", 4),
                                                                                ("levels", 0), ("refine", 1)]
    assert list(inspect.signature(engine.CarveEngine.fetch_motion_level).parameters) == ["self", "level"]
    assert list(inspect.signature(engine.CarveEngine.fetch_motion_occupancy).parameters) == ["self", "level", "which"]


def _motion_calls():
    return [(c[1], c[2]) for c in assignment._engine.calls if c[0] == "hull_motion"]


def test_stage_with_and_without_levels(chain):  # noqa: F811
    assert assignment._settings["motion_levels"] == 0 and assignment._settings["motion_refine"] == 1
    assert "motion_levels" in assignment.configure.__doc__ and "motion_refine" in assignment.configure.__doc__
    chain(frames=2, motion_block=8)
    assignment.set_voxel_positions(8, 4, 8)
    assignment.set_voxel_positions(8, 4, 8)
    assert _motion_calls() == [((1, 8, None, 4), {})]            # the call it always was
    chain(frames=2, motion_block=8, motion_refine=3)             # (a refine radius alone changes nothing)
    assignment.set_voxel_positions(8, 4, 8)
    assignment.set_voxel_positions(8, 4, 8)
    assert _motion_calls() == [((1, 8, None, 4), {})]
    chain(frames=3, motion_block=16, motion_apron=8, motion_search=8, motion_levels=2, motion_refine=2, motion_paint=True)
    for _ in range(3):
        assignment.set_voxel_positions(8, 4, 8)
    assert _motion_calls() == [((1, 16, 8, 8), {"levels": 2, "refine": 2})] * 2
    names = [c[0] for c in assignment._engine.calls]
    assert names.count("keep_hull") == 3 and names.count("paint_motion") == 2 and names.count("fetch_motion") == 2


def test_configure_refuses_bad_levels(chain):  # noqa: F811
    for bad in ({"motion_levels": 4}, {"motion_levels": -1}, {"motion_levels": None}, {"motion_levels": True}, {"motion_refine": 0},
                {"motion_refine": 5}, {"motion_refine": 3, "motion_search": 2}):
        with pytest.raises(ValueError):
            chain(motion_block=8, **bad)
        with pytest.raises(ValueError):
            chain(**bad)                                         # (checked whether or not the stage is on, as its other settings are)
    chain(motion_block=8, motion_search=8, motion_refine=8, motion_levels=3)
