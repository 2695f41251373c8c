"""The restatement of the motion-compensated vote (tests/temporal_motion_np.py) against itself and against its purpose, without a
device: the literal definition equals the whole-volume state machine; with nothing moving it is the plain vote call for call; on a
figure that walks it keeps the figure and the plain vote loses it; the ABI surface (header, signatures, stats fields); the
frame chain's temporal_motion setting, its validation and the recorded calls with it on and off."""
import ctypes
import os
import re

import numpy as np
import pytest

from unittest.mock import MagicMock

import fixtures_util as fx
import motion_np as mo
import temporal_motion_np as tm
import temporal_np as tn

from voxcarve import _lib, assignment, motion
from voxcarve.engine import CarveEngine


@pytest.mark.parametrize("grid,window,pairs,params", [((5, 7, 3), 3, [(2, 1), (3, 3)], (4, 0, 1)), ((9, 11, 7), 2, [(2, 2), (1, 1)], (4, 1, 1)),
                                                      ((5, 7, 3), 1, [(1, 1)], (4, 0, 1))])
def test_literal_equals_aligned_vote(grid, window, pairs, params):
    hulls = tm.moving_boxes(grid, 11 + grid[0], 2 * window + 2, params[2], bodies=2, flips=0.05)
    lit, av = tm.Literal(window), tm.AlignedVote()
    moved = 0
    for t, h in enumerate(hulls):
        on, off = pairs[(t * len(pairs)) // len(hulls)]
        a = lit.push(h, on, off, *params)
        b = av.push(h, window, on, off, *params)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert all(b[2][k] == v for k, v in a[2].items()), (a[2], b[2])
        for key in ("block", "d", "cost", "cost0", "count_a", "count_b", "ties", "flags"):
            assert np.array_equal(np.asarray(lit.rows[key]).astype(np.int64), np.asarray(av.rows[key]).astype(np.int64)), key
        for x, y in zip(lit.ring, av.ring):
            assert np.array_equal(x, y)
        moved += b[2]["moved"]
    assert moved > 0


def test_align_moves_listed_blocks_and_leaves_the_rest():
    grid, b = (9, 11, 7), 4
    rng = np.random.default_rng(2)
    vol = rng.random((7, 9, 11)) < 0.5
    # block (1, 2, 0) moves by (1, -2, 1), block (0, 0, 1) is listed with d = 0, every other block is unlisted
    nbx, nby, _ = mo.block_dims(grid, b)
    rows = mo._rows(grid, b, 2, [(0 * nbx + 1) * nby + 2, (1 * nbx + 0) * nby + 0], [(1, -2, 1), (0, 0, 0)], [0, 0], [0, 0], [1, 1], [1, 1], [1, 1])
    out = tm.align(rows, vol, grid, b)
    want = vol.copy()
    for iz in range(0, 4):
        for ix in range(4, 8):
            for iy in range(8, 11):
                sz, sx, sy = iz - 1, ix - 1, iy + 2
                want[iz, ix, iy] = vol[sz, sx, sy] if 0 <= sz < 7 and 0 <= sx < 9 and 0 <= sy < 11 else False
    assert np.array_equal(out, want) and (out != vol).any()
    assert not out[0, 4:8, 8:11].any()                          # (sources at z = -1 lie outside the grid)


@pytest.mark.parametrize("still", ["equal hulls", "nothing within reach"])
def test_without_motion_it_is_the_plain_vote(still):
    """Every hull equal: every listed block has cost 0 at d = 0.  Or hulls so far apart that no displacement of the range brings
    anything into a block's window: every cost is the same, and the smallest |d| wins."""
    grid = (12, 16, 10)
    if still == "equal hulls":
        base = tm.moving_boxes(grid, 5, 1, 1, flips=0.1)[0]
        hulls = [base] * 6
    else:
        hulls = []
        for t in range(6):
            h = np.zeros((10, 12, 16), dtype=bool)
            h[1 + 4 * (t % 2), 1 + 4 * (t % 3), 1 + 4 * (t % 4)] = True  # one voxel inside a block, a block away from the last one
            hulls.append(h)
    av, pv = tm.AlignedVote(), tn.Vote()
    for t, h in enumerate(hulls):
        on, off = ((2, 2), (3, 1))[t // 3]
        o, c, st = av.push(h, 3, on, off, 4, 0, 1)
        p, pc, pst = pv.push(h, 3, on, off)
        assert st["moved"] == 0
        assert np.array_equal(o, p) and np.array_equal(c, pc)
        assert all(st[k] == v for k, v in pst.items()) and st["aligned_changed"] == st["raw_changed"]
        for age in range(st["frames"]):
            assert np.array_equal(av.history(age), pv.history(age))


def _ellipsoid_run(centre, step):
    rng = np.random.default_rng(1)
    av, pv = tm.AlignedVote(), tn.Vote()
    out = []
    for t in range(9):
        clean, noisy = tm.ellipsoid_scene(t, centre, step, rng)
        o, _, st = av.push(noisy, 5, 3, 3, 8, 4, 4)
        p, _, _ = pv.push(noisy, 5, 3, 3)
        out.append((mo.iou(noisy, clean), mo.iou(p, clean), mo.iou(o, clean), st))
        print("frame %d: raw %.3f plain %.3f compensated %.3f raw_changed %d aligned_changed %d" % ((t,) + out[-1][:3] + (st["raw_changed"], st["aligned_changed"])))
    return out


def test_quality_moving_ellipsoid():
    """A 7 / 5 / 9 ellipsoid in 40^3 that moves (2, -1, 1) a frame, 10 % drop-outs and 0.3 % specks, 3 of 5, 8 / 4 / 4: from frame
    4 on the compensated vote is the clean figure to 0.95 and the plain vote has lost it (measured: 0.985 - 0.992, 0.299 - 0.307)."""
    for t, (raw, plain, comp, st) in enumerate(_ellipsoid_run((10, 26, 12), (2, -1, 1))):
        if t >= 4:
            assert comp >= 0.95 and plain <= 0.40, (t, raw, plain, comp)
            assert st["aligned_changed"] < st["raw_changed"] and st["moved"] > 0


def test_quality_at_rest():
    """The same figure standing still: the two votes agree to 0.02 in every frame (measured: 0.007)."""
    for t, (raw, plain, comp, st) in enumerate(_ellipsoid_run((20, 20, 20), (0, 0, 0))):
        assert abs(comp - plain) <= 0.02, (t, plain, comp)


# ---- the ABI surface ----
def _header():
    return open(os.path.join(fx.ROOT, "include", "voxcarve.h")).read()


def test_header_declares_the_calls():
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    flat = " ".join(h.split())
    assert ("int vc_hull_temporal_motion(vc_ctx *ctx, uint32_t window, uint32_t keep_on, uint32_t keep_off, uint32_t block, uint32_t apron, "
            "uint32_t search, uint32_t flags , vc_temporal_motion_stats_t *stats);") in flat
    assert "int vc_fetch_temporal_motion(vc_ctx *ctx, vc_motion_t *rows , uint64_t *count );" in flat
    assert "#define VC_KERNEL_KINDS 28" in _header()


def test_signatures_and_stats_fields():
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    res, args = _lib.SIGNATURES["vc_hull_temporal_motion"]
    assert res is ctypes.c_int and args == [_lib.c_ctx] + [u32] * 7 + [ctypes.POINTER(motion.TemporalMotionStats)]
    assert _lib.SIGNATURES["vc_fetch_temporal_motion"] == _lib.SIGNATURES["vc_fetch_motion"]
    # the struct against the header's typedef, field by field
    body = re.search(r"typedef struct \{([^}]*)\} vc_temporal_motion_stats_t;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            want += [(n.strip(), {"uint32_t": u32, "uint64_t": u64, "float": ctypes.c_float}[ctype]) for n in names.split(",")]
    assert motion.TemporalMotionStats._fields_ == want
    assert [n for n, _ in want] == ["window", "frames", "on", "off", "block", "apron", "search", "reserved", "survivors_before", "survivors_after",
                                    "added", "removed", "raw_changed", "aligned_changed", "out_changed", "blocks", "listed", "moved", "unique",
                                    "clipped", "cost0_sum", "cost_sum", "temporal_ms"]
    assert ctypes.sizeof(motion.TemporalMotionStats) == 32 + 14 * 8 + 8


def test_vote_params():
    assert motion.vote_params(None) is None
    assert motion.vote_params(True) == (8, 4, 4)
    assert motion.vote_params((16, None, 8)) == (16, 8, 8) and motion.vote_params([4, 0, 1]) == (4, 0, 1)
    for bad in (False, 8, "8", (8, 4), (8, 4, 4, 1), (5, 0, 1), (8, 17, 1), (8, 4, 0), (8, 4, 9), (16, 16, 9), (None, 4, 4), (8, 4, None),
                (8.0, 4, 4), (True, 4, 4)):
        with pytest.raises(ValueError):
            motion.vote_params(bad)


# ---- the frame chain ----
class _RecordingEngine:
    """CarveEngine replaced by a recorder of the methods called on it (a fixture of this file's own, after test_frame_chain's)."""
    radius_r2 = staticmethod(CarveEngine.radius_r2)
    _dist_flags = staticmethod(CarveEngine._dist_flags)
    temporal_thresholds = staticmethod(CarveEngine.temporal_thresholds)
    grid = bounds = cameras = image_size = None

    def __init__(self, device=0):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kwargs):
            if name == "set_grid":
                self.grid, self.bounds = tuple(args[:3]), tuple(args[3])
            if name == "set_cameras":
                self.cameras, self.image_size = list(args[0]), (args[1], args[2])
            out = (np.zeros(0, np.uint32), np.zeros((0, 3), np.uint8), np.zeros(0, bool)) if name == "fetch" else MagicMock(name=name)
            if name == "axes":
                out = tuple(np.arange(n, dtype=np.float64) for n in self.grid)
            self.calls.append((name, args, kwargs, out))
            return out
        return call


@pytest.fixture
def chain(monkeypatch):
    saved = dict(assignment._settings)
    monkeypatch.setattr(assignment, "CarveEngine", _RecordingEngine)
    monkeypatch.setattr(assignment, "load_cameras", lambda path, n: ["camera %d" % c for c in range(n)])

    def run(**settings):
        sets = [([np.zeros((4, 6, 3), np.uint8)] * 4, [np.zeros((4, 6), np.uint8)] * 4)] * 2
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), **dict(saved, **settings))
    try:
        yield run
    finally:
        assignment.configure(frame_source=None, **saved)


def _votes():
    return [(c[1], c[2]) for c in assignment._engine.calls if c[0] == "temporal_filter"]


def test_temporal_motion_is_a_setting_of_the_temporal_stage():
    stage = [s for s in assignment.STAGES if s.name == "temporal"][0]
    assert stage.defaults == {"temporal_window": 0, "temporal_keep": None, "temporal_keep_off": None, "temporal_motion": None}
    assert assignment._settings["temporal_motion"] is None
    assert "temporal_motion" in assignment.configure.__doc__


def test_chain_calls_the_vote_with_and_without_motion(chain):
    chain(mode="lut", temporal_window=3, hull_close_mm=1)
    assignment.set_voxel_positions(8, 4, 8)
    assert _votes() == [((3, None, None), {})]                   # the call it always was
    names = [c[0] for c in assignment._engine.calls]
    assert names.index("carve") < names.index("temporal_filter") < names.index("close_hull")
    for setting in (True, (4, 0, 1), (16, None, 8)):
        chain(mode="lut", temporal_window=5, temporal_keep=4, temporal_keep_off=2, temporal_motion=setting, hull_close_mm=1)
        assignment.set_voxel_positions(8, 4, 8)
        assert _votes() == [((5, 4, 2), {"motion": setting})]
        names = [c[0] for c in assignment._engine.calls]
        assert names.index("carve") < names.index("temporal_filter") < names.index("close_hull")
        assert assignment.temporal() is [c[3] for c in assignment._engine.calls if c[0] == "temporal_filter"][0]
    chain(mode="lut", temporal_motion=True)                      # the window is what turns the stage on
    assignment.set_voxel_positions(8, 4, 8)
    assert _votes() == []


def test_configure_refuses_bad_temporal_motion(chain):
    chain(mode="lut", temporal_window=3, temporal_motion=(8, 4, 4))
    before = dict(assignment._settings)
    for bad in (False, 8, (8, 4), (5, 0, 1), (8, 4, 9), (16, 16, 9), "fast"):
        with pytest.raises(ValueError):
            assignment.configure(temporal_motion=bad)
    assert all(assignment._settings[k] is before[k] for k in ("temporal_motion", "temporal_window"))
