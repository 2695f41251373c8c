"""The restatement of vc_hull_temporal (tests/temporal_np.py) against the definition, on the CPU: the vectorised state machine
against the literal per-voxel one on seeded boolean sequences, the algebra of the vote (window 1, union, intersection, fixed
points, the hysteresis between the two plain votes), the figures of DESIGN section 8 item 17 on the committed cameras and masks
with seeded mask noise, the records of restored voxels, and the public names (header, binding, engine, configure keys, demo)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import temporal_np as tn
from oracle import carve_np

SHAPES = ((5, 7, 3), (9, 11, 7), (12, 64, 10))
WINDOWS = (1, 2, 3, 5, 8, 15)
LOW = np.uint64(0xffffffff)


def _pairs(window, rng):
    """Every (keep_on, keep_off) of a small window, a seeded sample (with the corners) of a large one."""
    every = [(a, b) for a in range(1, window + 1) for b in range(1, a + 1)]
    if window <= 3:
        return every
    pick = {(window, 1), (window, window), (1, 1), (window // 2 + 1, window // 2 + 1)}
    pick |= {every[int(k)] for k in rng.choice(len(every), 3, replace=False)}
    return sorted(pick)


def _sequence(rng, shape, frames, k):
    """Hulls that share a figure and differ by noise; every fifth sequence holds an empty and a solid hull."""
    base = rng.random(shape) < 0.4
    seq = [base ^ (rng.random(shape) < 0.15) for _ in range(frames)]
    if k % 5 == 0 and frames > 3:
        seq[frames // 3] = np.zeros(shape, dtype=bool)
        seq[2 * frames // 3] = np.ones(shape, dtype=bool)
    return seq


def test_vectorised_equals_literal():
    rng = np.random.default_rng(1717)
    runs = 0
    for si, shape in enumerate(SHAPES):
        for window in WINDOWS:
            pairs = _pairs(window, rng)
            if shape == SHAPES[2]:
                pairs = pairs[:2]                                # (7 680 voxels a frame in Python loops)
            for k, (on, off) in enumerate(pairs):
                frames = 2 * window + 2 + (k % 2)
                seq = _sequence(rng, shape, frames, k + si)
                lit, vec = tn.Literal(window), tn.Vote()
                for t, hull in enumerate(seq):
                    want, wc, ws = lit.push(hull, on, off)
                    got, gc, gs = vec.push(hull, window, on, off)
                    assert np.array_equal(got, want) and np.array_equal(gc, wc), (shape, window, on, off, t)
                    assert {n: gs[n] for n in ws} == ws, (shape, window, on, off, t)
                    assert gs["survivors_after"] == gs["survivors_before"] + gs["added"] - gs["removed"] == int(want.sum())
                    assert gs["frames"] == min(t + 1, window) and int(gc.max()) <= gs["frames"] <= tn.MAX_WINDOW
                    for age in range(gs["frames"]):
                        assert np.array_equal(vec.history(age), seq[t - age])
                    with pytest.raises(IndexError):
                        vec.history(gs["frames"])
                runs += 1
    assert runs >= 60


def test_keep_changes_mid_sequence_and_a_window_change_starts_over():
    rng = np.random.default_rng(1718)
    shape = (9, 11, 7)
    seq = _sequence(rng, shape, 14, 0)
    lit, vec = tn.Literal(5), tn.Vote()
    for t, hull in enumerate(seq):
        on, off = ((3, 3), (5, 1), (4, 2))[t // 5]
        assert np.array_equal(vec.push(hull, 5, on, off)[0], lit.push(hull, on, off)[0])
    out, c, st = vec.push(seq[0], 3, 2, 2)                         # another window: the ring and P start over
    assert st["frames"] == 1 and st["on"] == st["off"] == 1 and np.array_equal(out, seq[0]) and st["raw_changed"] == 0
    assert st["out_changed"] == int(seq[0].sum())
    for bad in ((0, 1, 1), (16, 1, 1), (5, 6, 1), (5, 2, 3), (5, 3, 0)):
        with pytest.raises(ValueError):
            tn.Vote().push(seq[0], *bad)


def test_algebra_of_the_vote():
    rng = np.random.default_rng(1719)
    for shape in SHAPES[:2]:
        for window in WINDOWS:
            seq = _sequence(rng, shape, 2 * window + 3, 1)
            ident, union, inter = tn.Vote(), tn.Vote(), tn.Vote()
            hyst = {pair: tn.Vote() for pair in _pairs(window, rng)}
            for t, hull in enumerate(seq):
                m = min(t + 1, window)
                last = seq[t + 1 - m:t + 1]
                if window == 1:
                    out, _, st = ident.push(hull, 1, 1, 1)       # window 1 is the identity
                    assert np.array_equal(out, hull) and st["added"] == st["removed"] == 0
                assert np.array_equal(union.push(hull, window, 1, 1)[0], np.any(last, axis=0))
                got = inter.push(hull, window, window, window)[0]
                assert np.array_equal(got, np.all(last, axis=0))         # (while the ring fills, on = m too)
                for (on, off), v in hyst.items():
                    out, _, st = v.push(hull, window, on, off)
                    lo, hi = tn.plain_vote(last, st["on"]), tn.plain_vote(last, st["off"])
                    assert (lo <= out).all() and (out <= hi).all(), (shape, window, on, off, t)
                    if on == off:
                        assert np.array_equal(out, lo)
            # a constant sequence is a fixed point, whatever the thresholds and whatever came before
            for (on, off), v in hyst.items():
                for t in range(window + 1):
                    out, c, st = v.push(seq[0], window, on, off)
                assert np.array_equal(out, seq[0]) and st["added"] == st["removed"] == st["out_changed"] == st["raw_changed"] == 0
                assert np.array_equal(c, seq[0] * np.uint8(window))


@pytest.fixture(scope="module")
def noisy_hulls():
    """The 64^3 recipe: the four real cameras, the committed masks with 2 % of each mask's pixels flipped per frame, 16 frames, the
    centre rule, min_views = 4 (carved once, shared)."""
    cams, masks = fx.oracle_cams(fx.golden_cameras()), fx.golden_masks()
    n = 64
    hulls = [dn.volume(carve_np.carve(n, n, n, cams, tn.noisy_masks(masks, t))["idx"], (n, n, n)) for t in range(16)]
    clean = dn.volume(carve_np.carve(n, n, n, cams, masks)["idx"], (n, n, n))
    return clean, hulls


def _flicker(seq, first):
    return sum(int((seq[t] ^ seq[t - 1]).sum()) for t in range(first, len(seq)))


def test_flicker_figures_of_the_design(noisy_hulls):
    """The figures of DESIGN section 8 item 17.  Flicker is summed over the transitions between outputs of a full ring: frames 5..15
    for a window of 5, frames 8..15 for a window of 8."""
    clean, hulls = noisy_hulls
    assert int(clean.sum()) == 6981 and np.array_equal(dn.indices(clean), fx.expected(64)[0])

    def run(window, on, off):
        v = tn.Vote()
        return [v.push(h, window, on, off)[0] for h in hulls]

    raw = _flicker(hulls, 5)
    vote35, hyst, vote48 = run(5, 3, 3), run(5, 4, 2), run(8, 4, 4)
    figures = (raw, _flicker(vote35, 5), _flicker(hyst, 5), _flicker(vote48, 8))
    print("flicker raw %d, 3-of-5 %d, 4-on / 2-off %d, 4-of-8 %d" % figures)
    assert figures == (13925, 323, 192, 7)
    assert 10 * figures[1] <= raw                                 # the property that matters
    last = (int(hulls[15].sum()), int(vote35[15].sum()), int((vote35[15] & ~hulls[15]).sum()), int((hulls[15] & ~vote35[15]).sum()))
    assert last == (6539, 6958, 573, 154)
    # the vote is closer to the clean hull than the frame is
    assert int((vote35[15] ^ clean).sum()) < int((hulls[15] ^ clean).sum()) // 4


def test_records_of_restored_voxels(noisy_hulls):
    """records_after: kept records byte for byte, dropped ones gone, restored ones coloured by the pixel under the centre with
    seen = 1, vote bytes = the counts."""
    clean, hulls = noisy_hulls
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    H, W = masks[0].shape
    frames = fx.synthetic_frames(4, H, W)
    n = 64
    grid = (n, n, n)
    v = tn.Vote()
    for h in hulls[:5]:
        out, c, st = v.push(h, 5, 3, 3)
    hull = hulls[4]
    rec = dn.indices(hull).astype(np.uint64) | (np.uint64(0x01a1b2c3) << np.uint64(32))
    got, votes, added = tn.records_after(rec, hull, out, c, grid, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(cams)[1], frames[1], H, W)
    assert got.size == st["survivors_after"] and int(added.sum()) == st["added"] > 0 and st["removed"] > 0
    assert (np.diff((got & LOW).astype(np.int64)) > 0).all() and np.array_equal((got & LOW).astype(np.int64), np.flatnonzero(out.reshape(-1)))
    kept = rec[out.reshape(-1)[(rec & LOW).astype(np.int64)]]
    assert np.array_equal(got[added == 0], kept) and kept.size == rec.size - st["removed"]
    fresh = got[added == 1]
    pts = carve_np.points_of_indices((fresh & LOW).astype(np.int64), n, n, n)
    off = carve_np.pixel_offsets(carve_np.project_points(pts, cams[1].R, cams[1].tvec, cams[1].K, cams[1].dist), H, W)
    assert (off >= 0).all() and ((fresh >> np.uint64(56)) == 1).all()
    px = frames[1].reshape(-1, 3)[off]
    for shift, ch in ((32, 2), (40, 1), (48, 0)):
        assert np.array_equal(((fresh >> np.uint64(shift)) & np.uint64(255)).astype(np.uint8), px[:, ch])
    assert np.array_equal(votes, c.reshape(-1)[(got & LOW).astype(np.int64)]) and votes.min() >= 3 and votes.max() <= 5
    assert (votes[added == 1] <= 4).all()                        # (a restored voxel is not in the newest hull)
    bare, _, _ = tn.records_after(rec, hull, out, c, grid, carve_np.DEFAULT_BOUNDS)
    assert ((bare[added == 1] >> np.uint64(32)) == 0).all()


def test_public_names():
    from voxcarve import _lib, assignment
    from voxcarve.engine import CarveEngine
    header = open(os.path.join(fx.ROOT, "include", "voxcarve.h")).read()
    assert "#define VC_TEMPORAL_MAX_WINDOW 15u" in header and _lib.VC_TEMPORAL_MAX_WINDOW == 15 == tn.MAX_WINDOW
    for line in ("int vc_hull_temporal(vc_ctx *ctx, uint32_t window, uint32_t keep_on, uint32_t keep_off, uint32_t flags /* must be 0 */, "
                 "vc_temporal_stats_t *stats);",
                 "int vc_fetch_temporal(vc_ctx *ctx, uint8_t *votes, uint8_t *added);",
                 "int vc_fetch_temporal_history(vc_ctx *ctx, uint32_t age, uint8_t *bits);",
                 "int vc_temporal_reset(vc_ctx *ctx);",
                 "    uint32_t window, frames /* m */, on, off /* the effective thresholds of this call */;",
                 "    uint64_t survivors_before, survivors_after, added, removed, raw_changed, out_changed;",
                 "    float temporal_ms;\n} vc_temporal_stats_t;"):
        assert line in header, line
    for name in ("vc_hull_temporal", "vc_fetch_temporal", "vc_fetch_temporal_history", "vc_temporal_reset"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vc_hull_temporal"][1]) == 6
    fields = ["window", "frames", "on", "off", "survivors_before", "survivors_after", "added", "removed", "raw_changed", "out_changed",
              "temporal_ms"]
    assert [f[0] for f in _lib.VcTemporalStats._fields_] == fields
    assert ctypes.sizeof(_lib.VcTemporalStats) == 4 * 4 + 6 * 8 + 8 and _lib.VcTemporalStats.survivors_before.offset == 16
    # the kernel kinds: three new ones behind the geodesic's four, the grow kinds still last
    assert "#define VC_KERNEL_KINDS 28" in header and _lib.VC_KERNEL_KINDS == 28 == len(_lib.KERNEL_KINDS)
    enum = header[header.index("typedef enum {\n    VC_K_PREP_PACK"):header.index("} vc_kernel_kind;")]
    order = [w for w in enum.replace(",", " ").split() if w.startswith("VC_K_")]
    assert len(order) == 28
    at = order.index("VC_K_TEMPORAL_VOTE")
    assert order[at - 1] == "VC_K_GEO_ARGMAX" and order[at:] == ["VC_K_TEMPORAL_VOTE", "VC_K_TEMPORAL_RANK", "VC_K_TEMPORAL_MERGE",
                                                               "VC_K_GROW_MARK", "VC_K_GROW_RANK", "VC_K_GROW_MERGE"]
    assert _lib.KERNEL_KINDS[at:] == ("k_temporal_vote", "temporal_rank", "temporal_merge", "k_grow_mark", "grow_rank", "grow_merge")
    assert _lib.KERNEL_KINDS[at - 4:at] == ("geo_seed", "k_geo_tiles", "k_geo_sweep", "geo_argmax")
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    assert "vc_temporal.h" in makefile and "vc_merge.h" in makefile
    for name in ("temporal_filter", "fetch_temporal", "temporal_history", "temporal_reset"):
        assert callable(getattr(CarveEngine, name))
    assert CarveEngine.temporal_thresholds() == (5, 3, 3) and CarveEngine.temporal_thresholds(8) == (8, 5, 5)
    assert CarveEngine.temporal_thresholds(5, 4) == (5, 4, 4) and CarveEngine.temporal_thresholds(15, 15, 1) == (15, 15, 1)
    for bad in ((0,), (16,), (5, 6), (5, 2, 3), (5, 3, 0), (2.5,), (5, 2.0), (True,)):
        with pytest.raises(ValueError):
            CarveEngine.temporal_thresholds(*bad)
    saved = dict(assignment._settings)
    try:
        assert (saved["temporal_window"], saved["temporal_keep"], saved["temporal_keep_off"]) == (0, None, None)
        for bad in ({"temporal_window": -1}, {"temporal_window": 16}, {"temporal_window": 2.5}, {"temporal_window": 5, "temporal_keep": 6},
                    {"temporal_window": 5, "temporal_keep": 2, "temporal_keep_off": 3}, {"temporal_window": 5, "temporal_keep_off": 0}):
            with pytest.raises(ValueError):
                assignment.configure(**bad)
            assert assignment._settings["temporal_window"] == 0
        assignment.configure(temporal_window=5, temporal_keep=4, temporal_keep_off=2)
        assert assignment._settings["temporal_window"] == 5 and assignment._settings["temporal_keep"] == 4
        with pytest.raises(RuntimeError):
            assignment.temporal()
    finally:
        assignment.configure(frame_source=None, **saved)
    out = subprocess.run([sys.executable, os.path.join(fx.ROOT, "scripts", "demo.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--temporal T" in out.stdout and "--frames F" in out.stdout and "--noise P" in out.stdout
