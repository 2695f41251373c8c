"""The hull thinned to a curve skeleton on the device (vc_hull_thin, vc_fetch_thin, vc_fetch_skeleton, vc_fetch_thin_table;
csrc/vc_thin.h) against the restatement (tests/thin_np.py), bit for bit and on both routes of the predicate (registers, table),
which must also give equal bytes: the real cameras at 64^3 (with the pin) and 128^3, the extremities of a geodesic pass as
anchors, random scenes whose rows straddle occupancy words, the solid grid whose border lies on the grid's faces, the empty hull,
one voxel, anchors given twice, max_passes = 1; the outputs after every pass that changes the hull and after the colour pass; the
table against the restatement's predicate; every refusal; assignment.configure(skeleton=...), scripts/demo.py --skeleton,
vc_timing."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures_util as fx
import thin_np as tn
from test_geodesic_restatement import RANDOM, random_seeds

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)
ROUTES = (0, 1)                                                  # option thin_table: the predicate in registers, by look-up
DEFAULT_ROUTE = 0
SOLID_BOUNDS = (-200.0, 700.0, -700.0, 700.0, -1500.0, 0.0)     # every voxel centre projects into all four images


@pytest.fixture(scope="module")
def teng(built):
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


def _voxel_masks(cams, H, W, grid, voxels):
    from test_gpu_measure import _voxel_masks as vm
    return vm(cams, H, W, grid, voxels)


def _check(e, mode="curve", anchors=None, max_passes=4096, topology=True):
    """thin_hull over the current result on both routes: peel, skeleton rows and stats against the restatement, the routes'
    bytes against each other, records and occupancy left alone, the topology kept.  Returns the restatement and the stats."""
    rec, occ = e.fetch_records().copy(), e.fetch_occupancy().copy()
    idx = (rec & LOW).astype(np.int64)
    if isinstance(anchors, str):
        pinned = idx[e.fetch_geodesic() == 0]
    else:
        pinned = anchors
    want = tn.thin(idx, e.grid, mode, pinned, max_passes)
    got = {}
    try:
        for route in ROUTES:
            e.set_option("thin_table", route)
            st = e.thin_hull(mode, anchors, max_passes)
            peel, sk = e.fetch_thin(), e.fetch_skeleton()
            for name in tn.STATS:
                assert st[name] == want[name], (name, route, st[name], want[name])
            assert peel.dtype == np.uint16 and np.array_equal(peel, want["peel"]), "peel, thin_table = %d" % route
            for name, dtype in (("voxel", np.uint32), ("record", np.uint32), ("degree", np.uint8)):
                assert sk[name].dtype == dtype and np.array_equal(sk[name], want[name]), "%s, thin_table = %d" % (name, route)
            ix, iy, iz = tn.coords(want["voxel"], e.grid)
            assert np.array_equal(sk["index"], np.stack([ix, iy, iz], axis=1))
            assert st["launches"] >= 54 * st["passes"] or idx.size == 0
            assert st["thin_ms"] > 0 or idx.size == 0
            assert e.thin_valid()
            assert np.array_equal(e.fetch_records(), rec) and np.array_equal(e.fetch_occupancy(), occ), "the pass leaves the result alone"
            got[route] = (peel.tobytes(), sk["voxel"].tobytes(), sk["record"].tobytes(), sk["degree"].tobytes(),
                          tuple(st[name] for name in tn.STATS))
    finally:
        e.set_option("thin_table", DEFAULT_ROUTE)
    assert got[0] == got[1], "the two routes give equal bytes"
    if topology:
        assert tn.topology(want["voxel"], e.grid) == tn.topology(idx, e.grid)
    return want, st


@pytest.mark.parametrize("mode,kept", [("curve", 258), ("point", 138)])
def test_real_cameras_64(teng, cams, masks, frames, mode, kept):
    _setup(teng, (64, 64, 64), cams, masks, frames)
    assert teng.carve() == 6981
    want, st = _check(teng, mode)
    assert st["kept"] == kept and st["passes"] == 6 and st["stable"] == 1                  # the pin
    assert tn.topology(want["voxel"], teng.grid) == (4, 1, -4)  # 4 components, no cavity, Euler number -4


def test_real_cameras_64_extrema_anchors(teng, cams, masks, frames):
    _setup(teng, (64, 64, 64), cams, masks, frames)
    teng.carve()
    geo = teng.hull_geodesic(extrema=5)
    ex = teng.fetch_extrema()
    for mode in tn.MODES:
        want, st = _check(teng, mode, "extrema")
        assert st["anchors"] == geo["seeds"] + 5 and np.isin(ex["voxel"], want["voxel"]).all()
    assert teng.geodesic_valid()                                 # the pass leaves the geodesic outputs alone


def test_real_cameras_128(teng, cams, masks, frames):
    _setup(teng, (128, 128, 128), cams, masks, frames)
    assert teng.carve() == 57048
    want, st = _check(teng, "curve")
    assert (st["kept"], st["endpoints"], st["passes"]) == (1029, 115, 11)                  # the pin
    assert tn.topology(want["voxel"], teng.grid) == (2, 1, -9)


@pytest.mark.parametrize("grid,seed,mv", RANDOM)
def test_random_scenes(teng, grid, seed, mv):
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    _setup(teng, grid, cams3, masks3, frames3)
    S = teng.carve(min_views=mv)
    assert S > 0
    idx = teng.fetch()[0].astype(np.int64)
    pins = idx[random_seeds(seed, S)]
    for mode in tn.MODES:
        _check(teng, mode)
        want, st = _check(teng, mode, pins)
        assert st["anchors"] == 3 and np.isin(pins, want["voxel"]).all()


@pytest.mark.parametrize("grid", [(8, 8, 8), (5, 70, 3)])
def test_solid_grid(teng, cams, masks, frames, grid):
    """All masks full: every border voxel lies on a face of the grid, where the neighbourhood ends."""
    H, W = masks[0].shape
    _setup(teng, grid, cams, [np.full((H, W), 255, np.uint8)] * 4, frames, bounds=SOLID_BOUNDS)
    n = grid[0] * grid[1] * grid[2]
    assert teng.carve() == n
    want, st = _check(teng, "point")
    assert st["kept"] == 1
    want, st = _check(teng, "curve")
    assert st["kept"] >= 1 and st["stable"] == 1
    _check(teng, "curve", [0, n - 1])
    _check(teng, "point", [0, n - 1])


def test_empty_hull_one_voxel_and_anchors_twice(teng, cams, masks, frames):
    H, W = masks[0].shape
    _setup(teng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert teng.carve() == 0
    for mode in tn.MODES:
        want, st = _check(teng, mode)
        assert st["kept"] == 0 and st["passes"] == 1 and st["stable"] == 1
    _check(teng, "curve", [])
    assert teng.fetch_thin().size == 0 and teng.fetch_skeleton()["voxel"].size == 0
    _setup(teng, (8, 8, 8), cams, _voxel_masks(cams, H, W, (8, 8, 8), [213]), frames)
    assert teng.carve() == 1
    for anchors in (None, [213], [213, 213]):
        want, st = _check(teng, "curve", anchors)
        assert st["kept"] == 1 and st["isolated"] == 1 and want["voxel"].tolist() == [213]
    # three voxels in a row and one apart; the anchors given twice and out of order
    vox = [213, 214, 215, 362]
    _setup(teng, (8, 8, 8), cams, _voxel_masks(cams, H, W, (8, 8, 8), vox), frames)
    assert teng.carve() == 4 and teng.fetch()[0].tolist() == vox
    want, st = _check(teng, "point", [215, 213, 215, 213])
    assert st["anchors"] == 2 and want["voxel"].tolist() == vox  # (the middle voxel holds the two anchors together)
    want, st = _check(teng, "point")
    assert st["kept"] == 2


def test_max_passes_cuts_it_short(teng, cams, masks, frames):
    _setup(teng, (64, 64, 64), cams, masks, frames)
    teng.carve()
    want, st = _check(teng, "curve", max_passes=1)
    assert st["stable"] == 0 and st["passes"] == 1 and st["kept"] > 258 and int(want["peel"].max()) <= 6
    want, st = _check(teng, "point", max_passes=3)
    assert st["stable"] == 0 and st["passes"] == 3


def test_stale_after_the_passes_that_change_the_hull(teng, cams, masks, frames):
    from voxcarve import synthetic
    from voxcarve._lib import VoxcarveError
    _setup(teng, (64, 64, 64), cams, masks, frames)
    for c in range(4):                                           # (color_visible and photo_carve look through every camera)
        teng.upload_frame(c, frames[c])
    S = teng.carve()

    def stale():
        assert not teng.thin_valid()
        for call in (teng.fetch_thin, teng.fetch_skeleton):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no skeleton"):
                call()

    stale()
    want, _ = _check(teng, "curve")
    teng.color_visible()                                         # colours only: the outputs stay
    assert teng.thin_valid() and np.array_equal(teng.fetch_thin(), want["peel"])
    assert np.array_equal(teng.fetch_skeleton()["voxel"], want["voxel"])
    teng.hull_distance()                                         # leaves the result alone
    assert teng.thin_valid()
    assert teng.photo_carve(max_rounds=2)["survivors_after"] < S
    stale()
    _check(teng, "curve")
    teng.carve()
    stale()
    teng.thin_hull()
    assert teng.filter_components(keep_largest=1)["survivors_after"] < S
    stale()
    _check(teng, "point")
    teng.carve()
    teng.thin_hull()
    assert teng.open_hull(25)["survivors_after"] < S
    stale()
    _check(teng, "curve")
    teng.carve()
    teng.thin_hull()
    assert teng.close_hull(40)["added"] > 0
    stale()
    _check(teng, "curve")
    # a vote over two different hulls changes the second
    teng.temporal_reset()
    teng.carve()
    teng.temporal_filter(3)
    teng.upload_masks(synthetic.shifted_masks(masks, 3))
    teng.carve()
    teng.thin_hull()
    st = teng.temporal_filter(3)
    assert st["added"] + st["removed"] > 0
    stale()
    _check(teng, "curve")
    teng.temporal_reset()


def test_table_against_the_restatement(teng):
    rng = np.random.default_rng(26)

    def sparse(n):
        return np.array([sum(1 << int(b) for b in rng.choice(26, int(rng.integers(0, 7)), replace=False)) for _ in range(n)], dtype=np.int64)

    full = (1 << 26) - 1
    codes = np.concatenate([rng.integers(0, 1 << 26, 25000), sparse(12500), full ^ sparse(12500), [0, full]]).astype(np.int64)
    bits = teng.fetch_thin_table()
    assert bits.dtype == np.uint8 and bits.size == 1 << 23
    got = (bits[codes >> 3] >> (codes & 7).astype(np.uint8)) & 1
    want = tn.table_bits(codes)
    assert np.array_equal(got.astype(bool), want) and want.any() and not want.all()
    assert np.array_equal(teng.fetch_thin_table(), bits)


def test_refusals(built, cams, masks, frames):
    """Every refusal of the contract but one: a communicator of more than one rank needs two processes with a device each, and
    the message comes from the check the other post-carve passes share."""
    import voxcarve
    from voxcarve._lib import VoxcarveError, VcThinStats
    H, W = masks[0].shape
    with voxcarve.CarveEngine(0) as e:
        e.set_grid(64, 64, 64)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.thin_hull()
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        S = e.carve()
        idx = e.fetch()[0]
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no skeleton"):
            e.fetch_thin()
        st = VcThinStats()
        L = e._L
        err = lambda: L.vc_last_error(e._ctx).decode()
        two = (ctypes.c_uint32 * 2)(int(idx[0]), int(idx[1]))
        call = lambda mode=0, source=1, anchors=two, n=2, max_passes=4096, flags=0, stats=ctypes.byref(st): \
            L.vc_hull_thin(e._ctx, mode, source, anchors, n, max_passes, flags, stats)
        assert call(flags=1) == -1 and "flags" in err()
        assert call(stats=None) == -1 and "stats" in err()
        assert call(mode=2) == -1 and "mode 2" in err()
        assert call(source=3) == -1 and "anchor source 3" in err()
        for bad in (0, 10001):
            assert call(max_passes=bad) == -1 and "max_passes = %d" % bad in err()
        assert call(anchors=None) == -1 and "no list" in err()
        gap = int(np.setdiff1d(np.arange(idx[0], idx[0] + S + 1), idx)[0])       # the first hole behind the first survivor
        bad = (ctypes.c_uint32 * 4)(int(idx[0]), gap, 7, int(idx[1]))
        assert call(anchors=bad, n=4) == -1 and "anchor 1 (voxel %d) is no survivor" % gap in err()
        beyond = (ctypes.c_uint32 * 2)(int(idx[0]), 64 ** 3)
        assert call(anchors=beyond, n=2) == -1 and "anchor 1 (voxel %d) is no survivor" % 64 ** 3 in err()
        assert call(source=2) == -1 and "call vc_hull_geodesic first" in err()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no skeleton"):                            # a refused call leaves nothing
            e.fetch_skeleton()
        assert call() == 0 and st.anchors == 2 and call(source=0, anchors=None, n=7) == 0 and call(mode=1, max_passes=10000) == 0
        assert e.count == S and e.fetch_records().size == S
        assert L.vc_fetch_thin_table(e._ctx, None) == -1 and "bits" in err()
        for bad in ("middle", [-1], [2 ** 32], [0.5]):
            with pytest.raises(ValueError):
                e.thin_hull(anchors=bad)
        with pytest.raises(ValueError):
            e.thin_hull("surface")
        for bad in (0, 10001):
            with pytest.raises(ValueError):
                e.thin_hull(max_passes=bad)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*call vc_hull_geodesic first"):
            e.thin_hull(anchors="extrema")
        e.hull_geodesic(extrema=2)
        assert e.thin_hull(anchors="extrema")["anchors"] >= 3
        e.carve()                                                # the geodesic pass is of the carve before
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*call vc_hull_geodesic first"):
            e.thin_hull(anchors="extrema")
        # the refusals every pass over the result shares
        e.carve(records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.thin_hull()
        e.set_slab(0, 32)
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.thin_hull()
        e.set_slab(0, 64)
        e.carve()
        e.thin_hull()
        e.carve_begin()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
            e.thin_hull()
        e.carve_end()
        assert e.thin_hull()["survivors"] == S
    with voxcarve.CarveEngine(0) as e:
        _setup(e, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
        assert e.carve() == 0
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*anchor 0 .voxel 9. is no survivor"):
            e.thin_hull(anchors=[9])


# ---- the drop-in layer, the demo, the timing ----------------------------------------------------------------------------------------
def test_assignment_over_two_frames(built, cams, masks, frames):
    """Two frames, the second with its masks shifted: every frame ends with its own skeleton, pinned at its own extremities."""
    from voxcarve import assignment, skeleton, synthetic
    m1 = synthetic.shifted_masks(masks, 1)
    saved = dict(assignment._settings)
    try:
        with pytest.raises(ValueError):
            assignment.configure(skeleton="curve", skeleton_anchors="extrema")
        with pytest.raises(ValueError):
            assignment.configure(skeleton="surface")
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks), (frames, m1)]), data_path=fx.GOLDEN + "/data",
                             extremities=3, skeleton="curve", skeleton_anchors="extrema")
        with pytest.raises(RuntimeError):
            assignment.skeleton()
        found = []
        for _ in range(2):
            pos, col = assignment.set_voxel_positions(64, 32, 64)
            e = assignment._engine
            got = assignment.skeleton()
            idx = (e.fetch_records() & LOW).astype(np.int64)
            want = tn.thin(idx, e.grid, "curve", idx[e.fetch_geodesic() == 0])
            for name in tn.STATS:
                assert got["stats"][name] == want[name], name
            assert np.array_equal(got["skeleton"]["voxel"], want["voxel"]) and np.array_equal(got["skeleton"]["degree"], want["degree"])
            d = skeleton.describe(got["skeleton"], e.grid, e.bounds)
            assert np.array_equal(got["description"]["edges"], d["edges"]) and got["description"]["length_mm"] == d["length_mm"] > 0
            assert len(pos) == idx.size
            found.append(want["voxel"].tolist())
        assert found[0] != found[1]
    finally:
        assignment.configure(frame_source=None, **saved)


def test_demo_skeleton(built, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "demo.py"), "64", str(tmp_path / "hull.ply"), "--skeleton", "curve"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.strip().startswith("skeleton (curve):")]
    assert len(line) == 1 and "258 voxels" in line[0] and "end points" in line[0] and "junctions" in line[0] and " mm" in line[0]


def test_timing_holds_the_pass(built, cams, masks, frames):
    import voxcarve
    with voxcarve.CarveEngine(0) as e:
        _setup(e, (64, 64, 64), cams, masks, frames)
        e.carve()
        st = e.thin_hull()
        t = e.timing()
        assert t["thin_ms"] == pytest.approx(st["thin_ms"]) and t["thin_ms"] > 0 and t["thin_launches"] == 0 and t["thin_kernel_ms"] == 0
        e.set_option("timing_detail", 1)
        st = e.thin_hull()
        t = e.timing()
        # (the scans and the compactions of the lists carry no events: 3 launches per pass that removed something, 3 for the kept
        # voxels at the end, 1 inside the words' record offsets)
        assert t["thin_launches"] == st["launches"] - 3 * (st["passes"] - 1) - 3 - 1 and t["thin_launches"] >= 54 * st["passes"]
        assert 0 < t["thin_kernel_ms"] < t["thin_ms"] == pytest.approx(st["thin_ms"])
