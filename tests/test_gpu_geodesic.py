"""Geodesic distances through the hull, its extremities, regions and paths on the device (vc_hull_geodesic, vc_fetch_geodesic,
vc_fetch_geodesic_labels, vc_fetch_extrema, vc_geodesic_path, vc_fetch_extremum_path, vc_paint_geodesic; csrc/vc_geodesic.h)
against the restatement (tests/geodesic_np.py), bit for bit and on both relaxation routes (tiles in LDS, sweeps over the records),
which must also give equal bytes: the real cameras at 64^3 (with the pin) and 128^3 from the floor, three floor layers and the
top under all three connectivities, random scenes whose columns straddle occupancy words and whose hulls fall into components, a
bent hull that a straight line cannot measure, the solid grid, the empty hull, one voxel, every voxel a seed, K beyond what there
is, duplicate seeds, sources in the corner cells of a tile; the outputs after every pass that changes the hull and after the
colour passes; both paints; every refusal; assignment.configure(extremities=...), scripts/demo.py --extremities, vc_timing."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import geodesic_np as gn
from test_geodesic_restatement import RANDOM, random_seeds, u_masks

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)
ROUTES = (1, 0)                                                  # option geodesic_tiles: tiles in LDS, sweeps over the records
DEFAULT_ROUTE = 1
STATS = ("survivors", "seeds", "reached", "unreached", "max_d", "extremities", "edge_um", "q")
SOLID_BOUNDS = (-200.0, 700.0, -700.0, 700.0, -1500.0, 0.0)     # every voxel centre projects into all four images


@pytest.fixture(scope="module")
def geng(built):
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


def _hull(e):
    rec = e.fetch_records().copy()
    return rec, (rec & LOW).astype(np.int64), dn.steps_um(e.grid, e.bounds)


def _extrema_rows(ex):
    return [(int(ex["label"][k]), int(ex["voxel"][k]), int(ex["record"][k]), int(ex["d"][k])) + tuple(int(v) for v in ex["index"][k])
            for k in range(ex["label"].size)]


def _check(e, seeds, K, conn, layers=1, paths=False):
    """hull_geodesic over the current result on both routes: distances, labels, extremities and stats against the restatement,
    the routes' bytes against each other, the result left alone.  Returns the restatement and the stats of both routes."""
    rec, idx, q = _hull(e)
    srec = gn.seeds_by_layer(idx, e.grid, seeds, layers) if isinstance(seeds, str) else gn.records_of(idx, seeds)
    want = gn.geodesic(idx, e.grid, q, conn, srec, K, paths=paths)
    rows = [(x["label"], x["voxel"], x["record"], x["d"], x["ix"], x["iy"], x["iz"]) for x in want["extrema"]]
    got, stats = {}, {}
    try:
        for tiles in ROUTES:
            e.set_option("geodesic_tiles", tiles)
            st = e.hull_geodesic(seeds=seeds, layers=layers, extrema=K, connectivity=conn, paths=paths)
            d, lab, ex = e.fetch_geodesic(), e.fetch_geodesic_labels(), e.fetch_extrema()
            for name in STATS:
                assert st[name] == want[name], (name, tiles)
            assert d.dtype == np.uint64 and np.array_equal(d, want["d"]), "distances, geodesic_tiles = %d" % tiles
            assert lab.dtype == np.uint8 and np.array_equal(lab, want["labels"]), "labels, geodesic_tiles = %d" % tiles
            assert _extrema_rows(ex) == rows, "extremities, geodesic_tiles = %d" % tiles
            assert st["geodesic_ms"] > 0 or idx.size == 0
            assert st["rounds"] <= st["launches"] or st["seeds"] == 0
            if tiles:
                assert st["tile_visits"] >= st["launches"] and st["launches"] == st["rounds"]
            else:
                assert st["tile_visits"] == 0 and st["launches"] == 8 * st["rounds"]
            mm = e.fetch_geodesic_mm()
            assert np.array_equal(np.isinf(mm), want["d"] == gn.NONE)
            assert np.array_equal(mm[~np.isinf(mm)], want["d"][want["d"] != gn.NONE].astype(np.float64) / 1000.0)
            if paths:
                for x in want["extrema"]:
                    assert e.fetch_extremum_path(x["label"]).tolist() == x["path"], "path of extremity %d" % x["label"]
            assert np.array_equal(e.fetch_records(), rec), "the pass leaves the result alone"
            got[tiles] = (d.tobytes(), lab.tobytes(), _extrema_rows(ex), tuple(st[name] for name in STATS))
            stats[tiles] = st
    finally:
        e.set_option("geodesic_tiles", DEFAULT_ROUTE)
    assert got[1] == got[0], "the two routes give equal bytes"
    return want, stats


def _check_walks(e, want, idx, n=8, seed=5):
    """geodesic_path from reached voxels through the final keys."""
    reached = np.flatnonzero(want["d"] != gn.NONE)
    for r in np.random.default_rng(seed).choice(reached, min(n, reached.size), replace=False):
        assert e.geodesic_path(int(idx[r])).tolist() == gn.path(want["keys"], want["nbr"], want["w8"], idx, r)


@pytest.mark.parametrize("n", [64, 128])
def test_real_cameras(geng, cams, masks, frames, n):
    _setup(geng, (n, n, n), cams, masks, frames)
    geng.carve()
    idx, _, _ = fx.expected(n)
    assert np.array_equal(geng.fetch()[0], idx)
    for conn in (6, 18, 26):
        for seeds, layers in (("floor", 1), ("floor", 3), ("top", 1)):
            want, stats = _check(geng, seeds, 5, conn, layers=layers, paths=(conn == 26 and layers == 1))
            assert want["extremities"] == 5 and want["seeds"] > 0
            if n == 64 and conn == 26 and (seeds, layers) == ("floor", 1):           # the pin
                ex = geng.fetch_extrema()
                assert list(zip(ex["voxel"].tolist(), ex["d"].tolist())) == [(68056, 1738449), (207637, 1432178), (198372, 993329),
                                                                             (142307, 889404), (177880, 753272)]
                assert stats[1]["seeds"] == 2 and stats[1]["reached"] == 6977 and stats[1]["unreached"] == 4
                assert np.bincount(geng.fetch_geodesic_labels(), minlength=256)[:6].tolist() == [998, 958, 54, 412, 3332, 1223]
                assert stats[1]["q"] == (24381, 32508, 40635)
                assert np.allclose(ex["world_mm"][0], [-512 + ex["index"][0, 0] * 24.381, -1024 + ex["index"][0, 1] * 32.508,
                                                      -2048 + ex["index"][0, 2] * 40.635], atol=0.05)
    # the last run: connectivity 26 from the top; walks through its final keys, from an extremity too (it is a source)
    _check_walks(geng, want, idx.astype(np.int64))
    ex = geng.fetch_extrema()
    assert geng.geodesic_path(int(ex["voxel"][0])).tolist() == [int(ex["voxel"][0])]
    _check(geng, "floor", 5, 26, paths=True)
    fig = geng.stick_figure()
    assert len(fig) == 5 and all(p.shape[1] == 3 and p.shape[0] > 1 for p in fig)
    assert np.allclose(fig[0][0], geng.fetch_extrema()["world_mm"][0])


@pytest.mark.parametrize("grid,seed,mv", RANDOM)
def test_random_scenes(geng, grid, seed, mv):
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    _setup(geng, grid, cams3, masks3, frames3)
    S = geng.carve(min_views=mv)
    assert S > 0
    _, idx, _ = _hull(geng)
    seeds = idx[random_seeds(seed, S)]
    unreached = []
    for conn in (6, 18, 26):
        want, _ = _check(geng, seeds, 4, conn, paths=True)
        unreached.append(want["unreached"])
        _check_walks(geng, want, idx, n=4)
    if (grid, seed) == ((37, 53, 29), 4):
        assert unreached == [148, 8, 6]                           # (checked on the CPU: tests/test_geodesic_restatement.py)


@pytest.mark.parametrize("n,S", [(32, 7432), (48, 25337)])
def test_bent_hull(geng, cams, masks, frames, n, S):
    H, W = masks[0].shape
    _setup(geng, (n, n, n), cams, u_masks(H, W), frames)
    assert geng.carve() == S
    _, idx, q = _hull(geng)
    ix, iy, iz = gn.coords(idx, geng.grid)
    straight = np.sqrt(((ix - ix[0]) * q[0]) ** 2.0 + ((iy - iy[0]) * q[1]) ** 2.0 + ((iz - iz[0]) * q[2]) ** 2.0)
    occupied = gn.occupied_tiles(idx, geng.grid)
    for conn in (6, 18, 26):
        want, stats = _check(geng, [int(idx[0])], 0, conn)
        assert want["unreached"] == 0 and stats[1]["unreached"] == 0
        geng.hull_geodesic(seeds=[int(idx[0])], connectivity=conn)
        d = geng.fetch_geodesic().astype(np.float64)
        ratio = d[1:] / straight[1:]
        print("bent hull %d^3, connectivity %d: geodesic / straight at most %.4f; rounds %d, tile visits %d, occupied tiles %d" %
              (n, conn, ratio.max(), stats[1]["rounds"], stats[1]["tile_visits"], occupied))
        assert ratio.max() >= 1.25 and ratio.min() > 0.999
        assert stats[1]["rounds"] > 1 and stats[1]["tile_visits"] > occupied          # the outer loop and the re-activation ran
        assert stats[1]["tiles"] >= occupied
    _check(geng, [int(idx[0])], 3, 26, paths=True)


def _voxel_masks(cams, H, W, grid, voxels):
    """Masks in which only the pixels under the centres of `voxels` are foreground."""
    from oracle import carve_np
    pts = carve_np.points_of_indices(np.array(voxels), *grid)
    out = [np.zeros((H, W), np.uint8) for _ in cams]
    for c, cam in enumerate(cams):
        off = carve_np.pixel_offsets(carve_np.project_points(pts, cam.R, cam.tvec, cam.K, cam.dist), H, W)
        assert (off >= 0).all()
        out[c].reshape(-1)[off] = 255
    return out


def test_solid_grid_and_tile_corners(geng, cams, masks, frames):
    """All masks full on a grid that is no multiple of the tile in any axis; seeds in the first and the last voxel, and in the
    cells where eight tiles meet."""
    H, W = masks[0].shape
    grid = (10, 70, 9)
    _setup(geng, grid, cams, [np.full((H, W), 255, np.uint8)] * 4, frames, bounds=SOLID_BOUNDS)
    n = grid[0] * grid[1] * grid[2]
    assert geng.carve() == n
    assert all(g % t for g, t in zip(grid, gn.TILE))
    for conn in (6, 18, 26):
        for seed in (0, n - 1):
            want, stats = _check(geng, [seed], 3, conn, paths=True)
            assert want["unreached"] == 0 and want["extrema"][0]["voxel"] == n - 1 - seed
            assert stats[1]["tiles"] == 3 * 2 * 3
        corner = lambda ix, iy, iz: (iz * grid[0] + ix) * grid[1] + iy
        for seeds in ([corner(3, 63, 3)], [corner(4, 64, 4)], [corner(3, 63, 3), corner(4, 64, 4)], [corner(7, 0, 8), corner(8, 69, 3)]):
            _check(geng, seeds, 2, conn)
    want, _ = _check(geng, np.arange(n), 5, 26)                   # every voxel a seed
    assert want["extremities"] == 0 and not want["d"].any() and want["seeds"] == n
    _check(geng, [5, 5, 5, 2, 2, 5], 2, 26)                       # duplicates
    want, _ = _check(geng, [], 3, 26)                             # no seed at all: nothing is reached
    assert want["reached"] == 0 and want["extremities"] == 0 and (want["labels"] == 255).all()


def test_empty_hull_one_voxel_and_k_beyond(geng, cams, masks, frames):
    H, W = masks[0].shape
    _setup(geng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert geng.carve() == 0
    for seeds in ("floor", "top", []):
        want, stats = _check(geng, seeds, 3, 26, paths=True)
        assert stats[1]["survivors"] == 0 and stats[1]["rounds"] == 0 and stats[1]["tiles"] == 0
    assert geng.fetch_geodesic().size == 0 and geng.stick_figure() == []
    geng.paint_geodesic("labels")                                 # nothing to paint is no error
    geng.paint_geodesic("distance")
    _setup(geng, (8, 8, 8), cams, _voxel_masks(cams, H, W, (8, 8, 8), [213]), frames)
    assert geng.carve() == 1
    for seeds in ("floor", [213]):
        want, _ = _check(geng, seeds, 3, 26, paths=True)
        assert want["d"].tolist() == [0] and want["extremities"] == 0
    assert geng.geodesic_path(213).tolist() == [213]
    # three voxels in a row and one apart: K = 32 finds what there is
    vox = [213, 214, 215, 362]
    _setup(geng, (8, 8, 8), cams, _voxel_masks(cams, H, W, (8, 8, 8), vox), frames)
    assert geng.carve() == 4 and geng.fetch()[0].tolist() == vox
    want, _ = _check(geng, [213], 32, 6, paths=True)
    assert want["extremities"] == 2 and want["unreached"] == 1 and [x["voxel"] for x in want["extrema"]] == [215, 214]


def test_stale_after_the_passes_that_change_the_hull(geng, cams, masks, frames):
    from voxcarve._lib import VoxcarveError
    _setup(geng, (64, 64, 64), cams, masks, frames)
    for c in range(4):                                           # (color_visible and photo_carve look through every camera)
        geng.upload_frame(c, frames[c])
    S = geng.carve()

    def stale():
        assert not geng.geodesic_valid()
        for call in (geng.fetch_geodesic, geng.fetch_geodesic_labels, geng.fetch_extrema, geng.stick_figure, geng.paint_geodesic,
                     lambda: geng.geodesic_path(68056)):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no geodesic distances"):
                call()

    stale()
    want, _ = _check(geng, "floor", 3, 26)
    assert geng.geodesic_valid()
    geng.color_visible()                                         # colours only: the outputs stay
    assert geng.geodesic_valid() and np.array_equal(geng.fetch_geodesic(), want["d"])
    geng.cluster_hull(2)
    geng.paint_clusters()
    assert geng.geodesic_valid() and np.array_equal(geng.fetch_geodesic_labels(), want["labels"])
    geng.hull_distance()                                         # leaves the result alone
    assert geng.geodesic_valid()
    assert geng.photo_carve(max_rounds=2)["survivors_after"] < S
    stale()
    _check(geng, "floor", 3, 26)
    geng.carve()
    stale()
    geng.hull_geodesic(extrema=3)
    assert geng.filter_components(keep_largest=1)["survivors_after"] < S
    stale()
    want, _ = _check(geng, "floor", 3, 26)
    assert want["unreached"] == 0
    geng.carve()
    geng.hull_geodesic(extrema=3)
    assert geng.open_hull(25)["survivors_after"] < S
    stale()
    _check(geng, "floor", 3, 26)
    geng.carve()
    geng.hull_geodesic(extrema=3)
    assert geng.close_hull(40)["added"] > 0
    stale()
    _check(geng, "floor", 3, 26)


def test_paint(geng, cams, masks, frames):
    from voxcarve import camera
    from voxcarve.geodesic import PALETTE, UNREACHED_RGB
    _setup(geng, (64, 64, 64), cams, masks, frames)
    geng.carve()
    rec = geng.fetch_records().copy()
    rgb = np.stack([(rec >> np.uint64(32 + 8 * c)).astype(np.uint8) for c in range(3)], axis=1)
    want, _ = _check(geng, "floor", 5, 26)
    assert want["unreached"] == 4

    def painted():
        r = geng.fetch_records()
        assert np.array_equal(r & ~(np.uint64(0xffffff) << np.uint64(32)), rec & ~(np.uint64(0xffffff) << np.uint64(32)))
        return np.stack([(r >> np.uint64(32 + 8 * c)).astype(np.uint8) for c in range(3)], axis=1)

    geng.paint_geodesic()
    assert np.array_equal(painted(), gn.paint(rgb, want["keys"], "labels", PALETTE))
    assert np.array_equal(geng.fetch_geodesic(), want["d"])      # painting leaves the outputs valid
    out = geng.render(camera.orbit(2, 4500.0, 25.0, 150.0, 90, 120), 90, 120, shade=(255,) * 7, background=(9, 9, 9))
    colours = set(map(tuple, out["rgb"].reshape(-1, 3).tolist()))
    assert colours <= set(map(tuple, PALETTE[:6].tolist())) | {(9, 9, 9), UNREACHED_RGB} and len(colours) >= 4
    own = np.arange(18, dtype=np.uint8).reshape(6, 3)
    geng.paint_geodesic("labels", own)
    assert np.array_equal(painted(), gn.paint(rgb, want["keys"], "labels", own))
    with pytest.raises(ValueError):
        geng.paint_geodesic("labels", own[:5])
    with pytest.raises(ValueError):
        geng.paint_geodesic("heat")
    geng.paint_geodesic("distance")
    grey = gn.paint(rgb, want["keys"], "distance", max_d=want["max_d"])
    assert np.array_equal(painted(), grey) and grey.max() == 255 and (grey[want["d"] == gn.NONE] == UNREACHED_RGB).all()
    geng.carve()
    assert np.array_equal(geng.fetch_records(), rec)             # the next carve: the camera's colours again


def test_refusals(built, cams, masks, frames):
    """Every refusal of the contract but one: a communicator of more than one rank needs two processes with a device each, and
    the message comes from the check the other post-carve passes share."""
    import voxcarve
    from voxcarve._lib import VoxcarveError, VcGeodesicStats
    H, W = masks[0].shape
    with voxcarve.CarveEngine(0) as e:
        e.set_grid(64, 64, 64)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.hull_geodesic()
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        S = e.carve()
        idx = e.fetch()[0]
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no geodesic distances"):
            e.fetch_geodesic()
        st = VcGeodesicStats()
        L = e._L
        err = lambda: L.vc_last_error(e._ctx).decode()
        two = (ctypes.c_uint32 * 2)(int(idx[0]), int(idx[1]))
        call = lambda conn=26, mode=0, seeds=two, n=2, layers=1, K=2, flags=0, stats=ctypes.byref(st): \
            L.vc_hull_geodesic(e._ctx, conn, mode, seeds, n, layers, K, flags, stats)
        assert call(flags=2) == -1 and "flags" in err()
        assert call(stats=None) == -1 and "stats" in err()
        for conn in (0, 4, 8, 27):
            assert call(conn=conn) == -1 and "connectivity %d" % conn in err()
        assert call(K=33) == -1 and "K = 33" in err()
        assert call(mode=3) == -1 and "seed mode 3" in err()
        assert call(mode=1, layers=0) == -1 and "layers" in err()
        assert call(seeds=None) == -1 and "no list" in err()
        gap = int(np.setdiff1d(np.arange(idx[0], idx[0] + S + 1), idx)[0])       # the first hole behind the first survivor
        bad = (ctypes.c_uint32 * 4)(int(idx[0]), gap, 7, int(idx[1]))
        assert call(seeds=bad, n=4) == -1 and "seed 1 (voxel %d) is no survivor" % gap in err()
        beyond = (ctypes.c_uint32 * 2)(int(idx[0]), 64 ** 3)
        assert call(seeds=beyond, n=2) == -1 and "seed 1 (voxel %d) is no survivor" % 64 ** 3 in err()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no geodesic distances"):                  # a refused call leaves nothing
            e.fetch_geodesic()
        assert call() == 0 and call(K=32, flags=1) == 0 and call(mode=2, seeds=None, n=0, layers=1000) == 0 and call(seeds=None, n=0) == 0
        assert e.count == S and e.fetch_records().size == S
        for bad in ("left", [-1], [2 ** 32], [0.5]):
            with pytest.raises(ValueError):
                e.hull_geodesic(seeds=bad)
        e.hull_geodesic("floor", extrema=2)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*without VC_GEO_PATHS"):
            e.stick_figure()
        # vc_geodesic_path: no survivor, unreached, a capacity too small (with the needed length)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*voxel %d is no survivor" % gap):
            e.geodesic_path(gap)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no survivor"):
            e.geodesic_path(64 ** 3)
        lab = e.fetch_geodesic_labels()
        lost = int(idx[np.flatnonzero(lab == 255)[0]])
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*voxel %d is unreached" % lost):
            e.geodesic_path(lost)
        far = int(idx[np.argmax(np.where(lab == 255, 0, e.fetch_geodesic()))])
        whole = e.geodesic_path(far)
        n, out = ctypes.c_uint32(0), (ctypes.c_uint32 * 3)()
        assert whole.size > 3 and L.vc_geodesic_path(e._ctx, far, out, 3, ctypes.byref(n)) == -1
        assert n.value == whole.size and "the path has %d voxels, the capacity is 3" % whole.size in err()
        assert L.vc_paint_geodesic(e._ctx, 2, None) == -1 and "mode 2" in err()
        assert L.vc_paint_geodesic(e._ctx, 0, None) == -1 and "palette" in err()
        # the refusals every pass over the result shares, and the metric's
        e.set_grid(64, 64, 64, bounds=(0, 63 * 1100.0, 0, 1, 0, 1))
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis x"):
            e.hull_geodesic()
        e.set_grid(64, 64, 1, bounds=(-512.0, 1024.0, -1024.0, 1024.0, -768.0, -768.0))
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis z has 1 cells"):
            e.hull_geodesic()
        e.set_grid(64, 64, 64)
        e.carve(records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.hull_geodesic()
        e.set_slab(0, 32)
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.hull_geodesic()
        e.set_slab(0, 64)
        e.carve()
        e.hull_geodesic()
        e.carve_begin()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
            e.hull_geodesic()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG"):
            e.geodesic_path(int(idx[0]))
        e.carve_end()
        assert e.hull_geodesic()["survivors"] == S
    _setup_empty = voxcarve.CarveEngine(0)
    with _setup_empty as e:
        _setup(e, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
        assert e.carve() == 0
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*seed 0 .voxel 9. is no survivor"):
            e.hull_geodesic(seeds=[9])


# ---- the drop-in layer, the demo, the timing ----------------------------------------------------------------------------------------
def test_assignment_end_to_end(built, cams, masks, frames):
    """Two frames, the second with its masks rolled by 3 columns: every frame ends with its own extremities."""
    from voxcarve import assignment, synthetic
    from voxcarve.geodesic import PALETTE
    m1 = synthetic.shifted_masks(masks, 1)
    saved = dict(assignment._settings)
    try:
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks), (frames, m1)]), data_path=fx.GOLDEN + "/data",
                             extremities=3)
        with pytest.raises(RuntimeError):
            assignment.extremities()
        found = []
        for _ in range(2):
            pos, col = assignment.set_voxel_positions(64, 32, 64)
            e = assignment._engine
            got = assignment.extremities()
            _, idx, q = _hull(e)
            want = gn.geodesic(idx, e.grid, q, 26, gn.seeds_by_layer(idx, e.grid, "floor", 1), 3, paths=True)
            assert got["extremities"] == 3 and got["extrema"]["voxel"].tolist() == [x["voxel"] for x in want["extrema"]]
            assert got["extrema"]["d"].tolist() == [x["d"] for x in want["extrema"]] and got["reached"] == want["reached"]
            assert [len(p) for p in got["paths"]] == [len(x["path"]) for x in want["extrema"]]
            assert np.array_equal(e.fetch_geodesic(), want["d"]) and len(pos) == idx.size
            found.append(got["extrema"]["voxel"].tolist())
        assert found[0] != found[1]
        assert assignment.set_voxel_positions(64, 32, 64) == ([], [])
        # painted: the viewer's colours are the palette's
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=fx.GOLDEN + "/data", extremities=3,
                             geodesic_paint="labels")
        pos, col = assignment.set_voxel_positions(64, 32, 64)
        labels = assignment._engine.fetch_geodesic_labels()
        pal = np.vstack([PALETTE, np.zeros((256 - 33, 3), np.uint8)])
        pal[255] = (255, 0, 255)
        assert np.array_equal((col * 255.0 + 0.5).astype(np.uint8), pal[labels])
    finally:
        assignment.configure(frame_source=None, **saved)


def test_demo_extremities(built, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "demo.py"), "64", str(tmp_path / "hull.ply"), "--extremities", "3",
                        "--geodesic-paint", "labels"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("extremity ")]
    assert len(lines) == 3 and "extremities: 3 found" in r.stdout
    from voxcarve.geodesic import PALETTE, UNREACHED_RGB
    body = open(tmp_path / "hull.ply").read().split("end_header\n")[1].splitlines()
    colours = set(tuple(int(v) for v in l.split()[3:6]) for l in body)
    assert colours and colours <= set(map(tuple, PALETTE[:4].tolist())) | {UNREACHED_RGB}


def test_timing_reports_the_kernels(built, cams, masks, frames):
    import voxcarve
    with voxcarve.CarveEngine(0) as e:
        _setup(e, (128, 128, 128), cams, masks, frames)
        e.set_option("timing_detail", 1)
        e.carve()
        e.timing(reset=True)
        st = e.hull_geodesic(extrema=3)
        k = e.timing()["kernels"]
        assert k["k_geo_tiles"]["launches"] == st["launches"] and "k_geo_sweep" not in k
        assert k["geo_seed"]["launches"] == 1 + 3 and k["geo_argmax"]["launches"] == 2 * 3 + 1 and k["k_dist_box"]["launches"] == 1
        assert all(k[name]["ms_sum"] > 0 for name in ("k_geo_tiles", "geo_seed", "geo_argmax"))
        e.set_option("geodesic_tiles", 0)
        e.timing(reset=True)
        st = e.hull_geodesic(extrema=3)
        k = e.timing()["kernels"]
        assert k["k_geo_sweep"]["launches"] == st["launches"] and "k_geo_tiles" not in k and k["k_geo_sweep"]["ms_sum"] > 0
