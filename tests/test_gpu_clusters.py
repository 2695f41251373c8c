"""The hull split into K figures on the floor plane on the device (vc_hull_clusters, the vc_fetch_cluster_* / vc_fetch_floor_*
calls, vc_paint_clusters; csrc/vc_clusters.h) against the restatement (tests/clusters_np.py), bit for bit on the labels, every
vc_cluster_t field, the histograms, the floor map, the floor labels and the stats: the real cameras at 64^3 and 128^3 in both
carve modes, three figures at 64^3 and 256^3, random scenes on grids whose layers start mid-word, one round only, the empty hull,
a single voxel, fewer weighted columns than K, after the passes that change the hull, painting, every refusal, the drop-in layer
over two frames and demo.py --clusters."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import clusters_np as cn
import distance_np as dn
import fixtures_util as fx

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)


@pytest.fixture(scope="module")
def ceng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def figures():
    return cn.three_figures()


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


def _init_um(e, init_mm):
    return np.rint((np.asarray(init_mm, dtype=np.float64) - np.array([e.bounds[0], e.bounds[2]])) * 1000.0).astype(np.int64)


def _check(e, K, max_iters=32, min_column=1, init_mm=None, hist_iz=None):
    """cluster_hull over the current result: every output against the restatement; the result is left alone."""
    rec = e.fetch_records().copy()
    idx = (rec & LOW).astype(np.uint32)
    occ = dn.volume(idx, e.grid)
    q = cn.steps_um_xy(e.grid, e.bounds)
    st = e.cluster_hull(K, max_iters=max_iters, min_column=min_column, init_mm=init_mm, hist_iz=hist_iz)
    want = cn.clusters(occ, q, K, max_iters=max_iters, min_column=min_column, init=None if init_mm is None else _init_um(e, init_mm))
    d = cn.describe(rec, e.grid, want, hist_iz)
    for k in ("survivors", "columns", "weight", "iterations", "q"):
        assert st[k] == want[k], (k, st[k], want[k])
    assert st["converged"] == bool(want["converged"]) and st["clusters_ms"] >= 0.0 and st["k"] == K
    cl = e.fetch_clusters()
    assert np.array_equal(cl["centre_um"], want["centres"]), (cl["centre_um"], want["centres"])
    assert np.array_equal(st["centres_mm"], cn.centres_world_mm(want["centres"], e.bounds))
    assert np.array_equal(e.fetch_floor_map().reshape(-1), want["floor_map"])
    assert np.array_equal(e.fetch_floor_labels().reshape(-1), want["floor_labels"])
    got = e.fetch_cluster_labels()
    assert got.dtype == np.uint8 and got.shape == (idx.size,)
    bad = np.flatnonzero(got != d["labels"])
    assert bad.size == 0, "%d of %d labels differ, first at record %d" % (bad.size, idx.size, bad[0])
    for k in ("voxels", "weight", "columns", "lo", "hi"):
        assert np.array_equal(cl[k], d[k]), (k, cl[k], d[k])
    assert cl["voxels"].dtype == np.uint64 and cl["lo"].shape == (K, 3)
    assert np.array_equal(e.fetch_cluster_histograms(), d["histograms"])
    assert np.array_equal(e.fetch_records(), rec), "the pass leaves the result alone"
    return st, cl, want, d


def _both_floor_maps(e, K, **kw):
    """The floor map from the occupancy words (option cluster_floor_records = 0) and by one atomic per record (the default):
    the same map, and everything behind it, against the restatement."""
    e.set_option("cluster_floor_records", 0)
    try:
        _check(e, K, **kw)
    finally:
        e.set_option("cluster_floor_records", 1)
    _check(e, K, **kw)


@pytest.mark.parametrize("mode", ["fused", "lut"])
@pytest.mark.parametrize("n", [64, 128])
def test_real_cameras_equal_restatement(ceng, cams, masks, frames, n, mode):
    _setup(ceng, (n, n, n), cams, masks, frames)
    if mode == "lut":
        ceng.build_lut()
    S = ceng.carve(mode=mode)
    assert np.array_equal(ceng.fetch()[0], fx.expected(n)[0])
    for K in (1, 2, 4):
        for mc in (1, 8):
            st, cl, want, d = _check(ceng, K, min_column=mc)
            assert st["survivors"] == S and int(cl["voxels"].sum()) == S
            assert st["converged"] == (not (n == 128 and K == 4 and mc == 1))    # (that one takes 46 rounds)
            assert int(d["histograms"].sum()) == S               # the colour camera sees every survivor of these carves
    st, cl, want, d = _check(ceng, 2, hist_iz=(n // 4, n // 2))
    assert 0 < int(d["histograms"].sum()) < S
    _check(ceng, 4, init_mm=[[0.0, 0.0], [300.5, -200.25], [900.0, 900.0], [-512.0, -1024.0]])
    _check(ceng, 2, init_mm=st["centres_mm"])
    _both_floor_maps(ceng, 3)                                    # (hierarchical carves leave dead groups in the words)


@pytest.mark.parametrize("n", [64, 256])
def test_three_figures(ceng, figures, n):
    cams8, masks8 = figures
    _setup(ceng, (n, n, n), cams8, masks8)
    S = ceng.carve()
    st, cl, want, d = _check(ceng, 3)
    assert st["converged"] and (cl["voxels"] > S // 4).all()
    if n == 64:
        assert S == 6143 and st["columns"] == 313 and st["q"] == (24381, 32508)
    truth = np.array(cn.FIGURE_CENTRES)[:, :2]
    step = np.array([24.381, 32.508])                            # one step of the 64^3 grid, at either size
    taken = sorted(int(np.flatnonzero((np.abs(truth - c) <= step).all(axis=1))[0]) for c in st["centres_mm"])
    assert taken == [0, 1, 2]
    warm, _, _, dw = _check(ceng, 3, init_mm=st["centres_mm"])
    assert warm["iterations"] == 1 and warm["converged"] and np.array_equal(dw["labels"], d["labels"])
    _check(ceng, 4, min_column=8)
    _both_floor_maps(ceng, 3)                                    # at 256^3 the walk over the words has 8 z chunks per column group


@pytest.mark.parametrize("K", [3, 16])
@pytest.mark.parametrize("grid,seed,mv", [((37, 53, 29), 3, 1), ((20, 70, 33), 5, 1), ((9, 130, 12), 6, 1)])
def test_random_scenes_on_grids_whose_layers_start_mid_word(ceng, grid, seed, mv, K):
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    _setup(ceng, grid, cams3, masks3, frames3)
    assert ceng.carve(min_views=mv) > 0
    assert (grid[0] * grid[1]) % 64 != 0 and grid[1] % 64 != 0
    st, cl, want, d = _check(ceng, K)
    _check(ceng, K, min_column=3, hist_iz=(1, grid[2] - 2))
    rng = np.random.default_rng(seed)
    b = ceng.bounds
    _check(ceng, K, init_mm=np.stack([rng.uniform(b[0], b[1], K), rng.uniform(b[2], b[3], K)], axis=1))
    _both_floor_maps(ceng, K, min_column=2)


def test_one_round_only(ceng, cams, masks, frames):
    _setup(ceng, (64, 64, 64), cams, masks, frames)
    ceng.carve()
    st, cl, want, d = _check(ceng, 3, max_iters=1)
    assert st["iterations"] == 1 and not st["converged"]
    full, clf, _, _ = _check(ceng, 3)
    assert full["iterations"] > 1 and not np.array_equal(cl["centre_um"], clf["centre_um"])
    st255, _, _, _ = _check(ceng, 3, max_iters=255)
    assert st255["iterations"] == full["iterations"]


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


def test_empty_hull_single_voxel_fewer_columns_than_k(ceng, cams, masks, frames):
    H, W = masks[0].shape
    _setup(ceng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert ceng.carve() == 0
    st, cl, want, d = _check(ceng, 3)
    assert st["iterations"] == 0 and st["converged"] and st["weight"] == 0 and not cl["centre_um"].any()
    assert (cl["lo"] == 0xffffffff).all() and (cl["hi"] == 0).all() and not cl["voxels"].any()
    assert (ceng.fetch_floor_labels() == 255).all() and ceng.fetch_cluster_labels().size == 0
    st, cl, _, _ = _check(ceng, 2, init_mm=[[10.0, 20.0], [-30.5, 40.0]])
    assert st["iterations"] == 0 and cl["centre_um"].tolist() == [[522000, 1044000], [481500, 1064000]]
    ceng.paint_clusters()                                        # nothing to paint is no error
    # a single voxel with K = 4: every seed falls on its column, three clusters stay empty with duplicate centres
    _setup(ceng, (8, 8, 8), cams, _voxel_masks(cams, H, W, (8, 8, 8), [292]), frames)
    assert ceng.carve() == 1 and int(ceng.fetch()[0][0]) == 292
    st, cl, want, d = _check(ceng, 4)
    assert cl["voxels"].tolist() == [1, 0, 0, 0] and len(set(map(tuple, cl["centre_um"].tolist()))) == 1
    assert cl["lo"][0].tolist() == cl["hi"][0].tolist() == [4, 4, 4] and (cl["lo"][1:] == 0xffffffff).all()
    assert st["converged"] and ceng.fetch_cluster_labels().tolist() == [0]
    # a result with fewer weighted columns than K: three voxels in three columns, five centres
    _setup(ceng, (8, 8, 8), cams, _voxel_masks(cams, H, W, (8, 8, 8), [213, 292, 362]), frames)
    assert ceng.carve() == 3 and ceng.fetch()[0].tolist() == [213, 292, 362]
    st, cl, want, d = _check(ceng, 5)
    assert st["columns"] == 3 and sorted(cl["voxels"].tolist()) == [0, 0, 1, 1, 1] and st["converged"]
    assert len(set(map(tuple, cl["centre_um"].tolist()))) == 3
    _check(ceng, 16)
    st, _, _, _ = _check(ceng, 2, min_column=2)                  # a floor no column reaches: no rounds, every label 0
    assert st["weight"] == 0 and st["iterations"] == 0 and st["converged"] and not ceng.fetch_cluster_labels().any()


def test_after_the_passes_that_change_the_hull(ceng, cams, masks, frames):
    from voxcarve._lib import VoxcarveError
    n = 128
    _setup(ceng, (n, n, n), cams, masks, frames)
    for c in range(4):
        ceng.upload_frame(c, frames[c])
    S = ceng.carve()

    def stale():
        assert not ceng.clusters_valid()
        for call in (ceng.fetch_cluster_labels, ceng.fetch_clusters, ceng.fetch_cluster_histograms, ceng.fetch_floor_map,
                     ceng.fetch_floor_labels, ceng.paint_clusters):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no clusters"):
                call()

    stale()
    _, before, _, _ = _check(ceng, 3)
    assert ceng.clusters_valid()
    ceng.color_visible()                                         # colours only: the split stays
    assert ceng.clusters_valid() and np.array_equal(ceng.fetch_clusters()["voxels"], before["voxels"])
    _check(ceng, 3)                                              # (the histograms follow the new colours)
    ceng.hull_distance()                                         # leaves the result alone
    assert ceng.clusters_valid()
    assert ceng.close_hull(0.0)["added"] == 0                    # a grow that adds nothing
    assert ceng.clusters_valid()
    assert ceng.photo_carve(max_rounds=2)["survivors_after"] < S
    stale()
    _check(ceng, 3)
    ceng.carve()
    stale()
    ceng.cluster_hull(3)
    assert ceng.filter_components(keep_largest=1)["survivors_after"] < S
    stale()
    _check(ceng, 3)
    ceng.carve()
    ceng.cluster_hull(3)
    assert ceng.open_hull(25)["survivors_after"] < S
    stale()
    _check(ceng, 3)
    ceng.carve()
    ceng.cluster_hull(3)
    assert ceng.close_hull(40)["added"] > 0
    stale()
    _check(ceng, 3)


def test_paint(ceng, figures):
    from voxcarve import camera
    from voxcarve.clusters import PALETTE
    cams8, masks8 = figures
    H, W = masks8[0].shape
    frames8 = fx.synthetic_frames(8, H, W)
    _setup(ceng, (64, 64, 64), cams8, masks8, frames8)
    ceng.carve()
    rec = ceng.fetch_records().copy()
    _, _, _, d = _check(ceng, 3)
    ceng.paint_clusters()
    assert np.array_equal(ceng.fetch_records(), cn.paint(rec, d["labels"], PALETTE[:3]))
    assert np.array_equal(ceng.fetch_cluster_labels(), d["labels"])               # painting leaves the split valid
    out = ceng.render(camera.orbit(2, 4500.0, 25.0, 150.0, 90, 120), 90, 120, shade=(255,) * 7, background=(9, 9, 9))
    colours = set(map(tuple, out["rgb"].reshape(-1, 3).tolist()))
    assert colours <= set(map(tuple, PALETTE[:3].tolist())) | {(9, 9, 9)} and len(colours) == 4
    own = np.array([[1, 2, 3], [250, 128, 0], [0, 0, 0]], dtype=np.uint8)
    ceng.paint_clusters(own)
    assert np.array_equal(ceng.fetch_records(), cn.paint(rec, d["labels"], own))
    with pytest.raises(ValueError):
        ceng.paint_clusters(own[:2])
    ceng.carve()
    assert np.array_equal(ceng.fetch_records(), rec)             # the next carve: the camera's colours again


def test_refusals(built, cams, masks, frames):
    """Every refusal of the contract but one: a communicator of more than one rank needs two processes with a device each, and
    the message comes from the check the other post-carve passes share."""
    import voxcarve
    from voxcarve._lib import VoxcarveError, VcClusterStats
    H, W = masks[0].shape
    with voxcarve.CarveEngine(0) as e:
        e.set_grid(64, 64, 64)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.cluster_hull(2)
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        S = e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no clusters"):
            e.fetch_cluster_labels()
        st = VcClusterStats()
        L = e._L
        err = lambda: L.vc_last_error(e._ctx).decode()
        call = lambda K=2, it=32, mc=1, lo=0, hi=63, init=None, flags=0, stats=ctypes.byref(st): \
            L.vc_hull_clusters(e._ctx, K, it, mc, lo, hi, init, flags, stats)
        assert call(flags=1) == -1 and "flags" in err()
        assert call(stats=None) == -1 and "stats" in err()
        assert call(K=0) == -1 and "K = 0" in err()
        assert call(K=17) == -1 and "K = 17" in err()
        assert call(it=0) == -1 and "max_iters" in err()
        assert call(it=256) == -1 and "max_iters" in err()
        assert call(lo=5, hi=4) == -1 and "band" in err()
        assert call(hi=64) == -1 and "band" in err()
        far = (ctypes.c_int64 * 4)(0, 0, (1 << 30) + 1, 0)
        assert call(init=far) == -1 and "init" in err()
        edge = (ctypes.c_int64 * 4)(-(1 << 30), 1 << 30, 1 << 30, -(1 << 30))
        assert call(init=edge) == 0 and call(K=16, it=255, lo=63, hi=63) == 0 and call(mc=0) == 0
        assert e.fetch_cluster_labels().size == S
        assert e.count == S and e.fetch_records().size == S
        for bad in ([[0.0, 0.0]], [[0.0, float("nan")], [1.0, 1.0]]):
            with pytest.raises(ValueError):
                e.cluster_hull(2, init_mm=bad)
        with pytest.raises(ValueError):
            e.cluster_hull(2, hist_iz=(-1, 3))
        # the refusals every pass over the result shares, and the metric's (x and y only: one layer of z is fine)
        e.set_grid(64, 64, 64, bounds=(0, 63 * 1100.0, 0, 1, 0, 1))
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis x"):
            e.cluster_hull(2)
        e.set_grid(64, 64, 64, bounds=(0, 1, 0, 63 * 1100.0, 0, 1))
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*axis y"):
            e.cluster_hull(2)
        e.set_grid(64, 64, 1, bounds=(-512.0, 1024.0, -1024.0, 1024.0, -768.0, -768.0))
        e.carve()
        assert e.cluster_hull(2)["survivors"] == e.count
        e.set_grid(64, 64, 64)
        e.carve(records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.cluster_hull(2)
        e.set_slab(0, 32)
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.cluster_hull(2)
        e.set_slab(0, 64)
        e.carve()
        e.cluster_hull(2)
        e.carve_begin()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
            e.cluster_hull(2)
        e.carve_end()
        assert e.cluster_hull(2)["survivors"] == S


# ---- the drop-in layer and the demo ----------------------------------------------------------------------------------------------
def test_assignment_end_to_end(built, cams, masks, frames):
    """Three figures seen by the calibrated cameras over two frames, the second with its masks rolled by 3 columns: label k of
    the second frame is the figure label k was in the first."""
    from voxcarve import assignment, synthetic
    from voxcarve.clusters import PALETTE
    H, W = masks[0].shape
    per = [synthetic.ellipsoid_masks(cams, H, W, radii=cn.FIGURE_RADII, centre=c, noise=0) for c in cn.FIGURE_CENTRES]
    m0 = [np.maximum(np.maximum(a, b), c) for a, b, c in zip(*per)]
    m1 = synthetic.shifted_masks(m0, 1)
    saved = dict(assignment._settings)
    try:
        for bad in (-1, 17, 2.5):
            with pytest.raises(ValueError):
                assignment.configure(clusters=bad)
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, m0), (frames, m1)]), data_path=fx.GOLDEN + "/data",
                             clusters=3)
        with pytest.raises(RuntimeError):
            assignment.clusters()
        pos0, col0 = assignment.set_voxel_positions(64, 32, 64)
        e = assignment._engine
        first = assignment.clusters()
        rec = e.fetch_records()
        occ = dn.volume((rec & LOW).astype(np.uint32), e.grid)
        want = cn.clusters(occ, cn.steps_um_xy(e.grid, e.bounds), 3)
        assert np.array_equal(first["figures"]["centre_um"], want["centres"]) and first["converged"]
        assert first["identity"] == (0, 1, 2) and (first["figures"]["voxels"] > 0).all()
        assert np.array_equal(first["histograms"], cn.describe(rec, e.grid, want)["histograms"])
        pos1, col1 = assignment.set_voxel_positions(64, 32, 64)
        second = assignment.clusters()
        rec = e.fetch_records()
        occ = dn.volume((rec & LOW).astype(np.uint32), e.grid)
        want = cn.clusters(occ, cn.steps_um_xy(e.grid, e.bounds), 3, init=first["figures"]["centre_um"])
        assert np.array_equal(second["figures"]["centre_um"], want["centres"])     # warm-started from the first frame's centres
        assert not np.array_equal(second["figures"]["centre_um"], first["figures"]["centre_um"])
        for k in range(3):
            d = ((first["centres_mm"] - second["centres_mm"][k]) ** 2).sum(axis=1)
            assert int(np.argmin(d)) == k
        assert sorted(second["identity"]) == [0, 1, 2]
        assert assignment.set_voxel_positions(64, 32, 64) == ([], [])
        # painted: the viewer's colours are the palette's
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, m0)]), data_path=fx.GOLDEN + "/data", clusters=3,
                             cluster_paint=True)
        pos, col = assignment.set_voxel_positions(64, 32, 64)
        assert np.array_equal(pos, pos0)
        labels = assignment._engine.fetch_cluster_labels()
        assert np.array_equal((col * 255.0 + 0.5).astype(np.uint8), PALETTE[labels])
        assert np.array_equal(assignment.clusters()["histograms"], first["histograms"])    # signatures come before the paint
    finally:
        assignment.configure(frame_source=None, **saved)


def test_demo_clusters(built, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "demo.py"), "64", str(tmp_path / "hull.ply"), "--clusters", "3",
                        "--cluster-paint"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("figure ")]
    assert len(lines) == 3 and "clusters: 3 figures" in r.stdout
    from voxcarve.clusters import PALETTE
    body = open(tmp_path / "hull.ply").read().split("end_header\n")[1].splitlines()
    colours = set(tuple(int(v) for v in l.split()[3:6]) for l in body)
    assert colours and colours <= set(map(tuple, PALETTE[:3].tolist()))
