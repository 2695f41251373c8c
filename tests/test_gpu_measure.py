"""The hull's figures measured on the device (vc_hull_measure, vc_fetch_measure, vc_fetch_measure_profile; csrc/vc_measure.h)
against the restatement (tests/measure_np.py) on the fetched records, bit for bit on every field of every group, the profile and
the stats: the real cameras at 64^3 in both carve modes with every label source, random scenes on grids whose rows and layers
start mid-word and whose hulls touch all six border planes, full grids, three figures at 256^3 where the second moments pass 32
bits, the empty hull, a single voxel, staleness, every refusal, the drop-in layer over two frames and demo.py --measure."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import clusters_np as cn
import fixtures_util as fx
import measure_np as mn

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)
FULL_BOUNDS = (-200.0, 600.0, -400.0, 400.0, -1200.0, -100.0)


@pytest.fixture(scope="module")
def meng(built):
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


def _labels(e, source, S, labels, groups):
    """The u32 labels (mn.NONE: no group) and G the restatement takes for what measure_hull is given."""
    if isinstance(source, str) and source == "all":
        return mn.labels_of("all", S)
    if isinstance(source, str) and source == "clusters":
        return mn.labels_of("clusters", S, e.fetch_cluster_labels(), e._cl_k)
    if isinstance(source, str) and source == "geodesic":
        return mn.labels_of("geodesic", S, e.fetch_geodesic_labels(), e._geo_k)
    return np.asarray(labels, dtype=np.uint32), int(groups)


def _check(e, labels="all", groups=None, profile=False):
    """measure_hull over the current result: every output against the restatement; the result is left alone."""
    rec = e.fetch_records().copy()
    lab, G = _labels(e, labels, rec.size, labels, groups)
    st = e.measure_hull(labels=labels, groups=groups, profile=profile)
    want = mn.measure(rec, e.grid, lab, G, with_profile=profile)
    got = e.fetch_measure()
    if profile:
        got["profile"] = e.fetch_measure_profile()
    mn.same(got, want, profile)
    ws = mn.stats(rec, lab, G)
    for k in ("survivors", "groups", "measured", "unlabelled"):
        assert st[k] == ws[k], (k, st[k], ws[k])
    assert st["measure_ms"] >= 0.0 and e.measure_valid()
    if not profile:
        from voxcarve._lib import VoxcarveError
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no measurements by layer"):
            e.fetch_measure_profile()
    assert np.array_equal(e.fetch_records(), rec), "the pass leaves the result alone"
    return st, got, rec


# ---- 1 the real cameras, every source -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "lut"])
def test_real_cameras_every_source(meng, cams, masks, frames, mode):
    _setup(meng, (64, 64, 64), cams, masks, frames)
    if mode == "lut":
        meng.build_lut()                                         # (the hierarchical carve leaves dead groups in the words)
    S = meng.carve(mode=mode)
    assert np.array_equal(meng.fetch()[0], fx.expected(64)[0])
    st, got, rec = _check(meng)
    assert st["measured"] == S and int(got["seen"][0]) == S
    _check(meng, profile=True)
    for K in (1, 2, 4):
        meng.cluster_hull(K)
        st, got, _ = _check(meng, "clusters", profile=(K == 2))
        assert st["groups"] == K and int(got["voxels"].sum()) == S
    geo = meng.hull_geodesic(extrema=5)
    st, got, _ = _check(meng, "geodesic")
    assert st["groups"] == geo["extremities"] + 1 == 6 and st["unlabelled"] == geo["unreached"]
    _check(meng, "geodesic", profile=True)
    assert meng.clusters_valid() and meng.geodesic_valid()       # the pass never advances the result's generation
    # host labels, 4096 groups: interleaved within every wave, and at random; a tenth of the records in no group
    rng = np.random.default_rng(64)
    G = 4096
    for lab in ((np.arange(S) % G).astype(np.uint32), (rng.permutation(S) % G).astype(np.uint32)):
        _check(meng, lab, G)
        lab = lab.copy()
        lab[rng.random(S) < 0.1] = mn.NONE
        st, _, _ = _check(meng, lab, G, profile=True)
        assert 0 < st["unlabelled"] < S
    # a few groups that sit in runs (whole waves of one label) next to lone records of the labels beyond the LDS table
    lab = (np.arange(S) // 500).astype(np.uint32)
    lab[::97] = 4000 + (np.arange(S)[::97] % 96).astype(np.uint32)
    _check(meng, lab, G)
    _check(meng, lab % 321, 321, profile=True)


# ---- 2 random scenes: rows and layers that start mid-word, hulls on all six border planes ------------------------------------------
@pytest.mark.parametrize("grid,seed,S", [((37, 53, 29), 3, 55010), ((20, 70, 33), 5, 38691), ((9, 130, 12), 6, 10954)])
def test_random_scenes_on_grids_whose_rows_start_mid_word(meng, grid, seed, S):
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    _setup(meng, grid, cams3, masks3, frames3)
    assert meng.carve(min_views=1) == S
    assert (grid[0] * grid[1]) % 64 != 0 and grid[1] % 64 != 0
    st, got, rec = _check(meng, profile=True)
    assert got["lo"][0].tolist() == [0, 0, 0] and got["hi"][0].tolist() == [g - 1 for g in grid]     # all six border planes
    idx = (rec & LOW).astype(np.int64)
    assert (idx % grid[1] == 0).any() and (idx % grid[1] == grid[1] - 1).any()
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 5, S).astype(np.uint32)
    lab[rng.random(S) < 0.1] = mn.NONE
    _check(meng, lab, 5, profile=True)
    meng.cluster_hull(3)
    _check(meng, "clusters")


# ---- 3 full grids ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(8, 8, 8), (5, 70, 3), (3, 130, 2)])
def test_full_grids(meng, cams, masks, frames, grid):
    H, W = masks[0].shape
    nx, ny, nz = grid
    _setup(meng, grid, cams, [np.full((H, W), 255, np.uint8)] * 4, frames, bounds=FULL_BOUNDS)
    S = meng.carve()
    assert S == nx * ny * nz
    st, got, _ = _check(meng, profile=True)
    # every face on the border is exposed and none inside
    assert got["faces"][0].tolist() == [ny * nz] * 2 + [nx * nz] * 2 + [nx * ny] * 2
    assert int(got["surface"][0]) == S - max(nx - 2, 0) * max(ny - 2, 0) * max(nz - 2, 0)
    if grid == (8, 8, 8):
        assert int(got["voxels"][0]) == 512 and int(got["surface"][0]) == 296
        assert got["s1"][0].tolist() == [1792] * 3 and got["s2"][0].tolist() == [8960] * 3 + [6272] * 3
        assert got["lo"][0].tolist() == [0, 0, 0] and got["hi"][0].tolist() == [7, 7, 7]
    lab = (np.arange(S) % 3).astype(np.uint32)                   # a neighbour of another group is still a neighbour
    st, got, _ = _check(meng, lab, 3)
    assert got["faces"].sum(axis=0).tolist() == [ny * nz] * 2 + [nx * nz] * 2 + [nx * ny] * 2


# ---- 4 sums past 32 bits -----------------------------------------------------------------------------------------------------------
def test_three_figures_256(meng):
    cams8, masks8 = cn.three_figures()
    _setup(meng, (256, 256, 256), cams8, masks8)
    S = meng.carve()
    assert S == 405719
    st, got, rec = _check(meng)
    want = mn.measure(rec, meng.grid, np.zeros(S, np.uint32), 1)
    assert all(6.0e9 < int(v) < 7.6e9 for v in want["s2"][0]) and 6.0e9 > 2 ** 32     # the precondition: u32 sums would wrap
    meng.cluster_hull(3)
    st, got, _ = _check(meng, "clusters", profile=True)
    assert (got["voxels"] > S // 4).all()


# ---- 5 edges -----------------------------------------------------------------------------------------------------------------------
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


def test_empty_hull_single_voxel_and_nobody_labelled(meng, cams, masks, frames):
    H, W = masks[0].shape
    _setup(meng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert meng.carve() == 0
    st, got, _ = _check(meng, profile=True)
    assert st["measured"] == 0 and not got["voxels"].any() and (got["lo"] == 0xffffffff).all() and (got["hi"] == 0).all()
    st, got, _ = _check(meng, np.zeros(0, np.uint32), 7)
    assert st["groups"] == 7 and got["lo"].shape == (7, 3) and (got["lo"] == 0xffffffff).all()
    meng.cluster_hull(3)
    _check(meng, "clusters")
    meng.hull_geodesic(extrema=2)
    st, _, _ = _check(meng, "geodesic")
    assert st["groups"] == 1
    # a single voxel
    _setup(meng, (8, 8, 8), cams, _voxel_masks(cams, H, W, (8, 8, 8), [292]), frames)
    assert meng.carve() == 1 and int(meng.fetch()[0][0]) == 292
    st, got, _ = _check(meng, profile=True)
    assert got["faces"][0].tolist() == [1] * 6 and got["lo"][0].tolist() == got["hi"][0].tolist() == [4, 4, 4]
    assert got["s2"][0].tolist() == [16] * 6
    _check(meng, np.array([2], np.uint32), 3)
    # S not a multiple of 64, and G = 1 with nobody in it
    _setup(meng, (64, 64, 64), cams, masks, frames)
    S = meng.carve()
    assert S % 64 != 0
    st, got, _ = _check(meng, np.full(S, mn.NONE, np.uint32), 1, profile=True)
    assert st["measured"] == 0 and st["unlabelled"] == S and not got["voxels"].any() and (got["lo"] == 0xffffffff).all()


# ---- 6 staleness and refusals ----------------------------------------------------------------------------------------------------------
def test_after_the_passes_that_change_the_hull(meng, cams, masks, frames):
    from voxcarve._lib import VoxcarveError
    n = 64
    _setup(meng, (n, n, n), cams, masks, frames)
    for c in range(4):
        meng.upload_frame(c, frames[c])
    S = meng.carve()

    def stale():
        assert not meng.measure_valid()
        for call in (meng.fetch_measure, meng.fetch_measure_profile):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no measurements"):
                call()

    stale()
    _, before, _ = _check(meng, profile=True)
    meng.color_visible()                                         # colours only: the measurements stay, as they were at the call
    assert meng.measure_valid()
    after = meng.fetch_measure()
    for k in mn.FIELDS:
        assert np.array_equal(after[k], before[k]), k
    _check(meng)                                                 # (measured again, the colour sums follow the new colours)
    meng.hull_distance()                                         # leaves the result alone
    assert meng.measure_valid()
    assert meng.close_hull(0.0)["added"] == 0                    # a grow that adds nothing
    assert meng.measure_valid()
    assert meng.photo_carve(max_rounds=2)["survivors_after"] < S
    stale()
    _check(meng)
    meng.carve()
    stale()
    meng.measure_hull()
    assert meng.filter_components(keep_largest=1)["survivors_after"] < S
    stale()
    _check(meng)
    meng.carve()
    meng.measure_hull()
    assert meng.open_hull(25)["survivors_after"] < S
    stale()
    _check(meng)
    meng.carve()
    meng.measure_hull()
    assert meng.close_hull(40)["added"] > 0
    stale()
    _check(meng, profile=True)


def test_components_as_groups(meng, cams, masks, frames):
    _setup(meng, (64, 64, 64), cams, masks, frames)
    S = meng.carve()
    with pytest.raises(ValueError, match="once more on its own output"):
        meng.measure_hull(labels="components")                   # no components at all yet
    cc = meng.filter_components(connectivity=6)
    assert cc["survivors_after"] == S and cc["components"] > 1
    comp = meng.fetch_components()
    ranks = mn.component_ranks(meng.fetch_component_labels(), comp["label"], comp["size"])
    st = meng.measure_hull(labels="components")
    by_name = meng.fetch_measure()
    assert st["groups"] == cc["components"] and st["unlabelled"] == 0
    _, by_ranks, _ = _check(meng, ranks, cc["components"])
    for k in mn.FIELDS:
        assert np.array_equal(by_name[k], by_ranks[k]), k
    assert (np.diff(by_name["voxels"].astype(np.int64)) <= 0).all() and int(by_name["voxels"][0]) == cc["largest"]
    assert meng.filter_components(connectivity=6, keep_largest=1)["survivors_after"] < S
    with pytest.raises(ValueError, match="once more on its own output"):
        meng.measure_hull(labels="components")
    assert meng.filter_components(connectivity=6)["components"] == 1
    assert meng.measure_hull(labels="components")["groups"] == 1
    for bad in ("figures", np.zeros(3, np.uint32), np.zeros(meng.count, np.float64)):
        with pytest.raises(ValueError):
            meng.measure_hull(labels=bad, groups=2)
    with pytest.raises(ValueError):
        meng.measure_hull(labels=np.zeros(meng.count, np.uint32))    # an array needs groups=G


def test_refusals(built, cams, masks, frames):
    """Every refusal of the contract but one: a communicator of more than one rank needs two processes with a device each, and
    the message comes from the check the other post-carve passes share."""
    import voxcarve
    from voxcarve._lib import VoxcarveError, VcMeasureStats
    from voxcarve import _lib
    H, W = masks[0].shape
    with voxcarve.CarveEngine(0) as e:
        e.set_grid(64, 64, 64)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.measure_hull()
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        S = e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no measurements"):
            e.fetch_measure()
        st = VcMeasureStats()
        L = e._L
        err = lambda: L.vc_last_error(e._ctx).decode()
        zeros = np.zeros(S, np.uint32)
        ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        call = lambda source=_lib.VC_MEASURE_HOST, labels=ptr(zeros), G=1, flags=0, stats=ctypes.byref(st): \
            L.vc_hull_measure(e._ctx, source, labels, G, flags, stats)
        assert call(stats=None) == -1 and "stats" in err()
        assert call(flags=2) == -1 and "flags" in err()
        assert call(source=4) == -1 and "source" in err()
        assert call(labels=None) == -1 and "labels" in err()
        assert call(G=0) == -1 and "G = 0" in err()
        assert call(G=4097) == -1 and "G = 4097" in err()
        assert call(source=_lib.VC_MEASURE_CLUSTERS) == -1 and "vc_hull_clusters" in err()
        assert call(source=_lib.VC_MEASURE_GEODESIC) == -1 and "vc_hull_geodesic" in err()
        assert not e.measure_valid()                             # a refused call leaves no measurements behind ...
        assert call(G=4096, flags=1) == 0                        # 4096 x 64 layers: inside the profile's limit
        assert call(G=4097) == -1 and e.measure_valid()          # ... and takes none away: nothing was launched
        bad = zeros.copy()
        bad[S // 2] = 3
        assert call(labels=ptr(bad), G=3) == -1 and "record %d has label 3" % (S // 2) in err()
        bad[S // 2] = 0xffffffff
        assert call(labels=ptr(bad), G=3) == 0 and st.unlabelled == 1 and st.measured == S - 1 and st.groups == 3
        assert call(source=_lib.VC_MEASURE_ALL, labels=None, G=0) == 0 and st.groups == 1 and st.survivors == S
        # the labels of a pass that ran on another result
        e.cluster_hull(2)
        e.hull_geodesic(extrema=2)
        assert call(source=_lib.VC_MEASURE_CLUSTERS) == 0 and call(source=_lib.VC_MEASURE_GEODESIC) == 0
        e.carve()
        assert call(source=_lib.VC_MEASURE_CLUSTERS) == -1 and "vc_hull_clusters" in err()
        assert call(source=_lib.VC_MEASURE_GEODESIC) == -1 and "vc_hull_geodesic" in err()
        # a profile of more than 2^20 entries: 4096 groups x 512 layers
        e.set_grid(8, 8, 512)
        e.carve()
        one = np.zeros(max(e.count, 1), np.uint32)
        assert call(labels=ptr(one), G=4096, flags=1) == -1 and "profile" in err()
        assert call(labels=ptr(one), G=2048, flags=1) == 0 and call(labels=ptr(one), G=4096) == 0
        # the refusals every pass over the result shares
        e.set_grid(64, 64, 64)
        e.carve(records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.measure_hull()
        e.set_slab(0, 32)
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.measure_hull()
        e.set_slab(0, 64)
        e.carve()
        e.measure_hull()
        e.carve_begin()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
            e.measure_hull()
        e.carve_end()
        assert e.measure_hull()["survivors"] == S


# ---- 7 the drop-in layer and the demo ------------------------------------------------------------------------------------------------
def test_assignment_end_to_end(built, cams, masks, frames):
    """Three figures seen by the calibrated cameras over two frames, the second with its masks shifted: the measurements of
    each frame equal the restatement, and every figure's velocity is its centroid's step."""
    from voxcarve import assignment, measure, synthetic
    H, W = masks[0].shape
    per = [synthetic.ellipsoid_masks(cams, H, W, radii=cn.FIGURE_RADII, centre=c, noise=0) for c in cn.FIGURE_CENTRES]
    m0 = [np.maximum(np.maximum(a, b), c) for a, b, c in zip(*per)]
    m1 = synthetic.shifted_masks(m0, 1)
    saved = dict(assignment._settings)
    try:
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, m0), (frames, m1)]), data_path=fx.GOLDEN + "/data",
                             clusters=3, measure="clusters", measure_profile=True)
        with pytest.raises(RuntimeError):
            assignment.measurements()
        world = []
        for frame in range(2):
            assignment.set_voxel_positions(64, 32, 64)
            e = assignment._engine
            ms = assignment.measurements()
            rec = e.fetch_records()
            want = mn.measure(rec, e.grid, e.fetch_cluster_labels().astype(np.uint32), 3, with_profile=True)
            got = dict(ms["integers"], profile=ms["profile"])
            mn.same(got, want, True)
            assert ms["groups"] == 3 and ms["measured"] == rec.size and ms["source"] == "clusters"
            w = measure.describe(want, e.grid, e.bounds)
            for k in w:
                assert np.array_equal(ms["world"][k], w[k], equal_nan=True), k
            world.append(w)
            if frame == 0:
                assert ms["velocity_mm"] is None
            else:
                assert np.array_equal(ms["velocity_mm"], world[1]["centroid_mm"] - world[0]["centroid_mm"])
                assert np.isfinite(ms["velocity_mm"]).all() and np.abs(ms["velocity_mm"]).max() > 0
        assert assignment.set_voxel_positions(64, 32, 64) == ([], [])
        # the component filter's labels, after a filter that removed something: the layer labels its output once more
        assignment.configure(frame_source=assignment.StaticFrameSource([(frames, m0)]), data_path=fx.GOLDEN + "/data",
                             keep_components=2, measure="components")
        assignment.set_voxel_positions(64, 32, 64)
        ms = assignment.measurements()
        assert ms["groups"] == 2 and ms["unlabelled"] == 0 and (np.diff(ms["integers"]["voxels"].astype(np.int64)) <= 0).all()
    finally:
        assignment.configure(frame_source=None, **saved)


def test_demo_measure(built, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "demo.py"), "64", "-", "--clusters", "3", "--measure", "clusters"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("group ")]
    assert len(lines) == 3 and "measure: 3 groups by clusters" in r.stdout
    assert all("mm3" in l and "centroid" in l for l in lines)
