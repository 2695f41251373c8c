"""The hull's shell on the device (vc_hull_shell, vc_fetch_shell, vc_fetch_shell_viewer; csrc/vc_shell.h) against the restatement
(tests/shell_np.py) on the fetched records, bit for bit on the records, the face bytes, the stats and the viewer's arrays: the
real cameras at 64^3 in both carve modes at levels 0, 1, 2, 3 and 6, random scenes on grids whose rows and layers start mid-word
and whose hulls touch all six border planes, a full grid, the empty hull, a single voxel, the measurements and the renderer as
independent witnesses, staleness, every refusal, the drop-in layer over two frames and demo.py --shell."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures_util as fx
import shell_np as sn

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)
FULL_BOUNDS = (-200.0, 600.0, -400.0, 400.0, -1200.0, -100.0)


@pytest.fixture(scope="module")
def seng(built):
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


def _check(e, level, scaling=64):
    """hull_shell over the current result: every output against the restatement; the result is left alone."""
    rec = e.fetch_records().copy()
    occ = e.fetch_occupancy().copy()
    st = e.hull_shell(level)
    want = sn.shell(rec, e.grid, level)
    got_rec, got_faces = e.fetch_shell()
    sn.same({"records": got_rec, "faces": got_faces, "stats": {k: st[k] for k in want["stats"]}}, want)
    assert st["shell_ms"] >= 0.0 and e.shell_valid()
    pos, col = e.fetch_shell_viewer(scaling)
    wp, wc = sn.viewer(want["records"], e.grid, e.axes(), level, scaling)
    sn.same_bits(pos, wp)
    sn.same_bits(col, wc)
    assert np.array_equal(e.fetch_records(), rec) and np.array_equal(e.fetch_occupancy(), occ), "the pass leaves the result alone"
    assert e.count == rec.size
    return st, want


# ---- 1 the real cameras ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "lut"])
def test_real_cameras_every_level(seng, cams, masks, frames, mode):
    from voxcarve.engine import unpack_records, viewer_colors, viewer_positions, voxel_keys
    _setup(seng, (64, 64, 64), cams, masks, frames)
    if mode == "lut":
        seng.build_lut()                                         # (the hierarchical carve leaves dead groups in the words)
    S = seng.carve(mode=mode)
    assert S == 6981 > 4096 and np.array_equal(seng.fetch()[0], fx.expected(64)[0])     # more than one compaction group
    pins = {0: (6981, 2703), 1: (1178, 652), 2: (231, 170), 3: (49, 43), 6: (1, 1)}
    for L in (0, 1, 2, 3, 6):
        st, want = _check(seng, L)
        assert (st["cells_on"], st["shell"]) == pins[L] and st["cube_scale"] == 1 << L
        if L == 0:
            assert st["faces"] == [772, 772, 864, 864, 856, 856]
            # the host's arithmetic on the selected records
            idx, rgb, _ = unpack_records(want["records"])
            pos, col = seng.fetch_shell_viewer()
            sn.same_bits(pos, viewer_positions(voxel_keys(idx, seng.grid, seng.axes())))
            sn.same_bits(col, viewer_colors(rgb))
            # the measurements count the same surface and faces with a kernel of their own
            seng.measure_hull()
            m = seng.fetch_measure()
            assert int(m["surface"][0]) == st["shell"] and m["faces"][0].tolist() == st["faces"]
            assert seng.shell_valid() and seng.measure_valid()
    _check(seng, 2, scaling=-37.5)                               # any finite scaling but 0


def test_every_render_hit_lies_in_the_shell(seng, cams, masks, frames):
    _setup(seng, (64, 64, 64), cams, masks, frames)
    seng.carve()
    seng.hull_shell(0)
    rec, faces = seng.fetch_shell()
    face_of = np.zeros(64 ** 3, dtype=np.uint8)
    face_of[(rec & LOW).astype(np.int64)] = faces
    H, W = masks[0].shape
    r = seng.render(cams, H, W)
    assert seng.shell_valid()                                    # rendering leaves the result alone
    hit = r["index"] != 0xFFFFFFFF
    assert hit.sum() > 4000 and (face_of[r["index"][hit].astype(np.int64)] != 0).all()
    entered = hit & (r["face"] < 6)
    assert entered.any() and ((face_of[r["index"][entered].astype(np.int64)] >> r["face"][entered]) & 1).all()


# ---- 2 random scenes: rows and layers that start mid-word, hulls on all six border planes, survivors the colour camera misses -----------
@pytest.mark.parametrize("grid,min_views,S", [((13, 70, 9), 2, 2864), ((33, 31, 17), 2, 6183), ((5, 64, 3), 1, 798)])
def test_random_scenes(seng, grid, min_views, S):
    cams3, masks3, frames3 = fx.random_scene(5, C=3, fg=0.7)
    _setup(seng, grid, cams3, masks3, frames3)
    assert seng.carve(min_views=min_views) == S
    idx, _, seen = seng.fetch()
    idx = idx.astype(np.int64)
    nx, ny, nz = grid
    for c, n in ((idx % ny, ny), ((idx // ny) % nx, nx), (idx // (nx * ny), nz)):
        assert (c == 0).any() and (c == n - 1).any()             # all six border planes
    assert seen.any() and not seen.all()
    for L in (0, 1, 2, 3):
        st, want = _check(seng, L)
        assert 0 < st["shell"] <= st["cells_on"]
        if L == 1:
            assert ((want["records"] >> np.uint64(56)) == 0).any()     # a coarse cell none of whose shell voxels is seen


# ---- 3 edges -----------------------------------------------------------------------------------------------------------------------
def test_full_grid(seng, cams, masks, frames):
    H, W = masks[0].shape
    nx, ny, nz = grid = (16, 66, 8)
    _setup(seng, grid, cams, [np.full((H, W), 255, np.uint8)] * 4, frames, bounds=FULL_BOUNDS)
    assert seng.carve() == nx * ny * nz
    st, want = _check(seng, 0)
    assert st["shell"] == nx * ny * nz - 14 * 64 * 6 and st["faces"] == [ny * nz] * 2 + [nx * nz] * 2 + [nx * ny] * 2
    i = (want["records"] & LOW).astype(np.int64)
    iy, ix, iz = i % ny, (i // ny) % nx, i // (nx * ny)
    border = ((ix == 0) * 1 + (ix == nx - 1) * 2 + (iy == 0) * 4 + (iy == ny - 1) * 8 + (iz == 0) * 16 + (iz == nz - 1) * 32).astype(np.uint8)
    assert np.array_equal(seng.fetch_shell()[1], border)
    for L in (1, 2, 3):
        st, _ = _check(seng, L)
        assert st["cells_on"] == st["dims"][0] * st["dims"][1] * st["dims"][2]
    st, _ = _check(seng, 6)
    assert st["dims"] == [1, 2, 1] and st["shell"] == 2
    # one coarse cell remains where no axis has more than 64 cells
    _setup(seng, (16, 64, 8), cams, [np.full((H, W), 255, np.uint8)] * 4, frames, bounds=FULL_BOUNDS)
    assert seng.carve() == 16 * 64 * 8
    st, _ = _check(seng, 6)
    assert st["shell"] == st["cells_on"] == 1 and seng.fetch_shell()[1].tolist() == [63]


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


def test_empty_hull_and_single_voxel(seng, cams, masks, frames):
    H, W = masks[0].shape
    _setup(seng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    assert seng.carve() == 0
    for L in (0, 2):
        st, _ = _check(seng, L)
        assert st["shell"] == st["cells_on"] == 0 and st["faces"] == [0] * 6
        rec, faces = seng.fetch_shell()
        pos, col = seng.fetch_shell_viewer()
        assert rec.shape == (0,) and faces.shape == (0,) and pos.shape == (0, 3) and col.shape == (0, 3)
    _setup(seng, (8, 8, 8), cams, _voxel_masks(cams, H, W, (8, 8, 8), [292]), frames)
    assert seng.carve() == 1 and int(seng.fetch()[0][0]) == 292
    for L in (0, 1, 3):
        st, _ = _check(seng, L)
        assert st["shell"] == 1 and seng.fetch_shell()[1].tolist() == [63] and st["faces"] == [1] * 6
        assert int(seng.fetch_shell()[0][0] & LOW) == {0: 292, 1: (2 * 4 + 2) * 4 + 2, 3: 0}[L]


# ---- 4 around the pass: staleness and refusals ---------------------------------------------------------------------------------------
def test_around_the_pass(seng, cams, masks, frames):
    from voxcarve._lib import VoxcarveError
    _setup(seng, (64, 64, 64), cams, masks, frames)
    for c in range(4):
        seng.upload_frame(c, frames[c])
    S = seng.carve()

    def stale():
        assert not seng.shell_valid()
        for call in (seng.fetch_shell, seng.fetch_shell_viewer):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no shell"):
                call()

    stale()
    seng.measure_hull()
    _check(seng, 0)
    assert seng.measure_valid()                                  # the pass never advances the result's generation
    before = [a.copy() for a in seng.fetch_shell() + seng.fetch_shell_viewer()]
    old = seng.fetch_records().copy()
    seng.color_visible()                                         # colours only: the shell stays, with the colours it saw
    assert seng.shell_valid() and not np.array_equal(seng.fetch_records(), old)
    after = seng.fetch_shell() + seng.fetch_shell_viewer()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    _check(seng, 0)                                              # (listed again, the records follow the new colours)
    _check(seng, 1)
    seng.cluster_hull(2)
    seng.paint_clusters()
    assert seng.shell_valid()
    _check(seng, 2)
    assert seng.open_hull(25)["survivors_after"] < S
    stale()
    _check(seng, 0)
    seng.carve()
    stale()
    _check(seng, 3)
    assert seng.filter_components(keep_largest=1)["survivors_after"] <= S
    stale()


def test_refusals(built, cams, masks, frames):
    """Every refusal of the contract but one: a communicator of more than one rank needs two processes with a device each, and
    the message comes from the check the other post-carve passes share."""
    import voxcarve
    from voxcarve._lib import VoxcarveError, VcShellStats
    H, W = masks[0].shape
    with voxcarve.CarveEngine(0) as e:
        e.set_grid(64, 64, 64)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.hull_shell()
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        S = e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no shell"):
            e.fetch_shell()
        st = VcShellStats()
        L = e._L
        err = lambda: L.vc_last_error(e._ctx).decode()
        call = lambda level=0, flags=0, stats=ctypes.byref(st): L.vc_hull_shell(e._ctx, level, flags, stats)
        assert call(stats=None) == -1 and "stats" in err()
        assert call(flags=1) == -1 and "flags" in err()
        assert call(level=7) == -1 and "level 7" in err()
        assert not e.shell_valid()                               # a refused call leaves no shell behind ...
        assert call(level=6) == 0 and st.shell == 1 and st.cube_scale == 64
        assert call(level=7) == -1 and call(flags=2) == -1 and call(stats=None) == -1
        assert e.shell_valid()                                   # ... and takes none away: nothing was launched
        e.hull_shell(6)
        assert e.fetch_shell()[1].tolist() == [63]
        with pytest.raises(ValueError):
            e.hull_shell(-1)
        fp = ctypes.POINTER(ctypes.c_float)
        pos = np.zeros((1, 3), np.float32)
        for bad in (0.0, float("inf"), float("-inf"), float("nan")):
            assert L.vc_fetch_shell_viewer(e._ctx, bad, pos.ctypes.data_as(fp), pos.ctypes.data_as(fp)) == -1 and "scaling" in err()
        assert L.vc_fetch_shell_viewer(e._ctx, 64.0, None, None) == 0 and L.vc_fetch_shell(e._ctx, None, None) == 0
        # the refusals every pass over the result shares
        e.carve(records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.hull_shell()
        e.set_slab(0, 32)
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.hull_shell()
        e.set_slab(0, 64)
        e.carve()
        e.hull_shell()
        e.carve_begin()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
            e.hull_shell()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no shell"):
            e.fetch_shell_viewer()
        e.carve_end()
        assert e.hull_shell()["survivors"] == S


# ---- 5 the drop-in layer and the demo ------------------------------------------------------------------------------------------------
def test_assignment_end_to_end(built, cams, masks, frames):
    from voxcarve import assignment, synthetic
    sets = [(frames, masks), (frames, synthetic.shifted_masks(masks, 1))]
    saved = dict(assignment._settings)
    try:
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=fx.GOLDEN + "/data")
        full = []
        for frame in range(2):
            pos, col = assignment.set_voxel_positions(64, 32, 64)
            e = assignment._engine
            full.append((pos, col, e.fetch_records().copy(), e.fetch_occupancy().copy()))
        with pytest.raises(RuntimeError, match="no shell"):
            assignment.shell()
        assert not np.array_equal(full[0][2], full[1][2])
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=fx.GOLDEN + "/data", output="shell")
        for frame in range(2):
            pos, col = assignment.set_voxel_positions(64, 32, 64)
            apos, acol, rec, occ = full[frame]
            want = sn.shell(rec, (64, 64, 64), 0)
            keep = np.isin(rec & LOW, want["records"] & LOW)
            assert 0 < keep.sum() == want["stats"]["shell"] < rec.size
            sn.same_bits(pos, apos[keep])
            sn.same_bits(col, acol[keep])
            st = assignment.shell()
            assert {k: st[k] for k in want["stats"]} == want["stats"] and st["cube_scale"] == 1
            assert np.array_equal(assignment.voxels_status().reshape(-1), occ.reshape(-1))     # unaffected
        assert assignment.set_voxel_positions(64, 32, 64) == ([], [])
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=fx.GOLDEN + "/data", output="shell",
                             output_level=1)
        for frame in range(2):
            pos, col = assignment.set_voxel_positions(64, 32, 64)
            want = sn.shell(full[frame][2], (64, 64, 64), 1)
            wp, wc = sn.viewer(want["records"], (64, 64, 64), assignment._engine.axes(), 1, 64)
            sn.same_bits(pos, wp)
            sn.same_bits(col, wc)
            assert assignment.shell()["cube_scale"] == 2 and assignment.shell()["shell"] == want["stats"]["shell"] == len(pos)
        assert assignment.set_voxel_positions(64, 32, 64) == ([], [])
    finally:
        assignment.configure(frame_source=None, **saved)


def test_demo_shell(built, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "shell.ply"
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "demo.py"), "64", str(out), "--shell"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "shell (level 0, cubes x1 on a 64x64x64 grid): 6981 survivors in 6981 cells, 2703 with an exposed face (38.7 %" in r.stdout
    assert "faces -x 772 +x 772 -y 864 +y 864 -z 856 +z 856" in r.stdout and "6981 voxels of the 64x64x64 grid" in r.stdout
    assert "element vertex 2703\n" in out.read_text()[:200]
