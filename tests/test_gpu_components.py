"""Connected components of the hull on the device (vc_hull_components, vc_fetch_component_labels, vc_fetch_components;
csrc/vc_components.h) against the restatement (tests/components_np.py): records (order, colour, seen byte), labels per input
record, the component list (label, size, lo, hi, kept), occupancy words and stats bit for bit -- the real cameras at 64^3 to
512^3 in both carve modes and at 1024^3 (the bench's workload), separated ellipsoids with specks of noise, grids whose columns
straddle occupancy words, a solid hull, the empty hull, a single voxel, a second pass over its own output; every refusal; the
readers after the pass, the next carve, and set_voxel_positions under configure(min_component_voxels=...)."""
import ctypes
import os

import numpy as np
import pytest

import components_np as cn
import fixtures_util as fx
from voxcarve import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ceng(built):
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


def _words(e):
    raw = np.empty((e.n_voxels + 63) // 64, dtype=np.uint64)
    e._check(e._L.vc_fetch_occupancy(e._ctx, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "vc_fetch_occupancy")
    return raw


def _want_words(idx, n):
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    i = np.asarray(idx, dtype=np.uint64)
    np.bitwise_or.at(w, (i >> np.uint64(6)).astype(np.int64), np.uint64(1) << (i & np.uint64(63)))
    return w


def _check(e, conn=26, min_voxels=0, keep_largest=0, literal=False):
    """filter_components over the current result, everything compared with the restatement of its own input records."""
    rec0 = e.fetch_records().copy()
    idx0 = (rec0 & np.uint64(0xffffffff)).astype(np.uint32)
    st = e.filter_components(connectivity=conn, min_voxels=min_voxels, keep_largest=keep_largest)
    want = (cn.components_literal if literal else cn.components)(idx0, e.grid, conn, min_voxels, keep_largest)
    K, F = want["label"].size, want["idx"].size
    assert st["survivors_before"] == rec0.size and st["survivors_after"] == F == e.count
    assert st["components"] == K and st["components_kept"] == int(want["kept"].sum())
    assert st["largest"] == (int(want["size"].max()) if K else 0)
    assert st["components_ms"] > 0 or rec0.size == 0
    assert np.array_equal(e.fetch_component_labels(), want["labels"]), "labels"
    got = e.fetch_components()
    for k in ("label", "size", "lo", "hi", "kept"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(e.fetch_records(), rec0[want["keep"]]), "records"
    assert np.array_equal(_words(e), _want_words(want["idx"], e.n_voxels)), "occupancy words"
    return want, st


@pytest.mark.parametrize("n", [64, 128, 256, 512])
def test_golden_cameras_equal_restatement(ceng, cams, masks, frames, n):
    _setup(ceng, (n, n, n), cams, masks, frames)
    if n <= 128:
        ceng.build_lut()
    for mode in ("fused", "lut") if n <= 128 else ("fused",):
        rules = [(c, mv, kl) for c in cn.CONNECTIVITIES for mv, kl in ((0, 0), (3, 0), (0, 1), (2, 2))] if n <= 128 else \
            [(26, 0, 1), (6, 4, 0)]
        for conn, mv, kl in rules:
            S = ceng.carve(mode=mode)
            want, st = _check(ceng, conn, mv, kl)
            assert st["components"] > 1
        if n in (64, 128):                                       # the fixture table
            S = ceng.carve(mode=mode)
            idx, _, _ = fx.expected(n)
            assert np.array_equal(ceng.fetch()[0], idx)
            counts = {64: (9, 4, 4), 128: (11, 3, 2)}[n]
            for conn, k in zip(cn.CONNECTIVITIES, counts):
                ceng.carve(mode=mode)
                assert ceng.filter_components(connectivity=conn)["components"] == k


def test_bench_workload_1024(ceng, cams, masks, frames):
    _setup(ceng, (1024, 1024, 1024), cams, masks, frames)
    S = ceng.carve(mode="fused")
    want, st = _check(ceng, 26, 0, 1)
    assert st["survivors_before"] == S and st["components"] > 1 and st["components_kept"] == 1


def test_separated_ellipsoids_with_noise(ceng):
    H, W = 240, 320
    cams = synthetic.ring_cameras(8, H, W)
    ctr = np.array(synthetic.VOLUME_CENTRE)
    parts = []
    for k, (off, noise) in enumerate((((-550.0, 0.0, 0.0), 0.01), ((500.0, 300.0, 0.0), 0.0), ((0.0, -700.0, 300.0), 0.01))):
        r = tuple(0.45 * np.array(synthetic.ELLIPSOID_RADII))
        parts.append(synthetic.ellipsoid_masks(cams, H, W, radii=r, centre=tuple(ctr + np.array(off)), noise=noise, seed=1000 + k))
    masks = [np.maximum.reduce([p[c] for p in parts]) for c in range(len(cams))]
    _setup(ceng, (96, 80, 72), cams, masks)
    ceng.carve()
    want, st = _check(ceng, 26, 0, 0)
    assert st["components"] >= 3
    for conn, mv, kl in ((26, 0, 3), (18, 50, 0), (6, 0, 2), (26, 10 ** 9, 0)):
        ceng.carve()
        _check(ceng, conn, mv, kl)


@pytest.mark.parametrize("grid", [(40, 65, 36), (24, 130, 20), (30, 63, 30), (17, 1, 9)])
def test_columns_straddle_words(ceng, cams, masks, frames, grid):
    _setup(ceng, grid, cams, masks, frames)
    for conn in cn.CONNECTIVITIES:
        ceng.carve()
        _check(ceng, conn, 2, 0, literal=grid[0] * grid[1] * grid[2] < 50000)


def test_solid_empty_and_single(ceng, cams, masks, frames):
    H, W = masks[0].shape
    full = [np.full((H, W), 255, np.uint8)] * 4
    _setup(ceng, (32, 48, 40), cams, full, frames)
    ceng.carve()
    want, st = _check(ceng, 26, 0, 0)
    assert st["largest"] >= 0.99 * st["survivors_before"] > 0
    _setup(ceng, (64, 64, 64), cams, [np.zeros((H, W), np.uint8)] * 4, frames)
    ceng.carve()
    want, st = _check(ceng, 26, 5, 1)
    assert st == {"components": 0, "components_kept": 0, "survivors_before": 0, "survivors_after": 0, "largest": 0,
                  "components_ms": st["components_ms"]}
    assert ceng.fetch_component_labels().size == 0 and ceng.fetch_components()["label"].size == 0
    ring = synthetic.ring_cameras(4, 120, 160)
    x, y, z = synthetic.VOLUME_CENTRE
    _setup(ceng, (1, 1, 1), ring, [np.full((120, 160), 255, np.uint8)] * 4, bounds=(x, x, y, y, z, z))
    assert ceng.carve() == 1
    want, st = _check(ceng, 6, 1, 1, literal=True)
    assert st["components"] == 1 and st["survivors_after"] == 1
    ceng.carve()
    want, st = _check(ceng, 6, 2, 0)
    assert st["survivors_after"] == 0 and ceng.count == 0


def test_second_pass_and_readers(ceng, cams, masks, frames):
    """A second pass over the output, marching cubes / packing / colouring / photo carving of the filtered hull, the next carve."""
    n = 128
    _setup(ceng, (n, n, n), cams, masks, frames)
    S = ceng.carve()
    hull = ceng.fetch_records().copy()
    want, st = _check(ceng, 6, 3, 0)
    assert st["survivors_after"] < S
    again, st2 = _check(ceng, 6, 3, 0)
    assert st2["survivors_before"] == st2["survivors_after"] == st["survivors_after"]
    third, st3 = _check(ceng, 26, 0, 1)
    occ = ceng.fetch_occupancy()
    dense = np.zeros(n ** 3, dtype=bool)
    dense[third["idx"]] = True
    assert np.array_equal(occ, dense)
    verts, faces = ceng.marching_cubes(volume=None)
    v2, f2 = ceng.marching_cubes(volume=occ.reshape(n, n, n))
    assert np.array_equal(verts, v2) and np.array_equal(faces, f2) and faces.size > 0
    ent = ceng.pack_entries()
    assert int(np.bitwise_count(ent[:, 0]).sum()) == third["idx"].size
    bits = ent[:, 0]
    base = ent[:, 1]
    got = np.concatenate([b + np.flatnonzero(np.unpackbits(np.array([w], dtype=np.uint64).view(np.uint8), bitorder="little"))
                          for w, b in zip(bits.tolist(), base.tolist())]) if ent.size else np.zeros(0)
    assert np.array_equal(got.astype(np.int64), third["idx"].astype(np.int64))
    for c in range(4):
        ceng.upload_frame(c, frames[c])
    rec = ceng.fetch_records().copy()
    ceng.color_visible()
    assert ceng.fetch_visibility().size == rec.size
    assert np.array_equal(ceng.fetch_records() & np.uint64(0xffffffff), rec & np.uint64(0xffffffff))
    ph = ceng.photo_carve(max_rounds=2)
    assert ph["survivors_before"] == rec.size
    from voxcarve._lib import VoxcarveError
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no component labels"):
        ceng.fetch_component_labels()
    _check(ceng, 26, 0, 1)                                       # over the photo hull
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*(visibility|photo)"):
        ceng.fetch_photo_rounds()
    assert ceng.carve() == S
    assert np.array_equal(ceng.fetch_records(), hull)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no components"):
        ceng.fetch_components()


def test_refusals(ceng, cams, masks, frames):
    import voxcarve
    from voxcarve._lib import VoxcarveError, VcComponentStats
    H, W = masks[0].shape
    with voxcarve.CarveEngine(0) as e:
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.filter_components()
        e.set_grid(64, 64, 64)
        e.set_cameras(cams, H, W)
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no component labels"):
            e.fetch_component_labels()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no components"):
            e.fetch_components()
        for conn in (0, 4, 8, 27):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*connectivity"):
                e.filter_components(connectivity=conn)
        st = VcComponentStats()
        assert e._L.vc_hull_components(e._ctx, 26, 0, 0, 1, ctypes.byref(st)) == -1
        assert "flags" in e._L.vc_last_error(e._ctx).decode()
        assert e._L.vc_hull_components(e._ctx, 26, 0, 0, 0, None) == -1
        assert "stats" in e._L.vc_last_error(e._ctx).decode()
        e.carve(records=False)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
            e.filter_components()
        e.set_slab(0, 32)
        e.carve()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.filter_components()
        e.set_slab(0, 64)
        e.carve_begin()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
            e.filter_components()
        e.carve_end()
        S = e.count
        st = e.filter_components(min_voxels=2)
        assert st["survivors_before"] == S and e.fetch_component_labels().size == S


def test_set_voxel_positions_filters_after_the_carve(built):
    import test_gpu_contour as tc
    from voxcarve import assignment
    from voxcarve.engine import viewer_colors, viewer_positions, voxel_keys
    H, W = 486, 644
    bgs, frame_sets = tc._cams_and_scene(57, H, W, 2)
    data = os.path.join(fx.GOLDEN, "data")
    try:
        fsrc = assignment.DeviceVideoSource([[fs[c] for fs in frame_sets] for c in range(4)], bgs)
        assignment.configure(frame_source=fsrc, data_path=data)
        plain = [assignment.set_voxel_positions(64, 32, 64) for _ in frame_sets]
        sets, hulls = [], []
        fsrc = assignment.DeviceVideoSource([[fs[c] for fs in frame_sets] for c in range(4)], bgs)
        assignment.configure(frame_source=fsrc, data_path=data)
        for fs in frame_sets:
            assignment.set_voxel_positions(64, 32, 64)
            sets.append((fs, [assignment._engine.fetch_mask(c) for c in range(4)]))
            hulls.append(assignment._engine.fetch_records().copy())
        grid, axes = assignment._engine.grid, assignment._engine.axes()
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=data)
        for (p0, c0) in plain:                                   # the default: unchanged
            p1, c1 = assignment.set_voxel_positions(64, 32, 64)
            assert np.array_equal(p0, p1) and np.array_equal(c0, c1)
        for conn, mv, kl in ((26, 4, 0), (6, 0, 1)):
            assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=data, min_component_voxels=mv,
                                 keep_components=kl, component_connectivity=conn)
            for (fs, ms), rec in zip(sets, hulls):
                p, c = assignment.set_voxel_positions(64, 32, 64)
                want = cn.components((rec & np.uint64(0xffffffff)).astype(np.uint32), grid, conn, mv, kl)
                kept = rec[want["keep"]]
                idx = (kept & np.uint64(0xffffffff)).astype(np.uint32)
                rgb = np.stack([(kept >> np.uint64(k)) & np.uint64(0xff) for k in (32, 40, 48)], axis=1).astype(np.uint8)
                assert np.array_equal(p, viewer_positions(voxel_keys(idx, grid, axes)))
                assert np.array_equal(c, viewer_colors(rgb))
                dense = np.zeros(int(np.prod(grid)), dtype=bool)
                dense[idx] = True
                assert np.array_equal(assignment.voxels_status(), dense.reshape(grid))
    finally:
        assignment.configure(frame_source=None, min_component_voxels=0, keep_components=0, component_connectivity=26)
