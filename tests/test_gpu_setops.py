"""Set algebra on hulls on the device (vc_hull_keep, vc_hull_upload, vc_hull_release, vc_fetch_kept, vc_hull_combine,
vc_fetch_combined, vc_hull_compare; csrc/vc_setops.h) against the restatement (tests/setops_np.py), bit for bit: every op against a
kept carve and host uploads in all three forms, on grids of 2, 11, 120 and 889 words; edge operands and the reload path; the
upload's refusals; the registers' lifetime; the comparison against numpy and dn.outside with a pinned case on the real cameras;
what a combine invalidates; passes that read the combined hull; 128^3 on invariants; every refusal; configure(hull_subtract=...,
hull_clip=...)."""
import ctypes
import os

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import setops_np as sn
import temporal_np as tn

pytestmark = pytest.mark.gpu

LOW = np.uint64(0xffffffff)
GRIDS = [((5, 7, 3), 3, 1), ((9, 11, 7), 6, 1), ((12, 64, 10), 7, 2), ((37, 53, 29), 4, 2)]


@pytest.fixture(scope="module")
def seng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _words(e):
    raw = np.empty((e.n_voxels + 63) // 64, dtype=np.uint64)
    e._check(e._L.vc_fetch_occupancy(e._ctx, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "vc_fetch_occupancy")
    return raw


def _want_words(occ):
    return np.packbits(np.asarray(occ, dtype=bool).reshape(-1), bitorder="little").tobytes().ljust((occ.size + 63) // 64 * 8, b"\0")


def _start(e, grid, cams, masks, frames=None, cc=1):
    H, W = masks[0].shape
    e.set_grid(*grid)
    e.set_cameras(cams, H, W)
    e.upload_masks(masks)
    if frames is not None and cc is not None:
        e.upload_frame(cc, frames[cc])


def _other_masks(seed, fg, C=3):
    """The scene's own masks with a fifth of the pixels drawn again: a hull that overlaps the scene's and differs from it."""
    _, base, _ = fx.random_scene(seed, C=C, fg=fg)
    rng = np.random.default_rng(100 * seed + 1)
    return [np.where(rng.random(m.shape) < 0.2, np.where(rng.random(m.shape) < fg, 255, 0), m).astype(np.uint8) for m in base]


def _hull(e):
    rec = e.fetch_records().copy()
    return rec, dn.volume((rec & LOW).astype(np.uint32), e.grid)


def _check_combine(e, op, reg, occ_b, rec_b, cam, frame):
    """combine_hull over the current result: records (order, all 8 bytes), added bytes, occupancy words and every stat."""
    rec, occ = _hull(e)
    H, W = e.image_size
    want, wadded, r, ws = sn.combine(rec, occ, occ_b, rec_b, op, e.grid, e.bounds, cam, frame, H, W)
    st = e.combine_hull(op, reg)
    ms = st.pop("setop_ms")
    assert st == ws, (op, st, ws)
    assert ms > 0 and e.count == want.size
    got = e.fetch_records()
    assert np.array_equal(got & LOW, want & LOW), "indices and order"
    assert np.array_equal(got, want), "records"
    assert np.array_equal(e.fetch_combined(), wadded), "added bytes"
    assert _words(e).tobytes() == _want_words(r), "occupancy words"
    return st, want, wadded


@pytest.mark.parametrize("grid,seed,mv", GRIDS)
def test_every_op_equals_restatement(seng, grid, seed, mv):
    """B is another carve of the scene, kept on the device (records) and uploaded as records, as a bool volume and as indices (no
    records: fresh voxels are coloured from the colour camera, some outside its image)."""
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    cam = fx.oracle_cams(cams3)[1]
    _start(seng, grid, cams3, masks3, frames3)
    seng.upload_masks(_other_masks(seed, 0.7))
    assert seng.carve(min_views=mv) > 0
    rec_b, occ_b = _hull(seng)
    seng.keep_hull(0)
    seng.upload_hull(rec_b, 1)
    seng.upload_hull(occ_b, 2)
    seng.upload_hull((rec_b & LOW).astype(np.uint32), 3)
    for reg in range(4):
        k = seng.fetch_kept(reg)
        assert k["count"] == rec_b.size and k["has_records"] == (reg < 2) and k["words"].tobytes() == _want_words(occ_b)
        assert np.array_equal(k["records"], rec_b) if reg < 2 else k["records"] is None
    seng.upload_masks(masks3)
    added = removed = coloured = unseen = taken = 0
    for op in sn.OPS:
        for reg in range(4):
            assert seng.carve(min_views=mv) > 0
            st, want, wadded = _check_combine(seng, op, reg, occ_b, rec_b if reg < 2 else None, cam, frames3[1])
            added += st["added"]
            removed += st["removed"]
            fresh = want[wadded == 1]
            if reg >= 2:
                coloured += int((((fresh >> np.uint64(32)) & np.uint64(0xffffff)) != 0).sum())
                unseen += int(((fresh >> np.uint64(56)) == 0).sum())
            else:
                taken += fresh.size
                assert np.isin(fresh, rec_b).all()
    assert added > 0 and removed > 0 and coloured > 0 and taken > 0
    if grid == (37, 53, 29):
        assert unseen > 0


def test_no_colour_camera_and_no_image(built):
    import voxcarve
    cams3, masks3, _ = fx.random_scene(11, C=3, fg=0.7)
    with voxcarve.CarveEngine(0) as e:
        _start(e, (9, 11, 7), cams3, masks3)                     # no image uploaded
        e.upload_masks(_other_masks(11, 0.7))
        e.carve(min_views=1)
        _, occ_b = _hull(e)
        e.upload_hull(occ_b, 0)
        e.upload_masks(masks3)
        for cc in (None, 2):
            e.carve(min_views=1, color_cam=cc)
            st, want, wadded = _check_combine(e, "or", 0, occ_b, None, None if cc is None else fx.oracle_cams(cams3)[cc], None)
            fresh = want[wadded == 1]
            assert fresh.size > 0
            if cc is None:
                assert ((fresh >> np.uint64(32)) == 0).all()
            else:
                assert (((fresh >> np.uint64(32)) & np.uint64(0xffffff)) == 0).all()      # seen, colour 0


@pytest.mark.parametrize("grid,seed,mv", GRIDS[:2] + GRIDS[3:])
def test_edge_operands(seng, grid, seed, mv):
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    cam = fx.oracle_cams(cams3)[1]
    H, W = masks3[0].shape
    n = grid[0] * grid[1] * grid[2]
    _start(seng, grid, cams3, masks3, frames3)
    assert seng.carve(min_views=mv) > 0
    rec_a, occ_a = _hull(seng)
    seng.keep_hull(0)                                            # B = A
    seng.upload_hull(np.zeros(n, dtype=bool), 1)                 # B empty, by bits
    seng.upload_hull(np.empty(0, dtype=np.uint64), 2)            # B empty, with records
    seng.upload_hull(np.ones(n, dtype=bool), 3)                  # B the full grid, by bits
    operands = [(occ_a, rec_a), (np.zeros_like(occ_a), None), (np.zeros_like(occ_a), np.empty(0, np.uint64)), (np.ones_like(occ_a), None)]
    assert seng.fetch_kept(2)["has_records"] and seng.fetch_kept(2)["count"] == 0 and seng.fetch_kept(3)["count"] == n
    for op in sn.OPS:
        for reg, (occ_b, rec_b) in enumerate(operands):
            seng.carve(min_views=mv)
            st, want, _ = _check_combine(seng, op, reg, occ_b, rec_b, cam, frames3[1])
            if reg == 0:
                assert st["common"] == st["other"] == rec_a.size and st["added"] == 0
            if reg == 3 and op in ("copy", "or"):
                assert st["survivors_after"] == n
    # the reload path: A empty, then COPY from records gives B's records byte for byte
    seng.upload_hull(rec_a, 1)
    seng.upload_masks([np.zeros((H, W), np.uint8)] * 3)
    assert seng.carve(min_views=mv) == 0
    st, want, wadded = _check_combine(seng, "copy", 1, occ_a, rec_a, cam, frames3[1])
    assert np.array_equal(seng.fetch_records(), rec_a) and wadded.all() and st["added"] == rec_a.size
    assert np.array_equal(seng.fetch()[0], (rec_a & LOW).astype(np.uint32))
    seng.carve(min_views=mv)
    assert seng.set_hull(rec_a, 2)["survivors_after"] == rec_a.size and np.array_equal(seng.fetch_records(), rec_a)
    # ... and on an empty result every other op against an empty operand stays empty
    seng.carve(min_views=mv)
    seng.upload_hull(np.zeros(n, dtype=bool), 0)
    for op in sn.OPS:
        st, _, _ = _check_combine(seng, op, 0, np.zeros_like(occ_a), None, cam, frames3[1])
        assert st["survivors_after"] == 0


def test_upload_refusals_leave_the_register(seng):
    from voxcarve._lib import VoxcarveError
    cams3, masks3, frames3 = fx.random_scene(3, C=3, fg=0.7)
    grid = (5, 7, 3)
    n = 105
    _start(seng, grid, cams3, masks3, frames3)
    keep = np.array([1, 64, 104], dtype=np.uint64) | (np.uint64(0x01223344) << np.uint64(32))
    seng.upload_hull(keep, 1)
    before = seng.fetch_kept(1)
    up = seng._L.vc_hull_upload
    err = lambda: seng._L.vc_last_error(seng._ctx).decode()
    u8, u64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    bits = np.zeros(16, dtype=np.uint8)
    bits[13] = 1 << 1                                            # bit 105
    assert up(seng._ctx, 1, bits.ctypes.data_as(u8), None, 0) == -1 and "beyond" in err()
    bits[:] = 0
    bits[15] = 0x80                                              # the last bit of the last word
    assert up(seng._ctx, 1, bits.ctypes.data_as(u8), None, 0) == -1 and "beyond" in err()
    for bad in ([5, 3, 9], [3, 3], [3, 3 | (1 << 40)], [3, 105], [3, 200], [1 << 31]):
        rec = np.array(bad, dtype=np.uint64)
        assert up(seng._ctx, 1, None, rec.ctypes.data_as(u64), rec.size) == -1 and "out of order" in err(), bad
    rec = np.array([1, 2], dtype=np.uint64)
    assert up(seng._ctx, 1, None, None, 0) == -1 and "exactly one" in err()
    assert up(seng._ctx, 1, bits.ctypes.data_as(u8), rec.ctypes.data_as(u64), 2) == -1 and "exactly one" in err()
    assert up(seng._ctx, 4, None, rec.ctypes.data_as(u64), 2) == -1 and "register 4" in err()
    after = seng.fetch_kept(1)
    assert after["count"] == before["count"] == 3 and after["has_records"] and np.array_equal(after["records"], keep)
    assert np.array_equal(after["words"], before["words"])
    for bad in (np.zeros(n + 1, dtype=bool), np.array([5, 3], dtype=np.uint32), np.array([3, n], dtype=np.uint64), np.array([1.5])):
        with pytest.raises(ValueError):
            seng.upload_hull(bad, 1)
    assert np.array_equal(seng.fetch_kept(1)["records"], keep)
    # the largest valid hulls are taken
    bits[:] = 0xff
    bits[13] = 1
    bits[14:] = 0
    assert up(seng._ctx, 2, bits.ctypes.data_as(u8), None, 0) == 0 and seng.fetch_kept(2)["count"] == n
    seng.upload_hull(np.arange(n, dtype=np.uint64), 3)
    assert seng.fetch_kept(3)["count"] == n and seng.fetch_kept(3)["words"].tobytes() == _want_words(np.ones(n, dtype=bool))
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*holds no records"):
        seng._check(seng._L.vc_fetch_kept(seng._ctx, 2, None, rec.ctypes.data_as(u64), None, None), "vc_fetch_kept")


def test_register_lifetime(seng):
    from voxcarve._lib import VoxcarveError
    cams3, masks3, frames3 = fx.random_scene(6, C=3, fg=0.7)
    grid = (9, 11, 7)
    H, W = masks3[0].shape
    _start(seng, grid, cams3, masks3, frames3)
    seng.carve(min_views=1)
    rec_a, occ_a = _hull(seng)
    seng.keep_hull(2)
    seng.upload_hull(occ_a, 0)
    seng.upload_masks(_other_masks(6, 0.7))
    seng.carve(min_views=1)                                      # registers survive a carve ...
    seng.close_hull(300)                                         # ... and a pass
    k = seng.fetch_kept(2)
    assert np.array_equal(k["records"], rec_a) and k["words"].tobytes() == _want_words(occ_a)
    assert seng.fetch_kept(0)["count"] == rec_a.size
    seng.release_hull(2)
    seng.release_hull(2)                                         # (an empty register is no error)
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*register 2 is empty"):
        seng.fetch_kept(2)
    assert seng.fetch_kept(0)["count"] == rec_a.size
    for change in (lambda: seng.set_cameras(cams3, H, W), lambda: seng.set_grid(*grid)):
        seng.upload_hull(occ_a, 0)
        seng.upload_hull(rec_a, 3)
        change()
        for reg in range(4):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*is empty"):
                seng.fetch_kept(reg)
    seng.upload_hull(rec_a, 3)                                   # a grid is enough: no masks, no carve
    assert seng.fetch_kept(3)["count"] == rec_a.size


def _check_compare(e, occ_b, distance):
    rec, occ = _hull(e)
    want = sn.compare(occ, occ_b, dn.steps_um(e.grid, e.bounds) if distance else None)
    st = e.compare_hull(0, distance=distance)
    assert st.pop("compare_ms") > 0
    derived = {k: st.pop(k) for k in ("iou", "dice", "hausdorff_mm")}
    assert st == want, (st, want)
    assert derived == sn.derived(want)
    assert np.array_equal(e.fetch_records(), rec)
    return st


@pytest.mark.parametrize("grid,seed,mv", GRIDS)
def test_compare_equals_restatement(seng, grid, seed, mv):
    from voxcarve._lib import VoxcarveError
    cams3, masks3, frames3 = fx.random_scene(seed, C=3, fg=0.7)
    H, W = masks3[0].shape
    n = grid[0] * grid[1] * grid[2]
    _start(seng, grid, cams3, masks3, frames3)
    seng.upload_masks(_other_masks(seed, 0.7))
    seng.carve(min_views=mv)
    _, occ_b = _hull(seng)
    seng.upload_masks(masks3)
    seng.carve(min_views=mv)
    _, occ_a = _hull(seng)
    metric = grid != (5, 7, 3)                                   # (its z step is 1.28 m: outside the metric of vc_hull_distance)
    lone = np.zeros(n, dtype=bool)
    lone[n - 1] = True
    for occ in (occ_b, occ_a, np.zeros_like(occ_a), np.ones_like(occ_a), lone.reshape(occ_a.shape)):
        seng.upload_hull(occ, 0)
        _check_compare(seng, occ, False)
        if metric:
            _check_compare(seng, occ, True)
        else:
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*the step of axis z"):
                seng.compare_hull(0, distance=True)
    seng.upload_masks([np.zeros((H, W), np.uint8)] * 3)          # A empty
    assert seng.carve(min_views=mv) == 0
    for occ in (occ_b, np.zeros_like(occ_a)):
        seng.upload_hull(occ, 0)
        st = _check_compare(seng, occ, metric)
        if metric and occ.any():
            assert st["h2_ba"] == sn.U64_MAX and st["h2_ab"] == 0


def test_compare_real_cameras_64_pinned(seng, cams, masks, frames):
    """A = the golden masks' hull, B = the hull of tn.noisy_masks(masks, 1); the figures were computed with the C oracle."""
    n = 64
    _start(seng, (n, n, n), cams, masks, frames)
    seng.upload_masks(tn.noisy_masks(masks, 1))
    assert seng.carve() == 6593
    _, occ_b = _hull(seng)
    seng.keep_hull(0)
    seng.upload_masks(masks)
    assert seng.carve() == 6981
    seng.filter_components(min_voxels=1)
    seng.hull_distance(outside=True)
    seng.measure_hull("all")
    rec, d, dout = seng.fetch_records().copy(), seng.fetch_record_distance().copy(), seng.fetch_distance_raw("outside").copy()
    lab, ms = seng.fetch_component_labels().copy(), seng.fetch_measure()
    st = _check_compare(seng, occ_b, True)
    assert (st["a"], st["b"], st["common"], st["only_a"], st["only_b"]) == (6981, 6593, 6443, 538, 150)
    assert st["h2_ab"] == 1651203225 and st["h2_ba"] == 510023652138
    assert (st["diff_lo"], st["diff_hi"]) == ((17, 2, 16), (54, 50, 53)) and (st["arg_ab"], st["arg_ba"]) == (141737, 140738)
    full = seng.compare_hull(0, distance=True)
    assert abs(full["hausdorff_mm"] - 714.2) < 0.05 and abs(np.sqrt(full["h2_ab"]) / 1000 - 40.6) < 0.05
    assert abs(full["iou"] - 6443 / 7131) < 1e-12 and abs(full["dice"] - 2 * 6443 / 13574) < 1e-12
    # nothing changed: the records' bytes, the stored distance fields, the labels and the measurements are still fetchable
    assert np.array_equal(seng.fetch_records(), rec) and np.array_equal(seng.fetch_record_distance(), d)
    assert np.array_equal(seng.fetch_distance_raw("outside"), dout) and np.array_equal(seng.fetch_component_labels(), lab)
    ms2 = seng.fetch_measure()
    assert all(np.array_equal(ms[k], ms2[k]) for k in ms)


def test_invalidation(seng, cams, masks, frames):
    from voxcarve._lib import VoxcarveError
    n = 64
    _start(seng, (n, n, n), cams, masks, frames)
    seng.upload_masks(tn.noisy_masks(masks, 1))
    seng.carve()
    rec_b, occ_b = _hull(seng)
    seng.upload_hull(occ_b, 1)
    seng.upload_masks(masks)
    seng.carve()
    seng.keep_hull(0)
    seng.filter_components(min_voxels=1)
    seng.measure_hull("all")
    seng.temporal_reset()
    seng.temporal_filter(3)                                      # (the first hull of a ring comes back as it is)
    rec, lab, ms = seng.fetch_records().copy(), seng.fetch_component_labels().copy(), seng.fetch_measure()
    # R = A: "and" and "or" with A itself, "andnot" and "or" with the empty hull
    seng.upload_hull(np.zeros(n ** 3, dtype=bool), 2)
    for op, reg in (("and", 0), ("or", 0), ("andnot", 2), ("or", 2), ("xor", 2)):
        st = seng.combine_hull(op, reg)
        assert st["added"] == st["removed"] == 0 and st["survivors_after"] == rec.size
        assert not seng.fetch_combined().any()
        assert np.array_equal(seng.fetch_records(), rec) and np.array_equal(seng.fetch_component_labels(), lab)
        assert all(np.array_equal(ms[k], seng.fetch_measure()[k]) for k in ms)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*one push per result"):
            seng.temporal_filter(3)
    # a combine that changes the hull: every product of a pass is stale, and the vote may run again
    st = seng.combine_hull("andnot", 1)
    assert st["removed"] == 6443 and st["survivors_after"] == 538
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no component labels"):
        seng.fetch_component_labels()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG"):
        seng.fetch_measure()
    assert seng.temporal_filter(3)["frames"] == 2
    # a restore always counts as another result
    seng.carve()
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no added flags"):
        seng.fetch_combined()
    seng.filter_components(min_voxels=1)
    assert seng.combine_hull("copy", 0)["added"] == 0
    with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no component labels"):
        seng.fetch_component_labels()
    assert np.array_equal(seng.fetch_records(), rec)


def test_downstream_passes_read_the_combined_hull(seng, cams, masks, frames):
    from test_gpu_closing import _check_grow
    from test_gpu_measure import _check as check_measure
    from test_gpu_shell import _check as check_shell
    n = 64
    _start(seng, (n, n, n), cams, masks, frames)
    cam = fx.oracle_cams(cams)[1]
    seng.upload_masks(tn.noisy_masks(masks, 1))
    seng.carve()
    rec_b, occ_b = _hull(seng)
    seng.keep_hull(0)
    seng.upload_hull(occ_b, 1)
    seng.upload_masks(masks)
    for op, reg in (("or", 1), ("xor", 0)):
        seng.carve()
        st, want, _ = _check_combine(seng, op, reg, occ_b, rec_b if reg == 0 else None, cam, frames[1])
        idx, rgb, seen = seng.fetch()
        assert np.array_equal(idx, (want & LOW).astype(np.uint32)) and np.array_equal(np.flatnonzero(seng.fetch_occupancy()), idx)
        check_shell(seng, 0)
        check_measure(seng, "all")
        grown, _, _ = _check_grow(seng, "close", cams, frames, mm=40)
        assert grown["survivors_before"] == st["survivors_after"]
        check_measure(seng, "all")


def test_real_128_andnot_invariants(seng, cams, masks, frames):
    n = 128
    _start(seng, (n, n, n), cams, masks, frames)
    seng.upload_masks([np.roll(m, 6, axis=1) for m in masks])
    seng.carve()
    b = _words(seng)
    seng.keep_hull(1)
    seng.upload_masks(masks)
    assert seng.carve() == 57048
    rec, a = seng.fetch_records().copy(), _words(seng)
    st = seng.combine_hull("andnot", 1)
    out, got = _words(seng), seng.fetch_records()
    pop = lambda w: int(np.bitwise_count(w).sum())
    assert np.array_equal(out, a & ~b)
    assert st["survivors_before"] == 57048 == pop(a) and st["other"] == pop(b) and st["common"] == pop(a & b) > 0
    assert st["survivors_after"] == pop(out) == got.size == seng.count == st["survivors_before"] - st["removed"]
    assert st["added"] == 0 and 0 < st["removed"] == st["common"] < 57048 and not seng.fetch_combined().any()
    idx = (got & LOW).astype(np.int64)
    assert (np.diff(idx) > 0).all()
    kept = rec[((out[(rec & LOW).astype(np.int64) >> 6] >> ((rec & LOW) & np.uint64(63))) & np.uint64(1)).astype(bool)]
    assert np.array_equal(got, kept)                             # kept bytes equal
    cmp_ = seng.compare_hull(1)
    assert cmp_["common"] == 0 and cmp_["only_a"] == got.size and cmp_["only_b"] == pop(b)


def test_refusals(built, cams, masks, frames):
    """Every refusal of vc_hull_combine and vc_hull_compare but two: a communicator of more than one rank needs two processes with
    a device each, and a grid beyond the u32 index does not fit the suite."""
    import voxcarve
    from voxcarve import _lib
    from voxcarve._lib import VoxcarveError
    with voxcarve.CarveEngine(0) as e:
        with pytest.raises(VoxcarveError, match="no grid"):
            e.upload_hull(np.zeros(8, dtype=bool), 0)
        bits = np.zeros(8, dtype=np.uint8)
        assert e._L.vc_hull_upload(e._ctx, 0, bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None, 0) == -1
        assert "no grid" in e._L.vc_last_error(e._ctx).decode()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
            e.keep_hull(0)
        _start(e, (64, 64, 64), cams, masks, frames)
        e.upload_hull(np.zeros(64 ** 3, dtype=bool), 1)
        for call in (lambda: e.combine_hull("or", 1), lambda: e.compare_hull(1)):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no carve result"):
                call()
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*no added flags"):
            e.fetch_combined()
        S = e.carve()
        hull = e.fetch_records().copy()
        e.keep_hull(0)
        e.upload_hull(np.ones(64 ** 3, dtype=bool), 1)
        st, cs = _lib.VcSetopStats(), _lib.VcCompareStats()
        comb, comp = e._L.vc_hull_combine, e._L.vc_hull_compare
        err = lambda: e._L.vc_last_error(e._ctx).decode()
        assert comb(e._ctx, 5, 0, 0, ctypes.byref(st)) == -1 and "unknown op" in err()
        assert comb(e._ctx, 2, 0, 1, ctypes.byref(st)) == -1 and "flags" in err()
        assert comb(e._ctx, 2, 0, 0, None) == -1 and "stats" in err()
        assert comb(e._ctx, 2, 4, 0, ctypes.byref(st)) == -1 and "register 4" in err()
        assert comb(e._ctx, 2, 3, 0, ctypes.byref(st)) == -1 and "register 3 is empty" in err()
        assert comp(e._ctx, 0, 2, ctypes.byref(cs)) == -1 and "unknown flags" in err()
        assert comp(e._ctx, 0, 0, None) == -1 and "stats" in err()
        assert comp(e._ctx, 4, 0, ctypes.byref(cs)) == -1 and "register 4" in err()
        assert comp(e._ctx, 3, 0, ctypes.byref(cs)) == -1 and "register 3 is empty" in err()
        assert e._L.vc_hull_keep(e._ctx, 4) == -1 and e._L.vc_hull_release(e._ctx, 4) == -1 and e._L.vc_fetch_combined(e._ctx, None) == -1
        with pytest.raises(ValueError):
            e.combine_hull("nor", 0)
        assert e.count == S and np.array_equal(e.fetch_records(), hull)
        # a slot prepared again since the carve: refused only when fresh records would be coloured
        e.touch_masks(0)
        e.fetch_mask(0)
        for op in ("copy", "or", "xor"):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*prepared again"):
                e.combine_hull(op, 1)
        assert e.combine_hull("or", 0)["added"] == 0 and e.combine_hull("and", 1)["removed"] == 0
        assert e.combine_hull("andnot", 1)["survivors_after"] == 0 and e.combine_hull("or", 0)["added"] == S      # B's records: no colouring
        assert np.array_equal(e.fetch_records(), hull)
        e.compare_hull(1)
        e.carve(records=False)
        for call in (lambda: e.combine_hull("and", 0), lambda: e.compare_hull(0), lambda: e.keep_hull(2)):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*VC_FLAG_NO_RECORDS"):
                call()
        e.set_slab(0, 32)
        with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*narrower than the grid"):
            e.upload_hull(np.zeros(64 * 64 * 32, dtype=bool), 0)
        e.set_slab(0, 64)
        e.upload_hull(hull, 0)
        e.carve_begin()
        for call in (lambda: e.combine_hull("and", 0), lambda: e.compare_hull(0), lambda: e.keep_hull(2), lambda: e.upload_hull(hull, 2)):
            with pytest.raises(VoxcarveError, match="VC_ERR_ARG.*in flight"):
                call()
        e.carve_end()
        assert e.combine_hull("and", 0)["survivors_after"] == S


def test_save_and_load(seng, cams, masks, frames, tmp_path):
    n = 64
    _start(seng, (n, n, n), cams, masks, frames)
    seng.carve()
    rec = seng.fetch_records().copy()
    path = os.path.join(str(tmp_path), "hull.npz")
    seng.save_hull(path)
    seng.upload_masks(tn.noisy_masks(masks, 1))
    seng.carve()
    seng.load_hull(path, 2)
    assert np.array_equal(seng.fetch_kept(2)["records"], rec)
    assert seng.combine_hull("copy", 2)["survivors_after"] == rec.size and np.array_equal(seng.fetch_records(), rec)
    seng.set_grid(n, n, 32)
    with pytest.raises(ValueError, match="grid"):
        seng.load_hull(path, 2)
    seng.set_grid(n, n, n, bounds=(0, 1000, 0, 1000, 0, 1000))
    with pytest.raises(ValueError, match="bounds"):
        seng.load_hull(path, 2)


def test_configure_hull_subtract_and_clip(built, cams, masks, tmp_path):
    from voxcarve import assignment, hullio
    from voxcarve.engine import DEFAULT_BOUNDS
    frames = [np.dstack([m // 2 + 60, m // 3 + 40, 255 - m // 2]).astype(np.uint8) for m in masks]
    data = os.path.join(fx.GOLDEN, "data")
    sets = [(frames, tn.noisy_masks(masks, t)) for t in range(3)]
    n = 64
    scene = np.zeros((n, n, n), dtype=bool)                      # [iz, ix, iy]: a slab of "static scene"
    scene[:, :30, :] = True
    region = np.zeros((n, n, n), dtype=bool)
    region[:40] = True
    clip = os.path.join(str(tmp_path), "clip.npz")
    hullio.save(clip, (n, n, n), DEFAULT_BOUNDS, dn.indices(region).astype(np.uint64))
    try:
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=data, hull_subtract=scene, hull_clip=clip)
        with pytest.raises(RuntimeError):
            assignment.hull_ops()
        outs, stats = [], []
        for t in range(3):
            pos, _ = assignment.set_voxel_positions(n, n // 2, n)
            stats.append(assignment.hull_ops())
            outs.append(assignment._engine.fetch_records().copy())
            assert len(pos) == outs[-1].size == stats[-1]["clip"]["survivors_after"]
            assert stats[-1]["subtract"]["added"] == stats[-1]["clip"]["added"] == 0
            assert stats[-1]["clip"]["survivors_before"] == stats[-1]["subtract"]["survivors_after"]
        # equal to carve + the restatement by hand
        e = assignment._engine
        assert e.fetch_kept(3)["count"] == int(scene.sum()) and e.fetch_kept(2)["count"] == int(region.sum())
        for t in range(3):
            e.upload_masks(sets[t][1], slot=0)
            e.carve(slot=0, min_views=4, color_cam=assignment._settings["color_camera"])
            rec, occ = _hull(e)
            assert stats[t]["subtract"]["survivors_before"] == rec.size
            keep = (occ & ~scene & region).reshape(-1)[(rec & LOW).astype(np.int64)]
            assert np.array_equal(outs[t], rec[keep]) and 0 < outs[t].size < rec.size
        # the vote comes after the two operations
        assignment.configure(frame_source=assignment.StaticFrameSource(sets), data_path=data, hull_subtract=None, hull_clip=region,
                             temporal_window=3)
        for t in range(3):
            assignment.set_voxel_positions(n, n // 2, n)
            assert assignment.temporal()["survivors_before"] == assignment.hull_ops()["clip"]["survivors_after"]
            assert "subtract" not in assignment.hull_ops()
    finally:
        assignment.configure(frame_source=None, hull_subtract=None, hull_clip=None, temporal_window=0)
