"""The record expansion of mode=lut reads the colour camera's table in compact form (option emit_lut16, default 1: 16-bit
differences to the smallest offset of each tile word, k_pack_lut16) where the table fits, and as 4-byte entries otherwise.

Every expectation is the CPU oracle's (oracle.carve_np: survivors, pixel offsets, view masks; the records are put together from
those exactly as carve_np itself does, which one case checks); the two routes are asserted equal to it and so to each other.
Whether a camera's table fits is worked out here from the oracle's offsets per tile word (4 x-rows x 16 y of one layer) and compared
with the route the engine reports (debug_counters()["emit_lut16"])."""
import numpy as np
import pytest

import fixtures_util as fx

pytestmark = pytest.mark.gpu

# (grid, slab or None, emit_busy values): ny = 256 takes the brick pipeline, emit_busy = 2 the busy-list expansion on a small grid;
# the others tile words and the plain expansion.  COARSE: 4 x-rows 512 mm apart in one tile word -- camera 2's offsets span more
# than 16 bits there (found on the CPU; test_the_cases_hold_both_verdicts keeps that true).
COARSE = ((4, 64, 16), None, (1,))
CASES = [((16, 256, 20), None, (2, 1)), ((64, 64, 64), None, (1,)), ((8, 64, 12), None, (1,)), ((16, 256, 24), (5, 19), (2, 1)), COARSE]
IDS = ["16x256x20", "64x64x64", "8x64x12", "16x256x24-slab5-19", "4x64x16-coarse"]
SPAN_MAX = 65534                                 # 0xFFFF is "outside the image"


def _records(w, cam, frames):
    """u64 records of the oracle's survivors coloured by `cam`: idx | R << 32 | G << 40 | B << 48 | seen << 56 (0 colour unseen)."""
    idx = w["idx"].astype(np.int64) - w["i0"]
    seen = ((w["viewmask"][idx] >> cam) & 1).astype(bool)
    bgr = np.zeros((idx.size, 3), dtype=np.uint64)
    bgr[seen] = frames[cam].reshape(-1, 3)[w["offsets"][cam, idx[seen]]]
    return (w["idx"].astype(np.uint64) | (bgr[:, 2] << np.uint64(32)) | (bgr[:, 1] << np.uint64(40)) | (bgr[:, 0] << np.uint64(48)) |
            (seen.astype(np.uint64) << np.uint64(56)))


def _fits(off, grid, nzl):
    """Does every tile word of the y-major table `off` (one camera, nzl layers) span at most SPAN_MAX over its entries >= 0?"""
    nx, ny, _ = grid
    o = off.reshape(nzl, nx // 4, 4, ny // 16, 16).transpose(0, 1, 3, 2, 4).reshape(-1, 64).astype(np.int64)
    ok = o >= 0
    lo = np.where(ok, o, np.iinfo(np.int64).max).min(axis=1)
    hi = np.where(ok, o, -1).max(axis=1)
    return bool((np.where(ok.any(axis=1), hi - lo, 0) <= SPAN_MAX).all())


_ORACLE = {}


def _oracle(cams, masks, frames, grid, slab=None, min_views=None, perm=None):
    key = (grid, slab, min_views, perm)
    if key not in _ORACLE:
        from oracle import carve_np
        nx, ny, nz = grid
        p = perm or (0, 1, 2, 3)
        z0, z1 = slab or (0, nz)
        w = carve_np.carve(*grid, fx.oracle_cams([cams[k] for k in p]), [masks[k] for k in p], [frames[k] for k in p],
                           min_views=min_views, color_cam=1, index_range=(z0 * nx * ny, z1 * nx * ny))
        w["i0"] = z0 * nx * ny
        w["rec"] = [_records(w, c, [frames[k] for k in p]) for c in range(4)]
        w["fits"] = [_fits(w["offsets"][c], grid, z1 - z0) for c in range(4)]
        for a in ("idx", "offsets", "viewmask"):
            w[a].setflags(write=False)
        _ORACLE[key] = w
    return _ORACLE[key]


@pytest.fixture(scope="module")
def eng(built, cams, masks, frames):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _setup(e, cams, masks, frames, grid, slab=None, perm=(0, 1, 2, 3), slots=(0,)):
    e.set_option("emit_lut16", 1)
    e.set_option("emit_busy", 1)
    e.set_grid(*grid)
    if slab:
        e.set_slab(*slab)
    e.set_cameras([cams[k] for k in perm], *masks[0].shape)
    for s in slots:
        e.upload_masks([masks[k] for k in perm], slot=s)
        for c in range(4):
            e.upload_frame(c, frames[perm[c]], slot=s)
    e.build_lut()


def _carve(e, cam, opt, min_views=None):
    e.set_option("emit_lut16", opt)
    n = e.carve(mode="lut", color_cam=cam, min_views=min_views)
    rec = e.fetch_records()
    assert rec.size == n
    return rec, e.debug_counters()["emit_lut16"]


def test_the_cases_hold_both_verdicts(cams, masks, frames):
    """On the CPU: the required shapes fit for every camera, the coarse grid does not for at least one (and does for another), so
    test_both_routes meets both verdicts; the records put together here are carve_np's own."""
    from oracle import carve_np
    for grid, slab, _ in CASES[:-1]:
        assert all(_oracle(cams, masks, frames, grid, slab)["fits"]), grid
    coarse = _oracle(cams, masks, frames, COARSE[0])
    assert not all(coarse["fits"]) and any(coarse["fits"]), coarse["fits"]
    assert coarse["idx"].size > 0
    w = _oracle(cams, masks, frames, (8, 64, 12), None, 3)
    for c in (1, 2):
        o = carve_np.carve(8, 64, 12, fx.oracle_cams(cams), masks, frames, min_views=3, color_cam=c)
        bgr = o["bgr"].astype(np.uint64)
        want = (o["idx"].astype(np.uint64) | (bgr[:, 2] << np.uint64(32)) | (bgr[:, 1] << np.uint64(40)) | (bgr[:, 0] << np.uint64(48)) |
                (o["color_seen"].astype(np.uint64) << np.uint64(56)))
        assert not o["color_seen"].all() and np.array_equal(w["rec"][c], want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_both_routes(eng, cams, masks, frames, case):
    """Every colour camera, emit_lut16 1 and 0: the oracle's records byte for byte, and the route the oracle's offsets call for."""
    grid, slab, busy = case
    w = _oracle(cams, masks, frames, grid, slab)
    assert w["idx"].size > 0
    _setup(eng, cams, masks, frames, grid, slab)
    for b in busy:
        eng.set_option("emit_busy", b)
        for cam in range(4):
            for opt in (1, 0, 1):
                rec, route = _carve(eng, cam, opt)
                assert np.array_equal(rec, w["rec"][cam]), (grid, b, cam, opt)
                assert route == (1 if opt and w["fits"][cam] else 0), (grid, b, cam, opt, w["fits"])
    eng.set_option("emit_busy", 1)


def test_entries_outside_the_image(eng, cams, masks, frames):
    """The default bounds reach beyond the images of cameras 1 and 2 (entries -1: 0xFFFF in the compact table, left out of the
    tile words' bases).  With every camera required no survivor has such an entry, the compact route is taken; below that the
    one-thread-per-voxel carve and its y-major table are (4-byte entries, ALLSEEN = false): survivors outside the colour
    camera's image are records with seen = 0."""
    grid = (64, 64, 64)
    full = _oracle(cams, masks, frames, grid)
    assert (full["offsets"][2] < 0).sum() > 1000 and (full["offsets"][1] < 0).sum() > 1000 and all(full["fits"])
    _setup(eng, cams, masks, frames, grid)
    for cam in (1, 2):
        rec, route = _carve(eng, cam, 1)
        assert route == 1 and np.array_equal(rec, full["rec"][cam]), cam
    for mv in (3, 1):
        w = _oracle(cams, masks, frames, grid, None, mv)
        outside = w["offsets"][2][w["idx"]] < 0
        assert mv == 3 or outside.sum() > 1000
        assert ((w["rec"][2] >> np.uint64(56)) == 0).sum() >= max(1000, int(outside.sum()))
        for opt in (1, 0):
            rec, _ = _carve(eng, 2, opt, min_views=mv)
            assert np.array_equal(rec, w["rec"][2]), (mv, opt)
            assert (rec[outside] >> np.uint64(32) == 0).all()


def test_a_foreign_table_that_does_not_fit(eng, cams, masks, frames):
    """vc_upload_lut with camera 1's entries of every fourth x-row moved 150 000 pixels on: tile words far wider than 16 bits.  The
    4-byte route is taken; the records are those of emit_lut16 = 0 and of the table itself (numpy)."""
    grid = (64, 64, 64)
    nx, ny, nz = grid
    H, W = masks[0].shape
    lut = _oracle(cams, masks, frames, grid)["offsets"].copy()
    ix = (np.arange(nx * ny * nz) // ny) % nx
    move = (ix % 4 == 3) & (lut[1] >= 0)
    lut[1, move] = (lut[1, move] + 150000) % (H * W)
    assert not _fits(lut[1], grid, nz) and _fits(lut[0], grid, nz)
    keep = np.ones(nx * ny * nz, dtype=bool)
    for c in range(4):
        keep &= (lut[c] >= 0) & (masks[c].reshape(-1)[np.maximum(lut[c], 0)] > 0)
    idx = np.nonzero(keep)[0]
    assert idx.size > 500
    want = {}
    for cam in (0, 1):
        bgr = frames[cam].reshape(-1, 3)[lut[cam, idx]].astype(np.uint64)
        want[cam] = (idx.astype(np.uint64) | (bgr[:, 2] << np.uint64(32)) | (bgr[:, 1] << np.uint64(40)) | (bgr[:, 0] << np.uint64(48)) |
                     (np.uint64(1) << np.uint64(56)))
    _setup(eng, cams, masks, frames, grid)
    eng.upload_lut(lut)
    rec1, route1 = _carve(eng, 1, 1)
    rec0, route0 = _carve(eng, 1, 0)
    assert route1 == 0 and route0 == 0
    assert np.array_equal(rec1, rec0) and np.array_equal(rec1, want[1])
    rec, route = _carve(eng, 0, 1)                               # (camera 0 of the same foreign table fits)
    assert route == 1 and np.array_equal(rec, want[0])
    rec, route = _carve(eng, 1, 1)                               # (and the verdict on camera 1 stands)
    assert route == 0 and np.array_equal(rec, want[1])


def test_new_cameras_void_the_compact_table(eng, cams, masks, frames):
    grid = (16, 256, 20)
    perm = (2, 3, 0, 1)
    a, b = _oracle(cams, masks, frames, grid), _oracle(cams, masks, frames, grid, perm=perm)
    assert np.array_equal(a["idx"], b["idx"]) and not np.array_equal(a["rec"][1], b["rec"][1])
    _setup(eng, cams, masks, frames, grid)
    rec, route = _carve(eng, 1, 1)
    assert route == 1 and np.array_equal(rec, a["rec"][1])
    _setup(eng, cams, masks, frames, grid, perm=perm)
    rec, route = _carve(eng, 1, 1)
    assert route == 1 and np.array_equal(rec, b["rec"][1])


def test_a_new_slab_voids_the_compact_table(eng, cams, masks, frames):
    grid = (16, 256, 24)
    a, b = _oracle(cams, masks, frames, grid, (5, 19)), _oracle(cams, masks, frames, grid, (2, 12))
    _setup(eng, cams, masks, frames, grid, (5, 19))
    rec, route = _carve(eng, 1, 1)
    assert route == 1 and np.array_equal(rec, a["rec"][1])
    eng.set_slab(2, 12)
    eng.build_lut()
    rec, route = _carve(eng, 1, 1)
    assert route == 1 and np.array_equal(rec, b["rec"][1]) and not np.array_equal(a["rec"][1], b["rec"][1])


def test_the_colour_camera_changes_between_two_steps_in_flight(eng, cams, masks, frames):
    grid = (16, 256, 20)
    w = _oracle(cams, masks, frames, grid)
    _setup(eng, cams, masks, frames, grid, slots=(0, 1))
    for busy in (2, 1):
        eng.set_option("emit_busy", busy)
        for first, second in ((1, 2), (2, 1), (3, 3)):
            eng.carve_begin(slot=0, color_cam=first, mode="lut")
            eng.carve_begin(slot=1, color_cam=second, mode="lut")
            assert eng.carve_end() == w["idx"].size
            assert np.array_equal(eng.fetch_records(), w["rec"][first]), (busy, first, second)
            assert eng.carve_end() == w["idx"].size
            assert np.array_equal(eng.fetch_records(), w["rec"][second]), (busy, first, second)
            assert eng.debug_counters()["emit_lut16"] == 1
    eng.set_option("emit_busy", 1)
