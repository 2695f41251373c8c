"""Carve steps in flight that name different colour cameras (include/voxcarve.h, vc_carve_begin).

A VC_MODE_FUSED step colours its survivors from one whole-grid table, projected for one camera at a time.  A step begun with
another colour camera projects its table into the same buffer while the record expansion of the step before it may still be
reading the old one on the second stream: the projection has to wait for that expansion on the device.  Without the wait, 158 to
559 of the first step's 2797 records came back with colour and `seen` bytes of zero at this very shape.

Every sequence runs on chain_model's scene of 30 x 63 x 30 with the golden cameras, two frame sets on two slots, min_views = 4;
every collected step's records, all 8 bytes, are compared with oracle.carve_c as Scene.carve_records packs them.  All steps of a
sequence are collected before anything is asserted, so that a mismatch never leaves the engine with a step in flight."""
import numpy as np
import pytest

import chain_model as cm

pytestmark = pytest.mark.gpu

GRID = (30, 63, 30)
MIN_VIEWS = 4
REPEATS = 8
# (mode, colour camera) of the steps begun one after the other; step k reads frame set k & 1
SEQUENCES = ((("fused", 1), ("fused", 2)),
             (("fused", 2), ("fused", 1)),
             (("fused", 1), ("fused", 2), ("fused", 1)),
             (("fused", 1), ("lut", 2)))


def _setup(e, sc, cams, grid=None):
    e.set_grid(*(grid or sc.grid), bounds=sc.bounds)
    e.set_cameras(cams, sc.H, sc.W)
    for slot in (0, 1):
        e.upload_masks(sc.masks[slot], slot=slot)
        for c in cm.SLOT_IMAGES[slot]:
            e.upload_frame(c, sc.frames[slot][c], slot=slot)
    e.build_lut()


@pytest.fixture(scope="module")
def sc():
    return cm.scene(GRID)


@pytest.fixture(scope="module")
def eng(built, cams, sc):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    try:
        _setup(e, sc, cams)
        yield e
    finally:
        e.close()


def _collect(e, seq):
    """Begins every step of `seq`, then collects them all: [(count, records)] oldest first.  Whatever happens, no step stays in
    flight."""
    got, begun = [], 0
    try:
        for k, (mode, cam) in enumerate(seq):
            e.carve_begin(slot=k & 1, min_views=MIN_VIEWS, color_cam=cam, mode=mode)
            begun += 1
        while begun:
            begun -= 1
            n = e.carve_end()
            got.append((n, e.fetch_records()))
    finally:
        for _ in range(begun):
            e.carve_end()
    return got


def _check(sc, seq, got, what):
    assert len(got) == len(seq)
    for k, ((mode, cam), (n, rec)) in enumerate(zip(seq, got)):
        want = sc.carve_records(k & 1, MIN_VIEWS, cam)
        where = "%s, step %d of %r (%s, colour camera %d)" % (what, k, seq, mode, cam)
        assert n == want.size and rec.size == want.size, (where, n, want.size)
        assert np.array_equal(rec & cm.LOW, want & cm.LOW), where + ": indices and order"
        bad = np.flatnonzero(rec != want)
        assert bad.size == 0, "%s: %d of %d records differ, %d of them with colour and seen bytes of zero; first at %d: %#018x, want %#018x" % (
            where, bad.size, want.size, int(((rec[bad] >> np.uint64(32)) == 0).sum()), bad[0], int(rec[bad[0]]), int(want[bad[0]]))


def test_steps_in_flight_name_different_colour_cameras(eng, sc):
    for rep in range(REPEATS):
        for seq in SEQUENCES:
            _check(sc, seq, _collect(eng, seq), "repeat %d" % rep)


def test_steps_in_flight_without_the_colour_table(eng, sc):
    """The same sequences where every survivor is projected again (option fused_color_table = 0): no table, the same bytes."""
    eng.set_option("fused_color_table", 0)
    try:
        got = [_collect(eng, seq) for seq in SEQUENCES]
    finally:
        eng.set_option("fused_color_table", 1)
    for seq, g in zip(SEQUENCES, got):
        _check(sc, seq, g, "fused_color_table = 0")


@pytest.fixture()
def small_eng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    try:
        yield e
    finally:
        e.close()


def test_a_step_that_is_expanded_again_behind_another_camera(small_eng, sc, cams):
    """vc_carve_end expands a step once more when its record buffer was too small.  The three sets of result buffers are sized by
    the first grid they see, n / 16 + 1024 records: 1280 after three steps on 16^3, below the 2797 and 1439 records of the two
    frame sets on 30 x 63 x 30.  By then the table holds the second step's camera: the first step must not be coloured from it."""
    e = small_eng
    _setup(e, sc, cams, grid=(16, 16, 16))
    small = (("fused", 1), ("fused", 1), ("fused", 1))
    assert all(n <= 16 ** 3 // 16 + 1024 for n, _ in _collect(e, small))
    _setup(e, sc, cams)
    assert min(sc.carve_records(s, MIN_VIEWS, 1).size for s in (0, 1)) > 16 ** 3 // 16 + 1024
    for seq in SEQUENCES[:2]:
        _check(sc, seq, _collect(e, seq), "record buffers of 1280")
