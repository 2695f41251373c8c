"""The restatement of vc_hull_grow (tests/closing_np.py) against the definition, on the CPU: the separable forms against the
literal ones on seeded small grids (hulls touching the grid's faces, radii from 0 to beyond the grid), the box-restricted forms
against the whole-grid ones, the algebra of the contract's item 2 (hull <= C <= Dl, idempotent, increasing, r2 = 0 the identity,
dilation and erosion adjoint on the subsets of the grid), the two tables of DESIGN section 8 item 13 on the committed cameras
and masks, the records of added voxels, and the public names (header, binding, configure key, demo option)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import closing_np as cl
import components_np as cn
import distance_np as dn
import fixtures_util as fx
from oracle import carve_np

LOW = np.uint64(0xffffffff)


def _scene(rng, k):
    """A small random hull: every third one is confined to a sub-box, every third one touches faces, radii 0 .. beyond the grid."""
    shape = tuple(int(v) for v in rng.integers(2, 7, 3))
    q = tuple(int(v) for v in rng.integers(1, 40001, 3))
    occ = np.zeros(shape, dtype=bool)
    if k % 3 == 0:
        lo = [int(rng.integers(0, s)) for s in shape]
        hi = [int(rng.integers(l + 1, s + 1)) for l, s in zip(lo, shape)]
        sub = tuple(slice(l, h) for l, h in zip(lo, hi))
        occ[sub] = rng.random(tuple(h - l for l, h in zip(lo, hi))) < 0.6
    elif k % 3 == 1:
        occ[:] = rng.random(shape) < 0.25
        occ[0, 0, 0] = occ[-1, -1, -1] = True                   # the hull's box is the grid
    else:
        occ[:] = rng.random(shape) < (0.05, 0.5, 0.95)[(k // 3) % 3]
    span = max(qa * (s - 1) for qa, s in zip((q[2], q[0], q[1]), shape))
    radii = [0, min(q) ** 2, int(rng.integers(1, 4)) * max(q) ** 2, int(rng.integers(0, span + 1)) ** 2, 3 * (span + 1) ** 2 + 1]
    return occ, q, radii


def test_separable_equals_literal():
    rng = np.random.default_rng(13)
    n_sets = 0
    for k in range(48):
        occ, q, radii = _scene(rng, k)
        for r2 in radii:
            dl = cl.dilate_literal(occ, q, r2)
            c = cl.close_literal(occ, q, r2)
            got_c, got_dl = cl.close_(occ, q, r2)
            assert np.array_equal(cl.dilate(occ, q, r2), dl) and np.array_equal(got_dl, dl), (k, occ.shape, q, r2)
            assert np.array_equal(got_c, c), (k, occ.shape, q, r2)
            n_sets += 1
    assert n_sets == 240
    # no hull: nothing to dilate; a radius beyond the grid: everything, and its closing is the whole grid
    empty = np.zeros((3, 4, 5), dtype=bool)
    assert not cl.dilate(empty, (10, 20, 30), 10 ** 12).any() and not cl.close_(empty, (10, 20, 30), 10 ** 12)[0].any()
    one = empty.copy()
    one[1, 2, 3] = True
    assert cl.close_(one, (10, 20, 30), 10 ** 12)[0].all() and cl.close_literal(one, (10, 20, 30), 10 ** 12).all()
    assert cl.close_(one, (10, 20, 30), 2 ** 64 - 1)[0].all()


def test_box_restricted_forms_equal_the_full_grid():
    """The argument of DESIGN item 13: Dl lies inside the g-grown box, and the extra layer -- wherever a grid face does not cut it
    off -- is outside Dl, so clamping a far site of the second transform coordinate-wise into the box lands on a cell that is
    outside Dl too and no farther in any coordinate.  Without that layer the restricted closing is wrong (the last assertion
    finds such a case among the same scenes)."""
    rng = np.random.default_rng(14)
    layer_matters = False
    for k in range(60):
        shape = tuple(int(v) for v in rng.integers(4, 22, 3))
        q = tuple(int(v) for v in rng.integers(1, 50001, 3))
        occ = np.zeros(shape, dtype=bool)
        lo = [int(rng.integers(0, s - 1)) for s in shape]
        hi = [int(rng.integers(l + 1, s + 1)) for l, s in zip(lo, shape)]
        sub = tuple(slice(l, h) for l, h in zip(lo, hi))
        occ[sub] = rng.random(tuple(h - l for l, h in zip(lo, hi))) < (0.3, 0.7, 1.0)[k % 3]
        for r2 in (0, min(q) ** 2, max(q) ** 2, (2 * max(q)) ** 2 + 1, int(rng.integers(0, 6 * max(q))) ** 2, (25 * max(q)) ** 2):
            c, dl = cl.close_(occ, q, r2)
            cb, dlb, cells = cl.close_box(occ, q, r2)
            assert np.array_equal(dlb, dl) and np.array_equal(cl.dilate_box(occ, q, r2), dl), (shape, sub, q, r2)
            assert np.array_equal(cb, c), (shape, sub, q, r2)
            assert cells == cl.box_cells(occ, q, r2) <= occ.size
            sl = cl.grown_box(occ, q, r2)
            if sl is not None:
                for a in range(3):                               # the extra layer is outside Dl wherever it exists
                    g = (cl.reach(q, r2)[2], cl.reach(q, r2)[0], cl.reach(q, r2)[1])[a]
                    on = np.flatnonzero(occ.any(axis=tuple(b for b in range(3) if b != a)))
                    if int(on[0]) - g - 1 >= 0:
                        assert not np.take(dl, int(on[0]) - g - 1, axis=a).any()
                    if int(on[-1]) + g + 1 < shape[a]:
                        assert not np.take(dl, int(on[-1]) + g + 1, axis=a).any()
                tight = cl.grown_box(occ, q, r2, extra=0)
                dt = dn.field(occ[tight], q) <= np.uint64(r2)
                ct = np.zeros(shape, dtype=bool)
                ct[tight] = dt & cl._above(dn.field(~dt, q), r2)
                layer_matters |= not np.array_equal(ct, c)
    assert layer_matters
    # a radius that makes the box the grid
    occ = np.zeros((6, 7, 8), dtype=bool)
    occ[2:4, 3, 4] = True
    assert cl.box_cells(occ, (1000, 1000, 1000), 9000 ** 2) == occ.size and cl.box_cells(occ, (1000, 1000, 1000), 0) == 4 * 3 * 3


def _algebra(occ, q, r2):
    c, dl = cl.close_(occ, q, r2)
    assert (c >= occ).all() and (dl >= c).all()                 # hull <= C <= Dl
    c2, _ = cl.close_(c, q, r2)
    assert np.array_equal(c2, c)                                 # idempotent
    return c, dl


def test_algebra_of_the_contract_small_grids():
    rng = np.random.default_rng(15)
    for k in range(48):
        occ, q, radii = _scene(rng, k)
        bigger = occ | (rng.random(occ.shape) < 0.2)
        for r2 in radii:
            c, dl = _algebra(occ, q, r2)
            cb, dlb = cl.close_(bigger, q, r2)
            assert (cb >= c).all() and (dlb >= dl).all()         # increasing
            if r2 == 0:
                assert np.array_equal(c, occ) and np.array_equal(dl, occ)
            # the adjunction on the subsets of the grid: Dl(A) <= B  <=>  A <= E(B), E the erosion with nothing outside the grid
            b = rng.random(occ.shape) < 0.7
            e = cl.erode_grid_literal(b, q, r2)
            assert bool((dl <= b).all()) == bool((occ <= e).all())
            assert np.array_equal(c, cl.erode_grid_literal(dl, q, r2))           # C = E(Dl)


INTACT = {64: (6981, 4, {15: (0, 4), 25: (141, 3), 40: (160, 2)}),
          128: (57048, 2, {15: (341, 2), 25: (1168, 1), 40: (3460, 1)})}


def _components(occ):
    return int(cn.components(dn.indices(occ), occ.shape[1:] + occ.shape[:1], 26, 0, 0)["label"].size)


@pytest.mark.parametrize("n", [64, 128])
def test_intact_hull_table(n):
    """Table 1 of DESIGN item 13: voxels a closing adds to the committed hull and the 26-components left, and the algebra on it."""
    idx, _, _ = fx.expected(n)
    grid = (n, n, n)
    q = dn.steps_um(grid, carve_np.DEFAULT_BOUNDS)
    occ = dn.volume(idx, grid)
    size, comps, rows = INTACT[n]
    assert idx.size == size and _components(occ) == comps
    for mm, (added, left) in rows.items():
        r2 = dn.radius_r2(mm)
        c, dl, _ = cl.close_box(occ, q, r2)
        assert int(c.sum()) - size == added and _components(c) == left, (n, mm)
        assert (c >= occ).all() and (dl >= c).all()
        assert np.array_equal(cl.close_box(c, q, r2)[0], c)
        if added == 0:
            assert all(g == 0 for g in cl.reach(q, r2))          # the identity: the radius is below every step
    if n == 64:
        c, dl = cl.close_(occ, q, dn.radius_r2(25))              # the whole-grid form on a real hull
        cb, dlb, _ = cl.close_box(occ, q, dn.radius_r2(25))
        assert np.array_equal(c, cb) and np.array_equal(dl, dlb)
        _algebra(occ, q, dn.radius_r2(40))
    assert np.array_equal(cl.close_box(occ, q, 0)[0], occ) and np.array_equal(cl.dilate_box(occ, q, 0), occ)


def punched_masks(masks, cam, radius):
    """The masks with a disc of background of `radius` pixels at the centroid of camera cam's foreground, and whether the disc
    was all foreground before."""
    out = [m.copy() for m in masks]
    ys, xs = np.nonzero(out[cam])
    cy, cx = int(ys.mean()), int(xs.mean())
    yy, xx = np.mgrid[:out[cam].shape[0], :out[cam].shape[1]]
    disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius
    was_fg = bool((out[cam][disc] > 0).all())
    out[cam][disc] = 0
    return out, was_fg


# camera, disc radius in px -> voxels the hole carves away, of which a closing by 15 / 25 / 40 mm returns
PUNCHED = {(0, 2): (181, (46, 171, 177)), (1, 2): (130, (75, 128, 130)), (0, 3): (392, (28, 185, 383)),
           (1, 3): (259, (25, 212, 258)), (1, 5): (705, (26, 95, 466))}


def test_punched_mask_table():
    """Table 2 of DESIGN item 13 at 128^3: a hole in ONE camera's mask carves a tunnel through the hull; the closing returns it
    when the ball is as wide as the tunnel.  Bounds of the issue: the 2-px discs are recovered to at least three quarters at
    25 mm, the 5-px disc to less than half (the ball is the size limit), and nothing is added outside close(intact hull)."""
    n = 128
    grid = (n, n, n)
    cams, masks = fx.oracle_cams(fx.golden_cameras()), fx.golden_masks()
    q = dn.steps_um(grid, carve_np.DEFAULT_BOUNDS)
    idx, _, _ = fx.expected(n)
    occ = dn.volume(idx, grid)
    closed = {mm: cl.close_box(occ, q, dn.radius_r2(mm))[0] for mm in (15, 25, 40)}
    for (cam, radius), (lost_want, back_want) in PUNCHED.items():
        pm, was_fg = punched_masks(masks, cam, radius)
        assert was_fg
        hull = dn.volume(carve_np.carve(n, n, n, cams, pm)["idx"], grid)
        lost = occ & ~hull
        assert not (hull & ~occ).any() and int(lost.sum()) == lost_want
        for mm, want in zip((15, 25, 40), back_want):
            c = cl.close_box(hull, q, dn.radius_r2(mm))[0]
            back = int((c & lost).sum())
            print("camera %d, %d px, %d mm: %d of %d lost voxels returned" % (cam, radius, mm, back, lost_want))
            assert back == want
            assert not (c & ~closed[mm]).any()                   # nothing outside close(intact hull)
            if mm == 25 and radius == 2:
                assert 4 * back >= 3 * lost_want
            if mm == 25 and radius == 5:
                assert 2 * back < lost_want


def test_records_of_added_voxels():
    """records_after: old records byte for byte, new ones coloured by the pixel under the centre (BGR frame -> r, g, b bytes),
    seen = 1 inside the image, 0 outside or without a colour camera."""
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    H, W = masks[0].shape
    frames = fx.synthetic_frames(4, H, W)
    n = 64
    grid = (n, n, n)
    want = carve_np.carve(n, n, n, fx.oracle_cams(cams), masks, frames)
    idx = want["idx"]
    bgr = want["bgr"].astype(np.uint64)
    rec = idx.astype(np.uint64) | (bgr[:, 2] << np.uint64(32)) | (bgr[:, 1] << np.uint64(40)) | (bgr[:, 0] << np.uint64(48)) | \
        (np.uint64(1) << np.uint64(56))
    q = dn.steps_um(grid, carve_np.DEFAULT_BOUNDS)
    new_occ, dilated, cells = cl.grow(dn.volume(idx, grid), q, dn.radius_r2(45), "dilate")
    got, added = cl.records_after(rec, new_occ, grid, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(cams)[1], frames[1], H, W)
    assert got.size == dilated == int(new_occ.sum()) > idx.size and int(added.sum()) == got.size - idx.size
    assert np.array_equal(got[added == 0], rec) and (np.diff((got & LOW).astype(np.int64)) > 0).all()
    fresh = got[added == 1]
    pts = carve_np.points_of_indices((fresh & LOW).astype(np.int64), n, n, n)
    off = carve_np.pixel_offsets(carve_np.project_points(pts, cams[1].R, cams[1].tvec, cams[1].K, cams[1].dist), H, W)
    assert (off >= 0).any()
    seen = (fresh >> np.uint64(56)) & np.uint64(1)
    assert np.array_equal(seen.astype(bool), off >= 0) and ((fresh >> np.uint64(57)) == 0).all()
    ok = off >= 0
    px = frames[1].reshape(-1, 3)[off[ok]]
    for shift, ch in ((32, 2), (40, 1), (48, 0)):
        assert np.array_equal(((fresh[ok] >> np.uint64(shift)) & np.uint64(255)).astype(np.uint8), px[:, ch])
    assert ((fresh[~ok] >> np.uint64(32)) == 0).all()
    bare, _ = cl.records_after(rec, new_occ, grid, carve_np.DEFAULT_BOUNDS)
    assert ((bare[added == 1] >> np.uint64(32)) == 0).all() and np.array_equal(bare & LOW, got & LOW)
    # a grid that reaches outside the colour camera's image: seen = 0 there
    wide = (-6000, 6000, -6000, 6000, -3000, 3000)
    occ = np.zeros((16, 16, 16), dtype=bool)
    occ[7:9, 7:9, 7:9] = True
    o_rec = dn.indices(occ).astype(np.uint64)
    grown = cl.dilate(occ, dn.steps_um((16, 16, 16), wide), 10 ** 14)
    got, added = cl.records_after(o_rec, grown, (16, 16, 16), wide, fx.oracle_cams(cams)[1], None, H, W)
    seen = ((got >> np.uint64(56)) & np.uint64(1))[added == 1]
    assert grown.all() and 0 < int(seen.sum()) < seen.size


def test_public_names():
    from voxcarve import _lib, assignment
    from voxcarve.engine import CarveEngine
    header = open(os.path.join(fx.ROOT, "include", "voxcarve.h")).read()
    assert "#define VC_GROW_DILATE 0u" in header and "#define VC_GROW_CLOSE  1u" in header
    assert "int vc_hull_grow(vc_ctx *ctx, uint32_t op, uint64_t r2, uint32_t flags /* must be 0 */, vc_grow_stats_t *stats);" in header
    assert "int vc_fetch_grown(vc_ctx *ctx, uint8_t *added);" in header
    assert (_lib.VC_GROW_DILATE, _lib.VC_GROW_CLOSE) == (0, 1)
    assert "vc_hull_grow" in _lib.SIGNATURES and "vc_fetch_grown" in _lib.SIGNATURES
    assert [f[0] for f in _lib.VcGrowStats._fields_] == ["survivors_before", "dilated", "survivors_after", "added", "box_cells", "q", "grow_ms"]
    assert "#define VC_KERNEL_KINDS %d" % _lib.VC_KERNEL_KINDS in header and len(_lib.KERNEL_KINDS) == _lib.VC_KERNEL_KINDS
    for name in ("VC_K_GROW_MARK", "VC_K_GROW_RANK", "VC_K_GROW_MERGE"):
        assert name in header
    assert _lib.KERNEL_KINDS[-3:] == ("k_grow_mark", "grow_rank", "grow_merge")
    for name in ("dilate_hull", "close_hull", "fetch_added"):
        assert callable(getattr(CarveEngine, name))
    saved = dict(assignment._settings)
    try:
        assert assignment._settings["hull_close_mm"] == 0.0
        for bad in (-1, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                assignment.configure(hull_close_mm=bad)
        assert assignment._settings["hull_close_mm"] == 0.0
        assignment.configure(hull_close_mm=25)
        assert assignment._settings["hull_close_mm"] == 25
    finally:
        assignment.configure(frame_source=None, **saved)
    out = subprocess.run([sys.executable, os.path.join(fx.ROOT, "scripts", "demo.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--close MM" in out.stdout and "--open MM" in out.stdout
