"""Photo-consistency carving, CPU side: the vectorised restatement (tests/photo_np.py) against the literal round-by-round,
voxel-by-voxel, camera-by-camera loop, the properties the contract implies (nothing removed without colour disagreement, F inside
A1, a converged F a fixed point), and what it must do geometrically: carve the pit of a textured block that the visual hull fills,
keep the solid, leave a textured ellipsoid alone."""
import numpy as np
import pytest

import fixtures_util as fx
import photo_np as pn
import visible_np as vn
from oracle import carve_np
from voxcarve import synthetic


def _carve(grid, cams, masks, frames, bounds=carve_np.DEFAULT_BOUNDS, min_views=None):
    r = carve_np.carve(*grid, fx.oracle_cams(cams), masks, frames, bounds=bounds, min_views=min_views, color_cam=1)
    return r["idx"], np.asarray(r["bgr"])[:, ::-1]


def _agree(idx, rgb, grid, bounds, ocams, frames, H, W, **kw):
    a = pn.photo_carve(idx, rgb, grid, bounds, ocams, frames, H, W, **kw)
    b = pn.photo_carve_literal(idx, rgb, grid, bounds, ocams, frames, H, W, **kw)
    for k in ("idx", "rgb", "zmaps", "vis", "rounds"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["n_rounds"], a["converged"]) == (b["n_rounds"], b["converged"])
    assert set(a["idx"].tolist()) <= set(np.asarray(idx).tolist())                 # F within A1
    assert a["rounds"].max(initial=0) <= a["n_rounds"]
    assert np.array_equal(np.asarray(idx)[a["rounds"] == 0], a["idx"])
    return a


def _textured(cams, H, W):
    return synthetic.textured_scene(cams, H, W)[1]


@pytest.mark.parametrize("seed,grid", [(3, (9, 11, 8)), (11, (12, 10, 14))])
def test_literal_and_vectorised_agree_random_scenes(seed, grid):
    cams, masks, frames = fx.random_scene(seed, C=3, H=37, W=53, fg=0.8)
    H, W = masks[0].shape
    oc = fx.oracle_cams(cams)
    idx, rgb = _carve(grid, cams, masks, frames, min_views=2)
    assert idx.size > 0
    for fr in (frames, _textured(cams, H, W)):
        for m, R in ((2, 1), (2, 32), (3, 2)):               # m = 2 and C; R hit and not hit
            _agree(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, oc, fr, H, W, var_threshold=300, min_views=m, max_rounds=R)
    out = _agree(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, oc, frames, H, W, var_threshold=100, min_views=2, max_rounds=32)
    assert out["idx"].size < idx.size                         # random colours disagree


def test_literal_and_vectorised_agree_golden_16():
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    H, W = masks[0].shape
    frames = fx.synthetic_frames(4, H, W)
    grid = (16, 16, 16)
    idx, rgb = _carve(grid, cams, masks, frames)
    assert idx.size > 20
    for m in (2, 4):
        out = _agree(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(cams), frames, H, W, min_views=m, max_rounds=3)
    assert out["n_rounds"] >= 1


def test_constant_colours_huge_threshold_and_too_few_views_remove_nothing():
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    H, W = masks[0].shape
    oc = fx.oracle_cams(cams)
    grid = (24, 24, 24)
    frames = fx.synthetic_frames(4, H, W)
    idx, rgb = _carve(grid, cams, masks, frames)
    const = [np.full((H, W, 3), (10, 200, 90), np.uint8)] * 4
    for fr, kw in ((const, {}), (frames, {"var_threshold": 0xffffffff})):
        out = pn.photo_carve(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, oc, fr, H, W, **kw)
        assert out["converged"] and out["n_rounds"] == 1 and (out["rounds"] == 0).all()
        zmaps, vis, col = vn.color_visible(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, oc, fr, H, W)
        assert np.array_equal(out["idx"], idx) and np.array_equal(out["rgb"], col)
        assert np.array_equal(out["vis"], vis) and np.array_equal(out["zmaps"], zmaps)
    # min_views above every voxel's visible count: nothing can be tested
    _, vis, _ = vn.color_visible(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, oc, frames, H, W)
    most = max(bin(int(v)).count("1") for v in vis)
    out = pn.photo_carve(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, oc[:], frames, H, W, min_views=most + 1, var_threshold=0)
    assert (out["rounds"] == 0).all()


def test_converged_result_is_a_fixed_point_and_empty_input():
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    H, W = masks[0].shape
    oc = fx.oracle_cams(cams)
    grid = (24, 24, 24)
    frames = fx.synthetic_frames(4, H, W)
    idx, rgb = _carve(grid, cams, masks, frames)
    out = pn.photo_carve(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, oc, frames, H, W, var_threshold=1200, max_rounds=64)
    assert out["converged"] and out["idx"].size < idx.size
    again = pn.photo_carve(out["idx"], out["rgb"], grid, carve_np.DEFAULT_BOUNDS, oc, frames, H, W, var_threshold=1200)
    assert again["n_rounds"] == 1 and again["converged"] and (again["rounds"] == 0).all()
    assert np.array_equal(again["idx"], out["idx"]) and np.array_equal(again["rgb"], out["rgb"])
    e = _agree(np.zeros(0, np.uint32), np.zeros((0, 3), np.uint8), grid, carve_np.DEFAULT_BOUNDS, oc, frames, H, W)
    assert e["n_rounds"] == 1 and e["converged"] and e["idx"].size == 0 and (e["zmaps"] == vn.INF_BITS).all()


def pit_setup(H=240, W=320, n=64):
    """8 ring cameras, all 45 degrees above the block (the even ones of a 16-camera ring), bounds 15 % around the block."""
    cams = synthetic.ring_cameras(16, H, W, radius=2500.0, elevation_deg=45.0)[::2]
    ctr, half = np.array(synthetic.VOLUME_CENTRE), 1.15 * np.array(synthetic.PIT_HALF)
    lo, hi = ctr - half, ctr + half
    return cams, (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]), (n, n, n)


def test_pit_is_carved_and_the_solid_kept():
    H, W = 240, 320
    cams, bounds, grid = pit_setup(H, W)
    masks, frames = synthetic.textured_scene(cams, H, W)
    idx, rgb = _carve(grid, cams, masks, frames, bounds=bounds)
    out = pn.photo_carve(idx, rgb, grid, bounds, fx.oracle_cams(cams), frames, H, W, max_rounds=64)
    solid, pit = synthetic.in_pit_solid(carve_np.points_of_indices(idx, *grid, bounds))
    kept = out["rounds"] == 0
    assert pit.sum() > 10000 and solid.sum() > 100000       # the visual hull fills the pit
    # measured: 68 % of the hull's pit voxels removed, every solid voxel kept (converged in 20 rounds)
    assert 1 - kept[pit].mean() > 0.55
    assert kept[solid].mean() > 0.99
    assert out["converged"]


def test_textured_ellipsoid_keeps_almost_everything():
    H, W = 240, 320
    cams = synthetic.ring_cameras(16, H, W, radius=2500.0, elevation_deg=45.0)[::2]
    ctr, radii = np.array(synthetic.VOLUME_CENTRE), np.array(synthetic.ELLIPSOID_RADII)
    lo, hi = ctr - 1.15 * radii, ctr + 1.15 * radii
    bounds = (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])
    masks, frames = synthetic.textured_scene(cams, H, W, shape="ellipsoid")
    grid = (64, 64, 64)
    idx, rgb = _carve(grid, cams, masks, frames, bounds=bounds)
    out = pn.photo_carve(idx, rgb, grid, bounds, fx.oracle_cams(cams), frames, H, W, max_rounds=64)
    assert idx.size > 50000
    assert (out["rounds"] != 0).mean() < 0.02                # measured: 0.4 %
