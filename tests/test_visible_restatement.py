"""Occlusion-aware colouring, CPU side: the vectorised restatement (tests/visible_np.py) against the literal per-voxel,
per-camera, per-pixel loop, and what the contract must mean geometrically (a hidden face has no bit; an ellipsoid's survivors take
the mean of exactly the cameras they face, never one they face away from)."""
import numpy as np
import pytest

import fixtures_util as fx
import visible_np as vn
from oracle import carve_np
from voxcarve import synthetic
from voxcarve.camera import Camera


def _carve(grid, cams, masks, frames, bounds=carve_np.DEFAULT_BOUNDS, min_views=None, color_cam=1):
    r = carve_np.carve(*grid, fx.oracle_cams(cams), masks, frames, bounds=bounds, min_views=min_views, color_cam=color_cam)
    return r["idx"], np.asarray(r["bgr"])[:, ::-1]


def _agree(idx, rgb, grid, bounds, ocams, frames, H, W, tol=None):
    a = vn.color_visible(idx, rgb, grid, bounds, ocams, frames, H, W, tol)
    b = vn.color_visible_literal(idx, rgb, grid, bounds, ocams, frames, H, W, tol)
    for x, y, what in zip(a, b, ("maps", "masks", "colours")):
        assert np.array_equal(x, y), what
    return a


def test_literal_and_vectorised_agree_golden():
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    H, W = masks[0].shape
    frames = fx.synthetic_frames(4, H, W)
    grid = (24, 24, 24)
    idx, rgb = _carve(grid, cams, masks, frames)
    assert idx.size > 50
    zmaps, vis, out = _agree(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(cams), frames, H, W)
    surf = vn.surface(idx, grid)
    assert (vis[~surf] == 0).all() and (out[~surf] == rgb[~surf]).all()
    assert (vis[surf] != 0).mean() > 0.5                    # most of the hull's skin is seen by some camera
    assert (zmaps != vn.INF_BITS).any(axis=1).all()         # every camera's map holds splats
    # a zero tolerance hides more, never less
    _, vis0, _ = _agree(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(cams), frames, H, W, tol=0.0)
    assert ((vis0 & ~vis) == 0).all()


@pytest.mark.parametrize("seed", [3, 11])
def test_literal_and_vectorised_agree_synthetic(seed):
    cams, masks, frames = fx.random_scene(seed, C=3, H=37, W=53, fg=0.8)
    H, W = masks[0].shape
    grid = (9, 11, 7)
    idx, rgb = _carve(grid, cams, masks, frames, min_views=2)
    assert idx.size > 0
    _agree(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(cams), frames, H, W)
    # one axis of a single voxel (half extent 0 there), every pixel foreground
    grid1 = (6, 1, 8)
    idx1, rgb1 = _carve(grid1, cams, [np.full((H, W), 255, np.uint8)] * 3, frames, min_views=1)
    _agree(idx1, rgb1, grid1, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(cams), frames, H, W)


@pytest.mark.parametrize("gap", [300.0, 100.0, -300.0])     # outside the grid's z_min layer, its voxels straddling, inside it
def test_near_camera_and_empty(gap):
    cams = fx.golden_cameras()[:2]
    H, W = 30, 40
    K = np.array([[30.0, 0, 20], [0, 30.0, 15], [0, 0, 1]])
    R = np.eye(3)
    near = Camera(K, np.zeros(5), None, -R @ np.array([256.0, 0.0, -2048.0 - gap]), R=R)
    allcams = [Camera(c.K * [[W / 644, 0, W / 644], [0, H / 486, H / 486], [0, 0, 1]], c.dist, None, c.tvec, R=c.R) for c in cams] + [near]
    frames = fx.synthetic_frames(3, H, W)
    grid = (8, 8, 8)
    full = [np.full((H, W), 255, np.uint8)] * 3
    idx, rgb = _carve(grid, allcams, full, frames, min_views=1)
    zmaps, vis, out = _agree(idx, rgb, grid, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(allcams), frames, H, W)
    assert (zmaps[2] != vn.INF_BITS).mean() > 0.5           # the near camera's map is covered by few, large rectangles
    assert (vis >> 2 & 1).any()
    e = _agree(np.zeros(0, np.uint32), np.zeros((0, 3), np.uint8), grid, carve_np.DEFAULT_BOUNDS, fx.oracle_cams(allcams), frames, H, W)
    assert (e[0] == vn.INF_BITS).all() and e[1].size == 0


def _pinhole(pos, look, f, H, W):
    fwd = np.asarray(look, float) - pos
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 0.0, -1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]])
    return Camera(K, np.zeros(5), None, -R @ pos, R=R)


def test_hidden_face_of_rear_box():
    bounds = (0.0, 1000.0, -500.0, 500.0, -500.0, 500.0)
    grid = (21, 21, 21)
    xs, ys, zs = carve_np.axis_tables(*grid, bounds)
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")         # [ix, iy, iz]
    front = (X <= 300) & (np.abs(Y) <= 200) & (np.abs(Z) <= 200)
    rear = (X >= 600) & (X <= 900) & (np.abs(Y) <= 200) & (np.abs(Z) <= 200)
    occ = (front | rear).transpose(2, 0, 1).reshape(-1)      # voxel order i = iz*nx*ny + ix*ny + iy
    idx = np.nonzero(occ)[0].astype(np.uint32)
    H, W = 60, 80
    cam = _pinhole(np.array([-3000.0, 0.0, 0.0]), (500.0, 0.0, 0.0), 200.0, H, W)   # looks along +x: the front box hides the rear one
    frames = [np.full((H, W, 3), 40, np.uint8)]
    rgb = np.zeros((idx.size, 3), np.uint8)
    _, vis, out = _agree(idx, rgb, grid, bounds, fx.oracle_cams([cam]), frames, H, W)
    pts = carve_np.points_of_indices(idx, *grid, bounds)
    hidden = np.isclose(pts[:, 0], 600.0, atol=30)           # the rear box's face towards the camera
    facing = np.isclose(pts[:, 0], 0.0)
    assert hidden.sum() > 20 and facing.sum() > 20
    assert (vis[hidden] & 1).sum() == 0
    assert (vis[facing] & 1).all() and (out[facing] == 40).all()


def test_ellipsoid_colours_are_means_of_facing_cameras():
    H, W, C = 120, 160, 8
    cams = synthetic.ring_cameras(C, H, W)
    masks = synthetic.ellipsoid_masks(cams, H, W, noise=0)
    ctr, radii = np.array(synthetic.VOLUME_CENTRE), np.array(synthetic.ELLIPSOID_RADII)
    lo, hi = ctr - 1.15 * radii, ctr + 1.15 * radii
    bounds = (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])
    grid = (40, 36, 64)
    consts = [(c * 31 + 5, 200 - c * 23, 17 * c + 60) for c in range(C)]          # BGR per camera
    frames = [np.tile(np.array(b, np.uint8), (H, W, 1)) for b in consts]
    idx, rgb = _carve(grid, cams, masks, frames, bounds=bounds)
    assert idx.size > 1000
    _, vis, out = vn.color_visible(idx, rgb, grid, bounds, fx.oracle_cams(cams), frames, H, W)
    seen = vis != 0
    assert seen.sum() > 0.5 * vn.surface(idx, grid).sum()
    rgbc = np.array([b[::-1] for b in consts], dtype=np.int64)
    for s in np.nonzero(seen)[0]:
        cs = [c for c in range(C) if (vis[s] >> c) & 1]
        want = (rgbc[cs].sum(axis=0) + len(cs) // 2) // len(cs)
        assert (out[s] == want).all()
    # never visible from a camera it clearly faces away from
    pts = carve_np.points_of_indices(idx, *grid, bounds)
    normal = (pts - ctr) / radii ** 2
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    for c, cam in enumerate(cams):
        pos = -cam.R.T @ cam.tvec
        to_cam = pos - pts
        to_cam /= np.linalg.norm(to_cam, axis=1, keepdims=True)
        cos = (normal * to_cam).sum(axis=1)
        assert not ((vis >> c) & 1)[cos < -0.2].any(), c
