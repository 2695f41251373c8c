"""The ray caster's restatement (tests/render_np.py) on the CPU: the contract's voxel walk against a brute-force search over the
survivor boxes, the block-skipping walk against the voxel walk bit for bit, hand cases, the look_at / orbit cameras, and the
library's exports."""
import ctypes

import numpy as np
import pytest

import render_np as rn
from voxcarve import camera

BOUNDS = (-100.0, 100.0, -80.0, 120.0, -50.0, 60.0)


def _random_case(rng, sparse):
    grid = tuple(int(v) for v in rng.integers(8, 17, 3))
    occ = rng.random(int(np.prod(grid))) < sparse
    ctr = np.array([0.0, 20.0, 5.0]) + rng.normal(0, 20, 3)
    eye = ctr + rng.normal(0, 1, 3) * 400
    return grid, occ, camera.look_at(eye, ctr, rng.uniform(20, 40), 24, 32)


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert np.array_equal(a[2], b[2])


def test_voxel_walk_equals_brute_force():
    rng = np.random.default_rng(11)
    hits = 0
    for _ in range(12):
        grid, occ, cam = _random_case(rng, rng.choice([0.003, 0.02, 0.1]))
        o, d = rn.pixel_rays(rn.view_params(cam), 24, 32)
        d = d + rng.normal(0, 1e-7, d.shape)              # away from edges and corners
        idx, t, _ = rn.walk_voxels(occ, grid, BOUNDS, o, d)
        bi, bt = rn.brute_force(occ, grid, BOUNDS, o, d)
        assert np.array_equal(idx, bi)
        h = idx != rn.MISS
        assert np.allclose(t[h], bt[h], rtol=1e-9, atol=1e-9)
        hits += int(h.sum())
    assert hits > 200


@pytest.mark.parametrize("B", [2, 4, 8])
def test_block_walk_equals_voxel_walk(B):
    rng = np.random.default_rng(100 + B)
    for _ in range(10):
        grid, occ, cam = _random_case(rng, rng.choice([0.001, 0.005, 0.03]))
        o, d = rn.pixel_rays(rn.view_params(cam), 24, 32)
        st = {}
        _same(rn.walk_voxels(occ, grid, BOUNDS, o, d), rn.walk_blocks(occ, grid, BOUNDS, o, d, B, st))
        assert st["skips"] > 0


@pytest.mark.parametrize("B", [2, 4, 8])
def test_block_walk_through_block_edges_and_corners(B):
    """Rays from voxel corners through block corners / along block edges and faces: the (t, axis) order of ties decides."""
    n, s, e = rn.grid_params((16, 16, 16), BOUNDS)
    rng = np.random.default_rng(7 + B)
    for trial in range(6):
        occ = rng.random(16 ** 3) < (0.002, 0.01, 0.05)[trial % 3]
        P = 300
        a = rng.integers(0, 17, (P, 3)) // B * B          # block corners ...
        b = rng.integers(0, 17, (P, 3))                   # ... to voxel corners
        pa = np.stack([rn.boundary(e[k], s[k], a[:, k]) for k in range(3)], 1)
        pb = np.stack([rn.boundary(e[k], s[k], b[:, k]) for k in range(3)], 1)
        d = pb - pa
        d[np.all(d == 0, axis=1)] = (1.0, 0.0, 0.0)
        d[: P // 4, rng.integers(0, 3)] = 0.0             # some of them inside a block face
        for p in range(P):
            o = pa[p] - 3.0 * d[p]                        # (start outside or inside: both)
            _same(rn.walk_voxels(occ, (16, 16, 16), BOUNDS, o, d[p:p + 1]),
                  rn.walk_blocks(occ, (16, 16, 16), BOUNDS, o, d[p:p + 1], B))


def test_hand_cases():
    grid = (8, 8, 8)
    n, s, e = rn.grid_params(grid, BOUNDS)
    occ = np.zeros(512, bool)
    lin = lambda ix, iy, iz: (iz * 8 + ix) * 8 + iy
    occ[lin(5, 2, 3)] = True
    cy, cz = rn.boundary(e[1], s[1], 2) + 0.5 * s[1], rn.boundary(e[2], s[2], 3) + 0.5 * s[2]
    # parallel to x (d_y = d_z = 0 exactly), from outside on the -x side
    o = np.array([-500.0, cy, cz])
    d = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, -0.0, 0.0]])
    for walk in (rn.walk_voxels, lambda *a: rn.walk_blocks(*a, 4)):
        idx, t, f = walk(occ, grid, BOUNDS, o, d)
        assert idx[0] == lin(5, 2, 3) and f[0] == 0 and t[0] == (rn.boundary(e[0], s[0], 5) - o[0]) * 1.0
        assert idx[1] == rn.MISS and f[1] == 255 and np.isinf(t[1])     # the grid is behind the camera
        assert idx[2] == idx[0] and t[2] == t[0]                        # -0.0 is a zero too
    # a parallel ray outside the slab of its zero axes misses
    idx, _, _ = rn.walk_voxels(occ, grid, BOUNDS, np.array([-500.0, 1e4, cz]), d[:1])
    assert idx[0] == rn.MISS
    # camera inside the grid in empty space: walks to the survivor, entering through its +x side
    o = np.array([rn.boundary(e[0], s[0], 7) + 1.0, cy, cz])
    idx, t, f = rn.walk_voxels(occ, grid, BOUNDS, o, d[1:2])
    assert idx[0] == lin(5, 2, 3) and f[0] == 1 and t[0] == (rn.boundary(e[0], s[0], 6) - o[0]) * (1.0 / -1.0)
    # camera inside a survivor: face 6, depth 0
    o = np.array([rn.boundary(e[0], s[0], 5) + 1.0, cy, cz])
    idx, t, f = rn.walk_voxels(occ, grid, BOUNDS, o, d[:2])
    assert list(idx) == [lin(5, 2, 3)] * 2 and list(f) == [6, 6] and list(t) == [0.0, 0.0]
    # the empty hull: every pixel a miss, background colour
    cam = camera.look_at((0.0, 0.0, -900.0), (0.0, 20.0, 5.0), 30.0, 12, 16)
    out = rn.render(np.zeros(512, bool), np.zeros(0, np.uint32), np.zeros((0, 3), np.uint8), grid, BOUNDS,
                    [rn.view_params(cam)], 12, 16, background=(1, 2, 3))
    assert (out["index"] == rn.MISS).all() and np.isinf(out["depth"]).all() and (out["face"] == 255).all()
    assert (out["rgb"] == (1, 2, 3)).all()


def test_shading_arithmetic():
    rgb = np.array([[0, 255, 128], [255, 1, 254]], np.uint8)
    face = np.array([0, 6], np.uint8)
    assert rn.shade_rgb(rgb, face, [255] * 7).tolist() == rgb.tolist()
    assert rn.shade_rgb(rgb, face, [0] * 7).tolist() == [[0, 0, 0], [0, 0, 0]]
    sh = [128, 0, 0, 0, 0, 0, 1]
    assert rn.shade_rgb(rgb, face, sh).tolist() == [[0, 128, 64], [1, 0, 1]]


def test_undistortion_without_coefficients_is_exact():
    cam = camera.look_at((1000.0, -2000.0, -3000.0), (256.0, 0.0, -768.0), 700.0, 30, 40)
    view = rn.view_params(cam)
    o, d = rn.pixel_rays(view, 30, 40)
    u = (np.arange(1200) % 40 + 0.5 - 20.0) / 700.0
    v = (np.arange(1200) // 40 + 0.5 - 15.0) / 700.0
    R = cam.R
    assert np.array_equal(d[:, 0], (u * R[0, 0] + v * R[1, 0]) + R[2, 0])
    assert np.allclose(o, [1000.0, -2000.0, -3000.0], atol=1e-9)
    sub = rn.pixel_rays(view, 30, 40, pixels=[5, 77, 1199])[1]
    assert np.array_equal(sub, d[[5, 77, 1199]])


def test_look_at_and_orbit():
    ctr = np.array([256.0, 0.0, -768.0])
    cams = [camera.look_at((3000.0, 1000.0, -2000.0), ctr, 900.0, 480, 640)] + camera.orbit(6, 4000.0, 20.0, 1000.0, 240, 320)
    for cam in cams:
        assert cam.rvec is None and np.array_equal(cam.dist, np.zeros(5))
        assert np.allclose(cam.R @ cam.R.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(cam.R), 1.0)
        pc = cam.R @ ctr + cam.tvec
        assert pc[2] > 0
        assert np.allclose(pc[0] / pc[2] * cam.K[0, 0] + cam.K[0, 2], cam.K[0, 2], atol=1e-9)
        assert np.allclose(pc[1] / pc[2] * cam.K[1, 1] + cam.K[1, 2], cam.K[1, 2], atol=1e-9)
        up = cam.R @ np.array([0.0, 0.0, -1.0])
        assert up[1] < 0                                   # world up shows up in the image
    eyes = [-(c.R.T @ c.tvec) for c in cams[1:]]
    assert np.allclose([np.linalg.norm(p - ctr) for p in eyes], 4000.0)
    assert all(p[2] < ctr[2] for p in eyes)                # raised towards up = -z
    with pytest.raises(ValueError):
        camera.look_at((0.0, 0.0, -1000.0), (0.0, 0.0, 0.0), 100.0, 10, 10)


def test_library_exports_render(built):
    from voxcarve import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "vc_render") and hasattr(lib, "vc_fetch_render")
