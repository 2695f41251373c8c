"""Deterministic synthetic cameras, masks and frames.

Used by bench.py and the large-size property tests: there is no decoder for the
reference's videos here, and BASELINE.json's larger configurations (16 cameras at 1080p)
have no real data at all.  Cameras sit on a ring around the volume centre looking at it,
with a real-camera-like distortion; mask c = pixels whose ray hits an ellipsoid at the
centre, XOR 0.5 % salt noise; frames are seeded random BGR.
"""
import math

import numpy as np

from .camera import Camera

VOLUME_CENTRE = (256.0, 0.0, -768.0)          # centre of the reference's default bounds
ELLIPSOID_RADII = (300.0, 250.0, 800.0)
DIST = (-0.36, 0.19, 2e-4, 2e-4, -0.06)


def ring_cameras(n_cameras, H, W, radius=4000.0, elevation_deg=20.0, centre=VOLUME_CENTRE):
    if (H, W) == (1080, 1920):
        f, cx, cy = 1500.0, 960.0, 540.0
    else:
        f, cx, cy = 0.78 * W, W / 2.0, H / 2.0
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    ctr = np.asarray(centre, dtype=np.float64)
    cams = []
    for c in range(n_cameras):
        az = 2.0 * math.pi * c / n_cameras
        el = math.radians(elevation_deg if c % 2 == 0 else -elevation_deg)
        # world "up" of the reference's volume is -z (z runs -2048..512 below the floor plane)
        pos = ctr + radius * np.array([math.cos(az) * math.cos(el), math.sin(az) * math.cos(el), -math.sin(el)])
        fwd = ctr - pos
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, np.array([0.0, 0.0, -1.0]))
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])            # world -> camera rows
        t = -R @ pos
        cams.append(Camera(K.copy(), np.array(DIST), None, t, R=R))   # R given directly, no rvec
    return cams


def ellipsoid_masks(cams, H, W, radii=ELLIPSOID_RADII, centre=VOLUME_CENTRE, noise=0.005, seed=1000):
    """uint8 {0,255} masks: undistorted pixel rays against the ellipsoid, XOR salt noise."""
    ctr = np.asarray(centre, dtype=np.float64)
    inv_r = 1.0 / np.asarray(radii, dtype=np.float64)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    masks = []
    for c, cam in enumerate(cams):
        fx, fy, cx, cy = cam.K[0, 0], cam.K[1, 1], cam.K[0, 2], cam.K[1, 2]
        xd, yd = (u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy
        x, y = xd.copy(), yd.copy()
        k1, k2, p1, p2, k3 = cam.dist
        for _ in range(8):                                   # fixed-point undistortion
            r2 = x * x + y * y
            cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
            dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            x, y = (xd - dx) / cd, (yd - dy) / cd
        d_cam = np.stack([x, y, np.ones_like(x)], axis=-1)
        d = (d_cam @ cam.R) * inv_r                           # R^T d, scaled to the unit sphere
        o = ((-cam.R.T @ cam.tvec) - ctr) * inv_r
        a = (d * d).sum(-1)
        b = 2.0 * (d * o).sum(-1)
        cc = float((o * o).sum()) - 1.0
        hit = (b * b - 4 * a * cc) >= 0
        salt = np.random.default_rng(seed + c).random((H, W)) < noise
        masks.append(np.where(hit ^ salt, 255, 0).astype(np.uint8))
    return masks


def random_frames(n_cameras, H, W, seed=2000):
    return [np.random.default_rng(seed + c).integers(0, 256, (H, W, 3), dtype=np.uint8) for c in range(n_cameras)]


def shifted_masks(masks, step):
    """A different but equally sized workload per step: rotate every mask by `step` columns."""
    return [np.roll(m, 3 * step, axis=1) for m in masks]


# ---- a textured scene for photo-consistency carving ------------------------------------------------------------------------------
# Photo-consistency only means something when a surface point has the same colour in every camera.  The scenes below are
# analytic solids whose colour is a smooth function of the surface point alone (a linear field, COLOUR_GRADIENT levels per mm):
# a voxel on the true surface samples nearly the same colour in every camera that sees it, a voxel floating over a concavity
# samples the different points each camera sees behind it.

PIT_HALF = (300.0, 300.0, 250.0)               # the block's half extents (mm)
PIT_OPENING = (200.0, 200.0)                   # half extents of the pit's square opening in the top face
PIT_DEPTH = 150.0                              # from the top face (up is -z: the top face is the block's z minimum)
COLOUR_GRADIENT = 2.0                          # levels per mm near the centre: R along x, G along y, B along z
BACKGROUND_BGR = (40, 40, 40)


def _world_rays(cam, H, W):
    """Camera centre [3] and world directions [H, W, 3] of the pixel centres, undistorted as ellipsoid_masks does."""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    fx, fy, cx, cy = cam.K[0, 0], cam.K[1, 1], cam.K[0, 2], cam.K[1, 2]
    xd, yd = (u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy
    x, y = xd.copy(), yd.copy()
    k1, k2, p1, p2, k3 = cam.dist
    for _ in range(8):                                   # fixed-point undistortion
        r2 = x * x + y * y
        cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) / cd, (yd - dy) / cd
    d = np.stack([x, y, np.ones_like(x)], axis=-1) @ cam.R
    return -cam.R.T @ cam.tvec, d


def _ray_box(o, d, lo, hi):
    """Entry and exit parameters of rays o + t d through the box [lo, hi] (entry > exit: no hit)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (np.asarray(lo) - o) / d
        t2 = (np.asarray(hi) - o) / d
    t1, t2 = np.nan_to_num(t1, nan=-np.inf), np.nan_to_num(t2, nan=np.inf)
    return np.minimum(t1, t2).max(-1), np.maximum(t1, t2).min(-1)


def pit_boxes(centre=VOLUME_CENTRE, half=PIT_HALF, opening=PIT_OPENING, depth=PIT_DEPTH):
    """((block_lo, block_hi), (pit_lo, pit_hi)): the solid is the block minus the pit; the pit box reaches 1 m above the top face."""
    c = np.asarray(centre, dtype=np.float64)
    h = np.asarray(half, dtype=np.float64)
    top = c[2] - h[2]
    pit_lo = np.array([c[0] - opening[0], c[1] - opening[1], top - 1000.0])
    pit_hi = np.array([c[0] + opening[0], c[1] + opening[1], top + depth])
    return (c - h, c + h), (pit_lo, pit_hi)


def in_pit_solid(points, centre=VOLUME_CENTRE, half=PIT_HALF, opening=PIT_OPENING, depth=PIT_DEPTH):
    """(solid, pit) bool [N]: inside the block minus the pit; inside the pit (and inside the block's outline)."""
    (blo, bhi), (plo, phi) = pit_boxes(centre, half, opening, depth)
    P = np.asarray(points, dtype=np.float64)
    block = ((P >= blo) & (P <= bhi)).all(-1)
    pit = ((P > plo) & (P < phi)).all(-1)
    return block & ~pit, block & pit


def surface_colour(points, centre=VOLUME_CENTRE, gradient=COLOUR_GRADIENT):
    """u8 BGR [..., 3] of the colour field: per channel 128 + 127 sin(g (p - c) / 127) with p = x, y, z for R, G, B -- linear
    with slope g levels per mm near the centre, smooth and inside [1, 255] everywhere."""
    rgb = 128.0 + 127.0 * np.sin(gradient * (np.asarray(points, dtype=np.float64) - np.asarray(centre, dtype=np.float64)) / 127.0)
    return np.rint(rgb).astype(np.uint8)[..., ::-1]


def textured_scene(cams, H, W, shape="pit", centre=VOLUME_CENTRE, half=PIT_HALF, opening=PIT_OPENING, depth=PIT_DEPTH,
                   radii=ELLIPSOID_RADII, gradient=COLOUR_GRADIENT):
    """(masks, frames) of a textured analytic solid seen by `cams`: masks u8 {0, 255} [H, W] (no noise), frames BGR [H, W, 3]
    with the colour field of the first surface point each pixel ray hits, BACKGROUND_BGR where it hits nothing.
    shape "pit": a block (half extents `half`) with an open square pit (half `opening`, `depth` deep) in its top face (up is -z);
    shape "ellipsoid": the convex ellipsoid of ellipsoid_masks with the same colour field."""
    if shape not in ("pit", "ellipsoid"):
        raise ValueError("shape %r, expected 'pit' or 'ellipsoid'" % (shape,))
    masks, frames = [], []
    for cam in cams:
        o, d = _world_rays(cam, H, W)
        if shape == "pit":
            (blo, bhi), (plo, phi) = pit_boxes(centre, half, opening, depth)
            t0, t1 = _ray_box(o, d, blo, bhi)
            s0, s1 = _ray_box(o, d, plo, phi)
            block = (t0 <= t1) & (t1 > 0)
            in_pit = (s0 <= s1) & (s0 <= t0) & (t0 < s1)     # enters the block through the pit's opening
            t = np.where(in_pit, s1, t0)
            hit = block & (~in_pit | (s1 < t1))
        else:
            ctr = np.asarray(centre, dtype=np.float64)
            inv_r = 1.0 / np.asarray(radii, dtype=np.float64)
            ds, os_ = d * inv_r, (o - ctr) * inv_r
            a = (ds * ds).sum(-1)
            b = 2.0 * (ds * os_).sum(-1)
            cc = float((os_ * os_).sum()) - 1.0
            disc = b * b - 4 * a * cc
            hit = disc >= 0
            t = (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a)
        P = o + t[..., None] * d
        frame = np.empty((H, W, 3), dtype=np.uint8)
        frame[...] = BACKGROUND_BGR
        frame[hit] = surface_colour(P[hit], centre, gradient)
        masks.append(np.where(hit, 255, 0).astype(np.uint8))
        frames.append(frame)
    return masks, frames
