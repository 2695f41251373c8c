"""Silhouette-refined surface mesh, CPU side: the vectorised restatement (tests/surface_np.py) against the literal vertex-by-vertex,
step-by-step, camera-by-camera loop, the bisection's invariants, the topology against oracle/marching_np.py, what the refinement
is worth on a sphere whose visual hull is known in closed form, and the PLY writer."""
import math

import numpy as np
import pytest

import fixtures_util as fx
import surface_np as sn
from oracle import carve_np, marching_np
from voxcarve import camera, synthetic
from voxcarve.voxel_reconstruction import write_ply


def _occ(grid, ocams, masks, m, bounds=carve_np.DEFAULT_BOUNDS):
    nx, ny, nz = grid
    r = carve_np.carve(nx, ny, nz, ocams, masks, bounds=bounds, min_views=m)
    occ = np.zeros(nx * ny * nz, dtype=bool)
    occ[r["idx"]] = True
    return occ


def _bool_masks(masks):
    return np.stack([np.asarray(x) > 0 for x in masks])


def _agree(occ, grid, bounds, ocams, bm, m, steps, max_literal=400):
    a = sn.refine(occ, grid, bounds, ocams, bm, m, steps)
    V = a["verts"].shape[0]
    pick = np.arange(V) if V <= max_literal else np.unique(np.linspace(0, V - 1, max_literal).astype(np.int64))
    lv, lr = sn.refine_literal(occ, grid, bounds, ocams, bm, m, steps, vertices=pick)
    assert np.array_equal(a["verts"][pick].view(np.uint64), lv.view(np.uint64))
    assert np.array_equal(a["refined"][pick], lr)
    return a


@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("m", [4, 3])
def test_vectorised_equals_literal_golden(n, m):
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    ocams, bm = fx.oracle_cams(cams), _bool_masks(masks)
    grid = (n, n, n)
    occ = _occ(grid, ocams, masks, m)
    for steps in (0, 1, 8, 24):
        a = _agree(occ, grid, carve_np.DEFAULT_BOUNDS, ocams, bm, m, steps)
        assert a["verts"].shape[0] > 0
        if steps:
            assert a["refined"].sum() > 0.9 * a["refined"].size       # the carve's own test: the edge ends bracket the silhouettes


@pytest.mark.parametrize("seed,grid", [(3, (9, 1, 8)), (5, (7, 65, 5)), (11, (13, 11, 9)), (17, (1, 6, 5))])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_vectorised_equals_literal_random(seed, grid, m):
    cams, masks, _ = fx.random_scene(seed, C=3, H=37, W=53, fg=0.8)
    ocams, bm = fx.oracle_cams(cams), _bool_masks(masks)
    occ = _occ(grid, ocams, masks, m)
    for steps in (0, 1, 24):
        _agree(occ, grid, carve_np.DEFAULT_BOUNDS, ocams, bm, m, steps)


def test_edges_in_marching_cubes_vertex_order():
    rng = np.random.default_rng(7)
    for grid in ((9, 1, 8), (7, 65, 5), (13, 11, 9), (3, 4, 70)):
        nx, ny, nz = grid
        occ = rng.random(nx * ny * nz) < 0.45
        e, axis, on_low = sn.mesh_edges(occ, grid)
        verts, _ = marching_np.extract(occ.reshape(nz, nx, ny), level=0.25)
        lo3, ax2, ol2 = sn.edges_from_grid_verts(verts)
        assert np.array_equal(axis, ax2) and np.array_equal(on_low, ol2)
        assert np.array_equal(e, (lo3[:, 0] * nx + lo3[:, 1]) * ny + lo3[:, 2])


def test_bisection_invariants_midpoints_faces_and_volume():
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    ocams, bm = fx.oracle_cams(cams), _bool_masks(masks)
    m, grid, b = 4, (48, 48, 48), carve_np.DEFAULT_BOUNDS
    occ = _occ(grid, ocams, masks, m)
    r = sn.refine(occ, grid, b, ocams, bm, m, 8, with_interval=True)
    ref = r["refined"]
    P = lambda s: np.where((s == 1.0)[:, None], sn._at(r["base"], r["wa"], r["a_off"]),
                           sn._at(r["base"], r["wa"], r["a_on"] + s * (r["a_off"] - r["a_on"])))
    assert np.all(sn.count_views(P(r["lo"])[ref], ocams, bm) >= m)
    assert np.all(sn.count_views(P(r["hi"])[ref], ocams, bm) < m)
    assert np.all(r["hi"][ref] - r["lo"][ref] == 2.0 ** -8)
    # steps = 0: every vertex at its edge midpoint, refined or not
    r0 = sn.refine(occ, grid, b, ocams, bm, m, 0, with_interval=True)
    assert np.array_equal(r0["s"], np.full(r0["s"].size, 0.5))
    assert np.array_equal(r0["verts"], sn._at(r0["base"], r0["wa"], r0["a_on"] + 0.5 * (r0["a_off"] - r0["a_on"])))
    assert np.array_equal(r0["refined"], ref)
    # faces: marching_np.extract on the (nz, nx, ny) volume; outward with the cyclic axis map
    idx = np.nonzero(occ)[0]
    rgb = np.stack([idx % 251, idx % 241, idx % 239], 1).astype(np.uint8)
    mesh = sn.surface_mesh(occ, idx, rgb, grid, b, ocams, bm, m, 8)
    _, want_faces = marching_np.extract(occ.reshape(48, 48, 48))
    assert np.array_equal(mesh["faces"], want_faces)
    closed, oriented, _, vol = marching_np.mesh_invariants(mesh["verts"], mesh["faces"])
    assert oriented and vol > 0
    assert np.array_equal(mesh["rgb"], sn.colours(idx, rgb, r["e"], r["axis"], r["on_low"], grid))


def _sphere_rig():
    ctr = np.array(synthetic.VOLUME_CENTRE)
    H = W = 512
    cams = camera.orbit(6, 2000.0, 50.0, 1500.0, H, W, centre=ctr) + camera.orbit(6, 2000.0, -50.0, 1500.0, H, W, centre=ctr) + \
        camera.orbit(4, 2000.0, 0.0, 1500.0, H, W, centre=ctr)
    masks = synthetic.ellipsoid_masks(cams, H, W, radii=(250.0,) * 3, centre=ctr, noise=0)
    bounds = (ctr[0] - 400, ctr[0] + 400, ctr[1] - 400, ctr[1] + 400, ctr[2] - 400, ctr[2] + 400)
    return cams, masks, bounds, ctr


def _analytic_inside(P, cams, ctr, r):
    ok = np.ones(P.shape[0], dtype=bool)
    for cam in cams:
        C = -cam.R.T @ cam.tvec
        a, b = P - C, ctr - C
        cosang = (a @ b) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b))
        ok &= np.arccos(np.clip(cosang, -1.0, 1.0)) <= math.asin(r / np.linalg.norm(b))
    return ok


def test_refinement_halves_the_error_on_a_sphere():
    cams, masks, bounds, ctr = _sphere_rig()
    ocams, bm, grid, m = fx.oracle_cams(cams), _bool_masks(masks), (48, 48, 48), 16
    occ = _occ(grid, ocams, masks, m, bounds=bounds)
    r8 = sn.refine(occ, grid, bounds, ocams, bm, m, 8, with_interval=True)
    r0 = sn.refine(occ, grid, bounds, ocams, bm, m, 0)
    base, wa, a_on, a_off = r8["base"], r8["wa"], r8["a_on"], r8["a_off"]
    at = lambda s: sn._at(base, wa, a_on + s * (a_off - a_on))
    # the crossing of the continuous visual hull along each edge whose ends it brackets: 50 bisection steps
    sel = _analytic_inside(at(np.zeros(a_on.size)), cams, ctr, 250.0) & ~_analytic_inside(at(np.ones(a_on.size)), cams, ctr, 250.0)
    sel &= r8["refined"]
    lo, hi = np.zeros(a_on.size), np.ones(a_on.size)
    for _ in range(50):
        mid = (lo + hi) * 0.5
        ins = _analytic_inside(at(mid), cams, ctr, 250.0)
        lo, hi = np.where(ins, mid, lo), np.where(ins, hi, mid)
    cross = (lo + hi) * 0.5
    length = np.abs(a_off - a_on)
    err8 = float(np.mean(np.abs(r8["s"] - cross)[sel] * length[sel]))
    err0 = float(np.mean(np.abs(r0["s"] - cross)[sel] * length[sel]))
    assert sel.sum() > 0.8 * a_on.size, (int(sel.sum()), a_on.size)
    assert err8 <= 0.5 * err0, (err8, err0)


def read_ply(path):
    """A small binary little-endian PLY reader for what write_ply writes: (verts f32 [V, 3], faces u32 [F, 3], rgb or None)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    V = F = None
    props = []
    for line in head:
        t = line.split()
        if t[:2] == ["element", "vertex"]:
            V = int(t[2])
        elif t[:2] == ["element", "face"]:
            F = int(t[2])
        elif t[:1] == ["property"] and F is None:
            props.append((t[2], {"float": "<f4", "uchar": "u1"}[t[1]]))
    vrec = np.frombuffer(data, dtype=props, count=V, offset=end)
    frec = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<u4", (3,))], count=F, offset=end + vrec.nbytes)
    assert end + vrec.nbytes + frec.nbytes == len(data) and np.all(frec["n"] == 3)
    verts = np.stack([vrec["x"], vrec["y"], vrec["z"]], 1)
    rgb = np.stack([vrec["red"], vrec["green"], vrec["blue"]], 1) if "red" in vrec.dtype.names else None
    return verts, frec["v"].copy(), rgb


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    verts = rng.normal(size=(57, 3)) * 1000.0
    faces = rng.integers(0, 57, (91, 3)).astype(np.uint32)
    rgb = rng.integers(0, 256, (57, 3)).astype(np.uint8)
    p = write_ply(str(tmp_path / "a.ply"), verts, faces, rgb)
    v, f, c = read_ply(p)
    assert np.array_equal(v, verts.astype(np.float32)) and np.array_equal(f, faces) and np.array_equal(c, rgb)
    v, f, c = read_ply(write_ply(str(tmp_path / "b.ply"), verts, faces))
    assert np.array_equal(v, verts.astype(np.float32)) and np.array_equal(f, faces) and c is None
    v, f, c = read_ply(write_ply(str(tmp_path / "c.ply"), np.zeros((0, 3)), np.zeros((0, 3), np.uint32), np.zeros((0, 3), np.uint8)))
    assert v.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "d.ply"), verts, faces + 57)
