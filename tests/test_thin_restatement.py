"""The restatement of the thinning pass (tests/thin_np.py; contract of vc_hull_thin in include/voxcarve.h): the literal form
against the vectorised one on the hulls the GPU tests use (random scenes carved on the CPU, the real cameras at 64^3), the topology
before and after (26-components, 6-components of the complement, Euler number), the properties the contract promises (nothing
simple is left, anchors stay, peel is 0 on the kept voxels, thinning a skeleton removes nothing), the shapes (bar, cube, torus,
shell, anchored ball, the degenerate sets), the pins of the real cameras, the two forms of the predicate, and the host
arithmetic of voxcarve.skeleton."""
import os

import numpy as np
import pytest

import fixtures_util as fx
import thin_np as tn
from test_geodesic_restatement import BOUNDS, RANDOM, random_seeds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _carve(grid, cams, masks, mv=None):
    from oracle import carve_c
    return carve_c.carve(*grid, fx.oracle_cams(cams), masks, None, min_views=mv)["idx"].astype(np.int64)


def _solid(grid, inside):
    """The linear indices of the cells (ix, iy, iz) for which inside(ix, iy, iz) holds."""
    nx, ny, nz = grid
    iz, ix, iy = np.meshgrid(np.arange(nz), np.arange(nx), np.arange(ny), indexing="ij")
    return np.flatnonzero(inside(ix, iy, iz).reshape(-1))


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _simple_left(idx, grid, kept):
    """bool per kept voxel: simple in the kept set; and its degree."""
    ix, iy, iz = tn.coords(kept, grid)
    code = tn.gather_codes(tn._volume(kept, grid), ix, iy, iz)
    return tn.simple_codes(code), np.array([bin(c).count("1") for c in code.tolist()])


def _check(idx, grid, mode, anchors=None, literal=False, max_passes=tn.MAX_PASSES):
    """The properties every result has; the two forms against each other where asked.  Returns the vectorised result."""
    idx = np.asarray(idx, dtype=np.int64)
    r = tn.thin(idx, grid, mode, anchors, max_passes)
    if literal:
        _same(r, tn.thin_literal(idx, grid, mode, anchors, max_passes))
    kept = r["voxel"].astype(np.int64)
    assert tn.topology(kept, grid) == tn.topology(idx, grid)
    assert np.array_equal(r["peel"] == 0, np.isin(idx, kept)) and r["kept"] + r["removed"] == idx.size == r["survivors"]
    assert np.array_equal(idx[r["record"]], kept) and (np.diff(kept) > 0).all()
    pins = np.unique(np.asarray([] if anchors is None else anchors, dtype=np.int64))
    assert np.isin(pins, kept).all() and r["anchors"] == pins.size
    assert r["isolated"] + r["endpoints"] + r["junctions"] + int((r["degree"] == 2).sum()) == r["kept"]
    if r["removed"]:
        assert 1 <= int(r["peel"][r["peel"] > 0].min()) and int(r["peel"].max()) <= 6 * r["passes"]
    if r["stable"]:
        simple, degree = _simple_left(idx, grid, kept)
        assert np.array_equal(degree, r["degree"])
        free = ~np.isin(kept, pins)
        if mode == "point":
            assert not (simple & free).any()
        else:
            assert not (simple & free & (degree != 1)).any()
        again = tn.thin(kept, grid, mode, pins)                  # the skeleton as its own hull: nothing to remove
        assert again["removed"] == 0 and again["passes"] == 1 and np.array_equal(again["voxel"], r["voxel"])
    return r


def test_predicate_forms_agree():
    rng = np.random.default_rng(26)
    codes = np.concatenate([rng.integers(0, 1 << 26, 4000), [0, (1 << 26) - 1], 1 << np.arange(26)])
    for c in codes.tolist():
        assert tn.simple_code(c) == tn.simple_code_literal(c), c
    assert not tn.simple_code(0) and not tn.simple_code((1 << 26) - 1)                     # isolated; interior
    assert all(tn.simple_code(1 << k) for k in range(26))                                   # an end point is simple
    opposite = (1 << tn.BIT[(0, 0, -1)]) | (1 << tn.BIT[(0, 0, 1)])
    assert not tn.simple_code(opposite)                                                     # the middle of a line is not
    assert len(tn.OFFSETS) == 26 and len(tn.N18) == 18 and len(tn.N6) == 6


def test_pin_real_cameras_64():
    idx, _, _ = fx.expected(64)
    grid = (64, 64, 64)
    assert idx.size == 6981 and tn.topology(idx, grid) == (4, 1, -4)
    r = _check(idx, grid, "curve", literal=True)
    assert (r["kept"], r["passes"], r["steps"], r["stable"]) == (258, 6, 36, 1)
    r = _check(idx, grid, "point", literal=True)
    assert (r["kept"], r["passes"], r["endpoints"]) == (138, 6, 0)
    r = _check(idx, grid, "curve", max_passes=1)
    assert r["stable"] == 0 and r["passes"] == 1 and r["kept"] > 258


def test_pin_real_cameras_128():
    idx, _, _ = fx.expected(128)
    grid = (128, 128, 128)
    assert idx.size == 57048 and tn.topology(idx, grid) == (2, 1, -9)
    r = _check(idx, grid, "curve")
    assert (r["kept"], r["endpoints"], r["passes"]) == (1029, 115, 11)
    r = _check(idx, grid, "point")
    assert (r["kept"], r["passes"]) == (354, 11)


@pytest.fixture(scope="module")
def random_hulls():
    out = []
    for grid, seed, mv in RANDOM:
        cams3, masks3, _ = fx.random_scene(seed, C=3, fg=0.7)
        out.append((grid, seed, _carve(grid, cams3, masks3, mv)))
    return out


def test_random_scenes_literal_equals_vectorised_and_topology_stays(random_hulls):
    cavities = tunnels = 0
    for grid, seed, idx in random_hulls:
        assert idx.size > 0
        comp, back, euler = tn.topology(idx, grid)
        cavities += back - 1
        tunnels += comp + (back - 1) - euler                     # Euler number = components - tunnels + cavities
        pins = idx[random_seeds(seed, idx.size)]
        for mode in tn.MODES:
            _check(idx, grid, mode, literal=True)
            _check(idx, grid, mode, pins, literal=True)
    assert cavities > 0 and tunnels > 0                           # the precondition: there is topology to lose


def test_bar_thins_to_its_centre_line():
    grid = (11, 44, 11)
    idx = _solid(grid, lambda x, y, z: (x >= 1) & (x < 10) & (y >= 2) & (y < 42) & (z >= 1) & (z < 10))
    assert idx.size == 9 * 40 * 9
    r = _check(idx, grid, "curve", literal=True)
    ix, iy, iz = tn.coords(r["voxel"], grid)
    assert r["kept"] == 32 and (ix == 5).all() and (iz == 5).all() and iy.tolist() == list(range(6, 38))
    assert r["endpoints"] == 2 and r["junctions"] == 0
    assert _check(idx, grid, "point")["kept"] == 1


def test_cube_torus_shell_and_ball():
    grid = (10, 10, 10)
    cube = _solid(grid, lambda x, y, z: (x >= 1) & (x < 9) & (y >= 1) & (y < 9) & (z >= 1) & (z < 9))
    assert cube.size == 512 and _check(cube, grid, "point", literal=True)["kept"] == 1
    grid = (25, 25, 9)
    torus = _solid(grid, lambda x, y, z: (np.sqrt((x - 12.0) ** 2 + (y - 12.0) ** 2) - 8.0) ** 2 + (z - 4.0) ** 2 <= 9.0)
    assert tn.topology(torus, grid) == (1, 1, 0)
    r = _check(torus, grid, "point", literal=True)
    assert (r["degree"] == 2).all() and r["kept"] > 20            # a ring: every voxel has two neighbours
    _check(torus, grid, "curve")                                  # (with spurs where an end point formed: the hole is kept all the same)
    grid = (15, 15, 15)
    r2 = lambda x, y, z: (x - 7.0) ** 2 + (y - 7.0) ** 2 + (z - 7.0) ** 2
    shell = _solid(grid, lambda x, y, z: (r2(x, y, z) <= 36.0) & (r2(x, y, z) >= 9.0))
    assert tn.topology(shell, grid) == (1, 2, 2)
    for mode in tn.MODES:
        r = _check(shell, grid, mode)
        assert r["kept"] < shell.size // 2                        # a closed surface, one voxel thick
        assert mode == "curve" or r["endpoints"] == 0             # ("curve" keeps the single voxels at the sphere's poles as spurs)
    grid = (21, 21, 21)
    ball = _solid(grid, lambda x, y, z: (x - 10.0) ** 2 + (y - 10.0) ** 2 + (z - 10.0) ** 2 <= 81.0)
    pole = lambda iy: (10 * 21 + 10) * 21 + iy
    r = _check(ball, grid, "point", [pole(1), pole(19)], literal=True)
    ix, iy, iz = tn.coords(r["voxel"], grid)
    assert r["kept"] == 19 and (ix == 10).all() and (iz == 10).all() and iy.tolist() == list(range(1, 20))
    assert _check(ball, grid, "point")["kept"] == 1


def test_degenerate_sets():
    grid = (4, 5, 3)
    r = _check([], grid, "curve", literal=True)
    assert (r["kept"], r["passes"], r["steps"], r["stable"]) == (0, 1, 0, 1) and r["peel"].size == 0
    r = _check([27], grid, "point", literal=True)
    assert (r["kept"], r["isolated"], r["steps"]) == (1, 1, 6)
    at = lambda x, y, z: (z * 4 + x) * 5 + y
    for mode, kept in (("curve", 2), ("point", 1)):               # two voxels in diagonal contact: two end points
        r = _check([at(1, 1, 0), at(2, 2, 1)], grid, mode, literal=True)
        assert r["kept"] == kept
    full = np.arange(4 * 5 * 3)                                   # the hull fills the grid up to its faces
    for mode in tn.MODES:
        _check(full, grid, mode, literal=True)
        _check(full, grid, mode, [0, 59, 0], literal=True)
    assert _check(full, grid, "point")["kept"] == 1
    with pytest.raises(ValueError):
        tn.thin([3], grid, "curve", [4])
    with pytest.raises(ValueError):
        tn.thin([3], grid, "surface")
    for bad in (0, 10001):
        with pytest.raises(ValueError):
            tn.thin([3], grid, "curve", None, bad)


# ---- voxcarve.skeleton ------------------------------------------------------------------------------------------------------------
def _rows(r, grid):
    ix, iy, iz = tn.coords(r["voxel"], grid)
    return {"voxel": r["voxel"], "record": r["record"], "degree": r["degree"], "index": np.stack([ix, iy, iz], axis=1)}


def test_describe_and_branches():
    import distance_np as dn
    import geodesic_np as gn
    from voxcarve import skeleton
    idx, _, _ = fx.expected(64)
    grid = (64, 64, 64)
    r = tn.thin(idx, grid, "curve")
    sk = _rows(r, grid)
    d = skeleton.describe(sk, grid, BOUNDS)
    q = dn.steps_um(grid, BOUNDS)
    assert skeleton.steps_um(grid, BOUNDS) == q
    assert np.array_equal(np.bincount(d["edges"].reshape(-1), minlength=r["kept"]), r["degree"])       # degree = edges at the voxel
    assert (d["edges"][:, 0] < d["edges"][:, 1]).all()
    off = sk["index"][d["edges"][:, 1]] - sk["index"][d["edges"][:, 0]]
    assert (np.abs(off).max(axis=1) == 1).all()
    lengths = gn.edge_lengths(q)                                  # [m - 1], m = |dx| | |dy| << 1 | |dz| << 2
    m = (np.abs(off) * np.array([1, 2, 4])).sum(axis=1)
    assert np.array_equal(d["edge_mm"], np.array([lengths[k - 1] for k in m.tolist()]) / 1000.0)
    assert d["length_mm"] == pytest.approx(d["edge_mm"].sum()) and d["length_mm"] > 0
    assert d["endpoints"].tolist() == np.flatnonzero(r["degree"] == 1).tolist()
    assert d["junctions"].tolist() == np.flatnonzero(r["degree"] >= 3).tolist()
    lo = np.array([BOUNDS[0], BOUNDS[2], BOUNDS[4]])
    step = (np.array([BOUNDS[1], BOUNDS[3], BOUNDS[5]]) - lo) / 63.0
    assert np.allclose(d["positions_mm"], lo + sk["index"] * step) and "radius_mm" not in d
    depth = np.arange(idx.size, dtype=np.float64)
    assert np.array_equal(skeleton.describe(sk, grid, BOUNDS, depth)["radius_mm"], depth[r["record"]])
    for rows in (sk, _rows(tn.thin(fx.expected(128)[0], (128,) * 3, "curve"), (128,) * 3)):
        g = (64,) * 3 if rows is sk else (128,) * 3
        dd = skeleton.describe(rows, g, BOUNDS)
        br = skeleton.branches(rows, g, BOUNDS)
        two = np.flatnonzero(rows["degree"] == 2)
        inside = np.concatenate([np.unique(b["rows"])[rows["degree"][np.unique(b["rows"])] == 2] for b in br])
        assert np.array_equal(np.sort(inside), two)               # every degree-2 voxel in exactly one branch
        touch = (rows["degree"][dd["edges"]] == 2).any(axis=1)
        assert sum(b["length_mm"] for b in br) == pytest.approx(dd["edge_mm"][touch].sum())
        assert all((rows["degree"][b["rows"][1:-1]] == 2).all() for b in br)


def test_straight_line_and_ring():
    from voxcarve import skeleton
    grid, bounds = (12, 9, 7), (0.0, 110.0, 0.0, 160.0, 0.0, 90.0)          # steps of 10, 20 and 15 mm
    for axis, step in ((0, 10.0), (1, 20.0), (2, 15.0)):
        n = 6
        at = np.ones((n, 3), dtype=np.int64)
        at[:, axis] = np.arange(n)
        vox = (at[:, 2] * 12 + at[:, 0]) * 9 + at[:, 1]
        order = np.argsort(vox)
        sk = {"voxel": vox[order], "record": np.arange(n), "degree": np.array([1] + [2] * (n - 2) + [1], dtype=np.uint8)[order]}
        d = skeleton.describe(sk, grid, bounds)
        assert d["length_mm"] == pytest.approx((n - 1) * step) and d["edges"].shape == (n - 1, 2)
        br = skeleton.branches(sk, grid, bounds)
        assert len(br) == 1 and br[0]["length_mm"] == pytest.approx((n - 1) * step) and br[0]["rows"].size == n
    grid = (25, 25, 9)
    idx = _solid(grid, lambda x, y, z: (np.sqrt((x - 12.0) ** 2 + (y - 12.0) ** 2) - 8.0) ** 2 + (z - 4.0) ** 2 <= 9.0)
    r = tn.thin(idx, grid, "point")
    sk = _rows(r, grid)
    br = skeleton.branches(sk, grid, (0.0, 24.0, 0.0, 24.0, 0.0, 8.0))
    assert len(br) == 1 and br[0]["rows"][0] == br[0]["rows"][-1] == 0 and br[0]["rows"].size == r["kept"] + 1
    assert br[0]["length_mm"] == pytest.approx(skeleton.describe(sk, grid, (0.0, 24.0, 0.0, 24.0, 0.0, 8.0))["length_mm"])


def test_python_surface_without_a_device():
    from voxcarve import _lib, assignment
    header = open(os.path.join(ROOT, "include", "voxcarve.h")).read()
    for name in ("vc_hull_thin", "vc_fetch_thin", "vc_fetch_skeleton", "vc_fetch_thin_table"):
        assert name in _lib.SIGNATURES and "int %s(" % name in header
    assert "#define VC_THIN_MAX_PASSES %du" % _lib.VC_THIN_MAX_PASSES in header
    assert "#define VC_THIN_DEFAULT_PASSES %du" % _lib.VC_THIN_DEFAULT_PASSES in header and tn.MAX_PASSES == _lib.VC_THIN_DEFAULT_PASSES
    assert "#define VC_THIN_TABLE_BYTES (1u << 23)" in header and _lib.VC_THIN_TABLE_BYTES == 1 << 23
    import ctypes
    assert ctypes.sizeof(_lib.VcSkeletonVoxel) == 12 and ctypes.sizeof(_lib.VcThinStats) == 80
    saved = dict(assignment._settings)
    try:
        with pytest.raises(ValueError):
            assignment.configure(skeleton="curve", skeleton_anchors="extrema")
        with pytest.raises(ValueError):
            assignment.configure(skeleton="surface")
        with pytest.raises(ValueError):
            assignment.configure(skeleton="curve", skeleton_anchors="floor")
        assignment.configure(skeleton="point", skeleton_anchors="extrema", extremities=2)
        assert assignment._settings["skeleton"] == "point"
        with pytest.raises(RuntimeError):
            assignment.skeleton()
    finally:
        assignment.configure(frame_source=None, **saved)
