"""The restatement of the geodesic pass (tests/geodesic_np.py; contract of vc_hull_geodesic in include/voxcarve.h): the literal
Dijkstra against the vectorised Bellman-Ford on the hulls the GPU tests use (the real cameras at 64^3, random scenes carved on
the CPU, the bent hull), the properties the contract promises (seeds at 0, d6 >= d18 >= d26, E_k has label k and d 0, paths fall
strictly to d = 0, a warm start equals a cold start), the pin of the real cameras at 64^3, the edge lengths, the paint bytes, and
the Python surface that needs no device."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import geodesic_np as gn

BOUNDS = (-512.0, 1024.0, -1024.0, 1024.0, -2048.0, 512.0)
RANDOM = [((37, 53, 29), 3, 1), ((37, 53, 29), 4, 2), ((20, 70, 33), 5, 1), ((9, 130, 12), 6, 1), ((12, 64, 10), 7, 2)]


def u_masks(H, W):
    """A U in camera 0's mask, limbs and bar a twelfth of the image's width wide, over the middle half of the image; the other
    masks full."""
    m = np.zeros((H, W), np.uint8)
    r0, r1, c0, c1, t = H // 4, 3 * H // 4, W // 4, 3 * W // 4, W // 12
    m[r0:r1, c0:c0 + t] = 255
    m[r0:r1, c1 - t:c1] = 255
    m[r1 - t:r1, c0:c1] = 255
    return [m] + [np.full((H, W), 255, np.uint8)] * 3


def random_seeds(seed, S, n=3):
    return np.sort(np.random.default_rng(100 + seed).choice(S, n, replace=False))


def _carve(grid, cams, masks, mv=None):
    from oracle import carve_c
    return carve_c.carve(*grid, fx.oracle_cams(cams), masks, None, min_views=mv)["idx"]


def _check_properties(idx, grid, q, seeds, K, conn):
    """Both forms, warm and cold; the properties; returns the Bellman-Ford result."""
    a = gn.geodesic(idx, grid, q, conn, seeds, K, method="bellman")
    b = gn.geodesic(idx, grid, q, conn, seeds, K, method="dijkstra")
    c = gn.geodesic(idx, grid, q, conn, seeds, K, method="bellman", warm=False)
    for other in (b, c):
        assert np.array_equal(a["keys"], other["keys"]) and a["extrema"] == other["extrema"]
    assert (a["d"][np.asarray(seeds, dtype=np.int64)] == 0).all() and (a["labels"][np.asarray(seeds, dtype=np.int64)] == 0).all()
    assert a["reached"] + a["unreached"] == len(idx) and a["seeds"] == len(set(int(s) for s in seeds))
    assert ((a["d"] == gn.NONE) == (a["labels"] == 255)).all()
    for e in a["extrema"]:
        assert a["labels"][e["record"]] == e["label"] and a["d"][e["record"]] == 0 and e["d"] > 0
    assert [e["label"] for e in a["extrema"]] == list(range(1, len(a["extrema"]) + 1))
    ds = [e["d"] for e in a["extrema"]]
    assert ds == sorted(ds, reverse=True)                           # (a new source only lowers distances)
    reached = np.flatnonzero(a["d"] != gn.NONE)
    for r in np.random.default_rng(1).choice(reached, min(20, reached.size), replace=False):
        p = gn.path(a["keys"], a["nbr"], a["w8"], idx, r)
        rec = np.searchsorted(idx, p)
        d = a["d"][rec].astype(np.int64)
        assert p[0] == idx[r] and d[-1] == 0 and (np.diff(d) < 0).all() and (a["labels"][rec] == a["labels"][r]).all()
    return a


def test_pin_real_cameras_64():
    idx, _, _ = fx.expected(64)
    grid = (64, 64, 64)
    q = dn.steps_um(grid, BOUNDS)
    assert idx.size == 6981 and q == (24381, 32508, 40635)
    seeds = gn.seeds_by_layer(idx, grid, "floor", 1)
    assert seeds.size == 2 and (gn.coords(idx, grid)[2][seeds] == 54).all()
    a = _check_properties(idx, grid, q, seeds, 5, 26)
    assert [(e["voxel"], e["d"]) for e in a["extrema"]] == [(68056, 1738449), (207637, 1432178), (198372, 993329), (142307, 889404),
                                                            (177880, 753272)]
    assert a["reached"] == 6977 and a["unreached"] == 4
    assert np.bincount(a["labels"], minlength=256)[:6].tolist() == [998, 958, 54, 412, 3332, 1223]


def test_connectivities_order_the_distances():
    idx, _, _ = fx.expected(64)
    grid = (64, 64, 64)
    q = dn.steps_um(grid, BOUNDS)
    seeds = gn.seeds_by_layer(idx, grid, "floor", 3)
    d = {c: _check_properties(idx, grid, q, seeds, 0, c)["d"] for c in (6, 18, 26)}
    assert (d[6] >= d[18]).all() and (d[18] >= d[26]).all() and (d[6] > d[26]).any()
    top = gn.seeds_by_layer(idx, grid, "top", 2)
    assert (gn.coords(idx, grid)[2][top] <= gn.coords(idx, grid)[2].min() + 1).all()
    _check_properties(idx, grid, q, top, 3, 18)


@pytest.mark.parametrize("grid,seed,mv", RANDOM)
def test_random_scenes(grid, seed, mv):
    cams3, masks3, _ = fx.random_scene(seed, C=3, fg=0.7)
    idx = _carve(grid, cams3, masks3, mv)
    q = dn.steps_um(grid, BOUNDS)
    seeds = random_seeds(seed, idx.size)
    out = {c: _check_properties(idx, grid, q, seeds, 4, c) for c in (6, 18, 26)}
    d = {c: gn.geodesic(idx, grid, q, c, seeds, 0)["d"] for c in (6, 18, 26)}
    assert (d[6] >= d[18]).all() and (d[18] >= d[26]).all()
    if (grid, seed) == ((37, 53, 29), 4):
        assert [out[c]["unreached"] for c in (6, 18, 26)] == [148, 8, 6]           # several components: some stay unreached


def test_bent_hull():
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    H, W = masks[0].shape
    grid = (32, 32, 32)
    idx = _carve(grid, cams, u_masks(H, W))
    q = dn.steps_um(grid, BOUNDS)
    assert idx.size == 7432
    worst = 0.0
    for conn in (6, 18, 26):
        a = _check_properties(idx, grid, q, [0], 2, conn)
        assert a["unreached"] == 0
        g = gn.geodesic(idx, grid, q, conn, [0], 0)
        ix, iy, iz = gn.coords(idx, grid)
        straight = np.sqrt(((ix - ix[0]) * q[0]) ** 2.0 + ((iy - iy[0]) * q[1]) ** 2.0 + ((iz - iz[0]) * q[2]) ** 2.0)
        ratio = g["d"][1:].astype(np.float64) / straight[1:]
        assert ratio.min() > 0.999                                  # (rounding each edge to a um)
        worst = max(worst, float(ratio.max()))
        if conn == 26:
            assert ratio.max() >= 1.25
    assert worst >= 1.25


def test_edges_and_small_cases():
    q = (1000, 2000, 3000)
    assert gn.edge_lengths(q) == (1000, 2000, 2236, 3000, 3162, 3606, 3742)
    for qq in ((24381, 32508, 40635), (1, 1, 1), (1 << 20, 3, 77777)):
        for m, w in enumerate(gn.edge_lengths(qq), start=1):
            s = sum((qq[a] * ((m >> a) & 1)) ** 2 for a in range(3))
            assert (2 * w - 1) ** 2 <= 4 * s < (2 * w + 1) ** 2      # |w - sqrt(s)| <= 1/2
    assert [len(gn.offsets(c, q)) for c in (6, 18, 26)] == [6, 18, 26]
    lin = [dz * 100 + dx * 10 + dy for dx, dy, dz, _ in gn.offsets(26, q)]
    assert lin == sorted(lin)
    grid = (3, 4, 2)
    # the empty hull, one voxel, a solid grid from both ends, every voxel a seed, K beyond what there is, duplicate seeds
    e = gn.geodesic(np.zeros(0, np.int64), grid, q, 26, [], 3)
    assert e["survivors"] == 0 and e["extremities"] == 0 and e["max_d"] == 0 and e["d"].size == 0
    one = gn.geodesic([7], grid, q, 26, [0], 3)
    assert one["d"].tolist() == [0] and one["extremities"] == 0 and one["reached"] == 1
    solid = np.arange(24)
    for conn in (6, 18, 26):
        a = _check_properties(solid, grid, q, [0], 30, conn)
        b = _check_properties(solid, grid, q, [23], 30, conn)
        assert a["extremities"] == b["extremities"] == 23 and a["max_d"] == 0 and (a["d"] == 0).all()
        assert a["extrema"][0]["voxel"] == 23 and b["extrema"][0]["voxel"] == 0
        if conn == 6:
            assert a["extrema"][0]["d"] == 2 * 1000 + 3 * 2000 + 1 * 3000
    allv = gn.geodesic(solid, grid, q, 26, solid, 5)
    assert (allv["d"] == 0).all() and allv["extremities"] == 0 and allv["seeds"] == 24
    dup = gn.geodesic(solid, grid, q, 26, [5, 5, 5, 2, 2], 2)
    assert dup["seeds"] == 2 and np.array_equal(dup["keys"], gn.geodesic(solid, grid, q, 26, [2, 5], 2)["keys"])
    none = gn.geodesic(solid, grid, q, 26, [], 2)
    assert none["reached"] == 0 and none["extremities"] == 0 and (none["labels"] == 255).all()
    with pytest.raises(ValueError, match="seed 1 .voxel 30. is no survivor"):
        gn.records_of(solid, [3, 30])
    with pytest.raises(ValueError):
        gn.offsets(8, q)
    with pytest.raises(ValueError):
        gn.path(none["keys"], none["nbr"], none["w8"], solid, 3)


def test_paint_bytes():
    idx = np.arange(24)
    g = gn.geodesic(idx, (3, 4, 2), (1000, 2000, 3000), 6, [0], 2)
    keys = g["keys"].copy()
    keys[5] = gn.NONE
    rgb = np.zeros((24, 3), np.uint8)
    pal = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8)
    lab = gn.paint(rgb, keys, "labels", pal)
    assert lab[5].tolist() == list(gn.UNREACHED_RGB) and lab[0].tolist() == [1, 2, 3]
    assert set(map(tuple, lab.tolist())) <= {(1, 2, 3), (4, 5, 6), (7, 8, 9), gn.UNREACHED_RGB}
    md = int((keys[keys != gn.NONE] >> np.uint64(8)).max())
    ramp = gn.paint(rgb, keys, "distance", max_d=md)
    assert ramp.max() == 255 and ramp[0].tolist() == [0, 0, 0] and ramp[5].tolist() == list(gn.UNREACHED_RGB)
    assert (gn.paint(rgb, keys, "distance", max_d=0)[keys != gn.NONE] == 0).all()


def test_python_surface_without_a_device():
    """The header, the prototypes, the settings and the tools' options: what needs no GPU."""
    import ctypes
    from voxcarve import _lib, assignment, geodesic
    from voxcarve.engine import CarveEngine
    header = open(os.path.join(fx.ROOT, "include", "voxcarve.h")).read()
    for name in ("vc_hull_geodesic", "vc_fetch_geodesic", "vc_fetch_geodesic_labels", "vc_fetch_extrema", "vc_geodesic_path",
                 "vc_fetch_extremum_path", "vc_paint_geodesic"):
        assert "int %s(vc_ctx *ctx" % name in header and name in _lib.SIGNATURES
    assert "#define VC_GEO_MAX_K %d" % _lib.VC_GEO_MAX_K in header and geodesic.MAX_K == gn.MAX_K == _lib.VC_GEO_MAX_K
    for a, v in zip("XYZ", _lib.VC_GEO_TILE):
        assert "#define VC_GEO_TILE_%s %d" % (a, v) in header
    assert gn.TILE == _lib.VC_GEO_TILE and gn.UNREACHED_RGB == geodesic.UNREACHED_RGB == _lib.VC_GEO_UNREACHED_RGB
    for c, v in zip("RGB", gn.UNREACHED_RGB):
        assert "#define VC_GEO_UNREACHED_%s %d" % (c, v) in header
    assert "VC_ERR_INTERNAL = -6" in header and _lib.STATUS_NAMES[-6] == "VC_ERR_INTERNAL"
    assert "#define VC_KERNEL_KINDS %d" % _lib.VC_KERNEL_KINDS in header and len(_lib.KERNEL_KINDS) == _lib.VC_KERNEL_KINDS
    body = header.split("} vc_kernel_kind;")[0].rsplit("typedef enum {", 1)[1]
    order = re.findall(r"VC_K_[A-Z0-9_]+", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert len(order) == _lib.VC_KERNEL_KINDS and order.index("VC_K_GEO_SEED") == _lib.KERNEL_KINDS.index("geo_seed")
    assert _lib.KERNEL_KINDS[_lib.KERNEL_KINDS.index("geo_seed"):][:4] == ("geo_seed", "k_geo_tiles", "k_geo_sweep", "geo_argmax")
    assert ctypes.sizeof(_lib.VcExtremum) == 32 and ctypes.sizeof(_lib.VcGeodesicStats) == 152
    assert geodesic.PALETTE.shape == (33, 3) and geodesic.PALETTE.dtype == np.uint8
    for name in ("hull_geodesic", "fetch_geodesic", "fetch_geodesic_mm", "fetch_geodesic_labels", "fetch_extrema", "geodesic_path",
                 "stick_figure", "paint_geodesic"):
        assert callable(getattr(CarveEngine, name))
    saved = dict(assignment._settings)
    try:
        assert assignment._settings["extremities"] == 0 and assignment._settings["geodesic_seeds"] == "floor"
        for bad in (dict(extremities=-1), dict(extremities=33), dict(extremities=2.5), dict(geodesic_paint="red"),
                    dict(geodesic_seeds="left")):
            with pytest.raises(ValueError):
                assignment.configure(**bad)
        assert assignment._settings["extremities"] == 0
        assignment.configure(extremities=5, geodesic_paint="labels")
        assert assignment._settings["extremities"] == 5
        with pytest.raises(RuntimeError):
            assignment.extremities()
    finally:
        assignment.configure(frame_source=None, **saved)
    out = subprocess.run([sys.executable, os.path.join(fx.ROOT, "scripts", "demo.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--extremities K" in out.stdout and "--geodesic-paint labels|distance" in out.stdout
    assert math.isqrt(4 * 24381 ** 2) == 2 * 24381
