"""The lit pass's restatement (tests/light_np.py) on the CPU: the vectorised form against the literal one, the block-skipping
secondary walk against the voxel walk bit for bit, monotonicity under removing voxels, shadows on a floor against an analytic
slab test, the occlusion count on hand scenes, faces turned from the light, and the library's exports."""
import ctypes

import numpy as np
import pytest

import light_np as ln
import render_np as rn
from voxcarve import camera

BOUNDS = (-100.0, 100.0, -80.0, 120.0, -50.0, 60.0)
KEYS = ("rgb", "depth", "kind", "shadow", "ao")


def _records(rng, occ):
    idx = np.flatnonzero(occ).astype(np.uint32)
    rgb = rng.integers(0, 256, (idx.size, 3)).astype(np.uint8)
    n4 = rng.integers(-32767, 32768, (idx.size, 4)).astype(np.int16)
    n4[:, 3] = rng.random(idx.size) < 0.8                    # some records without a normal ...
    n4[rng.random(idx.size) < 0.1, :3] = 0                   # ... and some with a zero one
    return idx, rgb, n4


def _render(occ, idx, rgb, grid, bounds, cams, H, W):
    views = [rn.view_params(c) for c in cams]
    return views, rn.render(occ, idx, rgb, grid, bounds, views, H, W, background=(9, 8, 7))


def _same(a, b, what=""):
    for k in KEYS:
        x, y = a[k], b[k]
        if k == "depth":
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), (what, k, int((x != y).sum()))
    assert a["stats"] == b["stats"], (what, a["stats"], b["stats"])


def _floor(z, grow=60.0):
    return {"z": z, "rect": (BOUNDS[0] - grow, BOUNDS[1] + grow, BOUNDS[2] - grow, BOUNDS[3] + grow), "cell_mm": 37.0,
            "rgb": ((90, 100, 110), (200, 190, 180))}


def _random_case(rng, lo=8, hi=13, sparse=None):
    grid = tuple(int(v) for v in rng.integers(lo, hi, 3))
    occ = rng.random(int(np.prod(grid))) < (rng.choice([0.02, 0.06, 0.15]) if sparse is None else sparse)
    ctr = np.array([0.0, 20.0, 5.0]) + rng.normal(0, 15, 3)
    eye = ctr + rng.normal(0, 1, 3) * 300
    return grid, occ, camera.look_at(eye, ctr, rng.uniform(14, 30), 12, 16)


def _random_light(rng, k):
    pos = (tuple(rng.normal(0, 1, 3)) + (0.0,)) if k % 2 else (tuple(rng.normal(0, 150, 3)) + (1.0,))
    floor = None if k % 3 == 0 else _floor((70.0, 10.0)[k % 3 - 1])              # under the grid, and cutting through it
    return {"pos": pos, "ambient": int(rng.integers(0, 256)), "smooth": int(k % 4 < 2), "ao_reach": float(rng.choice([0.0, 1.5, 4.0, 50.0])),
            "floor": floor}


def test_vectorised_equals_literal():
    rng = np.random.default_rng(23)
    seen = {"hull": 0, "floor": 0, "shadowed": 0, "away": 0, "ao": 0}
    for k in range(12):
        grid, occ, cam = _random_case(rng)
        idx, rgb, n4 = _records(rng, occ)
        views, ren = _render(occ, idx, rgb, grid, BOUNDS, [cam], 12, 16)
        lt = _random_light(rng, k)
        a = ln.light(occ, idx, rgb, n4, grid, BOUNDS, views, 12, 16, ren, lt)
        _same(a, ln.light_literal(occ, idx, rgb, n4, grid, BOUNDS, views, 12, 16, ren, lt), k)
        st = a["stats"]
        assert st["pixels"] == 192 and st["hull_pixels"] == int((a["kind"] == 1).sum()) and st["floor_pixels"] == int((a["kind"] == 2).sum())
        seen["hull"] += st["hull_pixels"]; seen["floor"] += st["floor_pixels"]
        seen["shadowed"] += st["shadowed"]; seen["away"] += st["facing_away"]; seen["ao"] += int((a["ao"] < 16).sum())
    assert min(seen.values()) > 20, seen


def test_camera_inside_a_survivor_keeps_the_render():
    grid = (8, 8, 8)
    n, s, e = rn.grid_params(grid, BOUNDS)
    occ = np.zeros(512, bool)
    occ[(3 * 8 + 5) * 8 + 2] = True
    idx, rgb, n4 = _records(np.random.default_rng(1), occ)
    eye = (rn.boundary(e[0], s[0], 5) + 1.0, rn.boundary(e[1], s[1], 2) + 2.0, rn.boundary(e[2], s[2], 3) + 3.0)
    cam = camera.look_at(eye, (0.0, 0.0, 0.0), 20.0, 6, 8)
    views, ren = _render(occ, idx, rgb, grid, BOUNDS, [cam], 6, 8)
    assert (ren["face"] == 6).all()
    lt = {"pos": (0.0, 0.0, -500.0, 1.0), "ambient": 40, "smooth": 0, "ao_reach": 4.0, "floor": None}
    for out in (ln.light(occ, idx, rgb, n4, grid, BOUNDS, views, 6, 8, ren, lt),
                ln.light_literal(occ, idx, rgb, n4, grid, BOUNDS, views, 6, 8, ren, lt)):
        assert np.array_equal(out["rgb"], ren["rgb"]) and (out["kind"] == 1).all() and (out["shadow"] == 0).all() and (out["ao"] == 16).all()
        assert out["stats"]["hull_pixels"] == 48 and out["stats"]["rays_walked"] == 0


def test_entry_walk_is_the_renders_walk():
    """secondary() without a start cell is vc_render's items 3 and 4: from one origin it is render_np.walk_voxels."""
    rng = np.random.default_rng(5)
    for _ in range(6):
        grid, occ, cam = _random_case(rng)
        o, d = rn.pixel_rays(rn.view_params(cam), 12, 16)
        idx, t, _ = rn.walk_voxels(occ, grid, BOUNDS, o, d)
        hit, ts = ln.secondary(occ, grid, BOUNDS, np.broadcast_to(o, d.shape), d)
        assert np.array_equal(hit, idx != rn.MISS) and np.array_equal(ts.view(np.uint64), t.view(np.uint64))


@pytest.mark.parametrize("B", [2, 4, 8])
def test_block_walk_equals_voxel_walk_for_secondary_rays(B):
    rng = np.random.default_rng(300 + B)
    skips = 0
    for k in range(6):
        grid, occ, cam = _random_case(rng, 14, 22, sparse=rng.choice([0.002, 0.01, 0.04]))
        idx, rgb, n4 = _records(rng, occ)
        views, ren = _render(occ, idx, rgb, grid, BOUNDS, [cam], 12, 16)
        lt = _random_light(rng, k)
        lt["ao_reach"] = 50.0
        st = {}
        _same(ln.light(occ, idx, rgb, n4, grid, BOUNDS, views, 12, 16, ren, lt),
              ln.light(occ, idx, rgb, n4, grid, BOUNDS, views, 12, 16, ren, lt, block=B, stats=st), (B, k))
        skips += st.get("skips", 0)
        # start cells anywhere, directions along cell diagonals and axes (ties) and at random
        P = 400
        n, s, e = rn.grid_params(grid, BOUNDS)
        c0 = np.stack([rng.integers(-1, n[a] + 1, P) for a in range(3)], axis=1)
        q = np.stack([rn.boundary(e[a], s[a], c0[:, a]) + rng.choice([0.0, 0.5, 1.0], P) * s[a] for a in range(3)], axis=1)
        d = np.where(rng.random((P, 1)) < 0.5, rng.integers(-2, 3, (P, 3)) * np.array(s), rng.normal(0, 1, (P, 3)))
        d[np.all(d == 0, axis=1)] = (0.0, 1.0, 0.0)
        h0, t0 = ln.secondary(occ, grid, BOUNDS, q, d, c0)
        h1, t1 = ln.secondary(occ, grid, BOUNDS, q, d, c0, B)
        assert np.array_equal(h0, h1) and np.array_equal(t0.view(np.uint64), t1.view(np.uint64))
    assert skips > 0


def test_removing_a_voxel_never_adds_shadow_or_occlusion():
    """Per pixel whose primary ray sees the same thing before and after (the same kind, voxel and face: its secondary rays then
    start from the same point and cell, and a walk over fewer voxels hits no earlier)."""
    rng = np.random.default_rng(77)
    compared = changed = 0
    for k in range(10):
        grid, occ, cam = _random_case(rng, sparse=0.12)
        idx, rgb, n4 = _records(rng, occ)
        lt = _random_light(rng, k)
        lt["smooth"], lt["ao_reach"] = 0, 6.0
        views, ren = _render(occ, idx, rgb, grid, BOUNDS, [cam], 12, 16)
        a = ln.light(occ, idx, rgb, None, grid, BOUNDS, views, 12, 16, ren, lt)
        for victim in rng.choice(idx, size=min(6, idx.size), replace=False):
            occ2 = occ.copy()
            occ2[victim] = False
            keep = idx != victim
            _, ren2 = _render(occ2, idx[keep], rgb[keep], grid, BOUNDS, [cam], 12, 16)
            b = ln.light(occ2, idx[keep], rgb[keep], None, grid, BOUNDS, views, 12, 16, ren2, lt)
            same = (a["kind"] == b["kind"]) & (ren["index"] == ren2["index"]) & (ren["face"] == ren2["face"])
            assert not ((a["shadow"] == 0) & (b["shadow"] == 1) & same).any()
            assert not ((b["ao"] < a["ao"]) & same).any()
            assert np.array_equal((a["shadow"] == 2) & same, (b["shadow"] == 2) & same)
            compared += int((same & (a["kind"] != 0)).sum())
            changed += int((same & ((a["shadow"] != b["shadow"]) | (a["ao"] != b["ao"]))).sum())
    assert compared > 2000 and changed > 0


def _box_scene():
    """A solid box of cells standing on the plane z = b(nz) under a camera that looks down on it (world up is -z)."""
    grid = (20, 20, 12)
    n, s, e = rn.grid_params(grid, BOUNDS)
    occ3 = np.zeros((12, 20, 20), bool)                       # [iz, ix, iy]
    lo, hi = (7, 8, 6), (12, 14, 12)                          # cells [lo, hi) per axis (x, y, z): the box touches the floor
    occ3[lo[2]:hi[2], lo[0]:hi[0], lo[1]:hi[1]] = True
    box = [(rn.boundary(e[a], s[a], lo[a]), rn.boundary(e[a], s[a], hi[a])) for a in range(3)]
    floor = _floor(float(rn.boundary(e[2], s[2], 12)), 300.0)
    cam = camera.look_at((140.0, -190.0, -420.0), (0.0, 20.0, 40.0), 52.0, 48, 64)
    return grid, occ3.reshape(-1), box, floor, cam


def test_floor_shadow_equals_the_slab_test():
    """Directional light: a floor pixel is in shadow iff the ray from its point along the light's direction passes through the
    box.  Pixels whose ray only grazes the box (the interval inside it is shorter than 1e-6 of its far end) are left out; they
    must stay below 1 % of the floor pixels."""
    grid, occ, box, floor, cam = _box_scene()
    idx, rgb, _ = _records(np.random.default_rng(2), occ)
    views, ren = _render(occ, idx, rgb, grid, BOUNDS, [cam], 48, 64)
    L = (-0.9, 0.55, -0.5)                                   # low: a long shadow towards the camera's side
    lt = {"pos": L + (0.0,), "ambient": 50, "smooth": 0, "ao_reach": 0.0, "floor": floor}
    out = ln.light(occ, idx, rgb, None, grid, BOUNDS, views, 48, 64, ren, lt)
    o, d = rn.pixel_rays(views[0], 48, 64)
    isf, tf, Q = ln.floor_pixels(o, d, ren["index"][0], ren["depth"][0], floor)
    assert np.array_equal(isf, out["kind"][0] == 2) and isf.sum() > 1500
    t_in, t_out = np.zeros(isf.size), np.full(isf.size, np.inf)
    for a in range(3):
        ta, tb = (box[a][0] - Q[:, a]) / L[a], (box[a][1] - Q[:, a]) / L[a]
        t_in, t_out = np.maximum(t_in, np.minimum(ta, tb)), np.minimum(t_out, np.maximum(ta, tb))
    want = t_in < t_out
    graze = np.abs(t_out - t_in) < 1e-6 * np.abs(t_out)
    judged = isf & ~graze
    assert (isf & graze).sum() <= 0.01 * isf.sum()
    assert np.array_equal(out["shadow"][0][judged] == 1, want[judged])
    assert (out["shadow"][0][judged] != 2).all()
    assert 50 < (out["shadow"][0][isf] == 1).sum() < isf.sum() - 50      # (both outcomes are there to be judged)
    # a shadowed floor pixel takes the ambient term alone
    sh = np.nonzero(isf & (out["shadow"][0] == 1))[0]
    cell = floor["cell_mm"]
    base = np.asarray(floor["rgb"], np.int64)[(np.floor(Q[sh, 0] / cell).astype(np.int64) + np.floor(Q[sh, 1] / cell).astype(np.int64)) & 1]
    assert np.array_equal(out["rgb"][0][sh], (base * ((50 * 16 * 2 + 16) // 32) + 127) // 255)
    assert np.array_equal(out["depth"][0][isf], tf[isf].astype(np.float32))


def _slab_scene(wall):
    """A slab of cells over the whole grid (its top towards -z) and, with `wall`, a wall standing on it; seen from above."""
    grid = (16, 16, 10)
    occ3 = np.zeros((10, 16, 16), bool)
    occ3[6:8] = True
    if wall:
        occ3[1:6, 9:11, :] = True
    cam = camera.look_at((-40.0, 30.0, -600.0), (0.0, 20.0, 20.0), 80.0, 24, 32)
    return grid, occ3.reshape(-1), cam


def test_ao_on_a_flat_top_in_a_corner_and_without_reach():
    rng = np.random.default_rng(3)
    lt = {"pos": (0.1, 0.2, -1.0, 0.0), "ambient": 80, "smooth": 0, "ao_reach": 5.0, "floor": None}
    grid, occ, cam = _slab_scene(False)
    idx, rgb, _ = _records(rng, occ)
    views, ren = _render(occ, idx, rgb, grid, BOUNDS, [cam], 24, 32)
    flat = ln.light(occ, idx, rgb, None, grid, BOUNDS, views, 24, 32, ren, lt)
    top = (flat["kind"][0] == 1) & (ren["face"][0] == 4)
    assert top.sum() > 300 and (flat["ao"][0][top] == 16).all() and (flat["shadow"][0][top] == 0).all()
    grid, occ, cam = _slab_scene(True)
    idx, rgb, _ = _records(rng, occ)
    views, ren = _render(occ, idx, rgb, grid, BOUNDS, [cam], 24, 32)
    out = ln.light(occ, idx, rgb, None, grid, BOUNDS, views, 24, 32, ren, lt)
    n, s, e = rn.grid_params(grid, BOUNDS)
    ix = (ren["index"][0].astype(np.int64) // n[1]) % n[0]
    top = (out["kind"][0] == 1) & (ren["face"][0] == 4) & (ren["index"][0].astype(np.int64) // (n[0] * n[1]) == 6)
    near, far = top & ((ix == 8) | (ix == 11)), top & ((ix < 3) | (ix > 14))
    assert near.sum() > 10 and far.sum() > 10
    assert (out["ao"][0][near] < 16).all() and (out["ao"][0][far] == 16).all()
    assert out["ao"][0][near].max() <= 13                    # the wall takes at least the three rays that lean towards it most
    lt0 = dict(lt, ao_reach=0.0)
    none = ln.light(occ, idx, rgb, None, grid, BOUNDS, views, 24, 32, ren, lt0)
    assert (none["ao"] == 16).all() and none["stats"]["rays_walked"] == int((none["shadow"][none["kind"] == 1] != 2).sum())
    assert out["stats"]["rays_walked"] == none["stats"]["rays_walked"] + 16 * out["stats"]["hull_pixels"]


def test_a_face_turned_from_the_light_takes_the_ambient_term_only():
    grid, occ, box, floor, _ = _box_scene()
    cam = camera.look_at((260.0, -60.0, -60.0), (-5.0, 25.0, 30.0), 150.0, 48, 64)       # close, from the +x side
    idx, rgb, _ = _records(np.random.default_rng(4), occ)
    views, ren = _render(occ, idx, rgb, grid, BOUNDS, [cam], 48, 64)
    lt = {"pos": (1.0, 0.0, 0.0, 0.0), "ambient": 70, "smooth": 0, "ao_reach": 3.0, "floor": None}       # light from +x, level
    out = ln.light(occ, idx, rgb, None, grid, BOUNDS, views, 48, 64, ren, lt)
    hull = out["kind"][0] == 1
    face = ren["face"][0]
    # face 1: entered moving along -x, outward normal +x; the top (4) and the y sides have e_a = 0
    assert (out["shadow"][0][hull & (face == 1)] != 2).all() and (face[hull] == 1).sum() > 50
    away = hull & (face != 1)
    assert (out["shadow"][0][away] == 2).all() and out["stats"]["facing_away"] == int(away.sum())
    pos = np.searchsorted(idx, ren["index"][0][away])
    a_term = (70 * out["ao"][0][away].astype(np.int64) * 2 + 16) // 32
    assert np.array_equal(out["rgb"][0][away], (rgb[pos].astype(np.int64) * a_term[:, None] + 127) // 255)
    lit = hull & (face == 1) & (out["shadow"][0] == 0)
    assert lit.sum() > 50
    pos = np.searchsorted(idx, ren["index"][0][lit])
    s_full = (70 * out["ao"][0][lit].astype(np.int64) * 2 + 16) // 32 + 185      # c = 1: the light along the normal
    assert np.array_equal(out["rgb"][0][lit], (rgb[pos].astype(np.int64) * s_full[:, None] + 127) // 255)


def test_light_render_returns_the_stats_dict_without_a_device():
    """CarveEngine.light_render against a library that fills the stats it is handed with a counting pattern (the way
    tests/test_engine_stats.py holds the other passes): the dict follows the struct field by field."""
    import types
    from voxcarve import lighting
    from voxcarve.engine import DEFAULT_BOUNDS, CarveEngine

    seen = {}

    class FakeLib:
        def __getattr__(self, name):
            def call(*args):
                for a in args:
                    obj = getattr(a, "_obj", None)
                    if isinstance(obj, lighting.LightStats):
                        for k, (field, ctype) in enumerate(obj._fields_):
                            setattr(obj, field, k + 0.5 if ctype is ctypes.c_float else k)
                    elif isinstance(obj, lighting.Light):
                        seen["light"] = (tuple(obj.pos), obj.ambient, obj.smooth, obj.ao_reach, obj.floor, obj.floor_z,
                                         tuple(obj.floor_rect), obj.floor_cell_mm, [tuple(c) for c in obj.floor_rgb])
                return 0
            return call

    e = CarveEngine.__new__(CarveEngine)
    e._L, e._ctx = FakeLib(), None
    e.grid, e.bounds, e.slab = (4, 4, 5), DEFAULT_BOUNDS, (0, 5)
    e.n_cameras, e.image_size, e.count = 2, (3, 5), 0
    view = types.SimpleNamespace(K=np.diag([100.0, 100.0, 1.0]), dist=np.zeros(5), R=np.eye(3), tvec=np.array([1.0, 2.0, 3.0]))
    out = e.render_lit([view, view], 3, 5)
    assert list(out) == ["rgb", "depth", "index", "face", "stats", "rgb_flat", "depth_hull", "kind", "shadow", "ao", "light_stats"]
    assert out["light_stats"] == {"pixels": 0, "hull_pixels": 1, "floor_pixels": 2, "shadowed": 3, "facing_away": 4, "rays_walked": 5,
                                  "cells_visited": 6, "blocks_skipped": 7, "light_ms": 8.5}
    assert all(type(v) is (float if k == "light_ms" else int) for k, v in out["light_stats"].items())
    assert out["rgb"].shape == (2, 3, 5, 3) and out["ao"].shape == (2, 3, 5) and out["ao"].dtype == np.uint8
    # the defaults, spelled out: a point light 1000 mm above the first camera's centre, the floor under the grid
    sz = 2560.0 / 4
    assert seen["light"] == ((-1.0, -2.0, -1003.0, 1.0), 64, 0, 4.0, 1, (-2048.0 - 0.5 * sz) + 5.0 * sz,
                             (-512.0 - 768.0, 1024.0 + 768.0, -2048.0, 2048.0), 250.0, [(96, 96, 96), (160, 160, 160)])


def test_library_exports_light(built):
    from voxcarve import _lib, lighting
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "vc_light_render") and hasattr(lib, "vc_fetch_lit")
    assert ctypes.sizeof(lighting.Light) == 112 and ctypes.sizeof(lighting.LightStats) == 72
