"""The footprint carve on the device (vc_carve_footprint; csrc/vc_footprint.h) against the restatement (tests/footprint_np.py),
bit for bit: indices, order, colours, seen flags, occupancy, per-voxel camera bits and counts -- the real cameras at 64^3 and
128^3 under every rule with and without the 2x2 post-filter, 16 ring cameras at 1080p, grids whose words end mid-wave or span
columns, one-voxel-thick grids, empty and full masks, cameras inside the volume, a slot used again, z-slabs, the passes that
follow a carve, 1024^3, every refusal, assignment.configure(footprint=...) and demo.py --footprint."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures_util as fx
import footprint_np as fp
from oracle import carve_np, postfilter_np
from test_footprint_restatement import _hostile_cameras
from voxcarve import _lib, synthetic

pytestmark = pytest.mark.gpu

ALL_RULES = ("any", ("cover", 1), ("cover", 128), ("cover", 256))


@pytest.fixture(scope="module")
def feng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    yield e
    e.close()


def _setup(e, grid, cams, masks, frames=None, bounds=None, color_cam=1):
    H, W = masks[0].shape
    if bounds is None:
        e.set_grid(*grid)
    else:
        e.set_grid(*grid, bounds=bounds)
    e.set_cameras(cams, H, W)
    e.upload_masks(masks)
    if frames is not None:
        e.upload_frame(color_cam, frames[color_cam])


def _compare(e, want, rule, mv, cc=1):
    """Device result under `rule` / min_views `mv` against the restatement's dict, with and without the per-voxel camera bits
    (the second form is the one that may stop visiting cameras early)."""
    for vm in (True, False):
        n = e.carve(min_views=mv, color_cam=cc, footprint=rule, viewmask=vm)
        idx, rgb, seen = e.fetch()
        assert n == want["idx"].size, (rule, mv, vm, n, want["idx"].size)
        assert np.array_equal(idx, want["idx"]), (rule, mv, vm)
        assert np.array_equal(rgb, want["rgb"]) and np.array_equal(seen, want["seen"]), (rule, mv, vm)
        assert np.array_equal(e.fetch_occupancy(), want["occupancy"]), (rule, mv, vm)
        if vm:
            assert np.array_equal(e.fetch_viewmask(), want["viewmask"]), (rule, mv)
    return n


def _check_scene(e, grid, cams, masks, frames, rules, mvs, bounds=None, cc=1, prepared=None):
    """Everything of one scene: the restatement's boxes once, every rule and threshold against the device."""
    oc = fx.oracle_cams(cams)
    pm = masks if prepared is None else prepared
    b = carve_np.DEFAULT_BOUNDS if bounds is None else bounds
    N = grid[0] * grid[1] * grid[2]
    vms = fp.viewmasks_of_rules(np.arange(N, dtype=np.int64), grid, oc, pm, rules, b)
    counts = {}
    for rule, vm in zip(rules, vms):
        for mv in mvs:
            want = fp.carve(grid, oc, pm, rule, frames=frames, min_views=mv, color_cam=cc, bounds=b, viewmask=vm)
            counts[(rule, mv)] = _compare(e, want, rule, mv, cc)
    return counts


@pytest.mark.parametrize("post", [False, True])
def test_real_cameras_64_every_rule(feng, cams, masks, frames, post):
    _setup(feng, (64, 64, 64), cams, masks, frames)
    prepared = masks
    if post:
        feng.set_mask_postfilter([1, 0, 1, 1], [0, 1, 1, 0])
        feng.touch_masks(0)
        flags = list(zip([1, 0, 1, 1], [0, 1, 1, 0]))
        prepared = [postfilter_np.post_filter(m, bool(o), bool(c)) for m, (o, c) in zip(masks, flags)]
        assert any(not np.array_equal(a, b) for a, b in zip(prepared, masks))
    try:
        counts = _check_scene(feng, (64, 64, 64), cams, masks, frames, ALL_RULES, (3, 4), prepared=prepared)
        if post:
            for c in range(4):                                   # the table was made from the filtered bits
                assert np.array_equal(feng.fetch_mask(c) > 0, prepared[c] > 0)
    finally:
        feng.set_mask_postfilter(None, None)
    if not post:
        assert counts[("any", 4)] > fx.expected(64)[2]["survivors"] > counts[(("cover", 256), 4)] > 0
        assert counts[("any", 4)] == 10044 and counts[(("cover", 256), 4)] == 4642       # the issue's probe
    assert counts[("any", 4)] >= counts[(("cover", 1), 4)] >= counts[(("cover", 128), 4)] >= counts[(("cover", 256), 4)]


def test_real_cameras_128(feng, cams, masks, frames):
    _setup(feng, (128, 128, 128), cams, masks, frames)
    oc = fx.oracle_cams(cams)
    for rule, mv in (("any", 4), (("cover", 128), 3)):
        want = fp.carve((128, 128, 128), oc, masks, rule, frames=frames, min_views=mv)
        assert _compare(feng, want, rule, mv) > 0
    assert feng.carve(footprint="all") < fx.expected(128)[2]["survivors"] < feng.carve(footprint="any")


def test_sixteen_ring_cameras_1080p(feng):
    H, W = 1080, 1920
    cams = synthetic.ring_cameras(16, H, W)
    masks = synthetic.ellipsoid_masks(cams, H, W)
    frames = fx.synthetic_frames(16, H, W)
    _setup(feng, (48, 48, 48), cams, masks, frames, color_cam=5)
    counts = _check_scene(feng, (48, 48, 48), cams, masks, frames, ("any", ("cover", 128), "all"), (16, 12), cc=5)
    assert counts[("any", 16)] > counts[("all", 16)]
    assert counts[("any", 16)] > 0


# the one-voxel-thick grids lie in a plane through the figure (an axis of one cell sits at its lower bound)
@pytest.mark.parametrize("grid,bounds", [((40, 72, 24), None), ((8, 130, 9), None),
                                         ((40, 40, 1), (-512.0, 1024.0, -1024.0, 1024.0, -800.0, 512.0)),
                                         ((1, 40, 40), (300.0, 1024.0, -1024.0, 1024.0, -2048.0, 512.0))])
def test_odd_grids(feng, cams, masks, frames, grid, bounds):
    """Words that end mid-wave, span columns, more than 64 iy per column, one-voxel-thick grids (h = 0 on that axis)."""
    _setup(feng, grid, cams, masks, frames, bounds=bounds)
    counts = _check_scene(feng, grid, cams, masks, frames, ("any", ("cover", 64), "all"), (4, 2), bounds=bounds)
    assert counts[("any", 2)] > 0


def test_empty_and_full_masks(feng, cams, masks, frames):
    H, W = masks[0].shape
    grid = (24, 40, 12)
    N = grid[0] * grid[1] * grid[2]
    zero = [np.zeros((H, W), np.uint8)] * 4
    _setup(feng, grid, cams, zero, frames)
    for rule in ("any", "all"):
        assert feng.carve(footprint=rule, min_views=1, viewmask=True) == 0
        assert not feng.fetch_occupancy().any() and not feng.fetch_viewmask().any()
    full = [np.full((H, W), 255, np.uint8)] * 4
    _setup(feng, grid, cams, full, frames)
    counts = _check_scene(feng, grid, cams, full, frames, ("any", "all"), (4, 1))
    assert 0 < counts[("all", 4)] <= counts[("any", 4)] <= N


@pytest.mark.parametrize("seed,H,W", [(21, 37, 53), (22, 61, 45)])
def test_hostile_cameras_inside_the_volume(feng, seed, H, W):
    """Corners behind, beside and at the camera centres (NaN / inf projections); H W is no multiple of 8 or 64."""
    assert (H * W) % 8 != 0
    cams, masks, frames = _hostile_cameras(seed, C=4, H=H, W=W)                  # two of them with overflowing intrinsics
    Lx, Ly, Lz = fp.lattices((24, 20, 16))
    uv = np.concatenate([fp.project(np.array(np.meshgrid(Lx, Ly, Lz)).T.reshape(-1, 3), cam) for cam in fx.oracle_cams(cams)])
    assert np.isnan(uv).any() and np.isinf(uv).any()
    grid = (24, 20, 16)
    _setup(feng, grid, cams, masks, frames)
    counts = _check_scene(feng, grid, cams, masks, frames, ("any", ("cover", 100), "all"), (1, 2, 4))
    assert counts[("any", 1)] > 0
    # all cameras at one lattice point: that corner's camera-frame coordinates are zero to rounding, its neighbours' tiny
    from voxcarve.camera import Camera
    at = np.array([Lx[7], Ly[9], Lz[5]])
    cams2 = [Camera(c.K, c.dist, c.rvec, -(c.R @ at), R=c.R) for c in cams]
    _setup(feng, grid, cams2, masks, frames)
    _check_scene(feng, grid, cams2, masks, frames, ("any", "all"), (1, 3))


def test_slot_reuse_and_the_centre_carve_is_untouched(feng, cams, masks, frames):
    _setup(feng, (64, 64, 64), cams, masks, frames)
    idx, bgr, summary = fx.expected(64)
    oc = fx.oracle_cams(cams)

    def centre_equals_golden():
        for mode in ("fused",):
            assert feng.carve(mode=mode) == summary["survivors"]
            i, rgb, seen = feng.fetch()
            assert np.array_equal(i, idx) and np.array_equal(rgb[:, ::-1], bgr) and seen.all()

    centre_equals_golden()
    first = feng.carve(footprint="any")
    centre_equals_golden()
    feng.build_lut()
    assert feng.carve(mode="lut") == summary["survivors"] and np.array_equal(feng.fetch()[0], idx)
    # new masks in the same slot: the table is rebuilt
    moved = [np.roll(m, 9, axis=1) for m in masks]
    feng.upload_masks(moved)
    want = fp.carve((64, 64, 64), oc, moved, "any", frames=frames)
    _compare(feng, want, "any", 4)
    assert not np.array_equal(want["idx"], np.zeros(0)) and want["idx"].size != first
    feng.upload_masks(masks)
    assert feng.carve(footprint="any") == first
    centre_equals_golden()


def test_two_slabs_concatenate(feng, cams, masks, frames):
    grid = (40, 72, 24)
    _setup(feng, grid, cams, masks, frames)
    oc = fx.oracle_cams(cams)
    whole = fp.carve(grid, oc, masks, ("cover", 64), frames=frames, min_views=3)
    feng.carve(footprint=("cover", 64), min_views=3)
    rec_whole = feng.fetch_records().copy()
    parts, vms = [], []
    for z0, z1 in ((0, 11), (11, 24)):
        feng.set_slab(z0, z1)
        feng.carve(footprint=("cover", 64), min_views=3, viewmask=True)
        parts.append(feng.fetch_records().copy())
        vms.append(feng.fetch_viewmask().copy())
    feng.set_slab(0, 24)
    assert np.array_equal(np.concatenate(parts), rec_whole)
    assert np.array_equal((rec_whole & np.uint64(0xffffffff)).astype(np.uint32), whole["idx"])
    assert np.array_equal(np.concatenate(vms), whole["viewmask"])
    assert parts[0].size and parts[1].size


def test_downstream_passes_on_an_any_hull(built, cams, masks, frames):
    """filter_components, color_visible, render, marching_cubes(volume=None), surface_mesh: each equals its own restatement fed
    with the footprint hull's records / occupancy (the checks of their own test modules, after a footprint carve)."""
    import voxcarve
    import components_np as cn
    import visible_np as vn
    from oracle import marching_np as mc
    from test_gpu_components import _check as check_components
    from test_gpu_render import _check as check_render
    from test_gpu_surface import _check as check_surface
    grid = (64, 64, 64)
    H, W = masks[0].shape
    oc = fx.oracle_cams(cams)
    want = fp.carve(grid, oc, masks, "any", frames=frames)
    with voxcarve.CarveEngine(0) as e:
        _setup(e, grid, cams, masks)
        for c, f in enumerate(frames):
            e.upload_frame(c, f)
        assert e.carve(footprint="any") == want["idx"].size
        assert np.array_equal(e.fetch()[0], want["idx"])
        # marching cubes on the carve's own occupancy
        occ = e.fetch_occupancy()
        assert np.array_equal(occ, want["occupancy"])
        for axes in ("reference", "grid"):
            v, f = e.marching_cubes(level=0.0, axes=axes)
            wv, wf = mc.extract(occ.reshape(grid), 0.0)
            assert np.array_equal(v, wv) and np.array_equal(f, wf), axes
        # surface mesh: the centre rule brackets fewer edges of this hull, the others stay at the midpoint
        got = check_surface(e, cams, 4, 8)
        assert got["stats"]["unrefined"] > 0 and got["stats"]["refined"] > 0
        # render
        check_render(e, cams, H, W)
        # colour by visibility
        rec0 = e.fetch_records().copy()
        e.color_visible()
        idx = (rec0 & 0xffffffff).astype(np.uint32)
        rgb0 = np.stack([(rec0 >> np.uint64(k)) & np.uint64(0xff) for k in (32, 40, 48)], axis=1).astype(np.uint8)
        zmaps, vis, rgb = vn.color_visible(idx, rgb0, e.grid, e.bounds, oc, frames, H, W, None)
        wrec = (rec0 & np.uint64(0xff000000ffffffff)) | (rgb[:, 0].astype(np.uint64) << np.uint64(32)) | \
            (rgb[:, 1].astype(np.uint64) << np.uint64(40)) | (rgb[:, 2].astype(np.uint64) << np.uint64(48))
        assert np.array_equal(e.fetch_visibility(), vis) and np.array_equal(e.fetch_records(), wrec)
        # components, then the photo carve on what is left
        e.carve(footprint="any")
        w, st = check_components(e, 26, 0, 1)
        assert st["components"] >= 1 and st["survivors_after"] <= want["idx"].size
        e.carve(footprint="any")
        st = e.photo_carve(var_threshold=1200)
        assert st["survivors_before"] == want["idx"].size
        # the exchange form: packed entries expand to the same records
        e.carve(footprint="any")
        rec = e.fetch_records().copy()
        ent = e.pack_entries()
        assert e.expand_entries(ent) == rec.size and np.array_equal(e.fetch_gathered(), rec)


def _raw_words(e):
    raw = np.empty((e.n_voxels + 63) // 64, dtype=np.uint64)
    e._check(e._L.vc_fetch_occupancy(e._ctx, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))), "vc_fetch_occupancy")
    return raw


def test_1024_cubed(feng, cams, masks, frames):
    grid = (1024, 1024, 1024)
    _setup(feng, grid, cams, masks, frames)
    n_centre = feng.carve(records=False)
    w_centre = _raw_words(feng)
    n_all = feng.carve(footprint="all", records=False)
    w_all = _raw_words(feng)
    n_any = feng.carve(footprint="any", viewmask=True)
    w_any = _raw_words(feng)
    assert not (w_centre & ~w_any).any() and not (w_all & ~w_centre).any()
    assert n_any > n_centre > n_all > 0
    idx = feng.fetch()[0]
    assert idx.size == n_any and np.all(idx[1:] > idx[:-1])
    assert np.array_equal(np.flatnonzero(np.unpackbits(w_any[:4096].view(np.uint8), bitorder="little")), idx[idx < 4096 * 64])
    vm = feng.fetch_viewmask()
    rng = np.random.default_rng(1024)
    hull = idx[rng.integers(0, idx.size, 1024)].astype(np.int64)             # voxels of the hull and around it, and anywhere
    near = np.clip(hull + rng.integers(-3, 4, hull.size) * 1024 + rng.integers(-3, 4, hull.size), 0, 2 ** 30 - 1)
    pick = np.concatenate([hull, near, rng.integers(0, 2 ** 30, 2048)])
    busy = np.flatnonzero(w_any)
    words = np.concatenate([busy[rng.integers(0, busy.size, 6)], rng.integers(0, 2 ** 24, 2)])
    pick = np.unique(np.concatenate([pick] + [np.arange(64, dtype=np.int64) + 64 * int(w) for w in words]))
    assert pick.size >= 4096
    want = fp.viewmasks(pick, grid, fx.oracle_cams(cams), masks, "any")
    assert np.array_equal(vm[pick], want)
    assert (want == 0xf).sum() > 1000
    del vm


def test_refusals(built, cams, masks, frames):
    import voxcarve
    H, W = masks[0].shape

    def raw(e, slot=0, mv=4, cc=1, rule=_lib.VC_FOOT_ANY, q=0, flags=0, out=True):
        n = ctypes.c_uint64(123)
        rc = e._L.vc_carve_footprint(e._ctx, slot, mv, cc, rule, q, flags, ctypes.byref(n) if out else None)
        if out and rc != 0:
            assert n.value == 0
        return rc, _lib.load().vc_last_error(e._ctx).decode()

    with voxcarve.CarveEngine(0) as e:
        rc, msg = raw(e)
        assert rc == -1 and "grid and cameras" in msg                                # nothing set
        e.set_grid(32, 32, 32)
        assert raw(e)[0] == -1                                                       # no cameras
        e.set_cameras(cams, H, W)
        rc, msg = raw(e)
        assert rc == -1 and "no masks" in msg
        e.upload_masks(masks)
        e.upload_frame(1, frames[1])
        rc, msg = raw(e, slot=3)
        assert rc == -1 and "slot 3" in msg
        assert raw(e, out=False)[0] == -1
        n0 = e.carve()
        rec0 = e.fetch_records().copy()
        for kw, word in ((dict(rule=0), "rule"), (dict(rule=3), "rule"), (dict(rule=_lib.VC_FOOT_COVER, q=0), "1..256"),
                         (dict(rule=_lib.VC_FOOT_COVER, q=257), "1..256"), (dict(flags=4), "flags"), (dict(cc=4), "colour camera")):
            rc, msg = raw(e, **kw)
            assert rc == -1 and word in msg, (kw, msg)
            assert np.array_equal(e.fetch_records(), rec0)                           # nothing launched: the result stands
        e.carve_begin()
        rc, msg = raw(e)
        assert rc == -1 and "in flight" in msg
        assert e.carve_end() == n0
        assert raw(e)[0] == 0 and raw(e, rule=_lib.VC_FOOT_COVER, q=256)[0] == 0 and raw(e, rule=_lib.VC_FOOT_COVER, q=1)[0] == 0
        assert raw(e, mv=5)[0] == 0                                                  # above C: legal, empty
        for bad in ("center", ("cover", 0), ("cover", 257), ("cover", 2.5), ("any", 3), None):
            with pytest.raises(ValueError):
                e.carve(footprint=bad)
        t = e.timing()
        assert "work" in t and "foot_projections" in t["work"]


def test_work_counters_and_kernel_times(built, cams, masks, frames):
    import voxcarve
    with voxcarve.CarveEngine(0) as e:
        _setup(e, (128, 128, 128), cams, masks, frames)
        e.set_option("timing_detail", 1)
        e.carve(footprint="any")
        e.timing(reset=True)
        e.carve(footprint="any")
        t = e.timing()
        words = 128 ** 3 // 64
        assert t["work"]["foot_words"] == words
        assert 0 < t["work"]["foot_union_skips"] <= 4 * words
        # at most (5 per voxel + 4 per word) per camera, at least one camera's worth
        assert 128 ** 3 * 5 <= t["work"]["foot_projections"] <= 4 * (128 ** 3 * 5 + 4 * words)
        assert t["kernels"]["k_carve_foot"]["launches"] == 1 and t["kernels"]["k_carve_foot"]["ms_sum"] > 0
        assert "foot_table" not in t["kernels"]                                      # cached: the slot was not prepared again
        e.touch_masks(0)
        e.carve(footprint="any")
        assert e.timing()["kernels"]["foot_table"]["launches"] == 1


def test_assignment_and_demo(built, cams, masks, frames, tmp_path):
    from voxcarve import assignment
    from voxcarve.engine import viewer_colors, viewer_positions, voxel_keys
    saved = dict(assignment._settings)
    with pytest.raises(ValueError):
        assignment.configure(footprint="some")
    assignment.configure(frame_source=assignment.StaticFrameSource([(frames, masks)]), data_path=fx.GOLDEN + "/data", footprint="any")
    try:
        pos, col = assignment.set_voxel_positions(64, 32, 64)
        e = assignment._engine
        want = fp.carve((64, 64, 64), fx.oracle_cams(cams), masks, "any", frames=frames)
        keys = voxel_keys(want["idx"], e.grid, e.axes())
        assert np.array_equal(pos, viewer_positions(keys)) and np.array_equal(col, viewer_colors(want["rgb"]))
        assert len(pos) == 10044
    finally:
        assignment.configure(frame_source=None, **saved)
    assert assignment._settings["footprint"] == "centre"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for rule, count in (("any", 10044), ("all", 4642), ("centre", 6981)):
        r = subprocess.run([sys.executable, os.path.join(root, "scripts", "demo.py"), "64", "-", "--footprint", rule], cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.startswith("%d voxels" % count), r.stdout
