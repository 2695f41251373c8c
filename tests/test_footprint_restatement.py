"""CPU checks of the footprint carve's restatement (tests/footprint_np.py): the vectorised form against the literal one, the
chain any >= centre >= all against the reference rule (oracle/carve_np.carve), and what the rule is worth on a rod that is
thinner than a voxel."""
import numpy as np
import pytest

import components_np
import fixtures_util as fx
import footprint_np as fp
from oracle import carve_np

RULES = ("any", "all", ("cover", 96))


def _hostile_cameras(seed, C=3, H=37, W=53):
    """random_scene's cameras moved INSIDE the default volume: voxels behind, beside and at the camera centre.  The last two
    also get intrinsics that overflow: fx = 1e308 (u = +-inf wherever |x'| > 1) and k1 = -k2 = 1e308 (inf - inf = NaN wherever
    r^2 is not small), so that boxes are built from inf and NaN corners next to finite ones."""
    from voxcarve.camera import Camera
    cams, masks, frames = fx.random_scene(seed, C=C, H=H, W=W, fg=0.5)
    rng = np.random.default_rng(seed + 77)
    b = carve_np.DEFAULT_BOUNDS
    out = []
    for c in cams:
        centre = np.array([rng.uniform(b[0], b[1]), rng.uniform(b[2], b[3]), rng.uniform(b[4], b[5])])
        out.append(Camera(c.K, c.dist, c.rvec, -(c.R @ centre), R=c.R))
    K = out[-1].K.copy()
    K[0, 0] = 1e308
    out[-1] = Camera(K, out[-1].dist, out[-1].rvec, out[-1].tvec, R=out[-1].R)
    dist = out[-2].dist.copy()
    dist[0], dist[1] = 1e308, -1e308
    out[-2] = Camera(out[-2].K, dist, out[-2].rvec, out[-2].tvec, R=out[-2].R)
    return out, masks, frames


@pytest.mark.parametrize("seed,grid", [(1, (5, 6, 4)), (2, (3, 7, 5)), (3, (6, 2, 3))])
def test_vectorised_equals_literal(seed, grid):
    cams, masks, frames = fx.random_scene(seed)
    oc = fx.oracle_cams(cams)
    for rule in RULES:
        for mv in (len(cams), len(cams) - 1):
            got = fp.carve(grid, oc, masks, rule, frames=frames, min_views=mv, color_cam=1)
            idx, vm, rgb, seen = fp.carve_literal(grid, oc, masks, rule, frames=frames, min_views=mv, color_cam=1)
            assert np.array_equal(got["viewmask"], vm), (rule, mv)
            assert np.array_equal(got["idx"], idx), (rule, mv)
            assert np.array_equal(got["rgb"], rgb) and np.array_equal(got["seen"], seen), (rule, mv)
    assert fp.carve(grid, oc, masks, "any", min_views=len(cams) - 1)["idx"].size > 0


def test_vectorised_equals_literal_hostile():
    cams, masks, frames = _hostile_cameras(11)
    oc = fx.oracle_cams(cams)
    grid = (6, 5, 4)
    for rule in RULES:
        got = fp.carve(grid, oc, masks, rule, frames=frames, min_views=1, color_cam=0)
        idx, vm, rgb, seen = fp.carve_literal(grid, oc, masks, rule, frames=frames, min_views=1, color_cam=0)
        assert np.array_equal(got["viewmask"], vm) and np.array_equal(got["idx"], idx), rule
        assert np.array_equal(got["rgb"], rgb) and np.array_equal(got["seen"], seen), rule


def test_cover_256_is_all_and_rules_are_validated():
    cams, masks, _ = fx.random_scene(5)
    oc = fx.oracle_cams(cams)
    a = fp.carve((6, 6, 6), oc, masks, "all", min_views=1)
    b = fp.carve((6, 6, 6), oc, masks, ("cover", 256), min_views=1)
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["viewmask"], b["viewmask"])
    for bad in ("centre", ("cover", 0), ("cover", 257), ("cover", 1.5), ("any", 1)):
        with pytest.raises(ValueError):
            fp.normalise_rule(bad)


@pytest.mark.parametrize("grid", [(1, 1, 1), (1, 4, 3), (4, 1, 1)])
def test_degenerate_axes(grid):
    """n == 1 on an axis: h = 0, the cell collapses on that axis, the rules still run (and agree with the literal form)."""
    cams, masks, frames = fx.random_scene(6)
    oc = fx.oracle_cams(cams)
    L = fp.lattices(grid)
    for a in range(3):
        assert L[a].size == grid[a] + 1
        if grid[a] == 1:
            assert L[a][0] == L[a][1] == carve_np.DEFAULT_BOUNDS[2 * a]
    for rule in RULES:
        got = fp.carve(grid, oc, masks, rule, frames=frames, min_views=1)
        idx, vm, rgb, seen = fp.carve_literal(grid, oc, masks, rule, frames=frames, min_views=1)
        assert np.array_equal(got["viewmask"], vm) and np.array_equal(got["idx"], idx), rule


def test_lattice_neighbours_share_corners():
    Lx, Ly, Lz = fp.lattices((64, 64, 64))
    xs, ys, zs = carve_np.axis_tables(64, 64, 64)
    for L, c in ((Lx, xs), (Ly, ys), (Lz, zs)):
        assert np.all(np.diff(L) > 0) and np.all(L[:-1] < c) and np.all(c < L[1:])


def test_projection_is_the_carves_own(cams):
    """footprint_np.project == oracle/carve_np.project_points bit for bit wherever the latter is finite."""
    pts = carve_np.create_voxel_volume(16, 16, 16)
    for cam in fx.oracle_cams(cams) + fx.oracle_cams(_hostile_cameras(12)[0]):
        K, dist, R, t = cam
        want = carve_np.project_points(pts, R, t, K, dist)
        got = fp.project(pts, cam)
        fin = np.isfinite(want).all(axis=1)
        assert fin.any() and np.array_equal(got[fin], want[fin])
        assert not np.isfinite(got[~fin]).all(axis=1).any()


def _chain(grid, oc, masks):
    N = grid[0] * grid[1] * grid[2]
    centre = carve_np.carve(*grid, oc, masks, min_views=1)["viewmask"]
    idx = np.arange(N, dtype=np.int64)
    any_vm = fp.viewmasks(idx, grid, oc, masks, "any")
    all_vm = fp.viewmasks(idx, grid, oc, masks, "all")
    assert not (centre & ~any_vm).any(), "centre is not inside any"
    assert not (all_vm & ~centre).any(), "all is not inside centre"
    return any_vm, centre, all_vm


def test_chain_real_cameras_64(cams, masks):
    """Per camera and per voxel any >= centre >= all, hence for every min_views; strict for the all-cameras hull."""
    any_vm, centre, all_vm = _chain((64, 64, 64), fx.oracle_cams(cams), masks)
    full = np.uint16(0xf)
    n_any, n_centre, n_all = [int((v == full).sum()) for v in (any_vm, centre, all_vm)]
    assert n_centre == fx.expected(64)[2]["survivors"]
    assert n_any > n_centre > n_all > 0, (n_any, n_centre, n_all)


def test_chain_hostile_cameras():
    cams, masks, _ = _hostile_cameras(21, C=4)
    oc = fx.oracle_cams(cams)
    grid = (24, 20, 16)
    Lx, Ly, Lz = fp.lattices(grid)
    corners = np.array(np.meshgrid(Lx, Ly, Lz)).T.reshape(-1, 3)
    behind = sum(int((np.asarray(cam[2])[2] @ corners.T + np.asarray(cam[3]).reshape(3)[2] < 0).sum()) for cam in oc)
    assert behind > 0, "no corner lies behind a camera"
    uv = np.concatenate([fp.project(corners, cam) for cam in oc])
    assert np.isnan(uv).any() and np.isinf(uv).any() and np.isfinite(uv).any()
    any_vm, centre, all_vm = _chain(grid, oc, masks)
    assert any_vm.any()


# ----------------------------------------------------------------------------------------------- what it is worth
ROD_X, ROD_Y, ROD_Z0, ROD_Z1, ROD_R = 256.0, 0.0, -1400.0, -200.0, 4.0


def _rod_masks(oc, H, W):
    """Noise-free masks of a vertical rod 8 mm across: the pixels its sample points project to."""
    z = np.arange(ROD_Z0, ROD_Z1 + 0.25, 0.5)
    ang = np.arange(24) * (2 * np.pi / 24)
    ring = [(0.0, 0.0)] + [(r * np.cos(a), r * np.sin(a)) for r in (ROD_R / 2, ROD_R) for a in ang]
    pts = np.concatenate([np.stack([np.full_like(z, ROD_X + dx), np.full_like(z, ROD_Y + dy), z], axis=1) for dx, dy in ring])
    masks = []
    for K, dist, R, t in oc:
        off = carve_np.pixel_offsets(carve_np.project_points(pts, R, t, K, dist), H, W)
        m = np.zeros(H * W, dtype=np.uint8)
        m[off[off >= 0]] = 255
        masks.append(m.reshape(H, W))
    return masks


def _rod_layers(n):
    zs = carve_np.axis_tables(n, n, n)[2]
    return np.flatnonzero((zs >= ROD_Z0 + 30.0) & (zs <= ROD_Z1 - 30.0))


def _layers_of(idx, n):
    return np.unique(np.asarray(idx, dtype=np.int64) // (n * n))


@pytest.fixture(scope="module")
def rod(cams, masks):
    oc = fx.oracle_cams(cams)
    return oc, _rod_masks(oc, *masks[0].shape)


def test_rod_64(rod):
    """Probe of the issue: 0 / 124 voxels, 0 % / 100 % of the layers, "all" keeps none, one 26-connected component."""
    oc, rm = rod
    grid = (64, 64, 64)
    layers = _rod_layers(64)
    assert layers.size > 10
    centre = carve_np.carve(*grid, oc, rm)["idx"]
    got = fp.carve(grid, oc, rm, "any", color_cam=None)["idx"]
    print("rod 64^3: centre %d voxels, any %d voxels in %d of %d layers" % (centre.size, got.size,
                                                                           np.intersect1d(_layers_of(got, 64), layers).size, layers.size))
    assert np.intersect1d(_layers_of(centre, 64), layers).size == 0
    assert np.isin(layers, _layers_of(got, 64)).all()
    assert fp.carve(grid, oc, rm, "all", color_cam=None)["idx"].size == 0
    comp = components_np.components(got, grid, connectivity=26)
    assert comp["size"].size == 1 and int(comp["size"][0]) == got.size


def test_rod_128(rod):
    """Probe of the issue: the centre rule reaches 25 % of the rod's layers, "any" every one.  "any" is evaluated for the
    columns within 6 cells of the rod only (existence there is existence in the hull; the whole grid costs ~25 s)."""
    oc, rm = rod
    n = 128
    layers = _rod_layers(n)
    centre = carve_np.carve(n, n, n, oc, rm)["idx"]
    reached = np.intersect1d(_layers_of(centre, n), layers).size
    xs, ys, _ = carve_np.axis_tables(n, n, n)
    ix0, iy0 = int(np.argmin(np.abs(xs - ROD_X))), int(np.argmin(np.abs(ys - ROD_Y)))
    ix, iy, iz = np.meshgrid(np.arange(ix0 - 6, ix0 + 7), np.arange(iy0 - 6, iy0 + 7), np.arange(n), indexing="ij")
    cand = np.sort((iz * n * n + ix * n + iy).reshape(-1)).astype(np.int64)
    vm = fp.viewmasks(cand, (n, n, n), oc, rm, "any")
    got = cand[vm == 0xf]
    print("rod 128^3: centre %d voxels in %d of %d layers, any %d voxels near the rod" % (centre.size, reached, layers.size, got.size))
    assert 2 * reached < layers.size
    assert np.isin(layers, _layers_of(got, n)).all()
    assert np.isin(centre, got).all()


def test_interface_without_a_gpu(built):
    """The export, its constants and the host-side validation (no device needed)."""
    from voxcarve import _lib, assignment
    from voxcarve.engine import footprint_rule
    lib = _lib.load()
    assert hasattr(lib, "vc_carve_footprint") and "vc_carve_footprint" in _lib.SIGNATURES
    assert footprint_rule("centre") is None
    assert footprint_rule("any") == (_lib.VC_FOOT_ANY, 0)
    assert footprint_rule("all") == (_lib.VC_FOOT_COVER, 256) == footprint_rule(("cover", 256))
    assert footprint_rule(("cover", np.int64(7))) == (_lib.VC_FOOT_COVER, 7)
    for bad in ("center", "ANY", ("cover", 0), ("cover", 257), ("cover", 1.0), ("cover", True), ("all", 1), ("cover",), None, 3):
        with pytest.raises(ValueError):
            footprint_rule(bad)
    saved = dict(assignment._settings)
    try:
        with pytest.raises(ValueError):
            assignment.configure(footprint="some")
        assert assignment._settings["footprint"] == "centre"
        assignment.configure(footprint=("cover", 128))
        assert assignment._settings["footprint"] == ("cover", 128)
    finally:
        assignment.configure(frame_source=None, **saved)
    header = open(fx.ROOT + "/include/voxcarve.h").read()
    assert "VC_FOOT_ANY = 1u" in header and "VC_FOOT_COVER = 2u" in header and "#define VC_KERNEL_KINDS %d" % _lib.VC_KERNEL_KINDS in header
    assert len(_lib.KERNEL_KINDS) == _lib.VC_KERNEL_KINDS and len(_lib.WORK_KINDS) <= _lib.VC_WORK_KINDS
