"""The restatement of the hull's shell (tests/shell_np.py; contract of vc_hull_shell in include/voxcarve.h) against its own literal
form on random grids, against counts pinned from the committed fixtures, against the independent restatement of the
measurements, against the ray walk of the render contract ("what a ray can hit is in the shell"), and against the host's viewer
arithmetic; then the interface: the header, the ctypes mirrors, the Makefile, the drop-in layer's settings."""
import ctypes
import os
import re

import numpy as np
import pytest

import fixtures_util as fx
import measure_np as mn
import render_np as rn
import shell_np as sn

LEVELS = (0, 1, 2, 3, 6)
GRIDS = ((13, 70, 9), (33, 31, 17), (5, 64, 3), (1, 1, 1))
# the shell of the committed fixtures (real cameras, 64^3 and 128^3): T and the face counts at level 0, (cells_on, T) above it
PINS = {64: {"survivors": 6981, 0: (2703, [772, 772, 864, 864, 856, 856]), 1: (1178, 652), 2: (231, 170), 3: (49, 43)},
        128: {"survivors": 57048, 0: (12462, [3228, 3228, 3691, 3691, 3681, 3681]), 1: (8476, 3046), 2: (1394, 720), 3: (263, 183)}}


def _random_records(rng, grid, fill):
    nx, ny, nz = grid
    idx = np.flatnonzero(rng.random(nx * ny * nz) < fill)
    return mn.pack_records(idx, rng.integers(0, 256, (idx.size, 3)), rng.random(idx.size) < 0.7)


def _fixture_records(n):
    idx, bgr, _ = fx.expected(n)
    return mn.pack_records(idx, bgr[:, ::-1])


def _axes(grid, bounds):
    return [np.linspace(bounds[2 * a], bounds[2 * a + 1], num=grid[a]) for a in range(3)]


@pytest.fixture(scope="module")
def shells64():
    rec = _fixture_records(64)
    return rec, {L: sn.shell(rec, (64, 64, 64), L) for L in (0, 1, 2, 3)}


@pytest.mark.parametrize("grid", GRIDS)
def test_vectorised_equals_literal(grid):
    n = grid[0] * grid[1] * grid[2]
    cases = [_random_records(np.random.default_rng(seed), grid, fill) for seed, fill in ((1, 0.6), (2, 0.1), (3, 0.93))]
    cases.append(mn.pack_records(np.arange(n), np.full((n, 3), 200), np.arange(n) % 3 != 0))     # the full grid
    cases.append(mn.pack_records(np.zeros(0, np.int64)))                                        # the empty one
    for rec in cases:
        for L in LEVELS:
            a = sn.shell(rec, grid, L)
            sn.same(a, sn.shell_literal(rec, grid, L))
            st = a["stats"]
            assert st["dims"] == [-(-v // (1 << L)) for v in grid] and st["cube_scale"] == 1 << L and st["survivors"] == rec.size
            assert st["shell"] == a["records"].size <= st["cells_on"] <= rec.size
            assert (a["faces"] != 0).all() and (np.diff(a["records"] & np.uint64(0xffffffff)).astype(np.int64) > 0).all()
            assert (st["cells_on"] == 0) == (rec.size == 0)
        if rec.size and max(grid) <= 64:                         # one coarse cell remains at level 6
            top = sn.shell(rec, grid, 6)
            assert top["stats"]["shell"] == 1 == top["stats"]["cells_on"] and top["faces"].tolist() == [63]
    for bad in (-1, 7):
        with pytest.raises(ValueError):
            sn.shell(cases[0], grid, bad)
        with pytest.raises(ValueError):
            sn.shell_literal(cases[0], grid, bad)


def test_full_grid_by_hand():
    """Every voxel ON: the shell is the border layer, the faces are exactly the border bits; colours average over the seen."""
    grid = (16, 66, 8)
    n = 16 * 66 * 8
    rec = mn.pack_records(np.arange(n), np.full((n, 3), (10, 20, 31)), np.ones(n))
    a = sn.shell(rec, grid, 0)
    assert a["stats"]["shell"] == n - 14 * 64 * 6 and a["stats"]["faces"] == [66 * 8, 66 * 8, 16 * 8, 16 * 8, 16 * 66, 16 * 66]
    i = (a["records"] & np.uint64(0xffffffff)).astype(np.int64)
    iy, ix, iz = i % 66, (i // 66) % 16, i // (16 * 66)
    want = ((ix == 0) * 1 + (ix == 15) * 2 + (iy == 0) * 4 + (iy == 65) * 8 + (iz == 0) * 16 + (iz == 7) * 32).astype(np.uint8)
    assert np.array_equal(a["faces"], want)
    assert np.array_equal(a["records"] >> np.uint64(32), rec[i] >> np.uint64(32))
    b = sn.shell(rec, grid, 1)                                   # 8 x 33 x 4 cells, all ON
    assert b["stats"]["cells_on"] == 8 * 33 * 4 and b["stats"]["shell"] == 8 * 33 * 4 - 6 * 31 * 2
    assert set((b["records"] >> np.uint64(32)).tolist()) == {10 | 20 << 8 | 31 << 16 | 1 << 24}
    c = sn.shell(rec, grid, 6)                                   # 1 x 2 x 1 cells
    assert c["stats"]["dims"] == [1, 2, 1] and c["faces"].tolist() == [63 - 8, 63 - 4]
    one = sn.shell(mn.pack_records([1234]), grid, 0)
    assert one["faces"].tolist() == [63] and one["records"].tolist() == mn.pack_records([1234]).tolist()


def test_no_wrap_around_between_rows_and_layers():
    grid = (2, 3, 2)
    rec = mn.pack_records([2, 3, 5, 6])                          # (0, 2, 0), (1, 0, 0), (1, 2, 0), (0, 0, 1)
    for f in (sn.shell, sn.shell_literal):
        a = f(rec, grid, 0)
        assert a["faces"].tolist() == [63 - 2, 63, 63 - 1, 63] and a["stats"]["faces"] == [3, 3, 4, 4, 4, 4]


def test_rounded_means_and_unseen_cells():
    grid = (4, 4, 4)
    # cell (0, 0, 0) of level 1: three seen voxels and one unseen; cell (1, 1, 1): unseen voxels only
    idx = [0, 1, 4, 5, (2 * 4 + 2) * 4 + 2, (3 * 4 + 3) * 4 + 3]
    rgb = [(1, 2, 250), (2, 2, 251), (2, 3, 255), (99, 99, 99), (7, 7, 7), (8, 8, 8)]
    rec = mn.pack_records(idx, rgb, [1, 1, 1, 0, 0, 0])
    for f in (sn.shell, sn.shell_literal):
        a = f(rec, grid, 1)
        assert a["stats"]["cells_on"] == 2 and a["stats"]["shell"] == 2
        r = [int(v) for v in a["records"]]
        assert r[0] == 0 | ((5 + 1) // 3) << 32 | ((7 + 1) // 3) << 40 | ((756 + 1) // 3) << 48 | 1 << 56
        assert r[1] == (1 * 2 + 1) * 2 + 1                       # bytes 4..7 are 0, 0, 0, 0
        assert a["faces"].tolist() == [63, 63]


@pytest.mark.parametrize("n", [64, 128])
def test_fixture_pins(n):
    rec = _fixture_records(n)
    grid = (n, n, n)
    pin = PINS[n]
    assert rec.size == pin["survivors"]
    a = sn.shell(rec, grid, 0)
    assert (a["stats"]["shell"], a["stats"]["faces"]) == pin[0] and a["stats"]["cells_on"] == rec.size
    # the independent restatement of the measurements counts the same surface and the same faces
    m = mn.measure(rec, grid, np.zeros(rec.size, np.uint32), 1)
    assert int(m["surface"][0]) == a["stats"]["shell"] and m["faces"][0].tolist() == a["stats"]["faces"]
    fine = set((a["records"] & np.uint64(0xffffffff)).tolist())
    for L in (1, 2, 3):
        b = sn.shell(rec, grid, L)
        assert (b["stats"]["cells_on"], b["stats"]["shell"]) == pin[L]
        # every coarse shell cell holds a level-0 shell voxel
        i = (a["records"] & np.uint64(0xffffffff)).astype(np.int64)
        d = b["stats"]["dims"]
        cj = (((i // (n * n)) >> L) * d[0] + (((i // n) % n) >> L)) * d[1] + ((i % n) >> L)
        assert set((b["records"] & np.uint64(0xffffffff)).tolist()) <= set(cj.tolist())
    if n == 64:
        sn.same(a, sn.shell_literal(rec, grid, 0))
        sn.same(sn.shell(rec, grid, 2), sn.shell_literal(rec, grid, 2))
    assert len(fine) == pin[0][0]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_coarse_shell_cell_holds_a_fine_shell_voxel(seed):
    rng = np.random.default_rng(seed)
    for grid in GRIDS[:3]:
        for fill in (0.05, 0.5, 0.97, 1.0):
            rec = _random_records(rng, grid, fill)
            nx, ny, nz = grid
            i = (sn.shell(rec, grid, 0)["records"] & np.uint64(0xffffffff)).astype(np.int64)
            for L in (1, 2, 3):
                b = sn.shell(rec, grid, L)
                d = b["stats"]["dims"]
                cj = (((i // (nx * ny)) >> L) * d[0] + (((i // ny) % nx) >> L)) * d[1] + ((i % ny) >> L)
                assert set((b["records"] & np.uint64(0xffffffff)).tolist()) <= set(cj.tolist())


@pytest.mark.parametrize("c", [0, 1, 2, 3])
def test_what_a_ray_can_hit_is_in_the_shell(shells64, cams, masks, c):
    """The four real cameras at 64^3 (one per case): every voxel the render contract's walk returns is a level-0 shell voxel,
    and the face the ray enters through is exposed."""
    from voxcarve.engine import DEFAULT_BOUNDS
    rec, shells = shells64
    grid = (64, 64, 64)
    occ = np.zeros(64 ** 3, dtype=bool)
    occ[(rec & np.uint64(0xffffffff)).astype(np.int64)] = True
    face_of = np.zeros(64 ** 3, dtype=np.uint8)
    face_of[(shells[0]["records"] & np.uint64(0xffffffff)).astype(np.int64)] = shells[0]["faces"]
    H, W = masks[0].shape
    o, d = rn.pixel_rays(rn.view_params(cams[c]), H, W)
    idx, _, face = rn.walk_voxels(occ, grid, DEFAULT_BOUNDS, o, d)
    hit = idx != rn.MISS
    assert int(hit.sum()) > 1000
    assert (face_of[idx[hit].astype(np.int64)] != 0).all()
    entered = hit & (face < 6)
    assert entered.any() and ((face_of[idx[entered].astype(np.int64)] >> face[entered]) & 1).all()


def test_level0_viewer_arrays_are_the_hosts(shells64):
    from voxcarve.engine import DEFAULT_BOUNDS, unpack_records, viewer_colors, viewer_positions, voxel_keys
    _, shells = shells64
    grid = (64, 64, 64)
    axes = _axes(grid, DEFAULT_BOUNDS)
    rec = shells[0]["records"]
    idx, rgb, _ = unpack_records(rec)
    pos, col = sn.viewer(rec, grid, axes)
    sn.same_bits(pos, viewer_positions(voxel_keys(idx, grid, axes)))
    sn.same_bits(col, viewer_colors(rgb))
    lp, lc = sn.viewer_literal(rec[::7], grid, axes)
    sn.same_bits(lp, pos[::7])
    sn.same_bits(lc, col[::7])
    for L in (1, 3):
        r = shells[L]["records"]
        a, b = sn.viewer(r, grid, axes, L, 64.0), sn.viewer_literal(r, grid, axes, L, 64.0)
        sn.same_bits(a[0], b[0])
        sn.same_bits(a[1], b[1])
    # a grid whose axes cross zero: the negated zero keeps its sign, as -(0 / 64) does on the host
    grid, bounds = (5, 7, 3), (-100.0, 100.0, -30.0, 30.0, -64.0, 64.0)
    axes = _axes(grid, bounds)
    rec = mn.pack_records(np.arange(5 * 7 * 3), np.arange(5 * 7 * 3 * 3).reshape(-1, 3) % 256)
    pos, col = sn.viewer(rec, grid, axes, 0, 64)
    sn.same_bits(pos, viewer_positions(voxel_keys(np.arange(105), grid, axes)))
    sn.same_bits(col, viewer_colors(np.arange(315).reshape(-1, 3) % 256))
    assert np.signbit(pos[:, 1]).any() and (pos[:, 1] == 0).any()


def test_clipped_coarse_cell_sits_at_the_midpoint():
    """13 cells along x at level 2: the last coarse cell covers ix = 12 alone; 70 along y: iy = 68, 69."""
    grid, bounds = (13, 70, 9), (0.0, 768.0, -345.0, 345.0, -640.0, 0.0)
    axes = _axes(grid, bounds)
    d = sn.coarse_dims(grid, 2)
    assert d == (4, 18, 3)
    j = (2 * d[0] + 3) * d[1] + 17                               # cell (3, 17, 2): ix 12, iy 68..69, iz 8
    rec = np.array([j | (255 << 32) | (0 << 40) | (51 << 48) | (1 << 56)], dtype=np.uint64)
    for f in (sn.viewer, sn.viewer_literal):
        pos, col = f(rec, grid, axes, 2, 64.0)
        x = (np.trunc(axes[0][12]) / 64.0 + np.trunc(axes[0][12]) / 64.0) * 0.5
        y = (np.trunc(axes[1][68]) / 64.0 + np.trunc(axes[1][69]) / 64.0) * 0.5
        z = (np.trunc(axes[2][8]) / 64.0 + np.trunc(axes[2][8]) / 64.0) * 0.5
        assert pos.tolist() == [[np.float32(x), np.float32(-z), np.float32(y)]]
        assert col.tolist() == [[np.float32(1.0), np.float32(0.0), np.float32(51 / 255.0)]]
    # an unclipped cell: the midpoint of its first and last voxel
    rec0 = np.array([(1 * d[0] + 1) * d[1] + 2], dtype=np.uint64)
    pos, _ = sn.viewer(rec0, grid, axes, 2, 64.0)
    assert pos[0, 0] == np.float32((np.trunc(axes[0][4]) / 64.0 + np.trunc(axes[0][7]) / 64.0) * 0.5)


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def _struct_fields(header, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", v).strip() for v in decl.split(None, 1)[1].split(",")]
    return names


def test_interface_pins(built):
    from voxcarve import _lib
    header = open(os.path.join(fx.ROOT, "include", "voxcarve.h")).read()
    for name in ("vc_hull_shell", "vc_fetch_shell", "vc_fetch_shell_viewer"):
        assert "int %s(vc_ctx *ctx" % name in header and name in _lib.SIGNATURES
    assert "#define VC_SHELL_MAX_LEVEL 6u" in header and _lib.VC_SHELL_MAX_LEVEL == 6 == sn.MAX_LEVEL
    assert ctypes.sizeof(_lib.VcShellStats) == 3 * 8 + 6 * 8 + 5 * 4 + 4 == 96
    assert [f[0] for f in _lib.VcShellStats._fields_] == _struct_fields(header, "vc_shell_stats_t")
    assert _lib.VcShellStats.faces.offset == 24 and _lib.VcShellStats.dims.offset == 80 and _lib.VcShellStats.shell_ms.offset == 92
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    assert "vc_shell.h" in makefile.split("HEADERS =")[1].split("$(OUT):")[0]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vc_hull_shell", "vc_fetch_shell", "vc_fetch_shell_viewer"):
        assert hasattr(lib, name)
    from voxcarve import CarveEngine
    for name in ("hull_shell", "fetch_shell", "fetch_shell_viewer", "shell_valid"):
        assert callable(getattr(CarveEngine, name))


def test_configure_validates_the_output_settings():
    from voxcarve import assignment
    saved = dict(assignment._settings)
    try:
        assignment.configure(output="shell", output_level=2)
        assert assignment._settings["output"] == "shell" and assignment._settings["output_level"] == 2
        with pytest.raises(RuntimeError, match="no shell"):
            assignment.shell()
        for bad in ({"output": "faces"}, {"output_level": 7}, {"output_level": -1}, {"output_level": True}, {"output_level": 1.0},
                    {"output": "all", "output_level": 1}, {"output": "all"}):
            with pytest.raises(ValueError):
                assignment.configure(**bad)
        assert assignment._settings["output"] == "shell" and assignment._settings["output_level"] == 2     # a refused configure changes nothing
        assignment.configure(output="all", output_level=0)
        with pytest.raises(ValueError, match='output="shell"'):
            assignment.configure(output_level=1)
        assignment.configure(output="shell")
        assert assignment._settings["output_level"] == 0
    finally:
        assignment.configure(frame_source=None, **saved)
