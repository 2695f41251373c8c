"""Distance field of the hull, erosion and opening, CPU side: the separable restatement (tests/distance_np.py) against the
literal minimum over all sites on seeded random grids (both border modes, the outside field, erode and open, hull empty and grid
full), against scipy.ndimage.distance_transform_edt on the committed 64^3 / 128^3 hulls, the figures of those hulls (deepest
survivor, eroded and opened counts, 26-components), the algebra of the operators, a hull touching a grid face, and the claim the
device relies on: the transform restricted to the hull's box equals the one over the grid."""
import numpy as np
import pytest

import components_np as cn
import distance_np as dn
import fixtures_util as fx
from voxcarve.engine import DEFAULT_BOUNDS

DENSITIES = (0.02, 0.1, 0.5)


def _random_case(rng, k):
    shape = tuple(int(v) for v in rng.integers(2, 10, 3))
    q = tuple(int(v) for v in rng.integers(1, 50001, 3))
    occ = rng.random(shape) < DENSITIES[k % 3]
    return occ, q


def _agree(occ, q, r2s):
    for border in dn.BORDERS:
        want = dn.inside_literal(occ, q, border)
        assert np.array_equal(dn.inside(occ, q, border), want), ("inside", border, occ.shape, q)
        assert np.array_equal(dn.inside_box(occ, q, border), want), ("inside_box", border, occ.shape, q)
        for r2 in r2s:
            e = dn.erode_literal(occ, q, r2, border)
            o = dn.open_literal(occ, q, r2, border)
            assert np.array_equal(dn.erode(occ, q, r2, border), e), ("erode", border, r2)
            got_o, got_e = dn.open_(occ, q, r2, border)
            assert np.array_equal(got_o, o) and np.array_equal(got_e, e), ("open", border, r2)
    assert np.array_equal(dn.outside(occ, q), dn.outside_literal(occ, q)), ("outside", occ.shape, q)


def test_vectorised_equals_literal_on_seeded_grids():
    rng = np.random.default_rng(11)
    n = 0
    for k in range(66):
        occ, q = _random_case(rng, k)
        qm = max(q)
        _agree(occ, q, (0, int(rng.integers(1, 4 * qm * qm)), qm * qm))
        n += 1
    assert n >= 60


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 9, 4), (5, 2, 7)])
def test_empty_hull_and_full_grid(shape):
    q = (31000, 17, 50000)
    empty = np.zeros(shape, dtype=bool)
    full = np.ones(shape, dtype=bool)
    for occ in (empty, full):
        _agree(occ, q, (0, 10 ** 9))
    assert (dn.inside(empty, q) == 0).all() and (dn.outside(empty, q) == dn.NONE).all()
    assert (dn.inside(full, q, "open") == dn.NONE).all() and (dn.outside(full, q) == 0).all()
    assert (dn.inside(full, q, "off") != dn.NONE).all() and dn.inside(full, q, "off").min() == min(q) ** 2
    # no site at all: nothing is ever eroded, and the opening keeps everything
    assert dn.erode(full, q, 10 ** 18, "open").all() and dn.open_(full, q, 5, "open")[0].all()


def test_steps_and_their_refusals():
    assert dn.steps_um((128, 128, 128), DEFAULT_BOUNDS) == (12094, 16126, 20157)
    assert dn.steps_um((64, 64, 64), DEFAULT_BOUNDS) == (24381, 32508, 40635)
    for grid, bounds in (((1, 4, 4), DEFAULT_BOUNDS), ((4, 4, 4), (0, 0, 0, 1, 0, 1)), ((4, 4, 4), (0, 1e-4, 0, 1, 0, 1)),
                         ((2, 2, 2), (0, 2000.0, 0, 1, 0, 1)), ((4096, 4, 4), (0, 4095 * 300.0, 0, 1, 0, 1))):
        with pytest.raises(ValueError):
            dn.steps_um(grid, bounds)
    assert dn.steps_um((2, 2, 2), (0, 1048.576, 0, 1, 0, 1))[0] == 1 << 20                 # the largest step
    assert dn.radius_r2(25) == 625000000 and dn.radius_r2(0.0004) == 0 and dn.radius_r2(0.0016) == 4


FIGURES = {64: dict(S=6981, comps=4, q=(24381, 32508, 40635), max_d2=44912727720, depth=211.9,
                    opening={15: (6981, 6981, 4), 25: (5531, 6675, 1), 40: (4852, 6599, 1)}),
           128: dict(S=57048, comps=2, q=(12094, 16126, 20157), max_d2=39784228900, depth=199.5,
                     opening={15: (50811, 56387, 9), 25: (39714, 54466, 1), 40: (30357, 52773, 1)})}


@pytest.fixture(scope="module", params=[64, 128])
def hull(request):
    n = request.param
    idx, _, _ = fx.expected(n)
    grid = (n, n, n)
    q = dn.steps_um(grid, DEFAULT_BOUNDS)
    occ = dn.volume(idx, grid)
    return n, grid, q, occ, {b: dn.inside_box(occ, q, b) for b in dn.BORDERS}


def test_fixture_hull_equals_scipy(hull):
    ndimage = pytest.importorskip("scipy.ndimage")
    n, grid, q, occ, d_in = hull
    sampling = (q[2], q[0], q[1])                                # the volume's axes are (z, x, y)
    for border in dn.BORDERS:
        vol = np.pad(occ, 1, constant_values=False) if border == "off" else occ
        edt = ndimage.distance_transform_edt(vol, sampling=sampling)
        if border == "off":
            edt = edt[1:-1, 1:-1, 1:-1]
        want = np.rint(edt[occ] ** 2)
        assert np.array_equal(want, d_in[border][occ].astype(np.float64)), border
        assert np.array_equal(want.astype(np.uint64), d_in[border][occ]), border


def test_fixture_figures(hull):
    n, grid, q, occ, d_in = hull
    fig = FIGURES[n]
    assert int(occ.sum()) == fig["S"] and q == fig["q"]
    assert cn.components(dn.indices(occ), grid, 26)["label"].size == fig["comps"]
    assert int(d_in["open"].max()) == fig["max_d2"]
    assert round(float(dn.depth_mm(d_in["open"].max())), 1) == fig["depth"]
    # the hull touches no grid face: the two border modes agree on it
    assert np.array_equal(d_in["open"], d_in["off"])
    assert np.array_equal(d_in["open"], dn.inside(occ, q, "open"))
    for mm, (n_e, n_o, comps) in fig["opening"].items():
        r2 = dn.radius_r2(mm)
        o, e = dn.open_(occ, q, r2)
        assert int(e.sum()) == n_e and int(o.sum()) == n_o, mm
        assert np.array_equal(e, occ & (d_in["open"] > np.uint64(r2)))
        assert cn.components(dn.indices(o), grid, 26)["label"].size == comps, mm
        # a subset of the hull, and idempotent
        assert not (o & ~occ).any()
        again, _ = dn.open_(o, q, r2)
        assert np.array_equal(again, o), mm
    # at 64^3 15 mm is below every step: the identity
    if n == 64:
        assert np.array_equal(dn.open_(occ, q, dn.radius_r2(15))[0], occ)


def test_operator_algebra_on_random_grids():
    rng = np.random.default_rng(23)
    for k in range(30):
        shape = tuple(int(v) for v in rng.integers(3, 14, 3))
        q = tuple(int(v) for v in rng.integers(1000, 50001, 3))
        occ = rng.random(shape) < (0.5, 0.8, 0.95)[k % 3]
        for border in dn.BORDERS:
            r2s = sorted(int(v) for v in rng.integers(0, 6 * max(q) ** 2, 4))
            prev = occ
            for r2 in [0] + r2s:
                e = dn.erode(occ, q, r2, border)
                assert not (e & ~prev).any(), "erosion is monotone in r2"
                prev = e
                o, e2 = dn.open_(occ, q, r2, border)
                assert np.array_equal(e2, e) and not (o & ~occ).any() and not (e & ~o).any()
                assert np.array_equal(dn.open_(o, q, r2, border)[0], o), "opening is idempotent"
            if border == "off" or not occ.all():                 # a site exists: r2 = 0 is the identity
                assert np.array_equal(dn.erode(occ, q, 0, border), occ)
                assert np.array_equal(dn.open_(occ, q, 0, border)[0], occ)


def test_hull_on_a_grid_face():
    # a slab 3 cells thick lying on the face iz = 0 and spanning the grid in x and y
    occ = np.zeros((8, 6, 7), dtype=bool)
    occ[0:3] = True
    q = (10000, 10000, 10000)
    r2 = dn.radius_r2(15)                                        # between one step and two
    e_open, e_off = dn.erode(occ, q, r2, "open"), dn.erode(occ, q, r2, "off")
    assert e_open[0].all() and e_open[1].all() and not e_open[2].any()       # only the layer under the free surface goes
    assert not e_off[0].any() and not e_off[2].any()                         # "off" erodes the face layer too ...
    assert e_off[1, 1:-1, 1:-1].all() and not e_off[1, 0].any() and not e_off[1, :, 0].any()     # ... and the rim, from the sides
    assert np.array_equal(dn.erode_literal(occ, q, r2, "off"), e_off) and np.array_equal(dn.erode_literal(occ, q, r2, "open"), e_open)
    d_open, d_off = dn.inside(occ, q, "open"), dn.inside(occ, q, "off")
    assert d_open[0, 3, 3] == 30000 ** 2 and d_off[0, 3, 3] == 10000 ** 2


def test_box_restricted_transform_equals_the_full_one():
    rng = np.random.default_rng(5)
    for k in range(40):
        shape = tuple(int(v) for v in rng.integers(4, 20, 3))
        q = tuple(int(v) for v in rng.integers(1, 50001, 3))
        occ = np.zeros(shape, dtype=bool)
        lo = [int(rng.integers(0, s - 1)) for s in shape]
        hi = [int(rng.integers(l + 1, s + 1)) for l, s in zip(lo, shape)]
        sub = tuple(slice(l, h) for l, h in zip(lo, hi))
        occ[sub] = rng.random(tuple(h - l for l, h in zip(lo, hi))) < (0.3, 0.7, 1.0)[k % 3]
        for border in dn.BORDERS:
            assert np.array_equal(dn.inside_box(occ, q, border), dn.inside(occ, q, border)), (shape, sub, border)
