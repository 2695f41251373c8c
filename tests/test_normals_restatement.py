"""The restatement of the hull's surface normals (tests/normals_np.py; contract of vc_hull_normals in include/voxcarve.h) against
its own literal form and against what the contract promises: seeded random volumes whose y lines are shorter than, equal to and
longer than occupancy words, hulls on the grid faces, mirror symmetry, a half-space, a single voxel, truncation toward zero; the
committed hulls at 64^3 and 128^3; and what the estimate is worth against the cube-face normal on a sphere."""
import numpy as np
import pytest

import distance_np as dn
import fixtures_util as fx
import normals_np as nn


def _random(shape, seed, fill=0.6):
    rng = np.random.default_rng(seed)
    occ = rng.random(shape) < fill
    # blobs, so that most surface voxels have a neighbourhood worth a gradient, and ON voxels on every face of the grid
    occ[shape[0] // 3:, : shape[1] // 2 + 1, :] |= rng.random((shape[0] - shape[0] // 3, shape[1] // 2 + 1, shape[2])) < 0.9
    occ[0, :, :] |= rng.random(shape[1:]) < 0.5
    occ[:, -1, :] |= rng.random((shape[0], shape[2])) < 0.5
    occ[:, :, 0] = True
    return occ


# (nz, nx, ny): ny = 64 (one word), < 64, > 128 (more than two words), and a tiny one
@pytest.mark.parametrize("shape,q,r2", [((5, 6, 64), (30000, 17000, 52000), 60000 ** 2), ((6, 7, 13), (12090, 16130, 20160), 45000 ** 2),
                                         ((3, 4, 131), (41000, 9000, 88000), 100000 ** 2), ((4, 3, 5), (1, 1, 1), 2),
                                         ((7, 9, 11), (1000, 1000, 1000), 5000 ** 2)])
def test_vectorised_equals_literal(shape, q, r2):
    for seed in (1, 2):
        occ = _random(shape, seed)
        a, sa = nn.normals(occ, q, r2)
        b, sb = nn.normals_literal(occ, q, r2)
        assert a.dtype == np.int16 and a.shape == (int(occ.sum()), 4)
        assert np.array_equal(a, b) and sa == sb
        assert sa["surface"] == int((a[:, 3] == 1).sum()) > 0 and sa["survivors"] == int(occ.sum())
        assert sa["offsets"] == len(nn.ball(q, r2)[1])
        # a record that is not surface stores four zeros
        assert not a[a[:, 3] == 0].any()


def test_ball_and_refusals():
    from voxcarve.engine import DEFAULT_BOUNDS
    q = dn.steps_um((128, 128, 128), DEFAULT_BOUNDS)
    assert q == (12094, 16126, 20157) and nn.default_r2(q) == 60471 ** 2
    ext, offs = nn.ball(q, nn.default_r2(q))
    assert ext == (5, 3, 3) and len(offs) == 222
    # symmetric, without the origin
    s = set(map(tuple, offs.tolist()))
    assert (0, 0, 0) not in s and all((-a, -b, -c) in s for a, b, c in s)
    with pytest.raises(ValueError):
        nn.ball((1000, 1000, 1000), 999 ** 2)                    # empty
    with pytest.raises(ValueError):
        nn.ball((1000, 2000, 2000), 16000 ** 2)                  # ext_x = 16
    assert nn.ball((1000, 2000, 2000), 15999 ** 2)[0] == (15, 7, 7)


def test_mirror_symmetry():
    q, r2 = (12090, 16130, 20160), 50000 ** 2
    occ = _random((6, 7, 70), 5)
    n4, _ = nn.normals(occ, q, r2)
    iz, ix, iy = np.nonzero(occ)
    for axis, comp in ((0, 2), (1, 0), (2, 1)):                   # volume axis -> world component
        m4, _ = nn.normals(np.flip(occ, axis), q, r2)
        coords = [iz, ix, iy]
        coords[axis] = occ.shape[axis] - 1 - coords[axis]
        order = np.argsort(np.ravel_multi_index(coords, occ.shape), kind="stable")
        want = n4.copy()
        want[:, comp] = -want[:, comp]
        assert np.array_equal(m4, want[order])


def test_half_space_single_voxel_and_truncation():
    q, r2 = (12090, 16130, 20160), 61000 ** 2
    occ = np.zeros((16, 12, 20), dtype=bool)
    occ[:8] = True                                               # solid below iz = 8: the empty side is +z
    n4, st = nn.normals(occ, q, r2)
    vol = np.zeros(occ.shape + (4,), dtype=np.int16)
    vol[occ] = n4
    # away from the grid's faces the ball sees the half-space alone
    core = vol[7, 5:7, 6:14]
    assert (core == np.array([0, 0, 32767, 1], dtype=np.int16)).all()
    n4f, _ = nn.normals(np.flip(occ, 0), q, r2)
    volf = np.zeros(occ.shape + (4,), dtype=np.int16)
    volf[np.flip(occ, 0)] = n4f
    assert (volf[8, 5:7, 6:14] == np.array([0, 0, -32767, 1], dtype=np.int16)).all()
    assert not vol[3, 5, 10].any() and vol[0, 5, 10, 3] == 1      # deep inside: no surface; on the grid's bottom face: surface
    one = np.zeros((5, 5, 5), dtype=bool)
    one[2, 2, 2] = True
    n1, s1 = nn.normals(one, q, r2)
    assert n1.tolist() == [[0, 0, 0, 1]] and s1["zero"] == s1["surface"] == 1
    # truncation toward zero: n = (-1, 3, 0) q stores -32767 / 3 = -10922 (the floor would be -10923)
    assert nn.store_literal((-1, 3, 0)) == (-10922, 32767, 0, 1) and nn.store_literal((1, -3, 0)) == (10922, -32767, 0, 1)
    occ = np.zeros((3, 11, 11), dtype=bool)                      # v = (ix 5, iy 5, iz 1) with ON cells at +x and at -3 y: n = (-1, 3, 0)
    occ[1, 5, 5] = occ[1, 6, 5] = occ[1, 5, 2] = True
    a, _ = nn.normals(occ, (1, 1, 1), 9)
    b, _ = nn.normals_literal(occ, (1, 1, 1), 9)
    assert np.array_equal(a, b)
    assert a[1].tolist() == [-10922, 32767, 0, 1]                # records in ascending index: (5, 2), (5, 5), (6, 5)
    a, _ = nn.normals(np.flip(occ, (1, 2)), (1, 1, 1), 9)
    assert a[1].tolist() == [10922, -32767, 0, 1]


def _sphere(n, radius_mm, steps_um):
    """A sphere of radius_mm centred in an n^3 grid with the given steps: (occ, q, unit radial directions of the ON voxels)."""
    c = (n - 1) / 2.0
    z, x, y = np.meshgrid(np.arange(n) - c, np.arange(n) - c, np.arange(n) - c, indexing="ij")
    pos = np.stack([x * steps_um[0], y * steps_um[1], z * steps_um[2]], axis=-1) / 1000.0
    occ = (pos ** 2).sum(axis=-1) <= radius_mm ** 2
    rad = pos[occ]
    return occ, rad / np.maximum(np.sqrt((rad ** 2).sum(axis=1)), 1e-12)[:, None]


def _mean_error_deg(est, truth, sel):
    e = est[sel]
    e = e / np.sqrt((e ** 2).sum(axis=1))[:, None]
    return float(np.degrees(np.arccos(np.clip((e * truth[sel]).sum(axis=1), -1.0, 1.0))).mean())


def test_worth_on_a_sphere():
    """A sphere of radius 250 mm on a centred 48^3 grid with a 17.021 mm step: the normal from a ball of 60 mm is off the radial
    direction by at most a quarter of what the cube-face normal is off by, on average over the surface voxels (measured: 2.48
    against 21.55 degrees)."""
    q = (17021, 17021, 17021)
    occ, radial = _sphere(48, 250.0, q)
    n4, st = nn.normals(occ, q, 60000 ** 2)
    surf = n4[:, 3] == 1
    assert st["surface"] == int(surf.sum()) == 2136 and st["zero"] == 0
    ball = _mean_error_deg(n4[:, :3].astype(np.float64), radial, surf)
    face = _mean_error_deg(nn.face_normals(occ, q), radial, surf)
    print("sphere 48^3: ball 60 mm %.2f deg, face normal %.2f deg" % (ball, face))
    assert face > 15.0 and ball <= face / 4.0
    assert np.allclose(np.sqrt((nn.unit(n4)[surf] ** 2).sum(axis=1)), 1.0) and not nn.unit(n4)[~surf].any()


@pytest.mark.parametrize("n,surface,zero2", [(64, 2703, 1), (128, 12462, 2)])
def test_committed_hulls(n, surface, zero2):
    idx, _, _ = fx.expected(n)
    grid = (n, n, n)
    from voxcarve.engine import DEFAULT_BOUNDS
    q = dn.steps_um(grid, DEFAULT_BOUNDS)
    occ = dn.volume(idx, grid)
    big = max(q)
    n4, st = nn.normals(occ, q, (3 * big) ** 2)
    assert st["survivors"] == idx.size and st["surface"] == surface and st["zero"] == 0
    if n == 128:
        assert st["ext"] == (5, 3, 3) and st["offsets"] == 222
    n2, st2 = nn.normals(occ, q, (2 * big) ** 2)
    assert st2["surface"] == surface and st2["zero"] == zero2
    assert np.array_equal(n2[:, 3], n4[:, 3])
