"""The restatement of the hull's measurements (tests/measure_np.py; contract of vc_hull_measure in include/voxcarve.h) against its
own literal form on random occupancies and labels, against a full grid worked out by hand, and -- through voxcarve.measure, the
host's derivation of world units -- against the analytic volume, covariance and major axis of an ellipsoid voxelised in numpy;
then the interface: the header, the ctypes mirrors, the Makefile, the drop-in layer's settings."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import fixtures_util as fx
import measure_np as mn


def _random_records(rng, grid, fill):
    nx, ny, nz = grid
    idx = np.flatnonzero(rng.random(nx * ny * nz) < fill)
    return mn.pack_records(idx, rng.integers(0, 256, (idx.size, 3)), rng.random(idx.size) < 0.8)


@pytest.mark.parametrize("grid", [(5, 7, 3), (9, 130, 12), (20, 70, 33)])
def test_vectorised_equals_literal(grid):
    for seed, fill in ((1, 0.6), (2, 0.12), (3, 1.0)):
        rng = np.random.default_rng(seed)
        rec = _random_records(rng, grid, fill)
        S = rec.size
        a = mn.measure(rec, grid, np.zeros(S, np.uint32), 1, with_profile=True)
        mn.same(a, mn.measure_literal(rec, grid, np.zeros(S, np.uint32), 1, with_profile=True), True)
        assert int(a["voxels"][0]) == S and int(a["profile"][0, :, 0].sum()) == S
        for G in (1, 3, 7, 200):
            lab = rng.integers(0, G, S).astype(np.uint32)
            lab[rng.random(S) < 0.1] = mn.NONE
            if G >= 7:
                lab[lab == 2] = 5                                # an empty group in the middle
            b = mn.measure(rec, grid, lab, G, with_profile=True)
            mn.same(b, mn.measure_literal(rec, grid, lab, G, with_profile=True), True)
            st = mn.stats(rec, lab, G)
            assert int(b["voxels"].sum()) == st["measured"] == S - st["unlabelled"]
            # the groups partition what "all" measures, but for the unlabelled records
            rest = mn.measure(rec[lab == mn.NONE], grid, np.zeros(st["unlabelled"], np.uint32), 1)
            assert int(b["s2"].sum()) + int(rest["s2"].sum()) == int(a["s2"].sum())
            assert int(b["seen"].sum()) + int(rest["seen"].sum()) == int(a["seen"][0])
            assert np.array_equal(b["profile"].sum(axis=1)[:, 0], b["voxels"])
            empty = b["voxels"] == 0
            assert (b["lo"][empty] == mn.EMPTY_LO).all() and (b["hi"][empty] == mn.EMPTY_HI).all()
            if G >= 7:
                assert empty[2]
        none = np.full(S, mn.NONE, np.uint32)                    # G = 1 and nobody in it
        c = mn.measure(rec, grid, none, 1)
        mn.same(c, mn.measure_literal(rec, grid, none, 1))
        assert not c["voxels"].any() and not c["faces"].any()
    with pytest.raises(ValueError):
        mn.measure(rec, grid, np.full(S, 3, np.uint32), 3)
    with pytest.raises(ValueError):
        mn.measure_literal(rec, grid, np.full(S, 3, np.uint32), 3)
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            mn.measure(rec, grid, np.zeros(S, np.uint32), bad)
    with pytest.raises(ValueError):
        mn.measure(rec[:0], (4, 4, 1024), np.zeros(0, np.uint32), 1025, with_profile=True)
    with pytest.raises(ValueError):
        mn.measure(rec[:0], (65537, 1, 1), np.zeros(0, np.uint32), 1)


def test_no_wrap_around_between_rows_and_layers():
    """i and i + 1 are no neighbours across the end of a row; the last cell of a layer and the first of the next neither."""
    grid = (2, 3, 2)
    rec = mn.pack_records([2, 3, 5, 6])                          # (0, 2, 0), (1, 0, 0), (1, 2, 0), (0, 0, 1)
    for f in (mn.measure, mn.measure_literal):
        m = f(rec, grid, np.zeros(4, np.uint32), 1)
        # 2 and 5 touch along x; nothing else touches: 24 faces less the two of that contact
        assert m["faces"][0].tolist() == [3, 3, 4, 4, 4, 4] and int(m["surface"][0]) == 4


def test_full_8x8x8_grid_by_hand():
    rec = mn.pack_records(np.arange(512))
    for f in (mn.measure, mn.measure_literal):
        m = f(rec, (8, 8, 8), np.zeros(512, np.uint32), 1, with_profile=True)
        assert int(m["voxels"][0]) == 512 and int(m["surface"][0]) == 512 - 6 ** 3 == 296 and int(m["seen"][0]) == 512
        assert m["faces"][0].tolist() == [64] * 6
        assert m["s1"][0].tolist() == [1792] * 3                 # 64 * (0 + .. + 7)
        assert m["s2"][0].tolist() == [8960] * 3 + [6272] * 3    # 64 * 140; 8 * 28 * 28
        assert m["lo"][0].tolist() == [0, 0, 0] and m["hi"][0].tolist() == [7, 7, 7]
        assert m["profile"][0].tolist() == [[64, 224, 224]] * 8


# ---- the world units of voxcarve.measure against analysis -------------------------------------------------------------------------
ELL_AXES = (300.0, 200.0, 120.0)
ELL_ANGLE = 30.0
ELL_CENTRE = (13.7, -21.3, 5.9)
ELL_GRID = (96, 96, 96)
ELL_BOUNDS = (-400.0, 400.0, -400.0, 400.0, -400.0, 400.0)
# the errors of this voxelisation against the analytic values: the largest relative error of the
# three eigenvalues of the covariance, and the angle between the major axis and the rotated x axis
ELL_EIGEN_ERR = 1.52e-3
ELL_AXIS_ERR_DEG = 0.0197


@pytest.fixture(scope="module")
def ellipsoid():
    from voxcarve import measure
    lo, step = measure.grid_metric(ELL_GRID, ELL_BOUNDS)
    ix, iy, iz = np.meshgrid(*[np.arange(n) for n in ELL_GRID], indexing="ij")
    p = np.stack([lo[0] + step[0] * ix, lo[1] + step[1] * iy, lo[2] + step[2] * iz], axis=-1) - np.array(ELL_CENTRE)
    t = math.radians(ELL_ANGLE)
    u = p[..., 0] * math.cos(t) + p[..., 1] * math.sin(t)
    v = -p[..., 0] * math.sin(t) + p[..., 1] * math.cos(t)
    inside = (u / ELL_AXES[0]) ** 2 + (v / ELL_AXES[1]) ** 2 + (p[..., 2] / ELL_AXES[2]) ** 2 <= 1.0
    nx, ny, nz = ELL_GRID
    idx = np.sort(((iz[inside] * nx + ix[inside]) * ny + iy[inside]).astype(np.int64))
    m = mn.measure(mn.pack_records(idx), ELL_GRID, np.zeros(idx.size, np.uint32), 1)
    return m, measure.describe(m, ELL_GRID, ELL_BOUNDS), step


def test_ellipsoid_volume_and_centroid(ellipsoid):
    m, w, step = ellipsoid
    a, b, c = ELL_AXES
    cell = float(step[0] * step[1] * step[2])
    assert w["volume_mm3"][0] == int(m["voxels"][0]) * step[0] * step[1] * step[2]
    # only the cells the surface crosses can be wrong, and each by at most one cell
    err = abs(w["volume_mm3"][0] - 4.0 * math.pi * a * b * c / 3.0)
    print("ellipsoid: volume error %.4g mm3 of %.4g, bound %.4g" % (err, w["volume_mm3"][0], int(m["surface"][0]) * cell))
    assert err <= int(m["surface"][0]) * cell
    assert np.abs(w["centroid_mm"][0] - np.array(ELL_CENTRE)).max() <= float(step.max()) / 2
    assert w["height_mm"][0] == (int(m["hi"][0][2]) - int(m["lo"][0][2]) + 1) * step[2] and abs(w["height_mm"][0] - 2 * c) <= 2 * step[2]
    assert abs(w["top_mm"][0] - (ELL_CENTRE[2] - c)) <= step[2]


def test_ellipsoid_axes(ellipsoid):
    m, w, step = ellipsoid
    want = np.array([v * v / 5.0 for v in ELL_AXES])
    got = w["std_mm"][0] ** 2
    eigen_err = float(np.abs(got / want - 1.0).max())
    t = math.radians(ELL_ANGLE)
    major = np.array([math.cos(t), math.sin(t), 0.0])
    axis_err = math.degrees(math.acos(min(1.0, abs(float(w["axes"][0][0] @ major)))))
    print("ellipsoid: eigenvalue error %.3g, major axis error %.3g deg" % (eigen_err, axis_err))
    assert eigen_err <= 2 * ELL_EIGEN_ERR and axis_err <= 2 * ELL_AXIS_ERR_DEG
    assert (np.diff(w["std_mm"][0]) <= 0).all()
    for k in range(3):                                           # unit vectors, the largest component positive
        ax = w["axes"][0][k]
        assert abs(float(ax @ ax) - 1.0) < 1e-12 and ax[np.argmax(np.abs(ax))] > 0
    assert abs(w["lean_deg"][0] - 90.0) < 2 * ELL_AXIS_ERR_DEG   # the major axis lies in the floor plane
    assert np.allclose(w["covariance_mm2"][0], w["covariance_mm2"][0].T)


def test_ellipsoid_area_is_the_voxel_boundary(ellipsoid):
    """A property, no pass criterion beyond its range: the face count overstates the smooth surface -- the area of the voxel
    boundary is the sum of the ellipsoid's three axis-aligned shadows, twice each."""
    m, w, step = ellipsoid
    a, b, c = ELL_AXES
    p = 1.6075                                                   # Knud Thomsen's formula, within 1.1 %
    smooth = 4.0 * math.pi * (((a * b) ** p + (a * c) ** p + (b * c) ** p) / 3.0) ** (1.0 / p)
    ratio = w["area_mm2"][0] / smooth
    print("ellipsoid: face-count area %.4g mm2, smooth surface %.4g mm2, ratio %.3f (1.5 for a sphere in the limit)" %
          (w["area_mm2"][0], smooth, ratio))
    assert 1.2 < ratio < 1.6
    assert np.array_equal(m["faces"][0][0::2], m["faces"][0][1::2])      # a closed boundary: as many faces towards - as towards +


def test_describe_empty_groups_and_colours():
    from voxcarve import measure
    rec = mn.pack_records([0, 1, 9], [[10, 20, 30], [30, 40, 50], [200, 200, 200]], [1, 1, 0])
    m = mn.measure(rec, (4, 4, 4), np.array([0, 0, 2], np.uint32), 3)
    w = measure.describe(m, (4, 4, 4), (0.0, 30.0, 0.0, 60.0, -90.0, 0.0))
    assert w["mean_rgb"][0].tolist() == [20.0, 30.0, 40.0] and np.isnan(w["mean_rgb"][1:]).all()
    assert w["volume_mm3"].tolist() == [2 * 10 * 20 * 30.0, 0.0, 10 * 20 * 30.0]
    assert np.isnan(w["centroid_mm"][1]).all() and w["centroid_mm"][0].tolist() == [0.0, 10.0, -90.0]
    assert w["centroid_mm"][2].tolist() == [20.0, 20.0, -90.0]
    # two cells of 10 x 20 x 30 mm side by side along y: four faces across x, two across y, four across z
    assert w["area_mm2"][0] == 4 * (20 * 30) + 2 * (10 * 30) + 4 * (10 * 20)
    # a single cell: the covariance of a uniform box, s^2 / 12
    assert np.allclose(np.sort(w["std_mm"][2] ** 2), np.sort(np.array([100.0, 400.0, 900.0]) / 12.0))
    area, centre, z = measure.profile_mm(mn.measure(rec, (4, 4, 4), np.zeros(3, np.uint32), 1, True)["profile"], (4, 4, 4),
                                         (0.0, 30.0, 0.0, 60.0, -90.0, 0.0))
    assert area[0].tolist() == [600.0, 0.0, 0.0, 0.0] and z.tolist() == [-90.0, -60.0, -30.0, 0.0] and np.isnan(centre[0, 1:]).all()


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
    for name in ("vc_hull_measure", "vc_fetch_measure", "vc_fetch_measure_profile"):
        assert "int %s(vc_ctx *ctx" % name in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vc_hull_measure"][1]) == 6
    for text in ("#define VC_MEASURE_ALL      0u", "#define VC_MEASURE_CLUSTERS 1u", "#define VC_MEASURE_GEODESIC 2u",
                 "#define VC_MEASURE_HOST     3u", "#define VC_MEASURE_PROFILE  1u", "#define VC_MEASURE_MAX_GROUPS 4096u"):
        assert text in header, text
    assert (_lib.VC_MEASURE_ALL, _lib.VC_MEASURE_CLUSTERS, _lib.VC_MEASURE_GEODESIC, _lib.VC_MEASURE_HOST) == (0, 1, 2, 3)
    assert _lib.VC_MEASURE_PROFILE == 1 and _lib.VC_MEASURE_MAX_GROUPS == 4096 == mn.MAX_GROUPS
    assert _lib.VC_MEASURE_MAX_PROFILE == 1 << 20 == mn.MAX_PROFILE and _lib.VC_MEASURE_MAX_AXIS == 65536 == mn.MAX_AXIS
    assert ctypes.sizeof(_lib.VcMeasure) == 192 and ctypes.sizeof(_lib.VcMeasureStats) == 32
    assert [f[0] for f in _lib.VcMeasure._fields_] == _struct_fields(header, "vc_measure_t") == list(mn.FIELDS)
    assert [f[0] for f in _lib.VcMeasureStats._fields_] == _struct_fields(header, "vc_measure_stats_t")
    assert _lib.VcMeasure.lo.offset == 21 * 8 and _lib.VcMeasure.s2.offset == 6 * 8 and _lib.VcMeasure.rgb.offset == 18 * 8
    # the pass adds no kernel kind and no work kind
    assert "#define VC_KERNEL_KINDS 28" in header and _lib.VC_KERNEL_KINDS == 28 == len(_lib.KERNEL_KINDS)
    assert "#define VC_WORK_KINDS 10" in header and _lib.VC_WORK_KINDS == 10
    makefile = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    assert "vc_measure.h" in makefile.split("HEADERS =")[1].split("$(OUT):")[0]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vc_hull_measure", "vc_fetch_measure", "vc_fetch_measure_profile"):
        assert hasattr(lib, name)
    from voxcarve import CarveEngine
    for name in ("measure_hull", "fetch_measure", "fetch_measure_profile", "measure_valid"):
        assert callable(getattr(CarveEngine, name))


def test_configure_validates_the_measure_settings():
    from voxcarve import assignment
    saved = dict(assignment._settings)
    try:
        for bad in ("figures", 3, True):
            with pytest.raises(ValueError):
                assignment.configure(measure=bad)
        with pytest.raises(ValueError):
            assignment.configure(measure="all", measure_profile=1)
        with pytest.raises(ValueError, match="clusters=K"):
            assignment.configure(measure="clusters")
        with pytest.raises(ValueError, match="extremities=K"):
            assignment.configure(measure="geodesic")
        with pytest.raises(ValueError, match="component filter"):
            assignment.configure(measure="components")
        assert assignment._settings["measure"] is None           # a refused configure changes nothing
        assignment.configure(measure="clusters", clusters=3)
        assignment.configure(measure="geodesic", extremities=5, clusters=0)
        assignment.configure(measure="components", min_component_voxels=1, extremities=0)
        assignment.configure(measure="all", measure_profile=True, min_component_voxels=0)
        assert assignment._settings["measure"] == "all" and assignment._settings["measure_profile"] is True
        with pytest.raises(RuntimeError, match="no measurements"):
            assignment.measurements()
        assignment.configure(measure=None, measure_profile=False)
    finally:
        assignment.configure(frame_source=None, **saved)
