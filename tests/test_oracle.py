"""The oracle against the committed fixtures, and its three restatements against each other.

Parity vs OpenCV itself is UNPINNED (cv2 absent, reference has no golden vectors): these
tests pin the oracle to (a) the reference's data files and (b) agreement of independent
restatements.  Reference lines: voxel_reconstruction.py:35-124, assignment.py:116-133."""
import hashlib
import json
import os

import numpy as np
import pytest

import fixtures_util as fx
from oracle import carve_c, carve_literal, carve_np


def test_config_xml_matches_golden_hex(cams):
    g = json.load(open(os.path.join(fx.GOLDEN, "cameras.json")))
    for c in range(4):
        K, dist, rvec, tvec = carve_np.read_config_xml(os.path.join(fx.GOLDEN, "data", "cam%d" % (c + 1), "config.xml"))
        gc = g["cameras"][c]
        assert [float(v).hex() for v in K.reshape(-1)] == gc["K"]
        assert [float(v).hex() for v in dist.reshape(-1)] == gc["dist"]
        assert [float(v).hex() for v in rvec.reshape(-1)] == gc["rvec"]
        assert [float(v).hex() for v in tvec.reshape(-1)] == gc["tvec"]
        assert K.shape == (3, 3) and dist.shape == (1, 5) and rvec.shape == (3, 1) and tvec.shape == (3, 1)


def test_rodrigues_is_a_rotation_and_matches_golden(cams):
    g = json.load(open(os.path.join(fx.GOLDEN, "cameras.json")))
    for c, cam in enumerate(cams):
        R = carve_np.rodrigues(cam.rvec)
        want = np.array([float.fromhex(h) for h in g["cameras"][c]["R"]]).reshape(3, 3)
        # libm sin/cos may differ by an ulp between hosts; the carve tests use the pinned R
        assert np.max(np.abs(R - want)) <= 2 * np.finfo(np.float64).eps
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1) < 1e-14
    assert np.array_equal(carve_np.rodrigues(np.zeros(3)), np.eye(3))


@pytest.mark.parametrize("n", [1, 2, 3, 64, 100, 128, 1000, 1024])
def test_c_axis_equals_numpy_linspace(built, n):
    for lo, hi in ((-512, 1024), (-1024, 1024), (-2048, 512), (0.1, 0.7), (5, 5), (3, -9)):
        assert np.array_equal(carve_c.axis(lo, hi, n), np.linspace(lo, hi, num=n)), (lo, hi, n)


def test_voxel_order_matches_meshgrid_form():
    pts = carve_np.create_voxel_volume(5, 7, 3)
    idx = np.arange(5 * 7 * 3)
    assert np.array_equal(pts, carve_np.points_of_indices(idx, 5, 7, 3))
    # i = iz*nx*ny + ix*ny + iy, y fastest
    xs, ys, zs = carve_np.axis_tables(5, 7, 3)
    assert np.array_equal(pts[1], [xs[0], ys[1], zs[0]]) and np.array_equal(pts[7], [xs[1], ys[0], zs[0]])
    assert np.array_equal(pts[35], [xs[0], ys[0], zs[1]])


def test_projected_samples_golden(built, cams):
    g = json.load(open(os.path.join(fx.GOLDEN, "projected_samples.json")))
    pts = carve_np.points_of_indices(np.array(g["idx"]), *g["grid"])
    for c, cam in enumerate(cams):
        want = np.array([float.fromhex(h) for h in g["uv"][c]]).reshape(-1, 2)
        got = carve_np.project_points(pts, cam.R, cam.tvec, cam.K, cam.dist)
        assert np.array_equal(got, want)
        assert np.array_equal(carve_c.project(pts, (cam.K, cam.dist, cam.R, cam.tvec)), want)


def test_oracle_pinned_by_reference_arrow_tips(built, cams):
    """THE reference-produced pin of the oracle: the arrow tips the reference drew into data/cam{1..4}/test.jpg are
    cv2.projectPoints([[345,0,0],[0,345,0],[0,0,-345]], rvec, tvec, mtx, dist).astype(int32) for exactly the
    committed cameras (camera_calibration.py:753-789, 847-849, 967-974; fixture: tests/golden/make_arrow_tips.py).
    Every restatement must land within 2 px on all 12 tips.  Pins the K / distortion / Rodrigues / translation
    conventions and the axis order at pixel tolerance; cannot pin the last ulp."""
    from voxcarve.camera import Camera
    tol = fx.ARROW_TIP_TOL_PX
    e_np = fx.arrow_tip_error(lambda c, cam, p: carve_np.project_points(p, cam.R, cam.tvec, cam.K, cam.dist), cams)
    e_c = fx.arrow_tip_error(lambda c, cam, p: carve_c.project(p, (cam.K, cam.dist, cam.R, cam.tvec)), cams)
    # and with R recomputed from rvec by both Rodrigues restatements (oracle's and the product host's)
    e_rod = fx.arrow_tip_error(lambda c, cam, p: carve_np.project_points(p, carve_np.rodrigues(cam.rvec), cam.tvec, cam.K, cam.dist), cams)
    e_host = fx.arrow_tip_error(lambda c, cam, p: carve_np.project_points(p, Camera(cam.K, cam.dist, cam.rvec, cam.tvec).R, cam.tvec, cam.K, cam.dist), cams)
    assert e_np <= tol and e_c <= tol and e_rod <= tol and e_host <= tol, (e_np, e_c, e_rod, e_host)
    # the reference truncates (astype(int32) of the float32 result): the truncated pixels agree as well
    e_tr = fx.arrow_tip_error(lambda c, cam, p: np.trunc(carve_np.project_points(p, cam.R, cam.tvec, cam.K, cam.dist).astype(np.float32)), cams)
    assert e_tr <= tol, e_tr
    # the pin discriminates: each of these misreadings of the convention misses a tip by far more than the tolerance
    wrong = {
        "R transposed": lambda c, cam, p: carve_np.project_points(p, cam.R.T, cam.tvec, cam.K, cam.dist),
        "rvec negated": lambda c, cam, p: carve_np.project_points(p, carve_np.rodrigues(-np.asarray(cam.rvec)), cam.tvec, cam.K, cam.dist),
        "x and y swapped": lambda c, cam, p: carve_np.project_points(p[:, [1, 0, 2]], cam.R, cam.tvec, cam.K, cam.dist),
        "z sign": lambda c, cam, p: carve_np.project_points(p * [1, 1, -1], cam.R, cam.tvec, cam.K, cam.dist),
        "t as camera centre": lambda c, cam, p: carve_np.project_points(p - np.asarray(cam.tvec).reshape(1, 3), cam.R, np.zeros(3), cam.K, cam.dist),
        "no distortion": lambda c, cam, p: carve_np.project_points(p, cam.R, cam.tvec, cam.K, np.zeros(5)),
        "k1 sign": lambda c, cam, p: carve_np.project_points(p, cam.R, cam.tvec, cam.K, np.asarray(cam.dist).reshape(-1) * [-1, 1, 1, 1, 1]),
        "fx/fy swapped with cx/cy": lambda c, cam, p: carve_np.project_points(p, cam.R, cam.tvec, np.asarray(cam.K).T[::-1, ::-1].copy(), cam.dist),
    }
    for name, f in wrong.items():
        assert fx.arrow_tip_error(f, cams) > 2 * tol, name


@pytest.mark.parametrize("n", [64, 128])
def test_carve_matches_golden(built, cams, masks, frames, n):
    idx, bgr, summary = fx.expected(n)
    assert idx.size == summary["survivors"] == {64: 6981, 128: 57048}[n]   # SURVEY probe counts
    assert hashlib.sha256(idx.tobytes()).hexdigest() == summary["idx_sha256"]
    oc = fx.oracle_cams(cams)
    res = carve_np.carve(n, n, n, oc, masks, frames)
    assert np.array_equal(res["idx"], idx) and np.array_equal(res["bgr"], bgr)
    assert hashlib.sha256(res["viewmask"].tobytes()).hexdigest() == summary["viewmask_sha256"]
    assert hashlib.sha256(res["offsets"].tobytes()).hexdigest() == summary["offsets_sha256"]
    resc = carve_c.carve(n, n, n, oc, masks, frames, want_viewmask=True, want_lut=True)
    assert np.array_equal(resc["idx"], idx) and np.array_equal(resc["bgr"], bgr)
    assert np.array_equal(resc["viewmask"], res["viewmask"]) and np.array_equal(resc["offsets"], res["offsets"])
    assert int((res["viewmask"] != 0).sum()) == summary["any_view"]


def test_literal_dict_restatement_agrees(built, cams, masks, frames):
    """The dict/loop mirror of the reference's Python gives the numpy oracle's list, in order."""
    n, half = 24, 12
    data, cols = carve_literal.set_voxel_positions(n, half, n, fx.oracle_cams(cams), masks, frames)
    res = carve_np.carve(n, 2 * half, n, fx.oracle_cams(cams), masks, frames)
    assert len(data) == res["idx"].size > 0
    keys = carve_np.voxel_keys(res["idx"], n, 2 * half, n)
    assert np.array_equal(np.array(data), carve_np.viewer_positions(keys))
    assert np.array_equal(np.array(cols), carve_np.viewer_colors(res["bgr"]))


@pytest.mark.parametrize("seed", range(6))
def test_numpy_vs_c_on_random_scenes(built, seed):
    cams, masks, frames = fx.random_scene(seed, C=1 + seed % 4)
    oc = fx.oracle_cams(cams)
    nx, ny, nz = 9 + seed, 64 if seed % 2 else 17, 11
    for mv in (1, len(cams)):
        a = carve_np.carve(nx, ny, nz, oc, masks, frames, min_views=mv, color_cam=0)
        b = carve_c.carve(nx, ny, nz, oc, masks, frames, min_views=mv, color_cam=0, want_viewmask=True, want_lut=True)
        assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["viewmask"], b["viewmask"])
        assert np.array_equal(a["offsets"], b["offsets"]) and np.array_equal(a["bgr"], b["bgr"])


def _ring_scene(C, H, W, seed):
    """C ring cameras around the default volume, the ellipsoid's silhouettes with per-camera salt noise of different density
    (camera C-1 noise-free, camera 0 the densest) and random frames."""
    from voxcarve import synthetic
    cams = synthetic.ring_cameras(C, H, W)
    masks = synthetic.ellipsoid_masks(cams, H, W, noise=0.0)
    rng = np.random.default_rng(seed)
    for c, m in enumerate(masks):
        m[rng.random((H, W)) < 0.3 * (C - 1 - c) / max(C - 1, 1)] = 255
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(C)]
    return cams, masks, frames


@pytest.mark.parametrize("C", range(5, 17))
def test_numpy_vs_c_at_5_to_16_cameras(built, C):
    """The two oracles at every camera count the GPU rows above 4 cameras rest on: survivors, the u16 camera mask (bits up to
    15), the table, the colour camera's samples and its seen flag, at thresholds 1, ceil(C/2), C-1 and C, colour camera C-1."""
    grids = [(9, 17, 11), (6, 64, 5), (13, 7, 8)]
    scenes = [fx.random_scene(300 + C, C=C, fg=0.75), _ring_scene(C, 40, 56, 400 + C)]
    top = 0
    for k, (cams, masks, frames) in enumerate(scenes):
        oc = fx.oracle_cams(cams)
        grid = grids[(C + k) % 3]
        for mv in sorted({1, (C + 1) // 2, C - 1, C}):
            a = carve_np.carve(*grid, oc, masks, frames, min_views=mv, color_cam=C - 1)
            b = carve_c.carve(*grid, oc, masks, frames, min_views=mv, color_cam=C - 1, want_viewmask=True, want_lut=True)
            assert np.array_equal(a["idx"], b["idx"]) and b["count"] == a["idx"].size, (k, mv)
            assert np.array_equal(a["viewmask"], b["viewmask"]) and np.array_equal(a["offsets"], b["offsets"]), (k, mv)
            assert np.array_equal(a["bgr"], b["bgr"]), (k, mv)
            assert np.array_equal(a["color_seen"], ((b["viewmask"][b["idx"]] >> (C - 1)) & 1).astype(bool)), (k, mv)
            nviews = np.bitwise_count(a["viewmask"][a["idx"]])
            assert (nviews >= mv).all() and int((np.bitwise_count(a["viewmask"]) >= mv).sum()) == a["idx"].size
        top = max(top, int(a["viewmask"].max()))
        assert (a["viewmask"] >> (C - 1)).any(), k                 # the top camera's bit is set somewhere
    assert top.bit_length() == C


def test_literal_restatement_at_16_cameras(built):
    """The dict / loop mirror of the reference's Python at the camera cap: the same list, in order, as the numpy oracle and
    the C oracle, every voxel seen by all 16 cameras (the reference's threshold); colour camera key 2 as in the reference."""
    cams, masks, frames = _ring_scene(16, 30, 40, 16)
    for m in masks:
        m[:] = np.where(m > 0, 255, 0)
    oc = fx.oracle_cams(cams)
    n, half = 10, 6
    data, cols = carve_literal.set_voxel_positions(n, half, n, oc, masks, frames)
    res = carve_np.carve(n, 2 * half, n, oc, masks, frames)
    resc = carve_c.carve(n, 2 * half, n, oc, masks, frames, want_viewmask=True)
    assert len(data) == res["idx"].size > 0 and np.array_equal(res["idx"], resc["idx"]) and np.array_equal(res["bgr"], resc["bgr"])
    assert int(resc["viewmask"].max()) == 0xffff
    keys = carve_np.voxel_keys(res["idx"], n, 2 * half, n)
    assert np.array_equal(np.array(data), carve_np.viewer_positions(keys))
    assert np.array_equal(np.array(cols), carve_np.viewer_colors(res["bgr"]))


def test_degenerate_depth_zero_and_behind_camera(built):
    """z == 0 takes the `z ? 1/z : 1` branch; points behind the camera are not culled."""
    from voxcarve.camera import Camera
    cam = Camera(np.array([[50, 0, 20], [0, 50, 20], [0, 0, 1.0]]), np.zeros(5), np.zeros(3), np.zeros(3))
    pts = np.array([[1.0, 2.0, 0.0], [0.1, 0.1, -1.0], [0.0, 0.0, 5.0], [1e308, 1.0, 1e-308]])
    uv = carve_np.project_points(pts, cam.R, cam.tvec, cam.K, cam.dist)
    assert np.array_equal(uv[0], [70.0, 120.0])          # z = 0 -> scale 1
    assert np.array_equal(uv[1], [15.0, 15.0])           # behind the camera still projects
    assert np.array_equal(uv[2], [20.0, 20.0])
    uvc = carve_c.project(pts, (cam.K, cam.dist, cam.R, cam.tvec))
    off_np = carve_np.pixel_offsets(uv, 40, 40)
    off_c = carve_np.pixel_offsets(uvc, 40, 40)
    assert np.array_equal(off_np, off_c)                  # non-finite rows agree after the bounds test
    assert np.array_equal(uv[:3], uvc[:3])


def test_bounds_test_is_on_float_coordinates():
    uv = np.array([[-0.5, 3.0], [3.0, -0.25], [0.0, 0.0], [9.999, 4.999], [10.0, 1.0], [np.nan, 1.0], [np.inf, 1]])
    off = carve_np.pixel_offsets(uv, 5, 10)
    assert off.tolist() == [-1, -1, 0, 49, -1, -1, -1]


def test_index_range_slabs_concatenate(built, cams, masks, frames):
    oc = fx.oracle_cams(cams)
    full = carve_c.carve(32, 32, 32, oc, masks, frames)
    parts = [carve_c.carve(32, 32, 32, oc, masks, frames, index_range=(z0 * 1024, z1 * 1024))
             for z0, z1 in ((0, 10), (10, 11), (11, 32))]
    assert np.array_equal(np.concatenate([p["idx"] for p in parts]), full["idx"])
    assert np.array_equal(np.concatenate([p["bgr"] for p in parts]), full["bgr"])


def test_postfilter_restatement_small_cases():
    """2x2 open/close with OpenCV's top-left-biased window (background_subtraction.py:195-206); unpinned vs cv2."""
    from oracle import postfilter_np as pf
    a = np.zeros((5, 6), np.uint8)
    a[2, 3] = 255                                            # single pixel
    assert np.array_equal(pf.dilate2x2(a), np.pad(np.full((2, 2), 255, np.uint8), ((2, 1), (3, 1))))
    assert pf.erode2x2(a).sum() == 0
    assert pf.post_filter(a, True, False).sum() == 0         # opening removes a lone pixel
    b = np.full((5, 6), 255, np.uint8)
    b[2, 3] = 0                                              # single hole
    assert np.array_equal(pf.post_filter(b, False, True), np.full((5, 6), 255, np.uint8))   # closing fills it
    assert np.array_equal(pf.erode2x2(b) == 0, np.pad(np.ones((2, 2), bool), ((2, 1), (3, 1))))
    c = np.zeros((6, 6), np.uint8)
    c[1:4, 1:4] = 200                                        # 3x3 square survives, binarised -- and MOVES: erode and
    out = pf.post_filter(c, True, True)                      # dilate share the same un-reflected window, so each of
    assert out.dtype == np.uint8 and set(np.unique(out)) <= {0, 255}   # open and close shifts it one pixel down-right
    assert out[3:6, 3:6].all() and int((out > 0).sum()) == 9
    edge = np.zeros((4, 4), np.uint8)
    edge[0, :] = 255                                         # border row: outside pixels are ignored, not zero
    assert np.array_equal(pf.erode2x2(edge)[0], [255, 255, 255, 255])
    m = fx.golden_masks()[0]
    assert np.array_equal(pf.post_filter(m), m)              # no flags: only the binarisation


def test_marching_cubes_table_is_the_derived_one_and_sound():
    """SURVEY 8(f)-3.  The case table the HIP kernels include (csrc/mc_table.h, generated) equals the derivation in
    oracle/marching_np.py, and that table is sound: on spheres, a torus, a single voxel and noise (every ambiguous case) the
    mesh is closed, every edge is walked once in each direction (consistent ON -> OFF orientation), the Euler characteristic is
    that of the shape and the enclosed volume is positive and close to the voxel count.  Parity with scikit-image's Lewiner
    variant is UNPINNED (not importable here; the reference holds no mesh)."""
    import re
    from oracle import marching_np as mc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "voxel-based-3d-reconstruction_amd", "csrc", "mc_table.h")).read()
    ntri = [int(v) for v in re.search(r"kMcNtri\[256\] = \{([^}]*)\}", txt).group(1).split(",")]
    rows = re.findall(r"^    \{([^}]*)\},$", txt, re.M)
    assert ntri == [int(v) for v in mc.NTRI] and len(rows) == 256
    for c, row in enumerate(rows):
        assert [int(v) for v in row.split(",")][:15] == [int(v) for v in mc.TRI[c]], c

    def ball(n, r):
        g = np.indices((n, n, n)).astype(float) - (n - 1) / 2
        return (g ** 2).sum(0) <= r * r
    for vol, chi in ((ball(16, 5.3), 2), (ball(11, 3.0), 2)):
        for level in (0.5, 0.0):
            v, f = mc.extract(vol, level)
            closed, oriented, x, volume = mc.mesh_invariants(v, f)
            assert closed and oriented and x == chi and volume > 0
            if level == 0.5:
                assert abs(volume - vol.sum()) < 0.1 * vol.sum()
                assert np.all(np.isin((v * 2) % 2, (0, 1))) and np.all(((v * 2) % 2).sum(1) == 1)   # midpoints of grid edges
    n = 24
    g = np.indices((n, n, n)).astype(float) - (n - 1) / 2
    torus = ((np.sqrt(g[0] ** 2 + g[1] ** 2) - 7) ** 2 + g[2] ** 2) <= 3.2 ** 2
    assert mc.mesh_invariants(*mc.extract(torus, 0.5))[:3] == (True, True, 0)
    one = np.zeros((3, 3, 3), bool)
    one[1, 1, 1] = True
    v, f = mc.extract(one, 0.5)
    assert f.shape[0] == 8 and mc.mesh_invariants(v, f) == (True, True, 2, 1 / 6)          # an octahedron around the voxel
    rng = np.random.default_rng(0)
    noise = np.pad(rng.random((7, 8, 9)) < 0.5, 1)
    assert mc.mesh_invariants(*mc.extract(noise, 0.5))[:2] == (True, True)


def test_foreground_restatement_hsv_and_3x3_morphology():
    """oracle/foreground_np.py (parity with cv2 unpinned): the 8-bit HSV conversion against the textbook definition -- OpenCV's
    fixed-point result is within one count of the rounded real-valued H / 2, S, V on every one of 20 000 random colours and on
    the primaries exactly -- and the 3x3 erosion / dilation against a plain window loop."""
    import colorsys
    from oracle import foreground_np as fg
    prim = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [0, 255, 255], [255, 255, 0], [255, 0, 255], [0, 0, 0], [255, 255, 255],
                     [128, 128, 128]], np.uint8)                      # BGR: red, green, blue, yellow, cyan, magenta, black, white, grey
    want = [[0, 255, 255], [60, 255, 255], [120, 255, 255], [30, 255, 255], [90, 255, 255], [150, 255, 255], [0, 0, 0], [0, 0, 255], [0, 0, 128]]
    assert fg.bgr_to_hsv(prim).tolist() == want
    rng = np.random.default_rng(3)
    cols = rng.integers(0, 256, (20000, 3), dtype=np.uint8)
    got = fg.bgr_to_hsv(cols).astype(int)
    for (b, g, r), (h, s, v) in zip(cols.tolist()[:4000], got.tolist()[:4000]):
        hh, ss, vv = colorsys.rgb_to_hsv(r / 255.0, g / 255.0, b / 255.0)
        assert v == max(b, g, r) and abs(s - ss * 255.0) <= 1.0
        dh = abs(h - hh * 180.0)
        assert min(dh, 180.0 - dh) <= 1.0 or s == 0
    assert got[:, 0].max() < 180
    img = rng.integers(0, 256, (13, 17), dtype=np.uint8)
    ero, dil = fg.erode3x3(img), fg.dilate3x3(img)
    for y in range(13):
        for x in range(17):
            win = img[max(0, y - 1):y + 2, max(0, x - 1):x + 2]
            assert ero[y, x] == win.min() and dil[y, x] == win.max()
    assert np.array_equal(fg.pre_filter(img), img)
    assert np.array_equal(fg.pre_filter(img, True, True), fg.erode3x3(fg.dilate3x3(fg.dilate3x3(fg.erode3x3(img)))))


def test_mog_restatement_vectorised_equals_literal_and_behaves():
    """oracle/mog_np.py (parity with cv2 unpinned): the vectorised restatement of bgsegm's MOG against the literal per-pixel one --
    masks and every float of the state, bit for bit -- and the model's behaviour on what it is for: a static noisy background
    becomes background, a new object on it is foreground under learning rate 0, and learning rate 0 leaves the model untouched."""
    from oracle import mog_np
    rng = np.random.default_rng(5)
    bg = rng.integers(0, 256, (10, 14, 3), dtype=np.uint8)
    for kw in ({}, dict(history=5, nmixtures=2, backgroundRatio=0.5, noiseSigma=3), dict(nmixtures=8)):
        a, b = mog_np.MOG(**kw), mog_np.MOGLiteral(**kw)
        for t in range(22):
            f = rng.integers(0, 256, bg.shape).astype(np.uint8) if t % 6 == 4 else np.clip(bg.astype(int) + rng.integers(-15, 16, bg.shape), 0, 255).astype(np.uint8)
            lr = -1 if t < 12 else (0.1 if t < 18 else 0)
            assert np.array_equal(a.apply(f, lr), b.apply(f, lr)), (kw, t)
            assert np.array_equal(a.state.view(np.uint32), b.state.view(np.uint32)), (kw, t)
    m = mog_np.MOG()
    for t in range(40):
        mask = m.apply(np.clip(bg.astype(int) + rng.integers(-3, 4, bg.shape), 0, 255).astype(np.uint8), -1)
    assert not mask.any()
    before = m.state.copy()
    f = bg.copy(); f[2:6, 3:9] = 255 - f[2:6, 3:9]
    mask = m.apply(f, 0)
    assert mask[2:6, 3:9].all() and mask.sum() == 255 * 24 and np.array_equal(before, m.state)
    assert m.apply(f, -1)[2:6, 3:9].all()                       # a first sighting while learning is still foreground
