"""The carve at every camera count from 1 to 16 (VC_MAX_CAMERAS), against the C oracle: the camera-group loops of the box tests
(four cameras at a time: a short last group after a full one only at 6, 7, 9, 10, 11, 13, 14 and 15 cameras), the per-voxel level
one or two cameras per round trip, the camera visiting order, the brick pipeline's LDS budget edges, realistic rigs on the
automatic budget, a frame set carved by kernels of both LDS caps in turn, the launch-shape knobs at their limits and the post-carve
passes at mid camera counts.

Every row compares count, indices, order, colours and seen flags of both modes with the oracle (and the dense occupancy), and
asserts the kernel path it claims to run (timing_detail's per-kernel launches, the brick level's counters), so that a moved
threshold cannot silently turn a row into a copy of another."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fixtures_util as fx
from oracle import carve_c

pytestmark = pytest.mark.gpu

HIP = os.path.join(fx.ROOT, "voxel-based-3d-reconstruction_amd", "csrc")
H1, W1 = 1080, 1920
CLEAN = (2, 6, 10, 14)               # cameras without salt noise (the ones whose boxes can reject bricks)
HOLE, FULL = 6, 9                    # a camera with a wide band cut out of its silhouette, one almost all foreground

# every option a row below sets (restored to the library's initial value after each row)
OPTION_NAMES = ("lut_hier", "bricks", "cull", "lut_tile", "fused_tile", "fused_f32box", "fused_boxes", "fused_color_table", "first_kv",
                "refine_b", "reorder", "fused_hier", "refine_pair", "emit_lanes", "emit_busy", "force_generic", "grid_lds_kb",
                "voxel_pairs", "dbg", "voxel_batches", "hier_blocks_per_cu", "fused_blocks_per_cu", "first_blocks_per_cu",
                "refine_blocks_per_cu", "emit_waves_per_cu", "overlap")

# test_gpu_parity.py::test_every_kernel_family_agrees_with_oracle's list
FAMILIES = ({"lut_hier": 1}, {"bricks": 0}, {"cull": 0}, {"lut_tile": 0}, {"fused_tile": 0}, {"fused_color_table": 0}, {"fused_boxes": 0},
            {"fused_boxes": 0, "fused_f32box": 0}, {"fused_boxes": 0, "fused_tile": 0}, {"lut_hier": 0}, {"lut_hier": 0, "first_kv": 4},
            {"lut_hier": 1, "refine_b": 16, "refine_pair": 0}, {"reorder": 0}, {"fused_hier": 0}, {"refine_pair": 0}, {"emit_lanes": 0},
            {"emit_busy": 2}, {"emit_busy": 2, "lut_tile": 0, "fused_tile": 0}, {"grid_lds_kb": 64}, {"grid_lds_kb": 148, "voxel_pairs": 2},
            {"voxel_pairs": 1}, {"dbg": 8192}, {"grid_lds_kb": 148, "dbg": 8192}, {"grid_lds_kb": 148, "dbg": 16384}, {"force_generic": 1})


def _host_source():
    """The host side as the compiler reads it: voxcarve.hip and every host/*.h it includes, in its order."""
    top = open(os.path.join(HIP, "voxcarve.hip")).read()
    return top + "".join(open(os.path.join(HIP, f)).read() for f in re.findall(r'^#include "(host/\w+\.h)"', top, re.M))


def _constants():
    """The launch code's LDS constants, read from the sources (so that the rows follow them if they move)."""
    src = _host_source() + open(os.path.join(HIP, "vc_kernels.h")).read()
    val = {}
    for name in ("kMaxCameras", "kHdrShift", "kGridHeader", "kWideBlock", "kMaxFirstLds", "kWideGridBytes", "kMaxWideLds",
                 "kBusyListMinGroups"):
        expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1)
        assert re.fullmatch(r"[\w\s*+]+", expr), (name, expr)
        val[name] = eval(expr, {"__builtins__": {}}, dict(val))
    return val


def _defaults():
    """The initial value of every option in OPTION_NAMES: the initialiser of the vc_ctx field vc_set_option writes (the C ABI
    has no getter), read from the source so that the rows restore whatever the library starts with."""
    src = _host_source()
    ctx = re.search(r"^struct vc_ctx \{(.*?)^\};", src, re.S | re.M).group(1)
    out = {}
    for name in OPTION_NAMES:
        v = re.search(r"^\s+(?:int|bool) %s = (-?\d+|true|false);" % name, ctx, re.M).group(1)
        out[name] = {"true": 1, "false": 0}[v] if v in ("true", "false") else int(v)
    return out


K = _constants()
DEFAULTS = _defaults()
LISTS = {"most": False}              # the last brick-level step listed nine bricks in ten (launch_bricks: the next lists them all)


def regime(budget_words, C, dbg=0):
    """launch_bricks' choices for a frame set prepared with `budget_words` of header + grids (voxcarve.hip)."""
    lds = (budget_words + 8) * 4
    grid_words = (lds // 4 + 63) // 64 * 64
    with_ = (grid_words + (K["kWideBlock"] // 64) * 256) * 4
    wide = lds > K["kWideGridBytes"]
    compact = wide and with_ <= K["kMaxWideLds"] + 6 * 1024 and 4 < C <= 23 and not dbg & 16384
    return {"lds": lds, "wide": wide, "coarse": budget_words * 4 > K["kWideGridBytes"], "optin": lds > K["kMaxFirstLds"],
            "compact": compact, "launched": with_ if compact else lds}


def auto_budget(C, H, W, grid_min_shift=1):
    """ensure_prepared's budget for grid_lds_kb = 0 on the brick pipeline (cap 148 KB): 16 KB unless the frame set holds more
    than 2 MB of mask bits, then what the uncropped grids of all cameras take at the finest block that fits the cap."""
    cap = 148 * 256
    if (H * W + 31) // 32 * C * 4 <= 2 << 20:
        return 16 * 256
    for sh in range(grid_min_shift, 15):
        bw, bh = -(-W // (1 << sh)), -(-H // (1 << sh))
        total = K["kGridHeader"] + C * 2 * -(-bw // 32) * bh
        if total <= cap or sh == 14:
            return max(total, 16 * 256)


def label(r):
    return "narrow" if not r["wide"] else "compacted" if r["compact"] else "opt-in" if r["optin"] else "wide"


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def eng(built):
    import voxcarve
    e = voxcarve.CarveEngine(0)
    e.set_option("timing_detail", 1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def rig():
    return make_rig()


def make_rig():
    """16 ring cameras at 1080p, masks whose selectivity differs strongly by camera: ellipsoid silhouettes with salt noise of
    four densities (none on CLEAN), a wide band cut out of camera HOLE's, camera FULL almost all foreground."""
    from voxcarve import synthetic
    cams = synthetic.ring_cameras(16, H1, W1)
    masks = synthetic.ellipsoid_masks(cams, H1, W1, noise=0.0)
    rng = np.random.default_rng(77)
    for c, m in enumerate(masks):
        d = (0.01, 0.001, 0.0, 0.0002)[c % 4]
        if d:
            m[rng.random(m.shape) < d] = 255
    ys = np.nonzero(masks[HOLE].any(axis=1))[0]
    masks[HOLE][ys[0] + (ys[-1] - ys[0]) // 3: ys[0] + 2 * (ys[-1] - ys[0]) // 3] = 0
    masks[FULL][rng.random((H1, W1)) < 0.97] = 255
    return cams, masks


def pick(C, seed):
    """C of the 16 cameras in a shuffled order, at least one of them without noise."""
    order = [int(c) for c in np.random.default_rng(seed).permutation(16)[:C]]
    if not any(c in CLEAN for c in order):
        order[-1] = CLEAN[seed % 4]
    return order


def frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def load(eng, grid, cams, masks, cc, fr):
    LISTS["most"] = False                          # (new boxes: the brick level's list lengths are unknown again)
    eng.set_grid(*grid)
    eng.set_cameras(cams, *masks[0].shape)
    eng.upload_masks(masks)
    eng.upload_frame(cc, fr)
    eng.build_lut()


def oracle(grid, cams, masks, cc, fr, mv=None):
    frames = [None] * len(cams)
    frames[cc] = fr
    return carve_c.carve(*grid, fx.oracle_cams(cams), masks, frames, min_views=mv, color_cam=cc, want_viewmask=True,
                         cap=grid[0] * grid[1] * grid[2])


def brick_shape(grid):
    nx, ny, _ = grid
    return ny in (256, 512, 1024, 2048, 4096) and nx % 4 == 0 and (ny >= 1024 or nx % (4096 // ny) == 0)


# the kinds of a step's launches that route() predicts: the carve stage, the counting pass and the scans (the preparation kinds
# depend on what the frame set has been through, k_emit on nothing)
STEP_KINDS = frozenset(("k_cull_bricks", "k_brick_words", "k_voxel_words", "k_assemble", "one_launch_carve", "k_cull", "k_count_groups",
                        "k_scan_groups", "k_finish_scan"))


def route(grid, C, H, W, mode, mv, viewmask, opts):
    """The kinds of STEP_KINDS one vc_carve launches under these options (voxcarve.hip: plan_route / settle_route, the step's
    route).  load() has built the table under the default lut_tile before a row sets its options, so on a grid of tile shape the
    tile-ordered table, the tile boxes and the brick boxes exist whatever the row says."""
    o = {**DEFAULTS, **opts}
    nx, ny, nz = grid
    lut = mode == "lut"
    tiles = nx % 4 == 0 and ny % 64 == 0
    # one thread per voxel: thresholds below C, view masks, force_generic, masks larger than k_lut_first's LDS
    fast = mv == C and not viewmask and not o["force_generic"] and \
        not (lut and not o["lut_hier"] and (H * W + 31) // 32 * 4 > K["kMaxFirstLds"])
    if lut:
        tile_words = fast and tiles and o["lut_hier"] and o["lut_tile"]
    else:
        tile_words = fast and tiles and o["fused_hier"] and o["fused_tile"] and o["fused_boxes"]   # (the boxes' owner: cull and bricks)
    bricks = bool(tile_words and brick_shape(grid) and o["bricks"] and o["cull"])
    counted = fast and (lut or (ny % 64 == 0 and o["fused_hier"]))      # the kernel leaves its group counts
    kinds = {"k_scan_groups"}
    kinds |= {"k_cull_bricks", "k_brick_words", "k_voxel_words", "k_assemble"} if bricks else {"one_launch_carve"}
    if tile_words and not bricks and o["cull"]:
        kinds.add("k_cull")
    if not counted:
        kinds.add("k_count_groups")
    groups = -(-nx * ny * nz // 8192) * 2
    if o["emit_lanes"] and (o["emit_busy"] == 2 or (o["emit_busy"] == 1 and groups >= K["kBusyListMinGroups"])):
        kinds.add("k_finish_scan")                                       # the busy list
    return kinds


class Options:
    """Options of one row, restored on the way out; the frame set is prepared again on both sides (its LDS budget is read
    when it is prepared, with the cap of the kernels that first want its grids)."""
    def __init__(self, eng, opts):
        self.eng, self.opts = eng, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.eng.set_option(k, v)
        self.eng.touch_masks(0)

    def __exit__(self, *exc):
        for k in self.opts:
            self.eng.set_option(k, DEFAULTS[k])
        self.eng.touch_masks(0)


def check(eng, want, grid, C, mv, cc, tag, opts={}, viewmask=False, touch=False, modes=("lut", "fused"), lists=True):
    """One carve per mode: the oracle's records, occupancy (and camera masks), by exactly the step kinds route() names -- the
    brick pipeline or a one-launch kernel, k_cull in front of it, k_count_groups behind the kernels that leave no group counts,
    the busy list's k_finish_scan.  lists: also what the brick level's counters say.  Returns the kernels each mode launched."""
    seen_want = ((want["viewmask"][want["idx"]] >> cc) & 1).astype(bool)
    occ = np.zeros(grid[0] * grid[1] * grid[2], bool)
    occ[want["idx"]] = True
    o = {**DEFAULTS, **opts}
    H, W = eng.image_size
    launched = {}
    for mode in modes:
        kinds = route(grid, C, H, W, mode, mv, viewmask, opts)
        if touch:
            eng.touch_masks(0)
        eng.timing(reset=True)
        n = eng.carve(mode=mode, min_views=mv, color_cam=cc, viewmask=viewmask)
        ks = eng.timing()["kernels"]
        t = (tag, mode, mv)
        assert n == want["count"], t
        idx, rgb, seen = eng.fetch()
        assert np.array_equal(idx, want["idx"]), t
        assert np.array_equal(rgb[:, ::-1], want["bgr"]), t
        assert np.array_equal(seen, seen_want), t
        assert np.array_equal(eng.fetch_occupancy(), occ), t
        if viewmask:
            assert np.array_equal(eng.fetch_viewmask(), want["viewmask"]), t
        launched[mode] = ks
        assert set(ks) & STEP_KINDS == kinds, (t, sorted(ks), sorted(kinds))
        if "k_brick_words" in kinds and lists:
            dc = eng.debug_counters()
            assert dc["words_undecided"] > 0, (t, dc)
            if o["dbg"] & 8192:
                assert dc["bricks_listed"] == dc["bricks"], (t, dc)
            elif not LISTS["most"]:
                assert 0 < dc["bricks_listed"] < dc["bricks"], (t, dc)
            else:
                assert 0 < dc["bricks_listed"] <= dc["bricks"], (t, dc)
            # a step after one that listed nine bricks in ten lists them all without testing (launch_bricks)
            LISTS["most"] = dc["bricks_listed"] * 10 >= dc["bricks"] * 9
    return launched


# -------------------------------------------------------------------------------------------------- a. camera-count sweep
SWEEP_GRIDS = {"tile": (16, 128, 12), "bricks": (24, 512, 19), "ragged": (9, 70, 11)}   # bricks: partial bricks in x and z


@pytest.mark.parametrize("C", range(1, 17))
def test_camera_count_sweep(eng, rig, C):
    cams16, masks16 = rig
    order = pick(C, 1000 + C)
    cams, masks = [cams16[c] for c in order], [masks16[c] for c in order]
    cc = C - 1
    fr = frame(H1, W1, 50 + C)
    r = regime(auto_budget(C, H1, W1), C)
    assert r["wide"] == (C >= 9) and r["compact"] == (C >= 9)       # 1080p: the narrow path up to 8 cameras, then wide + compacted
    total = 0
    for shape, grid in SWEEP_GRIDS.items():
        load(eng, grid, cams, masks, cc, fr)
        # C first: the frame set is prepared by the kernels of the shape (brick pipeline: the 148 KB cap of the automatic budget)
        for mv in sorted({1, (C + 1) // 2, max(C - 1, 1), C}, reverse=True):
            want = oracle(grid, cams, masks, cc, fr, mv)
            check(eng, want, grid, C, mv, cc, (shape, C), viewmask=mv == 1 and C > 1)
            total += want["count"]
            if mv != C:
                continue
            assert want["count"] > 0, (shape, C)
            if shape == "bricks":
                # forced two / one camera per round trip, the word level's every-brick-listed and lockstep forms
                for opts in ({"voxel_pairs": 1}, {"voxel_pairs": 2}, {"dbg": 16384}, {"dbg": 8192}):
                    with Options(eng, opts):
                        check(eng, want, grid, C, mv, cc, (shape, C, opts), opts=opts)
            if shape != "ragged" and C in (6, 7, 9, 11, 13, 15):
                # (1080p masks are larger than k_lut_first's LDS: lut_hier 0 falls back to the one-thread-per-voxel kernel in
                # LUT mode here, and check() asserts it does; test_launch_knobs_at_their_limits reaches k_lut_first)
                for opts in FAMILIES:
                    with Options(eng, opts):
                        check(eng, want, grid, C, mv, cc, (shape, C, opts), opts=opts)
    assert total > 0


ROUTE_GRIDS = ((16, 128, 12), (8, 192, 9), (5, 70, 11), (16, 256, 20))   # tile words | tile_whole == 0 (zeroed counts) | no tiles | bricks
ROUTE_ROWS = tuple(r for k, r in enumerate(FAMILIES + ({"emit_busy": 2},)) if r not in FAMILIES[:k])


def test_route_kinds_of_every_family(eng):
    """Every option row on the smallest grid of every shape the step's route tells apart, both modes, at the threshold C with and
    without view masks and at C - 1: the oracle's records, by exactly the kinds route() names."""
    C = 4
    cams, masks, frames = fx.random_scene(321, C=C, H=60, W=80, fg=0.55)
    cc = 2
    total = 0
    for grid in ROUTE_GRIDS:
        load(eng, grid, cams, masks, cc, frames[cc])
        wants = {mv: oracle(grid, cams, masks, cc, frames[cc], mv) for mv in (C, C - 1)}
        total += wants[C]["count"]
        for opts in ROUTE_ROWS:
            with Options(eng, opts):
                for mv, vm in ((C, False), (C, True), (C - 1, False)):
                    check(eng, wants[mv], grid, C, mv, cc, (grid, opts), opts=opts, viewmask=vm, lists=False)
    assert total > 0


# ------------------------------------------------------------------------------------------------------------ b. LDS edges
LDS_KB = (19, 20, 21, 47, 48, 56, 63, 64, 65, 141, 142, 148)


def test_lds_rows_straddle_every_edge():
    """The explicit budgets of the rows below sit on both sides of each of launch_bricks' LDS edges, as the constants stand."""
    edges = {"1024-thread workgroups": lambda r: r["wide"], "coarse brick-level grids": lambda r: r["coarse"],
             "compaction launched above 64 KB": lambda r: r["launched"] > K["kMaxFirstLds"], "opt-in": lambda r: r["optin"],
             "compaction ceiling": lambda r: r["compact"] or not r["optin"]}
    for name, f in edges.items():
        pairs = [kb for kb in LDS_KB if kb - 1 in LDS_KB and f(regime(kb * 256, 9)) != f(regime((kb - 1) * 256, 9))]
        assert pairs, name                        # two rows one KB apart, one on each side
    # the row between the first two edges: 1024-thread workgroups without coarse grids (a k_cull_bricks branch of its own)
    assert any(regime(kb * 256, 9)["wide"] and not regime(kb * 256, 9)["coarse"] for kb in LDS_KB)
    # the window where the compacted word level takes more than 64 KB of a frame set that did not ask for the opt-in
    assert any(not regime(kb * 256, 9)["optin"] and regime(kb * 256, 9)["launched"] > K["kMaxFirstLds"] for kb in LDS_KB)


@pytest.mark.parametrize("C", [4, 5, 9, 16])
def test_lds_budget_edges(eng, rig, C):
    cams16, masks16 = rig
    order = pick(C, 2000 + C)
    cams, masks = [cams16[c] for c in order], [masks16[c] for c in order]
    cc = C - 1
    fr = frame(H1, W1, 60 + C)
    grid = (24, 512, 20)
    load(eng, grid, cams, masks, cc, fr)
    want = oracle(grid, cams, masks, cc, fr)
    assert want["count"] > 0
    seen = set()
    for kb in LDS_KB:
        for dbg in (0, 16384):
            seen.add(label(regime(kb * 256, C, dbg)))
            opts = {"grid_lds_kb": kb, "dbg": dbg}
            with Options(eng, opts):
                for step in range(3):             # later steps: sized by the lists of the ones before (and the nine-in-ten rule)
                    check(eng, want, grid, C, C, cc, (kb, dbg, step), opts=opts, touch=True)
    assert seen == ({"narrow", "wide", "opt-in", "compacted"} if C > 4 else {"narrow", "wide", "opt-in"})


def window_rows():
    """(C, kb) of the rows whose compacted word level takes more than kMaxFirstLds of a frame set that stays at or below it
    (launch_bricks sets the opt-in attribute only for lds > kMaxFirstLds, and then once per context, for every later launch)."""
    rows = []
    for C in (5, 9, 16):
        for kb in LDS_KB:
            r = regime(kb * 256, C)
            if r["compact"] and not r["optin"] and r["launched"] > K["kMaxFirstLds"]:
                rows.append((C, kb))
    return rows


def window_child():
    """The window rows alone, in a process of their own: nothing here launches more than kMaxFirstLds except the compacted
    word level of these rows, so the opt-in attribute is never set in this process.  Parity as everywhere else."""
    import voxcarve
    rows = window_rows()
    cams16, masks16 = make_rig()
    grid = (24, 512, 20)
    with voxcarve.CarveEngine(0) as eng:
        eng.set_option("timing_detail", 1)
        for C in sorted({C for C, _ in rows}):
            order = pick(C, 2000 + C)
            cams, masks = [cams16[c] for c in order], [masks16[c] for c in order]
            cc = C - 1
            fr = frame(H1, W1, 60 + C)
            want = oracle(grid, cams, masks, cc, fr)
            assert want["count"] > 0
            for kb in (kb for c, kb in rows if c == C):
                eng.set_option("grid_lds_kb", kb)          # before the first preparation of the frame set
                load(eng, grid, cams, masks, cc, fr)
                r = regime(kb * 256, C)
                assert r["lds"] <= K["kMaxFirstLds"] < r["launched"], (C, kb, r)
                for step in range(3):
                    check(eng, want, grid, C, C, cc, ("window", kb, step), opts={"grid_lds_kb": kb}, touch=step > 0)
    print("window rows passed without the opt-in:", rows)


def test_compaction_window_without_the_opt_in_in_a_fresh_process(built):
    """Does the runtime hold the compacted word level to the 64 KB default when launch_bricks has not set the opt-in attribute?
    Settled where no launch of the process has set it: the window rows in a child process of their own (the attribute is per
    function and process, and the module's other rows set it)."""
    rows = window_rows()
    assert {C for C, _ in rows} == {5, 9, 16} and len(rows) >= 6, rows
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_camera_counts as t; t.window_child()" % (fx.ROOT, fx.HERE)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=fx.ROOT)
    assert out.returncode == 0, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    assert "window rows passed without the opt-in" in out.stdout, out.stdout[-3000:]


# ---------------------------------------------------------------------------------------- c. realistic rigs, automatic budget
RIGS = [(8, 1080, 1920, "narrow"), (9, 1080, 1920, "compacted"), (12, 1080, 1920, "compacted"), (15, 1080, 1920, "compacted"),
        (6, 1440, 2560, "compacted"), (3, 2160, 3840, "opt-in"), (4, 2160, 3840, "opt-in")]


@pytest.mark.parametrize("C,H,W,regime_want", RIGS)
def test_realistic_rigs_on_the_automatic_budget(eng, rig, C, H, W, regime_want):
    from voxcarve import synthetic
    cams16, masks16 = rig
    order = pick(C, 3000 + C)
    r = regime(auto_budget(C, H, W), C)
    assert label(r) == regime_want, (C, H, W, r)
    if regime_want != "narrow":
        assert r["optin"]                       # every wide rig here takes more than 64 KB
    # the 1080p silhouettes resampled to the rig's size, with cameras made for it
    rows, cols = np.arange(H) * H1 // H, np.arange(W) * W1 // W
    cams = [synthetic.ring_cameras(16, H, W)[c] for c in order]
    masks = [masks16[c] if (H, W) == (H1, W1) else masks16[c][np.ix_(rows, cols)] for c in order]
    cc = C - 1
    fr = frame(H, W, 70 + C)
    grid = (32, 256, 20)
    load(eng, grid, cams, masks, cc, fr)
    want = oracle(grid, cams, masks, cc, fr)
    assert want["count"] > 0
    check(eng, want, grid, C, C, cc, ("rig", C, H))
    want1 = oracle(grid, cams, masks, cc, fr, mv=1)
    check(eng, want1, grid, C, 1, cc, ("rig", C, H), viewmask=True)


# ------------------------------------------------------------------------------------ d. budget transitions on one frame set
def test_wide_frame_set_carved_by_both_caps_in_turn(eng, rig):
    """A frame set prepared wide (100 KB) for the brick pipeline, then carved by the one-launch kernels (their 64 KB cap: the
    set is prepared again), then by the brick pipeline on the grids that preparation left (64 KB: not prepared again), and
    after touch_masks on 100 KB grids again -- one upload, both modes, every result the oracle's, every preparation where
    the LDS caps call for one (k_prep_pack / k_prep_grid among the step's launches)."""
    cams16, masks16 = rig
    C = 12
    order = pick(C, 4000)
    cams, masks = [cams16[c] for c in order], [masks16[c] for c in order]
    cc = C - 1
    fr = frame(H1, W1, 80)
    grid = (32, 256, 24)
    load(eng, grid, cams, masks, cc, fr)
    want = oracle(grid, cams, masks, cc, fr)
    assert want["count"] > 0
    assert regime(100 * 256, C)["compact"] and regime(64 * 256, C)["compact"] and regime(64 * 256, C)["lds"] > K["kMaxFirstLds"]
    # (bricks, touch first, prepared): the fourth step may prepare again or not (a 64 KB budget + header padding vs the cap)
    steps = ((1, True, True), (0, False, True), (1, False, False), (0, False, None), (1, False, False), (1, True, True))
    with Options(eng, {"grid_lds_kb": 100}):
        for mode in ("lut", "fused"):
            for k, (bricks, touch, prepared) in enumerate(steps):
                eng.set_option("bricks", bricks)
                ks = check(eng, want, grid, C, C, cc, ("transition", k, bricks), opts={"bricks": bricks}, modes=(mode,),
                           touch=touch)[mode]
                if prepared is not None:
                    assert ("k_prep_pack" in ks) == prepared and ("k_prep_grid" in ks) == prepared, (mode, k, sorted(ks))
            eng.set_option("bricks", 1)


# ---------------------------------------------------------------------------------------- e. launch-shape knobs at their limits
def test_launch_knobs_at_their_limits(eng):
    """Each launch-shape knob at its minimum, on a grid whose minimum launch must stride (1 152 groups of 4 096 voxels; the
    streaming and chunked kernels' minimum grids of 256 workgroups cover less than that), 12 cameras."""
    from voxcarve import synthetic
    C, H, W = 12, 480, 640
    cams = synthetic.ring_cameras(C, H, W)
    masks = synthetic.ellipsoid_masks(cams, H, W, noise=0.0)
    rng = np.random.default_rng(5)
    for c, m in enumerate(masks):
        m[rng.random(m.shape) < (0.004, 0.0, 0.001)[c % 3]] = 255
    order = [int(c) for c in rng.permutation(C)]
    cams, masks = [cams[c] for c in order], [masks[c] for c in order]
    cc = C - 1
    fr = frame(H, W, 90)
    grid = (128, 256, 144)
    assert grid[0] * grid[1] * grid[2] // 4096 > 1024
    load(eng, grid, cams, masks, cc, fr)
    want = oracle(grid, cams, masks, cc, fr)
    assert want["count"] > 0
    check(eng, want, grid, C, C, cc, "defaults")
    for opts in ({"hier_blocks_per_cu": 1, "bricks": 0}, {"fused_blocks_per_cu": 1, "fused_hier": 0},
                 {"first_blocks_per_cu": 1, "lut_hier": 0}, {"refine_blocks_per_cu": 1, "lut_hier": 0},
                 {"emit_waves_per_cu": 4, "emit_busy": 2}, {"voxel_batches": 1}, {"voxel_batches": 3}, {"voxel_batches": 16},
                 {"first_kv": 2, "lut_hier": 0}, {"lut_hier": 0, "refine_b": 16}):
        with Options(eng, opts):
            check(eng, want, grid, C, C, cc, opts, opts=opts)
    # one stream: scan and record expansion behind the carve, two steps in flight
    from voxcarve.engine import unpack_records
    with Options(eng, {"overlap": 0}):
        for mode in ("lut", "fused"):
            eng.carve_begin(mode=mode, color_cam=cc)
            eng.carve_begin(mode=mode, color_cam=cc)
            for _ in range(2):
                assert eng.carve_end() == want["count"], mode
                idx, rgb, seen = unpack_records(eng.fetch_records())
                assert np.array_equal(idx, want["idx"]) and np.array_equal(rgb[:, ::-1], want["bgr"]), mode


# ------------------------------------------------------------------------------------- f. post-carve passes at mid camera counts
@pytest.mark.parametrize("C", [9, 13])
def test_visible_and_photo_passes_at_mid_camera_counts(eng, C):
    """color_visible and photo_carve against their restatements with the top camera bit at 8 / 12: the textured pit seen by C
    ring cameras 45 degrees above it, handed over in a shuffled order."""
    import visible_np as vn
    import photo_np as pn
    from voxcarve import synthetic
    H, W = 240, 320
    ring = synthetic.ring_cameras(C, H, W, radius=2500.0, elevation_deg=45.0)
    order = [int(c) for c in np.random.default_rng(C).permutation(C)]
    cams = [ring[c] for c in order]
    masks, frames = synthetic.textured_scene(cams, H, W)
    ctr, half = np.array(synthetic.VOLUME_CENTRE), 1.15 * np.array(synthetic.PIT_HALF)
    lo, hi = ctr - half, ctr + half
    bounds = (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])
    grid = (48, 48, 48)
    eng.set_grid(*grid, bounds=bounds)
    eng.set_cameras(cams, H, W)
    eng.upload_masks(masks)
    for c, f in enumerate(frames):
        eng.upload_frame(c, f)
    eng.build_lut()
    oc = fx.oracle_cams(cams)
    for mode in ("fused", "lut"):
        S = eng.carve(mode=mode)
        rec0 = eng.fetch_records().copy()
        assert S > 0
        idx = (rec0 & 0xffffffff).astype(np.uint32)
        rgb0 = np.stack([(rec0 >> np.uint64(k)) & np.uint64(0xff) for k in (32, 40, 48)], axis=1).astype(np.uint8)
        assert np.array_equal(idx, carve_c.carve(*grid, oc, masks, frames, bounds=bounds)["idx"]), mode
        eng.color_visible()
        zmaps, vis, rgb = vn.color_visible(idx, rgb0, eng.grid, eng.bounds, oc, frames, H, W)
        wrec = (rec0 & np.uint64(0xff000000ffffffff)) | (rgb[:, 0].astype(np.uint64) << np.uint64(32)) | \
            (rgb[:, 1].astype(np.uint64) << np.uint64(40)) | (rgb[:, 2].astype(np.uint64) << np.uint64(48))
        for c in range(C):
            assert np.array_equal(eng.fetch_depth(c).view(np.uint32).reshape(-1), zmaps[c]), (mode, "depth map", c)
        got_vis = eng.fetch_visibility()
        assert np.array_equal(got_vis, vis), (mode, "camera masks")
        assert ((vis >> (C - 1)) & 1).any() and int(vis.max()).bit_length() == C
        assert np.array_equal(eng.fetch_records(), wrec), (mode, "records")
        # photo-consistency carving of the same hull
        eng.carve(mode=mode)
        st = eng.photo_carve(var_threshold=1200, min_views=2, max_rounds=32)
        want = pn.photo_carve(idx, rgb0, eng.grid, eng.bounds, oc, frames, H, W, var_threshold=1200, min_views=2, max_rounds=32)
        keep = want["rounds"] == 0
        assert st["survivors_before"] == S and st["survivors_after"] == want["idx"].size == eng.count, mode
        assert st["rounds"] == want["n_rounds"] and st["converged"] == want["converged"], mode
        assert np.array_equal(eng.fetch_photo_rounds(), want["rounds"]), mode
        wrec = (rec0[keep] & np.uint64(0xff000000ffffffff)) | (want["rgb"][:, 0].astype(np.uint64) << np.uint64(32)) | \
            (want["rgb"][:, 1].astype(np.uint64) << np.uint64(40)) | (want["rgb"][:, 2].astype(np.uint64) << np.uint64(48))
        assert np.array_equal(eng.fetch_records(), wrec), mode
        assert np.array_equal(eng.fetch_visibility(), want["vis"]), mode
        for c in range(C):
            assert np.array_equal(eng.fetch_depth(c).view(np.uint32).reshape(-1), want["zmaps"][c]), (mode, "photo depth map", c)
        occ = np.zeros(eng.n_voxels, dtype=bool)
        occ[want["idx"]] = True
        assert np.array_equal(eng.fetch_occupancy(), occ), mode
