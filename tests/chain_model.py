"""What a context holds behind a carve, as include/voxcarve.h describes it, in numpy and without a GPU: the current records, and for
every product of a post-carve pass whether it is valid and its bytes.  Every operation goes through the restatements that the
per-pass tests already hold the device to (oracle.carve_c / carve_np, footprint_np, closing_np, distance_np, components_np,
visible_np, photo_np, clusters_np, geodesic_np, normals_np, render_np, surface_np, temporal_np, measure_np, thin_np, shell_np,
setops_np, motion_np, texture_np, light_np, oracle.marching_np); nothing is restated here.  What this module adds is how the passes COMBINE: which records a pass starts from,
which frame set it reads, whose labels it takes, what it invalidates, and the state that outlives a result (the vote's ring, the
four hull registers, the images of the last render and of the passes over them).

Five families of chains.  A (SEEDS, CHAIN_LEN, KINDS) is drawn as it was before the vote, the measurements and the skeleton existed
and does not know them: tests/golden/chain_digests.json holds its records, so that it cannot move.  B (SEEDS_B, CHAIN_LEN_B,
KINDS_B) draws from every kind, with carve -> temporal pairs on different slots in most chains.  tests/test_gpu_chain.py walks family
A on the device; family B is held to its coverage conditions, its literal twins and its faults in tests/test_chain_model.py, and
its walk on the device is not in the suite (REFUSAL_B names what its products' fetches are to refuse with there): alone it passed
on the device, all 24 chains, and exited clean; the whole suite's process with it aborted at exit once more ("The abort
at exit").

Family C (SEEDS_C, CHAIN_LEN_C, KINDS_C) is family A's kinds and the hull registers: keep, upload, release, combine, compare
(tests/setops_np.py), motion, warp, paint_motion (tests/motion_np.py).  The model holds the four registers -- each None or
{occ, records or None} -- which outlive carves, passes and results, and the motion field, which is a product of the current result
AND tied to the register it was made against (item 8 of vc_hull_motion): a write to that register makes it stale and leaves every
other product.  REFUSAL_C names the two new products, `combined` (the added bytes of vc_hull_combine) and `motion`, and what their
fetches refuse with; tests/golden/chain_digests_c.json holds the family's record digests; tests/test_gpu_chain.py walks it on
the device and compares the registers (vc_fetch_kept) after every step as well.

Family D (SEEDS_D, CHAIN_LEN_D, KINDS_D) is family A's kinds and the passes over a render's images: shade (normals_np.shade),
texture (texture_np), light (light_np), surface_normals, and `feed`, which uploads or touches the masks of the carve's frame set
without carving.  The images of the last render and the three passes' images -- the products `shaded` (rgb of every view),
`textured` (rgb, depth, count, best_cam, refined) and `lit` (rgb, depth, kind, shadow, ao), Model.pictures -- are kept apart from
the products of the result: a carve or a hull changer leaves them to be fetched, the next render drops them, and the three passes
ask for a render OF THE CURRENT RESULT ("render" among the products).  A pass that only recolours (color_visible, the paints of
clusters and geodesic) leaves the generation alone: the render stays current, its rgb stays that of the old colours and is what a
pixel without a normal, without a camera or inside a survivor keeps, while the base colours of shade and light are the records' at
the call.  The model also holds which colour pass the depth maps belong to ("visibility" among the products), which frame sets
have input waiting and whether the carve's has been prepared again since the carve (texture with steps > 0, vc_surface_mesh's
rule), and whether the normals are current.  An operation whose prerequisites are missing is not kept out of the draw: the model
returns the refusal (OP_REFUSAL_D: a substring of the library's message) and leaves every byte as it was; a carve may carry a
`probe`, an image pass tried while its step is in flight or behind the same carve without records.  REFUSAL_D names what the
fetches of the three products refuse with while there are no images; tests/golden/chain_digests_d.json holds, per chain and step,
the digests of the records and of the three products; tests/test_gpu_chain.py walks the family on the device and compares every
pixel after every step.

Family E (SEEDS_E, CHAIN_LEN_E, KINDS_E) is family C's kinds, `temporal_motion` (vc_hull_temporal_motion, through
temporal_motion_np.AlignedVote) and temporal_reset; every `motion` carries `levels` and `refine` from PYRAMID_SETTINGS and runs
through motion_pyramid_np.match_pyramid where levels > 0.  The aligned vote goes on the SAME ring and P as the plain one
(Model.ring()): a ring filled by the other kind of call starts over, in both directions; the ring keeps the aligned hulls; the
call's own field is the product `temporal_field` (REFUSAL_E), refused while the votes are stale and after a plain vote, with no
rows behind the first push of a ring.  A vote that changes nothing leaves the generation and every product, a current motion
field included; one that changes the result takes the field with it.  A pyramid's `motion` product covers the rows of every
level, the level words of A and B and the scalars; `warp` reads level 0; `paint_motion` scales by the reach behind a pyramid and
by the search range behind a single level; a single-level call behind a pyramid leaves the levels 0..0.  A second vote on one
result is drawn on purpose and refused with the library's words (OP_REFUSAL_E), also behind a vote that changed nothing;
temporal_reset lifts it.  The plain vote, the measurements, the skeleton and the shell are not drawn here: the family's walk does
not lean on family B's.  tests/golden/chain_digests_e.json holds, per chain and step, the digests of records, registers, products
and ring; tests/test_gpu_chain.py walks the family on the device (test_chain_e).

The hull's shell (vc_hull_shell) is no drawn kind: neither family's draws may move.  with_shell(ops, seed) puts `shell` operations
at fixed places of a chain instead, without a random number; trace, run and replay take shell=True and walk the interleaved chain,
whose original steps keep their records and their products (tests/test_chain_model.py asserts it).

  scene(grid)            one of GRIDS, the golden cameras, three frame sets (slots 0, 1, 2) with different hulls and colours
  draw_chain(seed)       (scene, ops): CHAIN_LEN (family B: CHAIN_LEN_B, C: CHAIN_LEN_C, D: CHAIN_LEN_D, E: CHAIN_LEN_E) operations with all their parameters, drawn
                         with numpy.random.default_rng(seed) alone; some draws (min_voxels, the sources of a measurement, anchors,
                         which registers are filled, the hull of an upload) look at the model's state, so the chain is applied while
                         it is drawn
  Model(scene).apply(op) applies one operation; returns what the call returns and produces (stats, flags, labels, fields, images)
  replay(seed, upto=k)   the model in front of step k of that chain
  trace(seed)            one row per step (what ran, on how many records, whether the hull changed, ...) for the coverage conditions
  with_shell(ops, seed)  (ops with `shell` operations put in, for each the step of `ops` it stands for or None)

A record is uint64: the linear index in the low 32 bits, r, g, b in bytes 4 - 6, `seen` in byte 7.  The product names are those of
test_gpu_result_generation.REFUSAL / BUILT and, for the three passes that only family B knows and for the shell, of REFUSAL_B; for
the combine's added bytes and the motion field, of REFUSAL_C; for the shaded, textured and lit images, of REFUSAL_D."""
import hashlib
import os
import sys

import numpy as np

import closing_np as cl
import clusters_np as cn
import components_np as ccn
import distance_np as dn
import fixtures_util as fx
import footprint_np as fp
import geodesic_np as gn
import light_np as ln
import measure_np as mn
import motion_np as mo
import motion_pyramid_np as mp
import normals_np as nn
import photo_np as pn
import render_np as rn
import setops_np as so
import shell_np as shn
import surface_np as sn
import temporal_motion_np as tmn
import temporal_np as tpn
import texture_np as tn
import thin_np as thn
import visible_np as vn

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import carve_c, carve_np, marching_np                    # noqa: E402
from test_gpu_result_generation import BUILT, REFUSAL, RENDER_HW, _views   # noqa: E402

SEEDS = tuple(range(601, 625))              # family A: the 24 chains drawn before the vote, the measurements and the skeleton existed
CHAIN_LEN = 10
SEEDS_B = tuple(range(701, 725))            # family B: every kind
CHAIN_LEN_B = 14
SEEDS_C = tuple(range(801, 817))            # family C: family A's kinds and the hull registers
CHAIN_LEN_C = 12
GRIDS = ((40, 65, 36), (24, 130, 20), (30, 63, 30), (37, 53, 29))
BOUNDS = carve_np.DEFAULT_BOUNDS
ROLLS = (0, 9, -13)                         # columns the golden masks are rolled by in slots 0, 1, 2
SLOT_IMAGES = ((0, 1, 2, 3), (0, 1, 2, 3), (1, 2))   # cameras with an image per slot: slot 2 cannot feed a colour pass
FULL_SLOTS = tuple(s for s, cams in enumerate(SLOT_IMAGES) if len(cams) == 4)
COLOUR_CAMERAS = (None, 1, 2)
# the products of the passes that only family B knows, and of the shell that with_shell puts into a chain -> the refusal of their
# fetches (fetch_temporal; fetch_measure and, after profile=True, fetch_measure_profile; fetch_thin + fetch_skeleton; fetch_shell +
# fetch_shell_viewer) once the result is another (include/voxcarve.h)
REFUSAL_B = {"temporal": "no votes", "measure": "no measurements", "skeleton": "no skeleton", "shell": "no shell"}
# the products that only family C knows -> the refusal of vc_fetch_combined (its first three words are also vc_fetch_grown's) and of
# vc_fetch_motion, vc_hull_warp and vc_paint_motion
REFUSAL_C = {"combined": "no added flags: call vc_hull_combine", "motion": "no motion field"}
PRODUCTS = tuple(REFUSAL) + ("render", "surface") + tuple(REFUSAL_B) + tuple(REFUSAL_C)
assert set(PRODUCTS) >= BUILT and not set(REFUSAL_B) & (set(REFUSAL) | BUILT) and not set(REFUSAL_C) & (set(REFUSAL) | BUILT | set(REFUSAL_B))

HULL_CHANGERS = ("close", "dilate", "erode", "open", "filter_components", "photo_carve")
COMPACTIONS = ("erode", "open", "filter_components", "photo_carve")
COLOUR_PASSES = ("color_visible", "photo_carve")
QUIET = ("hull_distance", "hull_normals", "render", "surface_mesh")
KINDS = ("carve",) + HULL_CHANGERS + ("color_visible", "clusters", "geodesic") + QUIET
NEW_KINDS = ("temporal", "measure", "thin")
KINDS_B = KINDS + NEW_KINDS + ("temporal_reset",)
RECOLOURING = ("color_visible", "clusters", "geodesic", "paint_motion")   # change record colours and leave the hull alone
REGISTER_KINDS = ("keep", "upload", "release", "combine", "compare", "motion", "warp", "paint_motion")
KINDS_C = KINDS + REGISTER_KINDS
REGISTERS = 4                               # VC_HULL_REGISTERS
REGISTER_WRITERS = ("keep", "upload", "release", "warp")
MOTION_PARAMS = ((4, 0, 1), (4, 2, 2), (8, 4, 4), (16, 8, 4), (8, 4, 8))     # block edge, apron, search range
MOTION_ROW_KEYS = ("block", "ijk", "d", "cost", "cost0", "count_a", "count_b", "ties", "flags")
UPLOAD_SOURCES = ("carve", "eroded", "shifted", "empty", "full")
FAULTS_C = ("combine_slot0", "copy_keeps_a", "motion_survives_keep", "register_dies_with_carve", "noop_combine_invalidates")
MEASURE_SOURCES = ("all", "clusters", "geodesic", "components", "host")
SEEDS_D = tuple(range(901, 917))            # family D: family A's kinds and the passes over a render's images
CHAIN_LEN_D = 12
HW_D = (24, 32)                             # the size of family D's views: light_np at RENDER_HW made the CPU checks too slow.  3 x 4
#                                             tiles of 8 x 8 pixels per view; every pixel is compared on the device
VIEW_EYES = ((2500.0, 1500.0, -2000.0), (-1800.0, 2600.0, -900.0))   # test_gpu_result_generation._views': from the grid's centre, mm
IMAGE_PASSES = ("shade", "texture", "light")                 # they read the images of the last vc_render and make images of their own
IMAGE_KINDS = IMAGE_PASSES + ("surface_normals", "feed")
KINDS_D = KINDS + IMAGE_KINDS
# the images of the three passes -> the refusal of vc_fetch_shaded, vc_fetch_textured, vc_fetch_lit while there are none: before the
# pass has run on the LAST render (a carve does not touch them, the next vc_render drops them)
REFUSAL_D = {"shaded": "no shaded images: call vc_shade_render", "textured": "no textured images: call vc_texture_render",
             "lit": "no lit images: call vc_light_render"}
PICTURE_KEYS = {"shaded": ("rgb",), "textured": ("rgb", "depth", "count", "best_cam", "refined"), "lit": ("rgb", "depth", "kind", "shadow", "ao")}
# why a call of family D is refused -> a substring of the library's message (include/voxcarve.h lists the cases; the words are the
# library's).  The first seven are the ones the chains draw on purpose.
OP_REFUSAL_D = {"no_render": "no images of the current carve result: call vc_render",
                "no_depth_maps": "no depth maps of the current carve result: call vc_color_visible",
                "no_image_in_slot": "has no frame in slot 2",
                "fed": "has been prepared again since the carve, or has masks or images that wait for it",
                "stale_normals": "smooth = 1 and no normals: call vc_hull_normals",
                "no_records": "the last carve ran with VC_FLAG_NO_RECORDS",
                "in_flight": "carve steps are in flight: collect them with vc_carve_end",
                "no_normals": "no normals: call vc_hull_normals on the current carve result",
                "no_mesh": "no mesh of the current carve result: call vc_surface_mesh"}
DRAWN_REFUSALS = ("no_render", "no_depth_maps", "no_image_in_slot", "fed", "stale_normals", "no_records", "in_flight")
FAULTS_D = ("textured_survives_render", "lit_dies_with_carve", "stale_depth_maps_accepted", "texture_carve_slot", "recolour_stales_render",
            "render_follows_records", "smooth_accepts_stale_normals", "steps_ignore_feed")
LIGHT_POINTS = ((900.0, -1400.0, -2600.0), (-2000.0, 800.0, -1500.0), (0.0, 0.0, -3000.0))    # from the grid's centre, mm (up is -z)
LIGHT_SUNS = ((0.35, -0.5, -1.0), (-0.6, 0.2, -0.7), (0.0, 0.0, -1.0))                         # from the surface towards the light
FLOOR_CELL_MM, FLOOR_RGB = 170.0, ((70, 80, 90), (210, 200, 190))                               # test_gpu_light._floor's

SEEDS_E = tuple(range(1001, 1013))          # family E: family C's kinds, the aligned vote and the motion pyramid
CHAIN_LEN_E = 12
VOTE_KINDS = ("temporal_motion", "temporal_reset")
KINDS_E = KINDS_C + VOTE_KINDS
PYRAMID_SETTINGS = ((0, 1), (1, 1), (2, 2), (3, 1), (1, 2), (2, 1))      # levels, refine (at most the search range) of a `motion`
VOTE_PARAMS = ((4, 2, 2), (8, 4, 4), (4, 0, 1), (8, 4, 8), (16, 8, 4))   # block edge, apron, search range of an aligned vote
# the product that only family E knows -> the refusal of vc_fetch_temporal_motion: while the votes are stale, and after a plain vote
REFUSAL_E = {"temporal_field": "no field: call vc_hull_temporal_motion"}
# why a call of family E is refused -> a substring of the library's message
OP_REFUSAL_E = {"one_push": "one push per result"}
FAULTS_E = ("field_survives_vote", "aligned_ring_keeps_raw", "plain_ring_kept_by_aligned", "pyramid_paint_by_search",
            "levels_survive_single_motion")
assert not set(REFUSAL_E) & set(PRODUCTS)

LOW = np.uint64(0xffffffff)
NOT_RGB = np.uint64(0xff000000ffffffff)


# ---- records ----------------------------------------------------------------------------------------------------------------------
def pack(idx, rgb, seen):
    rgb = np.asarray(rgb, dtype=np.uint64).reshape(-1, 3)
    return np.asarray(idx, dtype=np.uint64) | (rgb[:, 0] << np.uint64(32)) | (rgb[:, 1] << np.uint64(40)) | \
        (rgb[:, 2] << np.uint64(48)) | (np.asarray(seen, dtype=np.uint64) << np.uint64(56))


def index_of(rec):
    return (np.asarray(rec, dtype=np.uint64) & LOW).astype(np.int64)


def rgb_of(rec):
    rec = np.asarray(rec, dtype=np.uint64)
    return np.stack([(rec >> np.uint64(s)) & np.uint64(255) for s in (32, 40, 48)], axis=1).astype(np.uint8).reshape(-1, 3)


def seen_of(rec):
    return ((np.asarray(rec, dtype=np.uint64) >> np.uint64(56)) & np.uint64(255)).astype(np.uint8)


def with_rgb(rec, rgb):
    return (np.asarray(rec, dtype=np.uint64) & NOT_RGB) | pack(np.zeros(len(rec), np.uint64), rgb, np.zeros(len(rec), np.uint64))


# ---- the scene --------------------------------------------------------------------------------------------------------------------
class Scene:
    """One grid, the golden cameras and three frame sets.  masks[slot][c] uint8 [H, W]; frames[slot][c] uint8 [H, W, 3] BGR or None."""

    def __init__(self, grid):
        self.grid = tuple(int(v) for v in grid)
        self.bounds = tuple(float(v) for v in BOUNDS)
        self.cams = fx.golden_cameras()
        self.oc = fx.oracle_cams(self.cams)
        golden = fx.golden_masks()
        self.H, self.W = golden[0].shape
        self.C = len(self.cams)
        self.masks = [[np.ascontiguousarray(np.roll(m, r, axis=1)) for m in golden] for r in ROLLS]
        every = fx.synthetic_frames(self.C * len(ROLLS), self.H, self.W)         # (slot 0 holds the suite's `frames` fixture)
        self.frames = [[every[self.C * s + c] if c in SLOT_IMAGES[s] else None for c in range(self.C)] for s in range(len(ROLLS))]
        self.q = dn.steps_um(self.grid, self.bounds)
        self.views = _views(self)
        self._views_at = {RENDER_HW: self.views}
        self._carves = {}
        self._matches = {}
        self._memo = {}

    def views_at(self, hw):
        """The two views of test_gpu_result_generation._views at another image size."""
        if hw not in self._views_at:
            from voxcarve import camera
            b = self.bounds
            ctr = np.array([(b[0] + b[1]) / 2, (b[2] + b[3]) / 2, (b[4] + b[5]) / 2])
            self._views_at[hw] = [camera.look_at(ctr + np.array(eye), ctr, 60.0, hw[0], hw[1]) for eye in VIEW_EYES]
        return self._views_at[hw]

    def mm(self, factor):
        """A radius in mm: `factor` times the grid's largest step; "below" is half the smallest one."""
        if factor == "below":
            return 0.5 * min(self.q) / 1000.0
        return float(factor) * max(self.q) / 1000.0

    def carve_records(self, slot, min_views, color_cam, footprint="centre"):
        """The records a carve of frame set `slot` leaves (the restatements' own, cached: many chains carve the same)."""
        key = (slot, min_views, color_cam, footprint)
        if key not in self._carves:
            nx, ny, nz = self.grid
            frames = self.frames[slot] if color_cam is not None else None
            if footprint == "centre":
                w = carve_c.carve(nx, ny, nz, self.oc, self.masks[slot], frames, bounds=self.bounds, min_views=min_views,
                                  color_cam=0 if color_cam is None else color_cam, want_viewmask=True)
                idx = w["idx"]
                if color_cam is None:
                    rec = pack(idx, np.zeros((idx.size, 3)), np.zeros(idx.size))
                else:
                    rec = pack(idx, w["bgr"][:, ::-1], (w["viewmask"][idx.astype(np.int64)] >> color_cam) & 1)
            else:
                w = fp.carve(self.grid, self.oc, self.masks[slot], footprint, frames=frames, min_views=min_views, color_cam=color_cam,
                             bounds=self.bounds)
                rec = pack(w["idx"], w["rgb"], w["seen"])
            rec.setflags(write=False)
            self._carves[key] = rec
        return self._carves[key]

    def memo(self, what, parts, make):
        """make() under the key (what, the parts' bytes): the lit and the textured images are the dearest restatements of family D,
        and a chain is applied once while it is drawn and again by whoever walks it."""
        h = hashlib.sha1(what.encode())
        for x in parts:
            h.update(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
            h.update(b"|")
        key = h.digest()
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def match(self, a, b_occ, b, ap, s, literal=False):
        """motion_np.match of two hulls of this grid (cached: the block matching is the dearest restatement of family C, and a chain
        is applied once while it is drawn and once more by whoever walks it)."""
        key = (hashlib.sha1(np.packbits(a)).digest(), hashlib.sha1(np.packbits(b_occ)).digest(), b, ap, s, bool(literal))
        if key not in self._matches:
            rows = (mo.match_literal if literal else mo.match)(a, b_occ, self.grid, b, ap, s)
            for v in rows.values():
                v.setflags(write=False)
            self._matches[key] = rows
        return self._matches[key]

    def match_pyramid(self, a, b_occ, b, ap, s, levels, refine, literal=False):
        """motion_pyramid_np.match_pyramid of two hulls of this grid, cached as match is."""
        key = (hashlib.sha1(np.packbits(a)).digest(), hashlib.sha1(np.packbits(b_occ)).digest(), b, ap, s, levels, refine, bool(literal))
        if key not in self._matches:
            self._matches[key] = (mp.match_pyramid_literal if literal else mp.match_pyramid)(a, b_occ, self.grid, b, ap, s, levels, refine)
        return self._matches[key]


class AlignedVote(tmn.AlignedVote):
    """temporal_motion_np's state machine with the scene's cache of block matchings behind it."""

    def __init__(self, sc, literal=False):
        self.scene, self.literal = sc, literal
        super().__init__()

    def match(self, hull, last, grid, b, ap, s):
        assert tuple(grid) == self.scene.grid
        return self.scene.match(hull, last, b, ap, s, self.literal)


_SCENES = {}


def scene(grid):
    grid = tuple(grid)
    if grid not in _SCENES:
        _SCENES[grid] = Scene(grid)
    return _SCENES[grid]


# ---- the model --------------------------------------------------------------------------------------------------------------------
class Model:
    """fault: None, or one deliberate mistake of the kind the chains exist to catch (tests/test_chain_model.py feeds it to the
    comparison on the CPU): "grow_slot0" colours added and restored voxels from slot 0 instead of the carve's slot, "drop_paint" gives the
    records that a compaction keeps the colours of the carve again, "temporal_forgets_prev" empties the vote's previous output
    at every carve (no hysteresis across frames), "measure_carve_colours" sums the colours the carve gave the records instead of
    the ones they have at the call, "shell_repainted" lets a valid shell take the new colours when a pass repaints the records
    (item 5 of vc_hull_shell: it holds the colours the records had at the call).  Family C's (FAULTS_C): "combine_slot0" colours
    the fresh records of a combine from slot 0, "copy_keeps_a" lets a restore keep A's bytes on the voxels both hulls hold (item 4
    of vc_hull_combine: every record is B's), "motion_survives_keep" leaves the motion field valid when its register is written
    (item 8 of vc_hull_motion), "register_dies_with_carve" empties the registers at every carve (they survive carves, passes
    and results), "noop_combine_invalidates" drops every product at a combine with R = A (item 5 of vc_hull_combine).  Family D's
    (FAULTS_D), each a plausible misreading of the header: "textured_survives_render" keeps the textured images over a new render,
    "lit_dies_with_carve" drops the lit ones at a carve, "stale_depth_maps_accepted" lets texture read the depth maps of a colour
    pass made before the hull changed, "texture_carve_slot" samples the carve's frame set instead of the call's,
    "recolour_stales_render" makes the render stale at a pass that only recolours, "render_follows_records" gives the pixels that
    keep the render's rgb the colours the records have now, "smooth_accepts_stale_normals" lets a smooth light read normals of a
    hull that is gone, "steps_ignore_feed" lets texture refine against a frame set that has been fed since the carve.  Family E's
    (FAULTS_E): "field_survives_vote" keeps the motion field over a vote that changes the result, "aligned_ring_keeps_raw" lets the
    aligned vote's ring keep the hulls as they were pushed, "plain_ring_kept_by_aligned" lets the aligned vote go on with a ring
    and a P that the plain vote filled, "pyramid_paint_by_search" scales the paint behind a pyramid by the search range instead
    of the reach, "levels_survive_single_motion" leaves a pyramid's coarser levels in the field behind a single-level call."""

    def __init__(self, sc, fault=None, literal=False, hw=RENDER_HW):
        self.scene = sc
        self.hw = tuple(hw)                  # the size of the rendered views (family D: HW_D) ...
        self.views = sc.views_at(self.hw)    # ... and the views
        self.literal = literal               # the restatements' literal twins where a pass has one that is affordable here
        self.grid, self.bounds = sc.grid, sc.bounds
        self.fault = fault
        self.records = None                  # uint64 [S]; None before the first carve
        self.carve = None                    # slot, min_views, color_cam of the carve that made the result
        self.carved = None                   # its records
        self.products = {}                   # name -> bytes, for the valid ones
        self.mesh_shape = (0, 0)             # (V, F) of the last surface mesh
        self.painted = False                 # a colour pass or a paint has run since the carve
        self.vote = tpn.Vote()               # the ring and P of vc_hull_temporal: they outlive carves, passes and results
        self.avote = AlignedVote(sc, literal)  # the same ring and P while vc_hull_temporal_motion fills them (temporal_motion_np's
        self.aligned = False                 # words): `aligned` says which kind of call filled the ring; the other kind starts it over
        self.vote_params = None              # block, apron, search of the last aligned vote: the scalars of its field
        self.labels = {}                     # what a measurement or a skeleton may read while the product of that name is valid:
        #                                      "clusters" (u8 labels, K), "geodesic" (u8 labels, extremities, distances),
        #                                      "component_labels" (the dict of components_np)
        self.shell_level = 0                 # the level of the last shell
        self.registers = [None] * REGISTERS  # each None or {"occ": bool [nz, nx, ny], "records": uint64 [count] or None, "origin":
        #                                      what wrote it, for the traces}: they outlive carves, passes and results
        self.field = None                    # the last motion field: rows, b, a, s and the register it was made against; it is
        #                                      current while "motion" is among the products
        # family D: the images of the last render and of the passes over them.  They are kept apart from the products: a carve or a
        # hull changer leaves them to be fetched, and only the next render drops them.  "render" among the products says that the
        # images are OF THE CURRENT RESULT, which is what the three passes ask for.
        self.images = None                   # index, depth, face, rgb [V, H, W(, 3)] of the last render
        self.pictures = {}                   # "shaded" | "textured" | "lit" -> {key: array [V, H, W(, 3)]} (PICTURE_KEYS)
        self.n4 = None                       # the stored normals; current while "normals" is among the products
        self.zmaps = None                    # the depth maps of the last colour pass; current while "visibility" is among the products
        self.dirty = set()                   # frame sets with masks or images that wait to be prepared (a feed)
        self.prepared_again = False          # the carve's frame set has been prepared since the carve: its masks are others
        self.recoloured = False              # a pass has recoloured the records since the render: its rgb is of the old colours

    # what the result is
    @property
    def S(self):
        return int(self.records.size)

    @property
    def idx(self):
        return index_of(self.records)

    @property
    def rgb(self):
        return rgb_of(self.records)

    def occ(self):
        return dn.volume(self.idx, self.grid)

    def min_views(self):
        return max(int(self.carve["min_views"]), 1)

    def _changed(self, own=None):
        self.products = dict(own or {})

    def _compacted(self, keep):
        rec = self.records[keep]
        if self.fault == "drop_paint" and rec.size:
            base, i = self.carved, index_of(rec)
            pos = np.minimum(np.searchsorted(index_of(base), i), max(base.size - 1, 0))
            hit = index_of(base)[pos] == i if base.size else np.zeros(i.size, bool)
            rec = rec.copy()
            rec[hit] = base[pos[hit]]
        return rec

    # the operations
    def apply(self, op):
        out = getattr(self, "_" + op["op"])(op)
        if self.fault == "shell_repainted" and op["op"] in RECOLOURING and "shell" in self.products:
            self.products["shell"] = self._shell_product(shn.shell(self.records, self.grid, self.shell_level))
        if op["op"] in RECOLOURING and "render" in self.products:    # the generation stays: the render is still of the current
            self.recoloured = True                                   # result, and its rgb of the colours it saw
            if self.fault == "recolour_stales_render":
                del self.products["render"]
        out["survivors"] = self.S
        return out

    def _prepares(self, slot):
        """A pass that reads the images of frame set `slot` brings waiting input into the device's layout first: the set is
        prepared again, and if it is the carve's, its masks are no longer the ones the occupancy came from."""
        if slot in self.dirty:
            self.dirty.discard(slot)
            if slot == self.carve["slot"]:
                self.prepared_again = True

    def _carve(self, op):
        sc = self.scene
        out = {}
        if op.get("first") is not None:          # two steps in flight, both collected: the second one is current
            f = op["first"]
            out["first_records"] = sc.carve_records(f["slot"], f["min_views"], f["color_cam"])
            self.dirty.discard(f["slot"])
        if op.get("probe") is not None:          # family D: an image pass tried while this carve's step is in flight, or behind the
            why = op["probe"]["how"]             # same carve without records; the pass_open of every pass refuses it
            out.update(refused=why, refusal=OP_REFUSAL_D[why])
        self.dirty.discard(op["slot"])           # the carve prepares what waits for its frame set
        self.prepared_again = False
        if self.fault == "lit_dies_with_carve":
            self.pictures.pop("lit", None)
        rec = sc.carve_records(op["slot"], op["min_views"], op["color_cam"], op["footprint"])
        self.records = rec.copy()
        self.carved = rec
        self.carve = {k: op[k] for k in ("slot", "min_views", "color_cam")}
        self.painted = False
        self._changed()
        if self.fault == "temporal_forgets_prev":
            self.vote.prev = None
        if self.fault == "register_dies_with_carve":
            self.registers = [None] * REGISTERS
        out["count"] = int(rec.size)
        return out

    def _grow(self, op):
        sc = self.scene
        r2 = dn.radius_r2(op["radius_mm"])
        S0 = self.S
        new_occ, dilated, cells = cl.grow(self.occ(), sc.q, r2, op["op"])
        cc = self.carve["color_cam"]
        slot = 0 if self.fault == "grow_slot0" else self.carve["slot"]
        rec, added = cl.records_after(self.records, new_occ, self.grid, self.bounds, None if cc is None else sc.oc[cc],
                                      None if cc is None else sc.frames[slot][cc], sc.H, sc.W)
        n_added = int(added.sum())
        if n_added:
            self.records = rec
            self._changed({"grown": added.tobytes()})
        else:                                    # the result stays; the transforms took the distance field's buffer (no hull, no transform)
            assert np.array_equal(rec, self.records)
            if S0:
                self.products.pop("distance", None)
            self.products["grown"] = added.tobytes()
        return {"stats": {"survivors_before": S0, "dilated": dilated, "survivors_after": int(rec.size), "added": n_added,
                          "box_cells": cells, "q": sc.q}, "added": added, "changed": n_added > 0}

    _close = _grow
    _dilate = _grow

    def _shrink(self, op):
        sc = self.scene
        r2 = dn.radius_r2(op["radius_mm"])
        occ, idx, S0 = self.occ(), self.idx, self.S
        opened, eroded = dn.open_(occ, sc.q, r2, op["border"])
        keep = (opened if op["op"] == "open" else eroded).reshape(-1)[idx]
        d_in = dn.inside_box(occ, sc.q, op["border"]).reshape(-1)[idx]
        self.records = self._compacted(keep)
        self._changed()
        return {"stats": {"survivors_before": S0, "eroded": int(eroded.sum()), "survivors_after": self.S,
                          "max_d2": int(d_in.max()) if S0 else 0, "q": sc.q}, "changed": self.S != S0}

    _erode = _shrink
    _open = _shrink

    def _filter_components(self, op):
        S0 = self.S
        w = (ccn.components_literal if self.literal else ccn.components)(self.idx, self.grid, op["connectivity"], op["min_voxels"], op["keep_largest"])
        self.records = self._compacted(w["keep"])
        self._changed({"component_labels": w["labels"].tobytes()})
        self.labels["component_labels"] = w
        K = int(w["label"].size)
        return {"stats": {"components": K, "components_kept": int(w["kept"].sum()), "survivors_before": S0, "survivors_after": self.S,
                          "largest": int(w["size"].max()) if K else 0},
                "components": {k: w[k] for k in ("label", "size", "lo", "hi", "kept")}, "labels": w["labels"], "changed": self.S != S0}

    def _photo_carve(self, op):
        sc = self.scene
        S0, rec0 = self.S, self.records
        w = (pn.photo_carve_literal if self.literal else pn.photo_carve)(self.idx, self.rgb, self.grid, self.bounds, sc.oc, sc.frames[op["slot"]], sc.H, sc.W, max_rounds=op["max_rounds"])
        keep = w["rounds"] == 0
        kept = self._compacted(keep)
        if self.fault == "drop_paint":           # (the colouring of the kept records starts from what the compaction handed over)
            w = dict(w, rgb=vn.color_visible(index_of(kept), rgb_of(kept), self.grid, self.bounds, sc.oc, sc.frames[op["slot"]], sc.H, sc.W)[2])
        self.records = with_rgb(rec0[keep], w["rgb"])
        self.painted = True
        self._changed({"visibility": w["vis"].tobytes(), "photo_rounds": w["rounds"].tobytes()})
        self._prepares(op["slot"])
        self.zmaps = w["zmaps"]
        return {"stats": {"rounds": w["n_rounds"], "converged": bool(w["converged"]), "survivors_before": S0, "survivors_after": self.S},
                "rounds": w["rounds"], "vis": w["vis"], "zmaps": w["zmaps"], "changed": self.S != S0}

    def _color_visible(self, op):
        sc = self.scene
        zmaps, vis, rgb = (vn.color_visible_literal if self.literal else vn.color_visible)(self.idx, self.rgb, self.grid, self.bounds, sc.oc, sc.frames[op["slot"]], sc.H, sc.W)
        self.records = with_rgb(self.records, rgb)
        self.painted = True
        self.products["visibility"] = vis.tobytes()
        self._prepares(op["slot"])
        self.zmaps = zmaps
        return {"vis": vis, "zmaps": zmaps}

    def _clusters(self, op):
        qxy = cn.steps_um_xy(self.grid, self.bounds)
        w = (cn.clusters_literal if self.literal else cn.clusters)(self.occ(), qxy, op["k"], max_iters=op["max_iters"], min_column=op["min_column"])
        d = cn.describe(self.records, self.grid, w)                          # (the histograms: the colours in front of the paint)
        self.products["clusters"] = d["labels"].tobytes()
        self.labels["clusters"] = (d["labels"], int(op["k"]))
        self.records = cn.paint(self.records, d["labels"], op["palette"])
        self.painted = True
        return {"stats": {k: w[k] for k in ("survivors", "columns", "weight", "iterations", "q")}, "converged": bool(w["converged"]),
                "clusters": w, "describe": d}

    def _geodesic(self, op):
        sc = self.scene
        idx = self.idx
        srec = gn.seeds_by_layer(idx, self.grid, op["seeds"], op["layers"])
        w = gn.geodesic(idx, self.grid, sc.q, op["connectivity"], srec, op["extrema"], method="dijkstra" if self.literal else "bellman")
        self.products["geodesic"] = w["d"].tobytes()
        self.labels["geodesic"] = (w["labels"], int(w["extremities"]), w["d"])
        self.records = with_rgb(self.records, gn.paint(self.rgb, w["keys"], op["paint"], op["palette"], w["max_d"]))
        self.painted = True
        rows = [(x["label"], x["voxel"], x["record"], x["d"], x["ix"], x["iy"], x["iz"]) for x in w["extrema"]]
        return {"stats": {k: w[k] for k in ("survivors", "seeds", "reached", "unreached", "max_d", "extremities", "edge_um", "q")},
                "d": w["d"], "labels": w["labels"], "extrema": rows}

    def _hull_distance(self, op):
        sc = self.scene
        occ, idx = self.occ(), self.idx
        field = dn.inside_box(occ, sc.q, op["border"])
        wrec = field.reshape(-1)[idx]
        self.products["distance"] = field.tobytes()
        out = {"stats": {"survivors": self.S, "max_d2": int(wrec.max()) if self.S else 0, "q": sc.q}, "inside": field, "records": wrec}
        if op["outside"]:
            out["outside"] = dn.outside(occ, sc.q)
        return out

    def _hull_normals(self, op):
        n4, st = (nn.normals_literal if self.literal else nn.normals)(self.occ(), self.scene.q, dn.radius_r2(op["radius_mm"]))
        self.products["normals"] = n4.tobytes()
        self.n4 = n4
        return {"stats": st, "n4": n4}

    def _render(self, op):
        sc = self.scene
        H, W = self.hw
        w = rn.render(self.occ().reshape(-1), self.idx.astype(np.uint32), self.rgb, self.grid, self.bounds,
                      [rn.view_params(v) for v in self.views], H, W, block=8)
        V = len(self.views)
        index, depth = w["index"].reshape(V, H, W), w["depth"].reshape(V, H, W)
        self.products["render"] = index.tobytes() + depth.tobytes()
        self.images = {"index": index, "depth": depth, "face": w["face"].reshape(V, H, W), "rgb": w["rgb"].reshape(V, H, W, 3)}
        dropped = tuple(sorted(self.pictures))   # the images of the passes over the render before: they do not outlive it
        self.pictures = {k: v for k, v in self.pictures.items() if self.fault == "textured_survives_render" and k == "textured"}
        self.recoloured = False
        return dict(self.images, dropped=dropped, stats={"pixels": V * H * W, "hits": int((index != rn.MISS).sum())})

    # the passes over the render's images.  A call whose prerequisites are missing returns {"refused": the case, "refusal": a
    # substring of the library's message} and changes nothing; the cases are tried in the order the library tries them.
    @staticmethod
    def _refused(why):
        return {"refused": why, "refusal": OP_REFUSAL_D[why]}

    def render_rgb(self):
        """The render's own rgb, which a pixel without a normal, without a camera or inside a survivor keeps: of the colours the
        records had at the render."""
        if self.fault != "render_follows_records" or "render" not in self.products:
            return self.images["rgb"]
        rgb = self.images["rgb"].copy()          # (the wrong model: the colours the records have now)
        hit = self.images["index"] != rn.MISS
        if hit.any():
            rgb[hit] = self.rgb[np.searchsorted(self.idx, self.images["index"][hit].astype(np.int64))]
        return rgb

    def flat_images(self):
        V, (H, W) = len(self.views), self.hw
        ren = {k: self.images[k].reshape(V, H * W) for k in ("index", "depth", "face")}
        ren["rgb"] = self.render_rgb().reshape(V, H * W, 3)
        return ren

    def _pictured(self, name, w):
        V, (H, W) = len(self.views), self.hw
        self.pictures[name] = {k: np.ascontiguousarray(np.asarray(w[k]).reshape((V, H, W) + ((3,) if k == "rgb" else ())).astype(
            np.float32 if k == "depth" else np.uint8)) for k in PICTURE_KEYS[name]}

    def _shade(self, op):
        if "normals" not in self.products:
            return self._refused("no_normals")
        if "render" not in self.products:
            return self._refused("no_render")
        ren = self.flat_images()
        idx32, rgb = self.idx.astype(np.uint32), self.rgb
        self._pictured("shaded", {"rgb": np.stack([nn.shade(ren["index"][v], ren["rgb"][v], idx32, rgb, self.n4, op["light"][v], op["ambient"])
                                                   for v in range(len(self.views))])})
        return {}

    def texture_refusal(self, op):
        if "render" not in self.products:
            return "no_render"
        if "visibility" not in self.products and not (self.fault == "stale_depth_maps_accepted" and self.zmaps is not None):
            return "no_depth_maps"
        if len(SLOT_IMAGES[op["slot"]]) < self.scene.C:
            return "no_image_in_slot"
        fed = self.prepared_again or (op["slot"] == self.carve["slot"] and op["slot"] in self.dirty)
        if op["steps"] > 0 and fed and self.fault != "steps_ignore_feed":
            return "fed"
        return None

    def _texture(self, op):
        sc = self.scene
        why = self.texture_refusal(op)
        if why:
            return self._refused(why)
        self._prepares(op["slot"])
        H, W = self.hw
        ren = self.flat_images()
        slot = self.carve["slot"] if self.fault == "texture_carve_slot" and self.carve["slot"] in FULL_SLOTS else op["slot"]
        masks = np.stack([m > 0 for m in sc.masks[self.carve["slot"]]])
        views = [rn.view_params(v) for v in self.views]
        kw = dict(steps=op["steps"], reach=op["reach_mm"], tol=op["depth_tolerance"], best=op["best"], sharpen=op["sharpen"], filt=op["filter"])
        hit = ren["index"] != rn.MISS
        w = dict(sc.memo("texture", [ren["index"], ren["depth"], ren["rgb"], self.zmaps, self.carve["slot"], self.min_views(), slot, sorted(kw.items())],
                         lambda: tn.texture(views, H, W, hit, ren["depth"], ren["rgb"], sc.oc, masks, self.min_views(), self.zmaps, sc.frames[slot], **kw)))
        if self.literal:                         # the literal twin, one pixel at a time, on every pixel of view `literal_view`
            v = op.get("literal_view", 0)
            one = tn.texture_literal(views[v], H, W, hit[v], ren["depth"][v], ren["rgb"][v], sc.oc, masks, self.min_views(), self.zmaps,
                                     sc.frames[slot], **kw)
            for k in PICTURE_KEYS["textured"]:
                w[k] = np.array(w[k], copy=True)
                w[k][v] = one[k]
        self._pictured("textured", w)
        return {"stats": w["stats"]}

    def light_params(self, op):
        """The `lt` of light_np: the operation's light, with the floor (None or test_gpu_light._floor's) spelled out."""
        return {"pos": op["pos"], "ambient": op["ambient"], "smooth": int(op["smooth"]), "ao_reach": op["ao_reach"], "floor": op["floor"]}

    def _light(self, op):
        if "render" not in self.products:
            return self._refused("no_render")
        if op["smooth"] and "normals" not in self.products and not (self.fault == "smooth_accepts_stale_normals" and self.n4 is not None):
            return self._refused("stale_normals")
        sc = self.scene
        H, W = self.hw
        views = [rn.view_params(v) for v in self.views]
        args = (self.occ().reshape(-1), self.idx.astype(np.uint32), self.rgb, self._n4_for_light() if op["smooth"] else None, self.grid, self.bounds, views, H, W,
                self.flat_images(), self.light_params(op))
        w = dict(sc.memo("light", [self.records] + [args[9][k] for k in ("index", "depth", "face", "rgb")] + [args[3], sorted(args[10].items())],
                         lambda: ln.light(*args, block=8)))
        if self.literal:                         # the literal twin, one ray at a time, on the pixels of `literal_pixels`
            px = np.asarray(op.get("literal_pixels", np.arange(H * W)), dtype=np.int64)
            ren = {k: v[:, px] for k, v in args[9].items()}
            one = ln.light_literal(*args[:9], ren, args[10], pixels=px)
            for k in PICTURE_KEYS["lit"]:
                w[k] = np.array(w[k], copy=True)
                w[k][:, px] = one[k]
        self._pictured("lit", w)
        return {"stats": w["stats"]}

    def _n4_for_light(self):
        if "normals" in self.products:
            return self.n4
        return np.resize(self.n4, (self.S, 4)) if self.n4.size else np.zeros((self.S, 4), np.int16)   # (the wrong model's stale ones)

    def _surface_normals(self, op):
        if "normals" not in self.products:
            return self._refused("no_normals")
        if "surface" not in self.products:
            return self._refused("no_mesh")
        el, axis, on_low = sn.mesh_edges(self.occ().reshape(-1), self.grid)
        nx, ny, _ = self.grid
        on = np.where(on_low, el, el + np.array([nx * ny, ny, 1], dtype=np.int64)[axis])
        return {"n4": self.n4[np.searchsorted(self.idx, on)]}

    def _feed(self, op):
        """Masks of the carve's frame set uploaded again, or touched: the same bytes, which wait to be prepared."""
        self.dirty.add(op["slot"])
        return {}

    def picture_digest(self, name):
        """sha1 of one pass's images (PICTURE_KEYS' order), None while there are none."""
        if name not in self.pictures:
            return None
        return hashlib.sha1(b"".join(self.pictures[name][k].tobytes() for k in PICTURE_KEYS[name])).hexdigest()

    def pictures_digest(self):
        """sha1 over the images of the three passes that exist, sorted by name: each name and its bytes (PICTURE_KEYS' order)."""
        h = hashlib.sha1()
        for name in sorted(self.pictures):
            h.update(name.encode())
            for k in PICTURE_KEYS[name]:
                h.update(self.pictures[name][k].tobytes())
        return h.hexdigest()

    def _surface_mesh(self, op):
        sc = self.scene
        masks = np.stack([m > 0 for m in sc.masks[self.carve["slot"]]])
        w = sn.surface_mesh(self.occ().reshape(-1), self.idx, self.rgb, self.grid, self.bounds, sc.oc, masks, self.min_views(),
                            op["refine_steps"])
        self.mesh_shape = (int(w["verts"].shape[0]), int(w["faces"].shape[0]))
        self.products["surface"] = np.ascontiguousarray(w["verts"]).tobytes() + np.ascontiguousarray(w["faces"]).tobytes()
        return {"mesh": w, "stats": dict(w["stats"], n_faces=self.mesh_shape[1])}

    # the vote over the last hulls: the ring and P are the model's, not the result's
    def _temporal(self, op):
        sc = self.scene
        hull, S0 = self.occ(), self.S
        if self.aligned:                         # a ring filled by vc_hull_temporal_motion starts over
            self.vote.reset()
            self.avote.reset()
            self.aligned = False
        ring_before, window_before = len(self.vote.ring), self.vote.window
        out, counts, st = self.vote.push(hull, op["window"], op["keep"], op["keep_off"])
        cc = self.carve["color_cam"]             # restored voxels: the carve's own frame set and colour camera
        slot = 0 if self.fault == "grow_slot0" else self.carve["slot"]
        rec, votes, added = tpn.records_after(self.records, hull, out, counts, self.grid, self.bounds, None if cc is None else sc.oc[cc],
                                              None if cc is None else sc.frames[slot][cc], sc.H, sc.W)
        own = {"temporal": votes.tobytes() + added.tobytes()}
        changed = bool(st["added"] or st["removed"])
        if changed:
            self.records = rec
            self._changed(own)
        else:                                    # O_t == H_t: nothing is invalidated, the result generation stays
            assert np.array_equal(rec, self.records) and not added.any()
            self.products.update(own)
            self.products.pop("temporal_field", None)            # (the field of an aligned vote before: a plain vote has none)
        return {"stats": st, "votes": votes, "added": added, "changed": changed, "ring_before": ring_before,
                "window_before": window_before, "by_hysteresis": int((out & ~(counts >= st["on"])).sum())}

    def _temporal_reset(self, op):
        self.vote.reset()
        self.avote.reset()
        self.products.pop("temporal", None)
        self.products.pop("temporal_field", None)
        return {}

    def ring(self):
        """The hulls of the vote's ring, newest last: the raw ones of vc_hull_temporal, or the aligned ones (the newest raw) of
        vc_hull_temporal_motion."""
        return (self.avote if self.aligned else self.vote).ring

    def ring_digest(self):
        h = hashlib.sha1(b"aligned" if self.aligned else b"plain")
        for hull in self.ring():
            h.update(mo.words(hull).tobytes())
        return h.hexdigest()

    @staticmethod
    def field_bytes(rows, b, a, s):
        return Model.motion_bytes(rows, b, a, s)

    def _temporal_motion(self, op):
        """vc_hull_temporal_motion: the ring and P of _temporal, aligned by the block motion between the ring's newest hull and this
        one before the count.  A second vote on one result is refused, as the plain one's would be."""
        sc = self.scene
        if "temporal" in self.products:          # also behind a vote that changed nothing; vc_temporal_reset lifts it
            return {"refused": "one_push", "refusal": OP_REFUSAL_E["one_push"]}
        if not self.aligned:                     # a ring filled by vc_hull_temporal starts over, P with it
            if self.fault == "plain_ring_kept_by_aligned":
                self.avote.window, self.avote.ring, self.avote.prev = self.vote.window, list(self.vote.ring), self.vote.prev
            else:
                self.avote.reset()
            self.vote.reset()
            self.aligned = True
        hull = self.occ()
        b, ap, s = op["block"], op["apron"], op["search"]
        ring_before, window_before = len(self.avote.ring), self.avote.window
        raw_before = list(self.avote.ring) if op["window"] == self.avote.window else []
        out, counts, st = self.avote.push(hull, op["window"], op["keep"], op["keep_off"], b, ap, s)
        if self.fault == "aligned_ring_keeps_raw":
            self.avote.ring = (raw_before + [hull.copy()])[-op["window"]:]
        cc = self.carve["color_cam"]             # restored voxels: the carve's own frame set and colour camera
        rec, votes, added = tpn.records_after(self.records, hull, out, counts, self.grid, self.bounds, None if cc is None else sc.oc[cc],
                                              None if cc is None else sc.frames[self.carve["slot"]][cc], sc.H, sc.W)
        rows = self.avote.rows
        self.vote_params = (b, ap, s)            # the scalars of the field that vc_fetch_temporal_motion returns
        own = {"temporal": votes.tobytes() + added.tobytes(), "temporal_field": self.field_bytes(rows, b, ap, s)}
        changed = bool(st["added"] or st["removed"])
        field_before = "motion" in self.products
        if changed:
            kept = self.products.get("motion") if self.fault == "field_survives_vote" else None
            self.records = rec
            self._changed(own)
            if kept is not None:
                self.products["motion"] = kept
        else:                                    # O_t == H_t: the generation and every product stay, a current motion field included
            assert np.array_equal(rec, self.records) and not added.any()
            self.products.update(own)
        return {"stats": st, "votes": votes, "added": added, "changed": changed, "ring_before": ring_before, "window_before": window_before,
                "rows": rows, "field_before": field_before, "field_after": "motion" in self.products}

    def components_current(self):
        """The components of a filter_components that is current and removed nothing: its labels are in the result's order."""
        return "component_labels" in self.products and bool(self.labels["component_labels"]["keep"].all())

    def measure_labels(self, op):
        """(u32 labels [S], G) of a measurement's source, from what the model holds as current."""
        src = op["source"]
        if src == "all":
            return mn.labels_of("all", self.S)
        if src == "host":
            return mn.labels_of("host", self.S, op["labels"], op["groups"])
        if src == "clusters":
            assert "clusters" in self.products
            return mn.labels_of("clusters", self.S, *self.labels["clusters"])
        if src == "geodesic":
            assert "geodesic" in self.products
            return mn.labels_of("geodesic", self.S, *self.labels["geodesic"][:2])
        assert src == "components" and self.components_current()
        w = self.labels["component_labels"]
        return mn.component_ranks(w["labels"], w["label"], w["size"]), max(int(w["label"].size), 1)

    def _measure(self, op):
        lab, G = self.measure_labels(op)
        rec = self.records
        if self.fault == "measure_carve_colours" and rec.size and self.carved.size:
            base, i = self.carved, index_of(rec)
            pos = np.minimum(np.searchsorted(index_of(base), i), base.size - 1)
            hit = index_of(base)[pos] == i
            rec = rec.copy()
            rec[hit] = with_rgb(rec[hit], rgb_of(base[pos[hit]]))
        w = (mn.measure_literal if self.literal else mn.measure)(rec, self.grid, lab, G, op["profile"])
        self.products["measure"] = b"".join(np.ascontiguousarray(w[k]).tobytes() for k in mn.FIELDS) + \
            (w["profile"].tobytes() if op["profile"] else b"")
        return {"stats": mn.stats(rec, lab, G), "measure": w, "labels": lab, "groups": G}

    def thin_anchors(self, op):
        """The linear indices that a thinning pins: none, a list, or the voxels at distance 0 of the current geodesic pass."""
        if isinstance(op["anchors"], str):
            assert op["anchors"] == "extrema" and "geodesic" in self.products
            return self.idx[self.labels["geodesic"][2] == 0]
        return op["anchors"]

    def _thin(self, op):
        w = (thn.thin_literal if self.literal else thn.thin)(self.idx, self.grid, op["mode"], self.thin_anchors(op), op["max_passes"])
        rows = np.zeros((w["voxel"].size, 3), dtype=np.uint32)   # vc_skeleton_voxel_t: {u32 voxel, u32 record, u8 degree, 3 zero bytes}
        rows[:, 0], rows[:, 1], rows[:, 2] = w["voxel"], w["record"], w["degree"]
        self.products["skeleton"] = w["peel"].tobytes() + rows.tobytes()
        return {"stats": {k: w[k] for k in thn.STATS}, "thin": w}

    # the shell: read-only, the generation stays; it keeps the colours of the call across colour passes and paints, and goes stale
    # with everything else when the surviving voxels change (item 5 of vc_hull_shell)
    @staticmethod
    def _shell_product(w):
        return w["records"].tobytes() + w["faces"].tobytes()

    def _shell(self, op):
        w = (shn.shell_literal if self.literal else shn.shell)(self.records, self.grid, op["level"])
        self.shell_level = op["level"]
        self.products["shell"] = self._shell_product(w)
        return {"stats": w["stats"], "shell": w}

    # the hull registers: they are the model's, not the result's.  The motion field is a product of the result that is tied to one
    # of them as well (item 8 of vc_hull_motion).
    def _written(self, reg, hull):
        self.registers[reg] = hull
        if self.field is not None and self.field["reg"] == reg and self.fault != "motion_survives_keep":
            self.products.pop("motion", None)

    def filled(self, records=None):
        """The registers that hold a hull (records=True / False: with / without records)."""
        return [r for r, k in enumerate(self.registers) if k is not None and (records is None or (k["records"] is not None) == records)]

    def motion_valid(self, reg=None):
        return "motion" in self.products and (reg is None or self.field["reg"] == reg)

    def _keep(self, op):
        self._written(op["reg"], {"occ": self.occ(), "records": self.records.copy(),
                                  "origin": {"how": "keep", "slot": self.carve["slot"], "painted": self.painted}})
        return {}

    def upload_hull(self, op):
        """(occ, records) of an upload's hull, from what the model holds: the carve of another frame set, the current hull eroded by
        one step (with the colours its records have now) or moved by a small vector, the empty hull or the full grid.  Where no
        carve gives the colours they are made from the index, so that no two records of a register look alike."""
        sc, src = self.scene, op["source"]
        if src == "carve":
            rec = sc.carve_records(op["slot"], op["min_views"], op["color_cam"])
            return dn.volume(index_of(rec), self.grid), rec.copy()
        if src == "eroded":
            occ = dn.erode(self.occ(), sc.q, dn.radius_r2(sc.mm(1)))
            return occ, self.records[occ.reshape(-1)[self.idx]]
        if src == "shifted":
            occ = mo.shifted(self.occ(), op["shift"])
        else:
            occ = (np.zeros if src == "empty" else np.ones)(self.occ().shape, dtype=bool)
        i = dn.indices(occ).astype(np.uint64)
        return occ, pack(i, np.stack([i & np.uint64(255), (i >> np.uint64(8)) & np.uint64(255), (i * np.uint64(7)) & np.uint64(255)], axis=1),
                         np.ones(i.size))

    def _upload(self, op):
        occ, rec = self.upload_hull(op)
        self._written(op["reg"], {"occ": occ, "records": rec if op["form"] == "records" else None,
                                  "origin": {"how": "upload", "slot": op.get("slot"), "painted": False}})
        return {"occ": occ, "records": rec}

    def _release(self, op):
        self._written(op["reg"], None)
        return {}

    def _combine(self, op):
        sc = self.scene
        B = self.registers[op["reg"]]
        cc = self.carve["color_cam"]             # fresh records: the carve's own frame set and colour camera (items 3 of
        slot = 0 if self.fault == "combine_slot0" else self.carve["slot"]    # vc_hull_combine and of vc_hull_grow)
        a, rec_a = self.occ(), self.records
        rec, added, r, st = so.combine(rec_a, a, B["occ"], B["records"], op["setop"], self.grid, self.bounds, None if cc is None else sc.oc[cc],
                                       None if cc is None else sc.frames[slot][cc], sc.H, sc.W)
        restore = op["setop"] == "copy" and B["records"] is not None
        if self.fault == "copy_keeps_a" and restore:
            rec[added == 0] = rec_a[r.reshape(-1)[self.idx]]
        changed = bool(st["added"] or st["removed"] or restore)   # a restore always counts as another result (item 5)
        if changed or self.fault == "noop_combine_invalidates":
            self.records = rec
            self._changed({"combined": added.tobytes()})
        else:                                    # R = A: nothing is invalidated, the result generation stays
            assert np.array_equal(rec, self.records) and not added.any()
            self.products["combined"] = added.tobytes()
        return {"stats": st, "added": added, "changed": changed, "restore": restore, "fresh": int(st["added"]) if B["records"] is None else 0,
                "bytes_changed": bool(rec.size == rec_a.size and not np.array_equal(rec, rec_a))}

    def _compare(self, op):
        B = self.registers[op["reg"]]
        st = so.compare(self.occ(), B["occ"], self.scene.q if op["distance"] else None)
        return {"stats": st, "derived": so.derived(st)}

    @staticmethod
    def motion_bytes(rows, b, a, s):
        return b"".join(np.ascontiguousarray(rows[k]).tobytes() for k in MOTION_ROW_KEYS) + np.array([b, a, s], dtype=np.uint32).tobytes()

    def _motion(self, op):
        B = self.registers[op["reg"]]
        b, ap, s = op["block"], op["apron"], op["search"]
        a = self.occ()
        L, refine = op.get("levels", 0), op.get("refine", 1)
        if L:                                    # vc_hull_motion_pyramid: the field of every level, its rows' bytes, the level words
            res = self.scene.match_pyramid(a, B["occ"], b, ap, s, L, refine, self.literal)      # of A and B and the scalars
            self.field = {"rows": res["rows"][0], "b": b, "a": ap, "s": s, "reg": op["reg"], "levels": L, "refine": refine,
                          "reach": res["reach"], "res": res}
            self.products["motion"] = self.pyramid_bytes(res, b, ap, s)
            return {"stats": mp.stats(res, a, B["occ"], self.grid, b), "rows": res["rows"][0], "res": res}
        rows = self.scene.match(a, B["occ"], b, ap, s, self.literal)
        stale = self.field["res"] if self.fault == "levels_survive_single_motion" and self.field is not None and self.field.get("levels") else None
        self.field = {"rows": rows, "b": b, "a": ap, "s": s, "reg": op["reg"], "levels": 0, "refine": refine, "reach": s, "res": None}
        self.products["motion"] = self.motion_bytes(rows, b, ap, s)
        if stale is not None:                    # (the wrong model: the coarser levels of the pyramid before are still there)
            self.products["motion"] += self.pyramid_bytes(stale, b, ap, s, first=1)
        return {"stats": mo.stats(rows, a, B["occ"], self.grid, b), "rows": rows}

    @staticmethod
    def pyramid_bytes(res, b, a, s, first=0):
        """The rows of the levels first..L, the level words of A and B, and b, a, s, levels, refine, reach."""
        parts = []
        for l in range(first, res["levels"] + 1):
            parts += [np.ascontiguousarray(res["rows"][l][k]).tobytes() for k in MOTION_ROW_KEYS]
            parts += [mo.words(res["a"][l]).tobytes(), mo.words(res["b"][l]).tobytes()]
        return b"".join(parts) + np.array([b, a, s, res["levels"], res["refine"], res["reach"]], dtype=np.uint32).tobytes()

    def _warp(self, op):
        f = self.field
        assert self.motion_valid(op["src"]) and op["dst"] != op["src"]
        a = self.occ()
        P, st = mo.warp(f["rows"], a, self.registers[op["src"]]["occ"], self.grid, f["b"])
        self._written(op["dst"], {"occ": P, "records": None, "origin": {"how": "warp", "slot": None, "painted": False}})
        return {"stats": st, "predicted_iou": mo.iou(a, P), "P": P}

    def _paint_motion(self, op):
        f = self.field
        assert self.motion_valid()
        if f.get("levels") and self.fault != "pyramid_paint_by_search":      # behind a pyramid the colours scale by its reach
            self.records = mp.paint(self.records, f["res"], self.grid, f["b"])
        else:
            self.records = mo.paint(self.records, f["rows"], self.grid, f["b"], f["s"])
        self.painted = True
        return {}

    def registers_digest(self):
        """sha1 over the four registers: empty, or the hull's words and its records."""
        h = hashlib.sha1()
        for k in self.registers:
            h.update(b"-" if k is None else b"+" + mo.words(k["occ"]).tobytes() + (b"-" if k["records"] is None else b"+" + k["records"].tobytes()))
        return h.hexdigest()

    # what the end of a chain compares on the final hull
    def marching_cubes(self):
        """marching_cubes(volume=None): the occupancy in the reference's reshape, (nx, ny, nz) over the voxel order."""
        nx, ny, nz = self.grid
        return marching_np.extract(self.occ().reshape(nx, ny, nz))


# ---- chains -----------------------------------------------------------------------------------------------------------------------
def _draw_step(rng, sc, centre_only=False):
    step = {"slot": int(rng.integers(3)), "mode": ("fused", "lut")[int(rng.integers(2))],
            "min_views": sc.C - int(rng.integers(2)), "color_cam": COLOUR_CAMERAS[int(rng.choice(3, p=(0.25, 0.4, 0.35)))]}
    if not centre_only:
        step["footprint"] = ("centre", "any")[int(rng.random() < 0.25)]
    return step


def _draw_carve(rng, sc):
    op = dict(_draw_step(rng, sc), op="carve", first=None)
    if op["footprint"] == "centre" and rng.random() < 0.45:      # two steps begun on two slots, both collected
        first = _draw_step(rng, sc, centre_only=True)
        first["slot"] = (op["slot"] + 1 + int(rng.integers(2))) % 3
        op["first"] = first
    return op


def _palette(rng, rows):
    return rng.integers(0, 256, (rows, 3), dtype=np.uint8)


def _draw(rng, sc, model, kind, hint=None):
    """hint (families C and D): parameters that the chain's shape fixes -- a register, a set operation, a slot to stay away from or
    to take, the steps of a texture, whether a light is smooth."""
    pick = lambda seq, p=None: seq[int(rng.choice(len(seq), p=p))]
    hint = hint or {}
    if kind == "carve":
        op = _draw_carve(rng, sc)
        if hint.get("not_slot") == op["slot"]:   # (family C's "previous frame" pattern: the next carve is of another frame set)
            by = 1 + int(rng.integers(2))
            op["slot"] = (op["slot"] + by) % 3
            if op["first"] is not None:
                op["first"]["slot"] = (op["first"]["slot"] + by) % 3
        return op
    if kind in ("close", "dilate"):
        return {"op": kind, "radius_mm": sc.mm(pick(("below", 1, 1.5, 2, 3), (0.12, 0.3, 0.25, 0.2, 0.13)))}
    if kind == "erode":
        return {"op": kind, "radius_mm": sc.mm(pick(("below", 0.25, 0.5, 1, 40), (0.12, 0.25, 0.25, 0.13, 0.25))), "border": pick(dn.BORDERS)}
    if kind == "open":
        return {"op": kind, "radius_mm": sc.mm(pick(("below", 0.25, 0.5, 1, 2), (0.12, 0.3, 0.3, 0.18, 0.1))), "border": pick(dn.BORDERS)}
    if kind == "filter_components":
        op = {"op": kind, "connectivity": pick(ccn.CONNECTIVITIES), "min_voxels": 0, "keep_largest": int(rng.integers(2))}
        if not op["keep_largest"]:               # a floor from the hull's own component sizes: it sometimes drops something
            sizes = np.sort(ccn.components(model.idx, model.grid, op["connectivity"])["size"])
            if sizes.size:
                op["min_voxels"] = int(sizes[int(rng.integers(sizes.size))]) + int(rng.integers(2))
        return op
    if kind == "photo_carve":
        return {"op": kind, "slot": pick(FULL_SLOTS), "max_rounds": int(rng.integers(1, 4))}
    if kind == "color_visible":
        return {"op": kind, "slot": pick(FULL_SLOTS)}
    if kind == "clusters":
        k = int(rng.integers(1, 5))
        return {"op": kind, "k": k, "max_iters": 32, "min_column": int(rng.integers(1, 3)), "palette": _palette(rng, k)}
    if kind == "geodesic":
        k = int(rng.integers(0, 4))
        return {"op": kind, "seeds": pick(("floor", "top")), "layers": int(rng.integers(1, 3)), "extrema": k,
                "connectivity": pick(ccn.CONNECTIVITIES), "paint": pick(("labels", "distance")), "palette": _palette(rng, k + 1)}
    if kind == "hull_distance":
        return {"op": kind, "border": pick(dn.BORDERS), "outside": bool(rng.integers(2))}
    if kind == "hull_normals":
        return {"op": kind, "radius_mm": normals_radius_mm(sc, pick((1, 1.5)))}
    if kind == "render":
        return {"op": kind}
    if kind == "surface_mesh":
        return {"op": kind, "refine_steps": pick((0, 3, 8))}
    # family B
    if kind == "temporal":                       # mostly the ring's own window: another one starts the ring over
        window = model.vote.window if model.vote.window and rng.random() < 0.85 else pick((2, 3, 4))
        r = rng.random()                         # slow to take a voxel and slow to let it go; a plain vote; or any thresholds
        keep = window if r < 0.35 else int(rng.integers(1, window + 1))
        return {"op": kind, "window": window, "keep": keep, "keep_off": 1 if r < 0.35 else keep if r < 0.6 else int(rng.integers(1, keep + 1))}
    if kind == "temporal_reset":
        return {"op": kind}
    if kind == "temporal_motion":                # family E: mostly the ring's own window; hint "window": that one, or "other"
        cur = model.avote.window if model.aligned else 0
        window = hint.get("window", cur if cur and rng.random() < 0.9 else pick((2, 3, 4)))
        if window == "other":
            window = pick([w for w in (2, 3, 4) if w != cur])
        r = rng.random()
        keep = window if r < 0.35 else int(rng.integers(1, window + 1))
        b, ap, s = pick(VOTE_PARAMS, (0.3, 0.3, 0.15, 0.15, 0.1))
        return {"op": kind, "window": window, "keep": keep, "keep_off": 1 if r < 0.35 else keep if r < 0.6 else int(rng.integers(1, keep + 1)),
                "block": b, "apron": ap, "search": s}
    if kind == "measure":                        # among the sources that are current, the rarer ones more often
        have = [("all", 1.0), ("host", 1.0)] + [(s, 6.0) for s in ("clusters", "geodesic") if s in model.products] + \
            ([("components", 8.0)] if model.components_current() else [])
        p = np.array([w for _, w in have])
        op = {"op": kind, "source": pick([s for s, _ in have], p / p.sum()), "profile": bool(rng.integers(2))}
        if op["source"] == "host":
            G = int(rng.integers(1, 7))
            lab = rng.integers(0, G, model.S).astype(np.uint32)
            lab[rng.random(model.S) < 0.1] = mn.NONE
            op.update(labels=lab, groups=G)
        return op
    if kind == "thin":
        op = {"op": kind, "mode": pick(thn.MODES), "anchors": None, "max_passes": pick((thn.MAX_PASSES, 1, 2), (0.8, 0.1, 0.1))}
        r = rng.random()
        if "geodesic" in model.products and r < 0.85:
            op["anchors"] = "extrema"
        elif model.S and r > 0.55:               # a few survivors, one of them twice
            a = model.idx[rng.integers(0, model.S, int(rng.integers(1, 7)))].astype(np.uint32)
            op["anchors"] = np.concatenate([a, a[:1]])
        return op
    # family C
    if kind in ("keep", "upload"):               # mostly into an empty register; now and then over a filled one
        free = [r for r in range(REGISTERS) if model.registers[r] is None]
        reg = hint["reg"] if "reg" in hint else pick(free) if free and rng.random() < 0.7 else int(rng.integers(REGISTERS))
        if kind == "keep":
            return {"op": kind, "reg": reg}
        op = {"op": kind, "reg": reg, "form": pick(("bits", "records"), (0.6, 0.4)), "source": pick(UPLOAD_SOURCES, (0.35, 0.15, 0.25, 0.1, 0.15))}
        if op["source"] == "carve":              # the hull of another frame set than the current result's
            op.update(slot=(model.carve["slot"] + 1 + int(rng.integers(2))) % 3, min_views=sc.C - int(rng.integers(2)),
                      color_cam=COLOUR_CAMERAS[int(rng.integers(3))])
        if op["source"] == "shifted":
            op["shift"] = tuple(int(v) for v in rng.integers(-3, 4, 3))
        return op
    if kind == "release":
        filled = model.filled()
        return {"op": kind, "reg": hint["reg"] if "reg" in hint else pick(filled) if filled and rng.random() < 0.8 else int(rng.integers(REGISTERS))}
    if kind in ("combine", "compare", "motion"):     # only on a filled register: the header refuses an empty one
        reg = hint.get("reg")
        if reg is None or model.registers[reg] is None:
            reg = pick(model.filled())
        op = {"op": kind, "reg": reg}
        if kind == "combine":
            op["setop"] = hint["setop"] if "setop" in hint else pick(so.OPS)
        elif kind == "compare":
            op["distance"] = hint["distance"] if "distance" in hint else bool(rng.integers(2))
        else:
            op["block"], op["apron"], op["search"] = pick(MOTION_PARAMS, (0.25, 0.25, 0.25, 0.12, 0.13))
            if "pyramid" in hint:                # family E: True a pyramid, False a single level, None either
                some = [x for x in PYRAMID_SETTINGS if hint["pyramid"] is None or (x[0] > 0) == hint["pyramid"]]
                L, r = pick(some)
                op["levels"], op["refine"] = L, min(r, op["search"])
        return op
    if kind == "warp":
        src = model.field["reg"]
        return {"op": kind, "src": src, "dst": pick([r for r in range(REGISTERS) if r != src])}
    if kind == "paint_motion":
        return {"op": kind}
    # family D
    V = len(sc.views)
    if kind == "shade":
        return {"op": kind, "light": np.array([pick(LIGHT_SUNS) for _ in range(V)], dtype=np.float64), "ambient": pick((0, 64, 200))}
    if kind == "texture":
        diag = vn.default_tolerance(sc.grid, sc.bounds)
        slot = hint["slot"] if "slot" in hint else pick((0, 1, 2), (0.42, 0.42, 0.16))
        steps = hint["steps"] if "steps" in hint else pick((0, 3, 8), (0.3, 0.3, 0.4))
        return {"op": kind, "slot": slot, "steps": steps, "reach_mm": diag * pick((1.0, 2.0, 0.5)),
                "depth_tolerance": float(np.float32(diag * pick((1.0, 0.25)))), "best": pick((1, 2, 4)), "sharpen": pick((0, 2, 6)),
                "filter": int(rng.integers(2))}
    if kind == "light":
        b = sc.bounds
        sun = bool(rng.integers(2))
        at = pick(LIGHT_SUNS if sun else LIGHT_POINTS)
        pos = at + (0.0,) if sun else tuple(0.5 * (b[2 * a] + b[2 * a + 1]) + at[a] for a in range(3)) + (1.0,)
        floor = None
        if rng.random() < 0.6:                   # (as test_gpu_light._floor makes it)
            from voxcarve import lighting
            floor = dict(lighting.auto_floor(sc.grid, sc.bounds), cell_mm=FLOOR_CELL_MM, rgb=FLOOR_RGB)
        return {"op": kind, "pos": pos, "ambient": pick((0, 64, 120)), "smooth": hint["smooth"] if "smooth" in hint else bool(rng.random() < (0.8 if "normals" in model.products else 0.4)),
                "ao_reach": pick((0.0, 2.0, 4.0), (0.2, 0.3, 0.5)), "floor": floor}
    if kind == "surface_normals":
        return {"op": kind}
    if kind == "feed":
        return {"op": kind, "slot": model.carve["slot"], "how": pick(("touch", "upload"))}
    raise ValueError(kind)


def normals_radius_mm(sc, factor=1.5):
    """`factor` largest steps, or one where that ball reaches beyond normals_np.EXT_MAX cells on the finest axis."""
    for f in (factor, 1):
        mm = sc.mm(f)
        try:
            nn.ball(sc.q, dn.radius_r2(mm))
            return mm
        except ValueError:
            continue
    raise ValueError("no normals radius for grid %r" % (sc.grid,))


_WEIGHTS = {"carve": 1.2, "close": 0.8, "dilate": 0.7, "erode": 0.8, "open": 0.8, "filter_components": 0.9, "photo_carve": 0.8,
            "color_visible": 1.0, "clusters": 1.1, "geodesic": 1.0, "hull_distance": 1.1, "hull_normals": 1.1, "render": 1.1,
            "surface_mesh": 1.0}


_CHAINS = {}


def model_of(seed, fault=None, literal=False):
    """A fresh model of chain `seed`'s scene, with its family's view size."""
    return Model(draw_chain(seed)[0], fault, literal, hw=HW_D if family(seed) == "D" else RENDER_HW)


def family(seed):
    return "B" if seed in SEEDS_B else "C" if seed in SEEDS_C else "D" if seed in SEEDS_D else "E" if seed in SEEDS_E else "A"


def draw_chain(seed):
    """(scene, ops) of chain `seed`.  Family A: a carve, then CHAIN_LEN - 1 drawn operations; now and then a burst of hull-changing
    passes.  Family B: see _draw_chain_b.  Family C: see _draw_chain_c.  Family D: see _draw_chain_d."""
    if seed not in _CHAINS:
        _CHAINS[seed] = {"A": _draw_chain, "B": _draw_chain_b, "C": _draw_chain_c, "D": _draw_chain_d, "E": _draw_chain_e}[family(seed)](seed)
    return _CHAINS[seed]


def _draw_chain(seed):
    rng = np.random.default_rng(seed)
    sc = scene(GRIDS[int(rng.integers(len(GRIDS)))])
    model = Model(sc)
    kinds = list(_WEIGHTS)
    p = np.array([_WEIGHTS[k] for k in kinds])
    p /= p.sum()
    ops, burst = [], 0
    while len(ops) < CHAIN_LEN:
        if not ops:
            kind = "carve"
        elif model.S == 0 and rng.random() < 0.5:    # an empty hull: some passes run on it, then the chain goes on
            kind, burst = "carve", 0
        elif burst:
            burst -= 1
            kind = HULL_CHANGERS[int(rng.integers(len(HULL_CHANGERS)))]
        else:
            kind = kinds[int(rng.choice(len(kinds), p=p))]
            if kind in HULL_CHANGERS and rng.random() < 0.5:
                burst = int(rng.integers(2, 4))
        op = _draw(rng, sc, model, kind)
        model.apply(op)
        ops.append(op)
    return sc, ops


_WEIGHTS_B = {"carve": 1.5, "temporal": 2.0, "temporal_reset": 0.5, "measure": 1.5, "thin": 2.2, "close": 0.4, "dilate": 0.4,
              "erode": 0.4, "open": 0.4, "filter_components": 0.7, "photo_carve": 0.4, "color_visible": 0.7, "clusters": 0.8,
              "geodesic": 1.2, "hull_distance": 0.15, "hull_normals": 0.15, "render": 0.15, "surface_mesh": 0.15}
assert set(_WEIGHTS_B) == set(KINDS_B)


def _draw_chain_b(seed):
    """A carve, then CHAIN_LEN_B - 1 operations drawn from every kind.  More often than not a vote follows a carve at once, so most
    chains hold several carve -> temporal pairs on different slots; a vote drawn where the header refuses one (the current result is
    already the last vote's output, item 8) becomes the carve that it asks for, with the vote behind it.  Half of the
    filter_components runs drop nothing, and most of those are followed by a measurement, which may then take their labels; likewise
    a measurement or a skeleton often follows the clusters or the geodesic distances that it can read.
    The header refuses a vote in two more cases, which no chain can reach as the operations stand: with steps in flight (the
    model's pipelined carve collects both of its steps before it returns) and on a slot prepared again since the carve (no
    operation uploads or prepares anything behind a carve: the frame sets are fixed by the scene).  An operation that leaves a
    step in flight or feeds a slot new input has to keep `temporal` out of the draw until the next carve, as item 9 of
    vc_hull_temporal says."""
    rng = np.random.default_rng(seed)
    sc = scene(GRIDS[int(rng.integers(len(GRIDS)))])
    model = Model(sc)
    kinds = list(_WEIGHTS_B)
    p = np.array([_WEIGHTS_B[k] for k in kinds])
    p /= p.sum()
    ops, queue = [], []
    while len(ops) < CHAIN_LEN_B:
        if not ops:
            kind = "carve"
        elif model.S == 0 and rng.random() < 0.5:
            kind, queue = "carve", []
        elif queue:
            kind = queue.pop(0)
        else:
            kind = kinds[int(rng.choice(len(kinds), p=p))]
        if kind == "temporal" and "temporal" in model.products:
            kind, queue = "carve", ["temporal"]
        op = _draw(rng, sc, model, kind)
        if kind == "carve" and not queue and rng.random() < 0.6:
            queue = ["temporal"]
        if kind == "filter_components" and rng.random() < 0.5:
            op.update(min_voxels=0, keep_largest=0)
            if rng.random() < 0.8:
                queue = ["measure"]
        if kind in ("clusters", "geodesic") and not queue and rng.random() < 0.75:
            queue = ["measure" if kind == "clusters" or rng.random() < 0.4 else "thin"]
        if kind == "temporal_reset" and not queue and len(model.products) >= 2 and rng.random() < 0.8:
            queue = ["temporal"]                 # the first vote after a reset changes nothing: every product must stay
        model.apply(op)
        ops.append(op)
    return sc, ops


_WEIGHTS_C = {"carve": 0.9, "close": 0.4, "dilate": 0.4, "erode": 0.4, "open": 0.4, "filter_components": 0.5, "photo_carve": 0.4,
              "color_visible": 0.6, "clusters": 0.5, "geodesic": 0.4, "hull_distance": 1.0, "hull_normals": 0.3, "render": 0.2,
              "surface_mesh": 0.2, "keep": 0.8, "upload": 2.4, "release": 0.4, "combine": 3.2, "compare": 1.0, "motion": 1.6,
              "warp": 0.7, "paint_motion": 0.3}
assert set(_WEIGHTS_C) == set(KINDS_C) and not set(KINDS_C) & set(NEW_KINDS + ("temporal_reset", "shell"))


def _draw_chain_c(seed):
    """A carve, then CHAIN_LEN_C - 1 operations drawn from family A's kinds and the eight of the hull registers.  A combine, a
    comparison or a motion estimate drawn while every register is empty becomes the keep that it needs, with itself behind it; a
    warp or a paint drawn without a current field becomes the motion estimate (item 8 of vc_hull_combine, the refusals of
    vc_hull_warp).  Behind the draw, the pairs that matter are queued more often than chance would give them:
      carve -> keep -> carve of another slot [-> motion | hull changer -> combine or compare], the "previous frame" pattern;
      keep -> two quiet passes -> "and" / "or" with the kept hull (R = A with products to lose), or keep -> a colour pass -> "copy"
      (a restore whose sets are equal and whose bytes are not);
      motion -> warp | paint_motion | a colour pass | a hull changer | a write to its register (behind a quiet pass, so that
      another product is there to stay) | a write to another register;
      warp -> compare or combine with its target;  upload -> combine with it (bits: an operation that makes fresh records);
      hull_distance -> compare with distances."""
    rng = np.random.default_rng(seed)
    sc = scene(GRIDS[int(rng.integers(len(GRIDS)))])
    model = Model(sc)
    kinds = list(_WEIGHTS_C)
    p = np.array([_WEIGHTS_C[k] for k in kinds])
    p /= p.sum()
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    ops, queue = [], []
    while len(ops) < CHAIN_LEN_C:
        hint = None
        if not ops:
            kind = "carve"
        elif model.S == 0 and rng.random() < 0.5:
            kind, queue = "carve", []
        elif queue:
            kind, hint = queue.pop(0)
        else:
            kind = kinds[int(rng.choice(len(kinds), p=p))]
        if kind in ("combine", "compare", "motion") and not model.filled():
            queue.insert(0, (kind, None))
            kind, hint = "keep", None
        if kind in ("warp", "paint_motion") and not model.motion_valid():
            queue.insert(0, (kind, None))
            kind, hint = ("motion" if model.filled() else "keep"), None
        op = _draw(rng, sc, model, kind, hint)
        if not queue:
            r = rng.random()
            if kind == "carve" and hint is None and r < 0.45:
                reg = {"reg": int(rng.integers(REGISTERS))}
                other = ("carve", {"not_slot": op["slot"]})
                r = rng.random()
                if r < 0.3:
                    queue = [("keep", reg), other, ("motion", reg)]
                elif r < 0.5:
                    queue = [("keep", reg), other] + [(pick(HULL_CHANGERS), None)] * (1 + int(rng.integers(2))) + [(pick(("combine", "compare")), reg)]
                elif r < 0.65:
                    queue = [("keep", reg), (pick(QUIET), None), (pick(QUIET), None), ("combine", dict(reg, setop=pick(("and", "or"))))]
                elif r < 0.9:
                    queue = [("keep", reg), (pick(("color_visible", "clusters", "geodesic")), None), ("combine", dict(reg, setop="copy"))]
                else:
                    queue = [("keep", reg), other]
            elif kind == "keep" and r < 0.55:
                reg = {"reg": op["reg"]}
                if r < 0.3:
                    queue = [(pick(QUIET), None), (pick(QUIET), None), ("combine", dict(reg, setop=pick(("and", "or"))))]
                else:
                    queue = [(pick(("color_visible", "clusters", "geodesic")), None), ("combine", dict(reg, setop="copy"))]
            elif kind == "motion" and r < 0.85:
                own, others = {"reg": op["reg"]}, [q for q in range(REGISTERS) if q != op["reg"]]
                writer = pick(("keep", "upload", "release"))
                queue = [[("warp", None)], [(pick(QUIET), None), (writer, own)], [("paint_motion", None)], [("color_visible", None)],
                         [(pick(HULL_CHANGERS), None)], [(pick(QUIET), None), (writer, own)], [(writer, own)],
                         [(writer, {"reg": pick(others)}), ("paint_motion", None)]][int(rng.integers(8))]
            elif kind == "warp" and r < 0.9:             # (its target has no records: "or" and "xor" make fresh ones)
                queue = [("compare", {"reg": op["dst"]}) if r < 0.25 else ("combine", {"reg": op["dst"], "setop": pick(("or", "xor", "and"))})]
            elif kind == "upload" and r < 0.85:
                queue = [("combine", {"reg": op["reg"], "setop": pick(("or", "xor", "copy"))} if op["form"] == "bits" else {"reg": op["reg"]})]
            elif kind == "hull_distance" and model.filled() and r < 0.7:
                queue = [("compare", {"reg": pick(model.filled()), "distance": True})]
        model.apply(op)
        ops.append(op)
    return sc, ops


_WEIGHTS_D = {"carve": 1.0, "close": 0.3, "dilate": 0.3, "erode": 0.3, "open": 0.3, "filter_components": 0.4, "photo_carve": 0.4,
              "color_visible": 0.9, "clusters": 0.5, "geodesic": 0.4, "hull_distance": 0.2, "hull_normals": 0.8, "render": 1.2,
              "surface_mesh": 0.7, "shade": 0.9, "texture": 1.6, "light": 1.6, "surface_normals": 0.9, "feed": 0.4}
assert set(_WEIGHTS_D) == set(KINDS_D) and not set(KINDS_D) & set(NEW_KINDS + ("temporal_reset", "shell"))

_SEQUENCES_D = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.5, 1.0, 1.9, 1.0, 0.8, 1.8, 1.9])              # how often each queued sequence is taken
_SEQUENCES_D /= _SEQUENCES_D.sum()


def _draw_chain_d(seed):
    """A carve, then CHAIN_LEN_D - 1 operations drawn from family A's kinds, the three passes over a render's images, the mesh's
    normals and the feed.  Nothing keeps an image pass away from a state that refuses it: the model says what the refusal is.
    Behind a carve (nine times in ten), and behind every second other operation once the queue is empty, one of twelve sequences
    is queued (_SEQUENCES_D weighs them); CV is color_visible and N hull_normals, each left out where its product is current:
      CV N render, texture (steps > 0), shade, light;
      N render, texture (no depth maps), light (smooth), shade, surface_mesh, surface_normals, carve;
      CV render, texture, light, carve, any of four, render, light: images that outlive a carve and are dropped by the next render;
      CV N render, a recolouring pass, texture, light (smooth): the render's rgb is of the old colours, the records' of the new;
      a hull changer, CV, texture (the render is stale), N render, texture, light (smooth);
      CV N render, feed, texture (steps > 0, the carve's slot: refused), texture (steps = 0: accepted, and it prepares the set
      again), texture (steps > 0, any slot: refused), light;
      an erosion to nothing, CV N render, texture, light, carve;
      N surface_mesh, surface_normals, render, shade, light;
      CV render, texture of slot 2 (which has two images), light (smooth, no normals), carve, light (no render);
      CV N render, texture (steps = 0), carve, render, light;
      CV N, a hull changer, render, texture (the depth maps are stale), light (smooth: so are the normals), light;
      N surface_mesh, CV (the mesh stays), surface_normals, render, shade, texture.
    A surface_mesh drawn by chance is followed by the surface_normals that read it.
    A carve that is neither the first nor pipelined carries, more often than not, a `probe`: an image pass that is tried while the
    carve's step is in flight (not a footprint carve's: it has no begin), or behind the same carve without records, in turn, and
    refused.  Once the carve's frame set has been prepared again, vc_surface_mesh and vc_hull_grow refuse as well (their own tests hold them to that): a surface_mesh, a
    close or a dilate drawn then becomes the carve that ends the state."""
    rng = np.random.default_rng(seed)
    sc = scene(GRIDS[int(rng.integers(len(GRIDS)))])
    model = Model(sc, hw=HW_D)
    kinds = list(_WEIGHTS_D)
    p = np.array([_WEIGHTS_D[k] for k in kinds])
    p /= p.sum()
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    ops, queue = [], []
    while len(ops) < CHAIN_LEN_D:
        hint = None
        if not ops:
            kind = "carve"
        elif model.S == 0 and not queue and rng.random() < 0.5:
            kind = "carve"
        elif queue:
            kind, hint = queue.pop(0)
            while queue and hint and hint.get("unless") in model.products:   # (depth maps or normals that are current already)
                kind, hint = queue.pop(0)
        else:
            kind = kinds[int(rng.choice(len(kinds), p=p))]
        if kind in ("close", "dilate", "surface_mesh") and model.prepared_again:
            kind, hint = "carve", None
        op = _draw(rng, sc, model, kind, hint)
        if hint and hint.get("empty"):
            op["radius_mm"] = sc.mm(40)
        if kind == "carve" and ops and op["first"] is None and rng.random() < 0.85:
            probes = sum(o.get("probe") is not None for o in ops)             # (the two kinds in turn; a footprint carve has no begin)
            op["probe"] = {"how": ("in_flight", "no_records")[probes % 2] if op["footprint"] == "centre" else "no_records",
                           "op": _draw(rng, sc, model, pick(("texture", "light")))}
        if kind == "surface_mesh" and not queue:     # a mesh drawn by chance: its normals are read once they can be
            queue = [("hull_normals", {"unless": "normals"}), ("surface_normals", None)]
        if not queue and rng.random() < (0.9 if kind == "carve" else 0.5):
            own = {"slot": op["slot"] if kind == "carve" else model.carve["slot"]}
            tex = lambda **kw: ("texture", dict({"slot": pick(FULL_SLOTS)}, **kw))
            N, CV, R, any_light = ("hull_normals", {"unless": "normals"}), ("color_visible", {"unless": "visibility"}), ("render", None), ("light", None)
            smooth, flat = ("light", {"smooth": True}), ("light", {"smooth": False})
            queue = [[CV, N, R, tex(steps=pick((3, 8))), ("shade", None), any_light],
                     [N, R, tex(), smooth, ("shade", None), ("surface_mesh", None), ("surface_normals", None), ("carve", None)],
                     [CV, R, tex(), flat, ("carve", None), (pick(("color_visible", "hull_normals", "light", "texture")), None), R, any_light],
                     [CV, N, R, (pick(("clusters", "geodesic", "color_visible")), None), tex(), smooth],
                     [(pick(HULL_CHANGERS), None), CV, tex(), N, R, tex(), smooth],
                     [CV, N, R, ("feed", None), ("texture", dict(own, steps=8)), ("texture", dict(own, steps=0)), tex(steps=3), any_light],
                     [("erode", {"empty": True}), CV, N, R, tex(), any_light, ("carve", None)],
                     [N, ("surface_mesh", None), ("surface_normals", None), R, ("shade", None), any_light],
                     [CV, R, ("texture", {"slot": 2}), smooth, ("carve", None), any_light],
                     [CV, N, R, tex(steps=0), ("carve", None), R, any_light],
                     [CV, N, (pick(HULL_CHANGERS), None), R, tex(), smooth, flat],
                     [N, ("surface_mesh", None), CV, ("surface_normals", None), R, ("shade", None), tex()],
                     ][int(rng.choice(12, p=_SEQUENCES_D))]
        model.apply(op)
        ops.append(op)
    return sc, ops


_WEIGHTS_E = {"carve": 1.2, "close": 0.3, "dilate": 0.3, "erode": 0.3, "open": 0.3, "filter_components": 0.3, "photo_carve": 0.3,
              "color_visible": 0.4, "clusters": 0.3, "geodesic": 0.3, "hull_distance": 0.4, "hull_normals": 0.2, "render": 0.1,
              "surface_mesh": 0.1, "keep": 0.6, "upload": 1.0, "release": 0.3, "combine": 0.6, "compare": 0.4, "motion": 1.6,
              "warp": 0.5, "paint_motion": 0.5, "temporal_motion": 2.0, "temporal_reset": 0.2}
assert set(_WEIGHTS_E) == set(KINDS_E) and not set(KINDS_E) & set(NEW_KINDS + ("shell",))


def _draw_chain_e(seed):
    """A carve, then CHAIN_LEN_E - 1 operations drawn from family C's kinds, the aligned vote (temporal_motion) and temporal_reset;
    every `motion` draws its levels and its refine radius from PYRAMID_SETTINGS.  The plain vote, the measurements, the skeleton
    and the shell are family B's and are not drawn.  As in family C, a combine, a comparison or a motion estimate drawn while
    every register is empty becomes the keep that it needs, and a warp or a paint drawn without a current field the motion
    estimate.  A vote drawn on a result that is already a vote's output becomes the carve that it asks for, with the vote behind
    it; the refusal itself is drawn on purpose in the second sequence below.  The header refuses a vote in two more cases that no
    chain reaches, as in family B: steps in flight (a pipelined carve collects both of its steps) and a frame set with input
    waiting (nothing here feeds one).  Behind a carve (nine times in ten), and behind every second other operation once the queue
    is empty, one of ten sequences is queued: the chain's first two in turn from the seed on (twelve chains of twelve operations
    are too few to leave each sequence to chance), the later ones at random, the first of the list more often than not; T is the aligned vote, C' a carve of another frame
    set than the last one, P a motion pyramid and M a single-level estimate against the register just kept:
      T C' T C' T: carve -> vote pairs on frame sets whose masks are rolled against each other, so that blocks move;
      T T (refused: one push per result) reset T (accepted: the first push of a ring changes nothing) C' T;
      T keep C P T, with C the last carve once more: the ring holds this very hull, the vote changes nothing while a pyramid's
      field is current, and the field stays;
      T keep C' P T: a vote on a ring that holds another frame set's hull -- the result changes and the field dies;
      keep C' T P warp paint_motion;  keep C' T P M: a single level behind a pyramid;
      keep C' T P, a quiet pass, a write to the pyramid's register: the field of every level is stale, the quiet product stays;
      a hull changer, T C' T: a vote on a pass's hull;  T C' T with another window (the ring starts over) C' T;
      upload, combine or compare with it, release."""
    rng = np.random.default_rng(seed)
    sc = scene(GRIDS[int(rng.integers(len(GRIDS)))])
    model = Model(sc)
    kinds = list(_WEIGHTS_E)
    p = np.array([_WEIGHTS_E[k] for k in kinds])
    p /= p.sum()
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    ops, queue, queued = [], [], 0
    while len(ops) < CHAIN_LEN_E:
        hint = None
        if not ops:
            kind = "carve"
        elif model.S == 0 and rng.random() < 0.5:
            kind, queue = "carve", []
        elif queue:
            kind, hint = queue.pop(0)
        else:
            kind = kinds[int(rng.choice(len(kinds), p=p))]
        if kind in ("combine", "compare", "motion") and not model.filled():
            queue.insert(0, (kind, hint))
            kind, hint = "keep", None
        if kind in ("warp", "paint_motion") and not model.motion_valid():
            queue.insert(0, (kind, None))
            kind, hint = ("motion" if model.filled() else "keep"), None
        if kind == "temporal_motion" and "temporal" in model.products and not (hint or {}).get("refused"):
            queue.insert(0, (kind, hint))
            kind, hint = "carve", {"not_slot": model.carve["slot"]}
        if kind == "motion":
            hint = dict({"pyramid": None}, **(hint or {}))
        if kind == "carve" and (hint or {}).get("same"):         # the last carve once more: the same hull, another result
            op = dict(last_carve, first=None if last_carve["first"] is None else dict(last_carve["first"]))
        else:
            op = _draw(rng, sc, model, kind, hint)
        if kind == "carve":
            last_carve = op
        if not queue and rng.random() < (0.9 if kind == "carve" else 0.5):
            T, other = ("temporal_motion", None), ("carve", {"not_slot": op["slot"] if kind == "carve" else model.carve["slot"]})
            again = ("carve", {"same": True})
            reg = {"reg": int(rng.integers(REGISTERS))}
            K, P = ("keep", reg), ("motion", dict(reg, pyramid=True))
            writer = pick(("keep", "upload", "release"))
            which = (seed + 4 * queued) % 10 if queued < 2 else 0 if rng.random() < 0.6 else int(rng.integers(10))
            queued += 1
            queue = [[T, other, T, other, T],
                     [T, ("temporal_motion", {"refused": True}), ("temporal_reset", None), T, other, T],
                     [T, K, again, P, T],
                     [T, K, other, P, T],
                     [K, other, T, P, ("warp", None), ("paint_motion", None)],
                     [K, other, T, P, ("motion", dict(reg, pyramid=False))],
                     [K, other, T, P, (pick(QUIET), None), (writer, reg)],
                     [(pick(HULL_CHANGERS), None), T, other, T],
                     [T, other, ("temporal_motion", {"window": "other"}), other, T],
                     [("upload", reg), (pick(("combine", "compare")), reg), ("release", reg)],
                     ][which]
        model.apply(op)
        ops.append(op)
    return sc, ops


SHELL_AFTER = (2, 6, 10)                     # a shell behind these steps of a chain ...
SHELL_LEVELS = (0, 0, 1, 0, 2)               # ... at these levels in turn, starting at the seed's place in the list
SHELL_STALERS = HULL_CHANGERS + ("carve", "temporal")


def with_shell(ops, seed):
    """(walk, origin): `ops` with a `shell` operation behind every step of SHELL_AFTER, directly in front of the first pass that
    repaints the records (RECOLOURING) and directly in front of the first operation behind step 0 that may change the surviving
    voxels (SHELL_STALERS); never two in a row.  The levels follow SHELL_LEVELS from the seed on.  origin[k] is the step of `ops`
    that walk[k] is, None for a shell.  Nothing is drawn: the chain's own operations, and what they were drawn from, stay."""
    first = lambda kinds: next((k for k, op in enumerate(ops) if k and op["op"] in kinds), None)
    before = {first(RECOLOURING), first(SHELL_STALERS)} - {None}
    walk, origin = [], []

    def shell():
        if walk[-1]["op"] != "shell":
            walk.append({"op": "shell", "level": SHELL_LEVELS[(seed + origin.count(None)) % len(SHELL_LEVELS)]})
            origin.append(None)

    for k, op in enumerate(ops):
        if k in before:
            shell()
        walk.append(op)
        origin.append(k)
        if k in SHELL_AFTER:
            shell()
    return walk, origin


def walk_of(seed, shell=False):
    """(scene, operations, origin) of chain `seed` as trace, run and replay walk it: as drawn, or with the shell put in."""
    sc, ops = draw_chain(seed)
    if not shell:
        return sc, ops, list(range(len(ops)))
    walk, origin = with_shell(ops, seed)
    return sc, walk, origin


def final_ops(sc):
    """One run of every quiet pass, for the final hull of a chain."""
    return [{"op": "hull_distance", "border": "open", "outside": True}, {"op": "hull_normals", "radius_mm": normals_radius_mm(sc)},
            {"op": "render"}, {"op": "surface_mesh", "refine_steps": 8}]


def run(seed, fault=None, shell=False):
    """Yields (step, op, out, model) of chain `seed` (shell=True: of its walk with the shell put in), the model as the operation
    left it."""
    sc, ops, _ = walk_of(seed, shell)
    model = model_of(seed, fault)
    for step, op in enumerate(ops):
        out = model.apply(op)
        yield step, op, out, model


def replay(seed, upto=None, fault=None, literal=False, shell=False):
    """The model of chain `seed` in front of step `upto` (None: behind the last one); shell=True: steps of the walk with the shell."""
    sc, ops, _ = walk_of(seed, shell)
    model = model_of(seed, fault, literal)
    for op in ops[:upto]:
        model.apply(op)
    return model


def replay_out(seed, step, shell=False):
    """What step `step` of chain `seed` returns, on the model in front of it."""
    return replay(seed, upto=step, shell=shell).apply(walk_of(seed, shell)[1][step])


def describe_op(op):
    """The parameters of an operation as one short line (arrays as their type and shape), for the failure messages."""
    return ", ".join("%s=%s" % (k, ("%s%r" % (v.dtype.name, v.shape)) if isinstance(v, np.ndarray) else repr(v)) for k, v in op.items())


def products_digest(model, without=()):
    """sha1 over the valid products but those named in `without`, sorted by name: each name and its bytes."""
    h = hashlib.sha1()
    for name in sorted(set(model.products) - set(without)):
        h.update(name.encode())
        h.update(model.products[name])
    return h.hexdigest()


def trace(seed, fault=None, shell=False):
    """One dict per step (shell=True: of the walk with the shell put in; "origin" is then the step of the chain as drawn, None for a
    shell, and "products_digest_drawn" the digest without the shell's product): op, kind of carve, records before and after, whether the hull changed, what the records carried into
    the operation (seen == 0 bytes, painted colours), the valid products in front of and behind it and their digest, the carve that
    made the result, what made its hull last (the carve or a pass that changed it), and the call's stats."""
    rows = []
    sc, ops, origin = walk_of(seed, shell)
    model = model_of(seed, fault)
    carve_op = made_by = None
    since = [None] * REGISTERS                   # per register, since it was written: the slot then, carves of other slots, hull changes
    for step, op in enumerate(ops):
        before = None if model.records is None else model.records
        carve_slot = None if model.carve is None else model.carve["slot"]
        row = {"step": step, "op": op["op"], "before": 0 if before is None else int(before.size),
               "seen0": bool(before is not None and before.size and (seen_of(before) == 0).any()),
               "painted": bool(model.painted and before is not None and before.size), "carve_slot": carve_slot, "params": op,
               "carve_op": carve_op, "made_by": made_by, "valid_before": dict(model.products),
               "registers_before": [None if k is None else {"count": int(k["occ"].sum()), "has_records": k["records"] is not None,
                                                            "origin": k["origin"], "since": dict(since[r])}
                                    for r, k in enumerate(model.registers)],
               "motion_reg_before": model.field["reg"] if model.motion_valid() else None,
               "pictures_before": tuple(sorted(model.pictures)), "render_current_before": "render" in model.products,
               "recoloured_before": model.recoloured,
               "fed_before": bool(model.carve is not None and (model.prepared_again or model.carve["slot"] in model.dirty))}
        out = model.apply(op)
        row["refused"] = out.get("refused")
        row["ring_digest"] = model.ring_digest()
        row["field_levels"] = model.field.get("levels", 0) if model.motion_valid() else None
        for k in ("field_before", "field_after"):
            if k in out:
                row[k] = out[k]
        row["dropped"] = out.get("dropped", ())
        row["pictures"] = tuple(sorted(model.pictures))
        row["pictures_digest"] = model.pictures_digest()
        row["picture_digests"] = {name: model.picture_digest(name) for name in REFUSAL_D}
        row["registers_digest"] = model.registers_digest()
        row["motion_reg"] = model.field["reg"] if model.motion_valid() else None
        for k in ("restore", "fresh", "bytes_changed"):
            if k in out:
                row[k] = out[k]
        if op["op"] in REGISTER_WRITERS:
            since[op["dst" if op["op"] == "warp" else "reg"]] = {"slot": carve_slot, "other_carves": 0, "hull_changes": 0}
        for s in since:
            if s is not None:
                s["other_carves"] += op["op"] == "carve" and op["slot"] != s["slot"]
                s["hull_changes"] += op["op"] != "carve" and bool(out.get("changed", False))
        row["after"] = model.S
        row["digest"] = hashlib.sha1(model.records.tobytes()).hexdigest()
        row["products_digest"] = products_digest(model)
        row["products_digest_drawn"] = products_digest(model, without=("shell",))
        row["origin"] = origin[step]
        row["valid"] = dict(model.products)
        row["changed"] = bool(out.get("changed", False)) if op["op"] != "carve" else False
        row["stats"] = out.get("stats")
        for k in ("ring_before", "window_before", "by_hysteresis"):
            if k in out:
                row[k] = out[k]
        if op["op"] == "carve":
            carve_op = made_by = op
        elif row["changed"]:
            made_by = op
        rows.append(row)
    return rows
