"""Drop-in for ``set_voxel_positions`` of the reference's assignment.py:54-149.

Same signature and module-level lazy state as the reference; the carve itself runs on the
GPU through the array fast path and the result comes back as two float32 ndarrays that
``Mesh.set_multiple_positions`` (engine/renderable/mesh.py:80-94) accepts as they are.

Frame and mask acquisition (video decode + MOG background subtraction, reference
assignment.py:68-82,93-109) is OUT of this path: it is delegated to a *frame source*.
The default source reuses the reference's own ``background_subtraction`` module and cv2
when this file is dropped into a reference checkout; tests and benchmarks install a
``StaticFrameSource``.
"""
import collections
import os

import numpy as np

from ._lib import VoxcarveError
from .camera import load_cameras
from .engine import (COLOR_CAMERA_INDEX, DEFAULT_BOUNDS, CarveEngine, footprint_rule, viewer_colors, viewer_positions,
                     voxel_keys)

# reference assignment.py:28-33: figure_threshold, figure_inner_threshold, opening/closing pre/post
cam_bg_model_params = [
    [5000, 115, False, False, True, True],
    [5000, 115, False, False, True, True],
    [5000, 175, False, True, True, True],
    [5000, 115, False, False, False, True],
]


class StaticFrameSource:
    """Yields pre-computed (frames, masks) pairs; ``None`` when exhausted (end of video)."""

    def __init__(self, frame_sets):
        self._sets = list(frame_sets)
        self._pos = 0

    def next(self):
        if self._pos >= len(self._sets):
            return None
        item = self._sets[self._pos]
        self._pos += 1
        return item


class ReferenceVideoSource:
    """Reference acquisition (assignment.py:68-82, 93-109) through the reference's own modules.

    Needs cv2 (opencv-contrib) and the reference's ``background_subtraction`` / ``utils`` on
    sys.path -- true when this package is used from inside a reference checkout."""

    def __init__(self, data_path="data", num_cameras=4, post_on_device=False):
        # post_on_device: leave the 2x2 open/close tail of extract_foreground_mask to the GPU
        # (CarveEngine.set_mask_postfilter with cam_bg_model_params[c][4:6]); masks then come out unfiltered.
        self.post_on_device = post_on_device
        try:
            import cv2
            import background_subtraction
            import utils
        except ImportError as exc:
            # fail HERE, once and by name -- not with a bare ImportError out of the viewer's key callback
            raise VoxcarveError(
                "voxcarve.assignment.set_voxel_positions has no frame source: the default one decodes the videos and "
                "subtracts the background with the reference's own modules (cv2 / opencv-contrib, background_subtraction, "
                "utils), and %r is not importable here.  Run from inside a reference checkout with OpenCV installed, or "
                "call voxcarve.assignment.configure(frame_source=...) with an object whose next() returns "
                "(frames, masks) or None (e.g. StaticFrameSource)." % exc.name) from exc
        self._bs = background_subtraction
        self.videos, self.bg_models = [], []
        for camera in range(num_cameras):
            directory = os.path.join(data_path, "cam" + str(camera + 1))
            self.videos.append(cv2.VideoCapture(os.path.join(directory, "video.avi")))
            _, _, n_frames = utils.get_video_properties(directory, "background.avi")
            self.bg_models.append(background_subtraction.train_MOG_background_model(
                directory, "background.avi", use_hsv=True, history=n_frames, n_mixtures=50, bg_ratio=0.90,
                noise_sigma=0))

    def next(self):
        frames = [video.read()[1] for video in self.videos]
        if any(frame is None for frame in frames):
            return None
        masks = []
        for camera, frame in enumerate(frames):
            p = cam_bg_model_params[camera]
            post = (False, False) if self.post_on_device else (p[4], p[5])
            masks.append(np.array(self._bs.extract_foreground_mask(frame, self.bg_models[camera], 0, p[0], p[1],
                                                                   p[2], p[3], post[0], post[1])))
        return frames, masks


class DeviceVideoSource:
    """Reference acquisition (assignment.py:68-82, 93-109) on the GPU: one background model per camera trained with the
    reference's parameters, then every frame set through extract_foreground_mask straight into the carve slot
    (CarveEngine.foreground_to_slot with cam_bg_model_params; the 2x2 post-filter is the slot's, set by set_voxel_positions).
    Nothing returns to the host before the survivors do, and cv2 is needed only to decode videos (from_videos).

    frames_per_camera[c]: camera c's BGR video frames (uint8 [H, W, 3] each); background_frames_per_camera[c]: its
    background video's frames.  model: "MOG" (the default, assignment.py:79): BackgroundSubtractorMOG with history = number
    of background frames, 50 mixtures (the model keeps at most 8), backgroundRatio 0.90, noiseSigma 0; "MOG2": a
    BackgroundSubtractorMOG2 as the reference's comparison script trains it (background_subtraction.py:400-401): history =
    number of background frames, varThreshold 650, no shadow detection."""

    post_on_device = True

    def __init__(self, frames_per_camera, background_frames_per_camera, num_cameras=4, model="MOG"):
        if model not in ("MOG", "MOG2"):
            raise ValueError("DeviceVideoSource: model %r, expected \"MOG\" or \"MOG2\"" % (model,))
        self.model = model
        self.num_cameras = num_cameras
        self._frames = [list(frames_per_camera[c]) for c in range(num_cameras)]
        self._bg = [list(background_frames_per_camera[c]) for c in range(num_cameras)]
        self._pos = 0
        self._models = None
        self._engine = None
        H, W = np.asarray(self._frames[0][0]).shape[:2] if self._frames[0] else np.asarray(self._bg[0][0]).shape[:2]
        self.image_size = (int(H), int(W))

    @classmethod
    def from_videos(cls, data_path="data", num_cameras=4, model="MOG"):
        """Decodes data_path/cam<c>/video.avi and background.avi with cv2 (which must be importable)."""
        from .background_subtraction import _video_frames
        fr, bg = [], []
        for camera in range(num_cameras):
            directory = os.path.join(data_path, "cam" + str(camera + 1))
            f = _video_frames(os.path.join(directory, "video.avi"))
            b = _video_frames(os.path.join(directory, "background.avi"))
            if f is None or b is None:
                raise VoxcarveError("DeviceVideoSource: cannot open the videos of %s" % directory)
            fr.append(list(f))
            bg.append(list(b))
        return cls(fr, bg, num_cameras, model)

    def _train(self, engine):
        from .background_subtraction import train_MOG_background_model, train_MOG2_background_model
        if self.model == "MOG2":
            self._models = [train_MOG2_background_model(use_hsv=True, history=len(self._bg[c]), var_threshold=650, detect_shadows=False,
                                                        engine=engine, frames=self._bg[c])
                            for c in range(self.num_cameras)]
        else:
            self._models = [train_MOG_background_model(use_hsv=True, history=len(self._bg[c]), n_mixtures=50, bg_ratio=0.90,
                                                       noise_sigma=0, engine=engine, frames=self._bg[c])
                            for c in range(self.num_cameras)]
        self._engine = engine

    def fill_slot(self, engine, slot=0):
        """The next frame set's masks and images into `slot` of `engine`; False at the end of the video."""
        if self._pos >= min(len(f) for f in self._frames):
            return False
        if self._engine is not engine:
            self._train(engine)
        frames = [self._frames[c][self._pos] for c in range(self.num_cameras)]
        self._pos += 1
        engine.foreground_to_slot(self._models, frames, cam_bg_model_params[:self.num_cameras], slot=slot, learning_rate=0)
        return True


# module state, as the reference keeps it (assignment.py:22-40)
initialized = False
frame_count = 0
_engine = None
_source = None
_cameras, _sized = None, None        # the calibrated cameras of data_path; the (H, W) the engine was last given them for
_operands = False        # hull_subtract / hull_clip are in their registers (new cameras empty them)
_last = {}               # the last frame's results, by stage: what the accessors below hand out
_carry = {}              # what a frame leaves for the next: the clusters' centres_mm and references, the measure's centroids_mm
HULL_SUBTRACT_REG, HULL_CLIP_REG = 3, 2      # the registers of CarveEngine that hold the two operands
MOTION_REG = 1                               # ... and the one that holds the previous frame's hull for the motion stage
BASE_SETTINGS = {"data_path": "data", "num_cameras": 4, "device": 0, "mode": "fused", "views_threshold": 4,
                 "color_camera": COLOR_CAMERA_INDEX, "bounds": DEFAULT_BOUNDS, "footprint": "centre", "normal_radius_mm": None,
                 # how the motion stage matches, not whether it runs: the stage's check (_check_motion) covers them
                 "motion_levels": 0, "motion_refine": 1}


# -- the checks of configure(): a check takes the merged settings and raises ValueError; these make one for the setting `name` ----
def _one_of(name, allowed):
    def check(s):
        if s[name] not in allowed:
            raise ValueError("%s %r, expected one of %s" % (name, s[name], allowed))
    return check


def _integer(name, hi, bools=True):
    def check(s):
        if (isinstance(s[name], bool) and not bools) or not isinstance(s[name], (int, np.integer)) or not 0 <= s[name] <= hi:
            raise ValueError("%s %r, expected an integer in 0..%d" % (name, s[name], hi))
    return check


def _operand(name):
    def check(s):
        if s[name] is not None and not isinstance(s[name], (str, os.PathLike, np.ndarray)):
            raise ValueError("%s %r, expected a path, an array or None" % (name, s[name]))
    return check


def _check_temporal(s):
    t = s["temporal_window"]
    if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0:
        raise ValueError("temporal_window %r, expected an integer in 0..15" % (t,))
    CarveEngine.temporal_thresholds(t if t > 0 else 1, s["temporal_keep"] if t > 0 else None, s["temporal_keep_off"] if t > 0 else None)
    from . import motion
    motion.vote_params(s["temporal_motion"])


def _run_temporal(s):
    """The vote; with temporal_motion the motion-compensated one.  Without it the call is the three-argument one it always was."""
    if s["temporal_motion"] is None:
        _last.update(temporal=_engine.temporal_filter(s["temporal_window"], s["temporal_keep"], s["temporal_keep_off"]))
    else:
        _last.update(temporal=_engine.temporal_filter(s["temporal_window"], s["temporal_keep"], s["temporal_keep_off"], motion=s["temporal_motion"]))


def _check_min_column(s):
    if int(s["cluster_min_column"]) < 0:
        raise ValueError("cluster_min_column %r is negative" % (s["cluster_min_column"],))


def _check_seeds(s):
    if isinstance(s["geodesic_seeds"], str) and s["geodesic_seeds"] not in ("floor", "top"):
        raise ValueError("geodesic_seeds %r, expected \"floor\", \"top\" or an array of voxel indices" % (s["geodesic_seeds"],))


def _check_profile(s):
    if not isinstance(s["measure_profile"], (bool, np.bool_)):
        raise ValueError("measure_profile %r, expected True or False" % (s["measure_profile"],))


def _check_anchors(s):
    if s["skeleton_anchors"] not in (None, "extrema"):
        raise ValueError('skeleton_anchors %r, expected None or "extrema"' % (s["skeleton_anchors"],))


def _check_motion(s):
    from . import motion
    b = s["motion_block"]
    if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or (b != 0 and b not in motion.BLOCKS):
        raise ValueError("motion_block %r, expected 0 or one of %s" % (b, motion.BLOCKS))
    if not isinstance(s["motion_paint"], (bool, np.bool_)):
        raise ValueError("motion_paint %r, expected True or False" % (s["motion_paint"],))
    search = motion.check_params(b if b else motion.BLOCKS[0], s["motion_apron"], s["motion_search"])[2]
    motion.check_pyramid(s["motion_levels"], s["motion_refine"], search)
    if s["motion_paint"] and (s["cluster_paint"] or s["geodesic_paint"] is not None):
        raise ValueError("motion_paint excludes cluster_paint and geodesic_paint: one pass colours the records")


def _check_across(s):                                            # (what one stage's settings ask of another's)
    if s["measure"] == "clusters" and not s["clusters"] > 0:
        raise ValueError('measure="clusters" needs clusters=K')
    if s["measure"] == "geodesic" and not s["extremities"] > 0:
        raise ValueError('measure="geodesic" needs extremities=K')
    if s["measure"] == "components" and not _components_on(s):
        raise ValueError('measure="components" needs the component filter: min_component_voxels or keep_components')
    if s["skeleton"] is not None and s["skeleton_anchors"] == "extrema" and not s["extremities"] > 0:
        raise ValueError('skeleton_anchors="extrema" needs extremities=K')
    if s["output_level"] != 0 and s["output"] != "shell":
        raise ValueError('output_level=%d needs output="shell"' % s["output_level"])


def _components_on(s):
    return bool(s["min_component_voxels"] or s["keep_components"])


def _recolours(s):                                               # (from every camera's image: the frame uploads them all)
    return s["hull"] == "photo" or s["color_mode"] == "visible"


# -- what the stages run: each takes the settings, works on _engine and keeps what its accessor hands out in _last ---------------
def _run_clip(s):
    ops = _last["hull_ops"] if s["hull_subtract"] is not None else {}                        # (this frame's, made a moment ago)
    _last["hull_ops"] = dict(ops, clip=_engine.combine_hull("and", HULL_CLIP_REG))


def _run_clusters(s):
    """The frame's split into figures, warm-started from the previous frame's centres (see configure)."""
    from .clusters import MATCH_MAX_K, match
    K = int(s["clusters"])
    out = _engine.cluster_hull(K, min_column=int(s["cluster_min_column"]), init_mm=_carry.get("centres_mm"))
    out["figures"] = _engine.fetch_clusters()
    out["histograms"] = _engine.fetch_cluster_histograms()
    if _carry.get("references") is None:
        _carry["references"] = out["histograms"].copy()
    out["identity"] = match(_carry["references"], out["histograms"]) if K <= MATCH_MAX_K else None
    _carry["centres_mm"] = out["centres_mm"]
    _last["clusters"] = out
    if s["cluster_paint"]:
        _engine.paint_clusters()


def _run_extremities(s):
    """The frame's geodesic distances and extremities (see configure)."""
    out = _engine.hull_geodesic(seeds=s["geodesic_seeds"], extrema=int(s["extremities"]), paths=True)
    out["extrema"] = _engine.fetch_extrema()
    out["paths"] = _engine.stick_figure()
    _last["extremities"] = out
    if s["geodesic_paint"] is not None:
        _engine.paint_geodesic(s["geodesic_paint"])


def _run_measure(s):
    """The frame's measurements (see configure); with "clusters", label k is the same figure from frame to frame, so the
    centroid's step since the previous frame is the figure's displacement."""
    from . import measure
    source = s["measure"]
    if source == "components":
        try:
            _engine.component_ranks()
        except ValueError:                                       # the filter removed something: label its output
            _engine.filter_components(connectivity=s["component_connectivity"])
    out = _engine.measure_hull(labels=source, profile=bool(s["measure_profile"]))
    out["source"] = source
    out["integers"] = _engine.fetch_measure()
    out["world"] = measure.describe(out["integers"], _engine.grid, _engine.bounds)
    if s["measure_profile"]:
        out["profile"] = _engine.fetch_measure_profile()
    if source == "clusters":
        c = out["world"]["centroid_mm"]
        prev = _carry.get("centroids_mm")
        out["velocity_mm"] = None if prev is None or prev.shape != c.shape else c - prev
        _carry["centroids_mm"] = c.copy()
    _last["measure"] = out


def _run_skeleton(s):
    """The frame's skeleton (see configure)."""
    from . import skeleton as sk
    stats = _engine.thin_hull(s["skeleton"], anchors=s["skeleton_anchors"])
    rows = _engine.fetch_skeleton()
    _last["skeleton"] = {"stats": stats, "skeleton": rows, "description": sk.describe(rows, _engine.grid, _engine.bounds)}


def _run_motion(s):
    """The frame's motion field against the previous frame's hull (see configure); then this frame's hull is kept for the next."""
    from . import motion
    if _carry.get("motion_kept"):
        if s["motion_levels"]:
            stats = _engine.hull_motion(MOTION_REG, int(s["motion_block"]), s["motion_apron"], int(s["motion_search"]),
                                        levels=int(s["motion_levels"]), refine=int(s["motion_refine"]))
        else:                                    # (the four-argument call it always was)
            stats = _engine.hull_motion(MOTION_REG, int(s["motion_block"]), s["motion_apron"], int(s["motion_search"]))
        rows = _engine.fetch_motion()
        _last["motion"] = {"stats": stats, "rows": rows, "description": motion.describe(rows, _engine.grid, _engine.bounds)}
        if s["motion_paint"]:
            _engine.paint_motion()
    _engine.keep_hull(MOTION_REG)
    _carry["motion_kept"] = True


def _run_output(s):                                              # (returns what set_voxel_positions returns)
    if s["output"] == "shell":
        _last["shell"] = _engine.hull_shell(int(s["output_level"]))
        return _engine.fetch_shell_viewer()
    idx, rgb, _ = _engine.fetch()
    keys = voxel_keys(idx, _engine.grid, _engine.axes())
    return viewer_positions(keys), viewer_colors(rgb)


# The frame chain: what follows every carve, IN THIS ORDER.  This list is the one place that says it; configure()'s docstring
# numbers its paragraphs by it.  A stage names the settings it owns with their defaults, the checks of them (configure), whether
# the settings turn it on, and what it runs on _engine.  The last stage is always on and returns what set_voxel_positions does.
Stage = collections.namedtuple("Stage", "name defaults checks on run")
STAGES = [
    Stage("hull_subtract", {"hull_subtract": None}, [_operand("hull_subtract")], lambda s: s["hull_subtract"] is not None,
          lambda s: _last.update(hull_ops={"subtract": _engine.combine_hull("andnot", HULL_SUBTRACT_REG)})),
    Stage("hull_clip", {"hull_clip": None}, [_operand("hull_clip")], lambda s: s["hull_clip"] is not None, _run_clip),
    Stage("temporal", {"temporal_window": 0, "temporal_keep": None, "temporal_keep_off": None, "temporal_motion": None}, [_check_temporal],
          lambda s: s["temporal_window"] > 0, _run_temporal),
    Stage("close", {"hull_close_mm": 0.0}, [lambda s: CarveEngine.radius_r2(s["hull_close_mm"])], lambda s: s["hull_close_mm"] > 0,
          lambda s: _engine.close_hull(s["hull_close_mm"])),
    Stage("open", {"hull_open_mm": 0.0, "hull_border": "open"},
          [lambda s: CarveEngine.radius_r2(s["hull_open_mm"]), lambda s: CarveEngine._dist_flags(s["hull_border"])],
          lambda s: s["hull_open_mm"] > 0, lambda s: _engine.open_hull(s["hull_open_mm"], border=s["hull_border"])),
    Stage("components", {"min_component_voxels": 0, "keep_components": 0, "component_connectivity": 26}, [], _components_on,
          lambda s: _engine.filter_components(connectivity=s["component_connectivity"], min_voxels=s["min_component_voxels"],
                                              keep_largest=s["keep_components"])),
    Stage("colour", {"color_mode": "camera", "hull": "visual", "photo_var_threshold": 1200},
          [_one_of("color_mode", ("camera", "visible")), _one_of("hull", ("visual", "photo"))], _recolours,
          lambda s: (_engine.photo_carve(slot=0, var_threshold=s["photo_var_threshold"]) if s["hull"] == "photo"
                     else _engine.color_visible(slot=0))),
    Stage("clusters", {"clusters": 0, "cluster_min_column": 1, "cluster_paint": False}, [_integer("clusters", 16), _check_min_column],
          lambda s: s["clusters"] > 0, _run_clusters),
    Stage("extremities", {"extremities": 0, "geodesic_seeds": "floor", "geodesic_paint": None},
          [_integer("extremities", 32), _one_of("geodesic_paint", (None, "labels", "distance")), _check_seeds],
          lambda s: s["extremities"] > 0, _run_extremities),
    Stage("measure", {"measure": None, "measure_profile": False},
          [_one_of("measure", (None, "all", "clusters", "geodesic", "components")), _check_profile],
          lambda s: s["measure"] is not None, _run_measure),
    Stage("skeleton", {"skeleton": None, "skeleton_anchors": None}, [_one_of("skeleton", (None, "curve", "point")), _check_anchors],
          lambda s: s["skeleton"] is not None, _run_skeleton),
    Stage("motion", {"motion_block": 0, "motion_apron": None, "motion_search": 4, "motion_paint": False}, [_check_motion],
          lambda s: s["motion_block"] > 0, _run_motion),
    Stage("output", {"output": "all", "output_level": 0}, [_one_of("output", ("all", "shell")), _integer("output_level", 6, bools=False)],
          lambda s: True, _run_output),
]
_settings = dict(BASE_SETTINGS, **{name: default for stage in STAGES for name, default in stage.defaults.items()})


def configure(frame_source=None, **settings):
    """Install a frame source / override data_path, num_cameras, device, mode, ...; resets state.  A call that raises changes
    nothing.  Every carve is followed by the stages that the settings turn on, in the order of STAGES above -- the order of the
    numbered paragraphs here; by default none runs but the last, which returns every survivor.
    footprint: "centre" (default) asks, as the reference does, whether the pixel under a voxel's centre is foreground; "any",
    "all" and ("cover", q) test the pixel box the voxel's whole cell projects to (CarveEngine.carve(footprint=...)): "any" keeps
    what is thinner than a voxel (the outer hull), "all" gives the inner hull.
    normal_radius_mm: the radius of the ball that render_views(smooth=True) and surface_mesh(normals=True) estimate the hull's
    surface normals from (CarveEngine.hull_normals); None (the default) is 3 x the largest grid step.
    1, 2. hull_subtract, hull_clip: each a path to a file of CarveEngine.save_hull, a hull as an array (bool [n], ascending uint32
    indices or uint64 records: voxcarve.hullio.as_operand), or None (the default: nothing runs).  The operand is uploaded once,
    to registers 3 and 2 of the engine; the stages are CarveEngine.combine_hull("andnot", 3) (the static scene leaves the hull)
    and CarveEngine.combine_hull("and", 2) (the hull is clipped to a region of interest).  hull_ops() returns their stats.
    3. temporal_window, temporal_keep, temporal_keep_off, temporal_motion: when temporal_window = T > 0 (at most 15),
    CarveEngine.temporal_filter(T, temporal_keep, temporal_keep_off): the hull becomes the vote of the last T frames' hulls (keep
    defaults to the majority, keep_off to keep), which takes the frame-to-frame flicker of mask noise out and lags a moving
    figure by about T / 2 frames.  temporal_motion = True or (block, apron, search) makes it the motion-compensated vote
    (temporal_filter(..., motion=temporal_motion); True is (8, None, 4), apron None is block // 2): the older hulls are aligned
    to the frame's hull by the block motion field first, so a figure that walks is voted on where it is now; None (the default)
    is the plain vote.  temporal() returns the last frame's stats.  temporal_window = 0 (the default) runs nothing.
    4. hull_close_mm: when > 0, CarveEngine.close_hull(hull_close_mm) (close, then open, is the usual clean-up order): tunnels and
    dents narrower than a ball of that radius in world millimetres are filled -- what a hole in one camera's mask carves through
    the figure; the added voxels are coloured from the colour camera.  voxels_status() describes the closed hull.
    5. hull_open_mm, hull_border: when hull_open_mm > 0, CarveEngine.open_hull(hull_open_mm, border=hull_border): what is thinner
    than a ball of that radius in world millimetres leaves the hull (spurs, fins and specks of mask noise, attached to the figure
    or not); voxels_status() describes what is kept.  0 (the default) keeps every survivor.
    6. min_component_voxels, keep_components: when either is non-zero, CarveEngine.filter_components(connectivity=
    component_connectivity): components smaller than min_component_voxels, or beyond the keep_components largest, leave the
    hull (floating specks of mask noise); voxels_status() describes what is kept.  0 and 0 (the default) keep every survivor.
    7. hull, color_mode: hull="photo" refines the visual hull by photo-consistency (CarveEngine.photo_carve with var_threshold=
    photo_var_threshold), which needs every camera's image and colours the result as "visible" does; voxels_status() then
    describes the photo hull.  Otherwise color_mode="visible" recolours the surface voxels from every camera that sees them
    (CarveEngine.color_visible).  "visual" and "camera" (the defaults): every survivor of the carve's visual hull, coloured from
    the colour camera as the reference does (assignment.py:133).
    8. clusters, cluster_min_column, cluster_paint: when clusters = K > 0 (at most 16), CarveEngine.cluster_hull(K,
    min_column=cluster_min_column): the hull split into K figures on the floor plane.  The first frame seeds itself and keeps its
    colour signatures as the references; every later frame starts from the previous frame's centres, so label k stays the same
    figure while the figures keep apart.  clusters() returns the last frame's split.  cluster_paint=True then paints every voxel
    in its figure's colour (voxcarve.clusters.PALETTE).  0 (the default) runs nothing.
    9. extremities, geodesic_seeds, geodesic_paint: when extremities = K > 0 (at most 32),
    CarveEngine.hull_geodesic(seeds=geodesic_seeds, extrema=K, paths=True): geodesic distances through the hull from the seed set
    ("floor", the default, "top", or an array of voxel indices) and the K extremities by farthest-point selection (head, hands,
    feet).  extremities() returns the last frame's.  geodesic_paint = "labels" | "distance" then paints every voxel by its region
    or its distance (CarveEngine.paint_geodesic); None (the default) leaves the colours.  0 (the default) runs nothing.
    10. measure, measure_profile: when measure = "all" | "clusters" | "geodesic" | "components" (None, the default, runs nothing),
    CarveEngine.measure_hull(labels=measure, profile=measure_profile): the hull's figures measured on the device, per group of
    that source (the whole hull; the figures of clusters=K; the regions of extremities=K; the connected components, ranked by
    size, of the component filter -- which runs once more on its own output when it removed something, so that its labels
    describe the hull).  measurements() returns the last frame's.  A source whose own pass is not configured is refused.
    11. skeleton, skeleton_anchors: when skeleton = "curve" | "point" (None, the default, runs nothing),
    CarveEngine.thin_hull(skeleton, anchors=skeleton_anchors): the hull thinned to a centred, one-voxel-wide skeleton with its
    topology, on the device; the hull itself stays.  skeleton_anchors = "extrema" pins the skeleton at the floor contact and the
    extremities of extremities=K, which turns a noisy curve skeleton into a stick figure; it is refused without extremities=K.
    skeleton() returns the last frame's.
    12. motion_block, motion_apron, motion_search, motion_paint, motion_levels, motion_refine: when motion_block = b in {4, 8, 16} (0, the default, runs
    nothing), every frame's hull is kept in register 1 of the engine (CarveEngine.keep_hull), and from the second frame of a
    session on CarveEngine.hull_motion(1, b, motion_apron, motion_search) estimates, before that, where each block of b^3 voxels
    went since the previous frame (motion_apron = None is b // 2; b + 2 motion_apron + 2 motion_search <= 64).  motion() returns
    the last frame's field.  motion_paint=True then paints every voxel by its block's vector (CarveEngine.paint_motion); it
    excludes cluster_paint and geodesic_paint.  The hull that is matched and kept is the one the stages above leave.
    motion_levels = L in 1..3 (0, the default, is the single-level field) makes the call coarse to fine,
    CarveEngine.hull_motion(..., levels=L, refine=motion_refine): vectors up to motion_search 2^L + motion_refine (2^L - 1) voxels
    are found, and a block inside a solid body takes its surroundings' vector (motion_refine in 1..motion_search, default 1).
    13. output, output_level: "all" (the default) returns every survivor, as the reference does.  "shell" runs
    CarveEngine.hull_shell(output_level) and returns the arrays of CarveEngine.fetch_shell_viewer(), made on the device: only the
    voxels with an exposed face, which is everything an opaque cube viewer can show (at level 0 the same rows the full arrays
    hold for those voxels).  output_level = L in 1..6 lists the cells of a grid 2^L times coarser instead, with averaged colours:
    the viewer must draw each cube shell()["cube_scale"] times as large.  shell() returns the last frame's stats.
    voxels_status() is unaffected.  output_level needs output="shell"."""
    global _source, _engine, initialized, frame_count
    unknown = set(settings) - set(_settings)
    if unknown:
        raise TypeError("unknown settings: %s" % sorted(unknown))
    merged = dict(_settings, **settings)
    footprint_rule(merged["footprint"])                          # raises ValueError on anything else
    if merged["normal_radius_mm"] is not None:
        CarveEngine.radius_r2(merged["normal_radius_mm"])        # ... on a negative or non-finite radius
    for stage in STAGES:
        for check in stage.checks:
            check(merged)
    _check_across(merged)
    _settings.update(settings)
    _last.clear(), _carry.clear()
    _source = frame_source
    if _engine is not None:
        _engine.close()
    _engine = None
    initialized = False
    frame_count = 0


def set_voxel_positions(width, height, depth):
    """Voxels seen by all cameras and their colours; reference assignment.py:54-149.

    :param width: voxel volume width
    :param height: HALF of the voxel volume height (the volume has 2*height cells in y)
    :param depth: voxel volume depth
    :return: (positions float32 [S,3], colors float32 [S,3]); ([], []) at the end of the video
    """
    global initialized, frame_count, _engine, _source, _cameras, _sized, _operands
    if not initialized:
        if _source is None:
            _source = ReferenceVideoSource(_settings["data_path"], _settings["num_cameras"])
        _engine = CarveEngine(_settings["device"])
        _engine.set_grid(width, height * 2, depth, _settings["bounds"])        # assignment.py:85
        _cameras = load_cameras(_settings["data_path"], _settings["num_cameras"])   # :88
        _sized = None
        initialized = True

    device_source = hasattr(_source, "fill_slot")
    if device_source:
        H, W = _source.image_size
    else:
        item = _source.next()                                                   # assignment.py:94-96
        if item is None:
            return [], []
        frames, masks = item
        frame_count += 1
        H, W = np.asarray(masks[0]).shape[:2]
    if _sized != (H, W):
        _engine.set_cameras(_cameras, H, W)
        if hasattr(_source, "post_on_device") and _source.post_on_device:
            n = _settings["num_cameras"]
            _engine.set_mask_postfilter([cam_bg_model_params[c][4] for c in range(n)],
                                        [cam_bg_model_params[c][5] for c in range(n)])
        if _settings["mode"] == "lut":
            _engine.build_lut()
        _sized = (H, W)
        _operands = False                                                       # (new cameras empty the registers)
        _carry.pop("motion_kept", None)                                         # ... the previous frame's hull among them
    if not _operands:
        _upload_operands()
        _operands = True
    cc = _settings["color_camera"]
    if device_source:
        if not _source.fill_slot(_engine, 0):                                   # masks and images made on the device
            return [], []
        frame_count += 1
    else:
        _engine.upload_masks(masks, slot=0)
        for c in (range(len(frames)) if _recolours(_settings) else (cc,)):     # recolouring: every camera's image
            _engine.upload_frame(c, frames[c], slot=0)
    _engine.carve(slot=0, min_views=_settings["views_threshold"], color_cam=cc, mode=_settings["mode"],
                  footprint=_settings["footprint"])
    return [stage.run(_settings) for stage in STAGES if stage.on(_settings)][-1]       # (the last stage's: the output is always on)


def _upload_operands():
    """The operands of hull_subtract and hull_clip into their registers (see configure): once per camera set."""
    for name, reg in (("hull_subtract", HULL_SUBTRACT_REG), ("hull_clip", HULL_CLIP_REG)):
        h = _settings[name]
        if isinstance(h, (str, os.PathLike)):
            _engine.load_hull(h, reg)
        elif h is not None:
            _engine.upload_hull(h, reg)


def _last_result(stage, what, how):                              # (for the accessors below)
    if _engine is None or not initialized or _last.get(stage) is None:
        raise RuntimeError("no %s: configure(%s) and set_voxel_positions have not run" % (what, how))
    return _last[stage]


def hull_ops():
    """The stats of the last set_voxel_positions call's set operations (configure(hull_subtract=..., hull_clip=...)): a dict
    with "subtract" and / or "clip", each the dict of CarveEngine.combine_hull."""
    return _last_result("hull_ops", "hull operations", "hull_subtract=... or hull_clip=...")


def motion():
    """The motion field of the last set_voxel_positions call's hull against the previous frame's (configure(motion_block=b)):
    stats, the dict of CarveEngine.hull_motion; rows, the dict of CarveEngine.fetch_motion (block, ijk, d, cost, cost0, count_a,
    count_b, ties, flags); description, the dict of voxcarve.motion.describe (centre_mm, velocity_mm, speed_mm, median_mm).  The
    first frame of a session has no previous hull and so no field."""
    return _last_result("motion", "motion field", "motion_block=b")


def skeleton():
    """The skeleton of the last set_voxel_positions call's hull (configure(skeleton=...)): stats, the dict of
    CarveEngine.thin_hull; skeleton, the dict of CarveEngine.fetch_skeleton (voxel, record, degree, index); description, the
    dict of voxcarve.skeleton.describe (positions_mm, edges, edge_mm, length_mm, endpoints, junctions)."""
    return _last_result("skeleton", "skeleton", "skeleton=...")


def shell():
    """The stats of the last set_voxel_positions call's shell (configure(output="shell")): the dict of CarveEngine.hull_shell
    (survivors, cells_on, shell, faces, level, cube_scale, dims, shell_ms)."""
    return _last_result("shell", "shell", "output=\"shell\"")


def measurements():
    """The measurements of the last set_voxel_positions call's hull (configure(measure=...)): the dict of
    CarveEngine.measure_hull (survivors, groups, measured, unlabelled, measure_ms) with source; integers: the dict of
    CarveEngine.fetch_measure; world: the dict of voxcarve.measure.describe (volume_mm3, area_mm2 -- the voxel boundary's, which
    overstates a smooth surface --, centroid_mm, covariance_mm2, std_mm, axes, lean_deg, height_mm, top_mm, mean_rgb); profile:
    u64 [G, nz, 3] with measure_profile=True; and, with measure="clusters", velocity_mm: float64 [K, 3], each figure's centroid
    minus the previous frame's (None on the first frame; NaN rows for a figure that is empty in either)."""
    return _last_result("measure", "measurements", "measure=...")


def temporal():
    """The stats of the last set_voxel_positions call's vote over the last frames' hulls (configure(temporal_window=T)): the dict
    of CarveEngine.temporal_filter (with configure(temporal_motion=...) the longer one of the motion-compensated vote)."""
    return _last_result("temporal", "temporal vote", "temporal_window=T")


def extremities():
    """The extremities of the last set_voxel_positions call's hull (configure(extremities=K)): the dict of
    CarveEngine.hull_geodesic (survivors, seeds, reached, unreached, max_d, extremities, ...) with extrema: the dict of
    CarveEngine.fetch_extrema (label, voxel, record, d, d_mm, index, world_mm, in the order they were picked) and paths: the list
    of CarveEngine.stick_figure (world mm, one per extremity)."""
    return _last_result("extremities", "extremities", "extremities=K")


def clusters():
    """The split of the last set_voxel_positions call's hull into figures (configure(clusters=K)): the dict of
    CarveEngine.cluster_hull (survivors, columns, weight, iterations, converged, q, clusters_ms, k, centres_mm) with figures: the
    dict of CarveEngine.fetch_clusters (per figure centre_um, centre_mm, voxels, weight, columns, lo, hi), histograms u32
    [K, 512] and identity: the permutation voxcarve.clusters.match finds between the first frame's colour signatures and this
    frame's (identity[k] = the label that looks like the first frame's figure k; None above 8 figures)."""
    return _last_result("clusters", "clusters", "clusters=K")


def voxels_status():
    """Dense ON/OFF volume of the last set_voxel_positions call, shaped (width, height*2, depth) exactly as the
    reference builds it for voxel_reconstruction.plot_marching_cubes (assignment.py:143-146: the list of
    statuses in lookup-table order, reshaped): feed it to skimage.measure.marching_cubes as the reference does.
    The bits come straight off the device (vc_fetch_occupancy), no pass over Python dicts."""
    if _engine is None or not initialized:
        raise RuntimeError("set_voxel_positions has not run")
    nx, ny, nz = _engine.grid
    return _engine.fetch_occupancy().reshape(nx, ny, nz)


def _ensure_normals():
    if not _engine.normals_valid():
        _engine.hull_normals(_settings["normal_radius_mm"])


def render_views(views=None, width=None, height=None, shade=None, smooth=False, ambient=64, textured=False, texture_steps=8,
                 lit=False, light=None, floor="auto"):
    """Images of the hull of the last set_voxel_positions call, after whatever configure(...) asked for (component filter,
    photo carve, colouring), ray-cast on the device (CarveEngine.render): views = a list of camera.Camera (default: the
    calibrated cameras), width x height pixels (default: the mask size).  Returns the dict of CarveEngine.render: rgb
    [V, H, W, 3], depth, index, face and stats.  smooth=True shades every hit by the hull's surface normal under a headlight
    per view instead of the six face brightnesses of `shade` (CarveEngine.render_shaded: rgb is the shaded image, rgb_flat the
    unshaded one; ambient 0..255 is the brightness of a surface that faces away).  textured=True colours every hit from the
    frame's camera images instead of its voxel, after texture_steps bisection steps along the ray against the silhouettes
    (CarveEngine.render_textured: rgb is the textured image, rgb_voxels the render's own, depth the refined one); it needs
    configure(color_mode="visible"), whose depth maps say which cameras see a point, and excludes smooth and shade.
    lit=True adds cast shadows, ambient occlusion and a floor (CarveEngine.render_lit: rgb is the lit image, rgb_flat the
    render's own, with kind, shadow and ao per pixel): light = (x, y, z, w), None = a point light above the first view's
    camera; floor = None, "auto" or a dict (CarveEngine.light_render); smooth=True lights by the normals.  It excludes textured
    and shade."""
    if _engine is None or not initialized or _sized is None:
        raise RuntimeError("set_voxel_positions has not run")
    H, W = _engine.image_size
    views = _cameras if views is None else views
    H, W = H if height is None else height, W if width is None else width
    if lit:
        if textured:
            raise ValueError("render_views: lit=True lights the voxel render; textured=True takes its colours from the camera images")
        if shade is not None:
            raise ValueError("render_views: shade is the flat render's; lit=True shades by the light")
        if smooth:
            _ensure_normals()
        return _engine.render_lit(views, H, W, light=light, ambient=ambient, smooth=smooth, floor=floor)
    if textured:
        if smooth or shade is not None:
            raise ValueError("render_views: textured=True takes its colours from the camera images; smooth and shade are the voxel render's")
        if _settings["color_mode"] != "visible":
            raise ValueError("render_views: textured=True needs configure(color_mode=\"visible\")")
        return _engine.render_textured(views, H, W, slot=0, steps=texture_steps)
    if smooth:
        if shade is not None:
            raise ValueError("render_views: shade is the flat render's; smooth=True shades by the normals")
        _ensure_normals()
        return _engine.render_shaded(views, H, W, ambient=ambient)
    return _engine.render(views, H, W, shade=shade)


def surface_mesh(refine_steps=8, normals=False):
    """Surface mesh of the hull of the last set_voxel_positions call, after whatever configure(...) asked for (component filter,
    photo carve, colouring), refined against the silhouettes on the device (CarveEngine.surface_mesh): world millimetres,
    outward faces, the voxels' colours.  Returns the dict of CarveEngine.surface_mesh: verts [V, 3] float64, faces [F, 3], rgb
    [V, 3], refined [V] and stats; voxel_reconstruction.write_ply writes it out.  normals=True adds "normals": float64 [V, 3]
    unit vectors, the surface normal of the voxel each vertex takes its colour from (zero where that voxel has none)."""
    if _engine is None or not initialized or _sized is None:
        raise RuntimeError("set_voxel_positions has not run")
    mesh = _engine.surface_mesh(refine_steps)
    if normals:
        _ensure_normals()
        v = _engine.surface_normals()[:, :3].astype(np.float64)
        l = np.sqrt((v * v).sum(axis=1))
        mesh["normals"] = v / np.where(l == 0.0, 1.0, l)[:, None]
    return mesh
