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
_settings = {"data_path": "data", "num_cameras": 4, "device": 0, "mode": "fused",
             "views_threshold": 4, "color_camera": COLOR_CAMERA_INDEX, "bounds": DEFAULT_BOUNDS,
             "color_mode": "camera", "hull": "visual", "photo_var_threshold": 1200,
             "min_component_voxels": 0, "keep_components": 0, "component_connectivity": 26, "footprint": "centre",
             "hull_open_mm": 0.0, "hull_border": "open", "hull_close_mm": 0.0, "normal_radius_mm": None,
             "clusters": 0, "cluster_min_column": 1, "cluster_paint": False,
             "extremities": 0, "geodesic_seeds": "floor", "geodesic_paint": None,
             "temporal_window": 0, "temporal_keep": None, "temporal_keep_off": None,
             "hull_subtract": None, "hull_clip": None,
             "measure": None, "measure_profile": False,
             "skeleton": None, "skeleton_anchors": None,
             "output": "all", "output_level": 0}
_shell_state = {"last": None}
OUTPUTS = ("all", "shell")
_skeleton_state = {"last": None}
SKELETONS = (None, "curve", "point")
_measure_state = {"last": None, "centroids_mm": None}
MEASURES = (None, "all", "clusters", "geodesic", "components")
_temporal_state = {"last": None}
_hull_ops_state = {"last": None}
HULL_SUBTRACT_REG, HULL_CLIP_REG = 3, 2      # the registers of CarveEngine that hold the two operands
_cluster_state = {"centres_mm": None, "references": None, "last": None}
_geodesic_state = {"last": None}
GEODESIC_PAINTS = (None, "labels", "distance")
COLOR_MODES = ("camera", "visible")
HULLS = ("visual", "photo")


def configure(frame_source=None, **settings):
    """Install a frame source / override data_path, num_cameras, device, mode, ...; resets state.
    color_mode: "camera" (default) colours every survivor from the colour camera, as the reference does (assignment.py:133);
    "visible" recolours the surface voxels from every camera that sees them (CarveEngine.color_visible).
    hull: "visual" (default) is the carve's visual hull; "photo" refines it by photo-consistency after every carve
    (CarveEngine.photo_carve with var_threshold=photo_var_threshold), which needs every camera's image and colours the result as
    "visible" does; voxels_status() then describes the photo hull.
    min_component_voxels, keep_components: when either is non-zero, every carve is followed by CarveEngine.filter_components
    (connectivity=component_connectivity), before any colouring or photo carve: components smaller than min_component_voxels,
    or beyond the keep_components largest, leave the hull (floating specks of mask noise); voxels_status() describes what is
    kept.  0 and 0 (the default) keep every survivor.
    footprint: "centre" (default) asks, as the reference does, whether the pixel under a voxel's centre is foreground; "any",
    "all" and ("cover", q) test the pixel box the voxel's whole cell projects to (CarveEngine.carve(footprint=...)): "any" keeps
    what is thinner than a voxel (the outer hull), "all" gives the inner hull.
    hull_open_mm, hull_border: when hull_open_mm > 0, every carve is followed by CarveEngine.open_hull(hull_open_mm,
    border=hull_border), before the component filter, any photo carve and any colouring: what is thinner than a ball of that
    radius in world millimetres leaves the hull (spurs, fins and specks of mask noise, attached to the figure or not);
    voxels_status() describes what is kept.  0 (the default) keeps every survivor.
    hull_close_mm: when > 0, every carve is followed by CarveEngine.close_hull(hull_close_mm), before hull_open_mm, the component
    filter, any photo carve and any colouring (close, then open, is the usual clean-up order): tunnels and dents narrower than a
    ball of that radius in world millimetres are filled -- what a hole in one camera's mask carves through the figure; the added
    voxels are coloured from the colour camera.  voxels_status() describes the closed hull.  0 (the default) adds nothing.
    normal_radius_mm: the radius of the ball that render_views(smooth=True) and surface_mesh(normals=True) estimate the hull's
    surface normals from (CarveEngine.hull_normals); None (the default) is 3 x the largest grid step.
    clusters, cluster_min_column, cluster_paint: when clusters = K > 0 (at most 16), every frame ends -- after all hull passes
    and the colouring -- with CarveEngine.cluster_hull(K, min_column=cluster_min_column): the hull split into K figures on the
    floor plane.  The first frame seeds itself and keeps its colour signatures as the references; every later frame starts from
    the previous frame's centres, so label k stays the same figure while the figures keep apart.  clusters() returns the last
    frame's split.  cluster_paint=True paints every voxel in its figure's colour (voxcarve.clusters.PALETTE) before the
    positions and colours are returned.  0 (the default) runs nothing.
    extremities, geodesic_seeds, geodesic_paint: when extremities = K > 0 (at most 32), every frame ends -- after all hull passes,
    the colouring and the clusters -- with CarveEngine.hull_geodesic(seeds=geodesic_seeds, extrema=K, paths=True): geodesic
    distances through the hull from the seed set ("floor", the default, "top", or an array of voxel indices) and the K
    extremities by farthest-point selection (head, hands, feet).  extremities() returns the last frame's.  geodesic_paint =
    "labels" | "distance" paints every voxel by its region or its distance (CarveEngine.paint_geodesic) before the positions and
    colours are returned; None (the default) leaves the colours.  0 (the default) runs nothing.
    temporal_window, temporal_keep, temporal_keep_off: when temporal_window = T > 0 (at most 15), every carve is followed --
    before hull_close_mm and everything else -- by CarveEngine.temporal_filter(T, temporal_keep, temporal_keep_off): the hull
    becomes the vote of the last T frames' hulls (keep defaults to the majority, keep_off to keep), which takes the frame-to-frame
    flicker of mask noise out and lags a moving figure by about T / 2 frames.  temporal() returns the last frame's stats.
    0 (the default) runs nothing.
    hull_subtract, hull_clip: each a path to a file of CarveEngine.save_hull, a hull as an array (bool [n], ascending uint32
    indices or uint64 records: voxcarve.hullio.as_operand), or None.  The operand is uploaded once, to registers 3 and 2 of the
    engine, and every carve is followed -- before temporal_window and everything else -- by CarveEngine.combine_hull("andnot", 3)
    (the static scene leaves the hull) and then CarveEngine.combine_hull("and", 2) (the hull is clipped to a region of
    interest).  hull_ops() returns the last frame's stats.  None (the default) runs nothing.
    measure, measure_profile: when measure = "all" | "clusters" | "geodesic" | "components", every frame ends -- after the
    clusters and the extremities -- with CarveEngine.measure_hull(labels=measure, profile=measure_profile): the hull's figures
    measured on the device, per group of that source (the whole hull; the figures of clusters=K; the regions of extremities=K;
    the connected components, ranked by size, of the component filter -- which runs once more on its own output when it removed
    something, so that its labels describe the hull).  measurements() returns the last frame's.  A source whose own pass is not
    configured is refused.  None (the default) runs nothing.
    skeleton, skeleton_anchors: when skeleton = "curve" | "point", every frame ends -- after the frame's geodesic pass -- with
    CarveEngine.thin_hull(skeleton, anchors=skeleton_anchors): the hull thinned to a centred, one-voxel-wide skeleton with its
    topology, on the device; the hull itself stays.  skeleton_anchors = "extrema" pins the skeleton at the floor contact and the
    extremities of extremities=K, which turns a noisy curve skeleton into a stick figure; it is refused without extremities=K.
    skeleton() returns the last frame's.  None (the default) runs nothing.
    output, output_level: "all" (the default) returns every survivor, as the reference does.  "shell" ends every frame -- after
    every other pass and all painting -- with CarveEngine.hull_shell(output_level) and returns the arrays of
    CarveEngine.fetch_shell_viewer(), made on the device: only the voxels with an exposed face, which is everything an opaque
    cube viewer can show (at level 0 the same rows the full arrays hold for those voxels).  output_level = L in 1..6 lists the
    cells of a grid 2^L times coarser instead, with averaged colours: the viewer must draw each cube shell()["cube_scale"] times
    as large.  shell() returns the last frame's stats.  voxels_status() is unaffected.  output_level needs output="shell"."""
    global _source, _engine, initialized, frame_count
    unknown = set(settings) - set(_settings)
    if unknown:
        raise TypeError("unknown settings: %s" % sorted(unknown))
    if settings.get("color_mode", _settings["color_mode"]) not in COLOR_MODES:
        raise ValueError("color_mode %r, expected one of %s" % (settings["color_mode"], COLOR_MODES))
    if settings.get("hull", _settings["hull"]) not in HULLS:
        raise ValueError("hull %r, expected one of %s" % (settings["hull"], HULLS))
    footprint_rule(settings.get("footprint", _settings["footprint"]))          # raises ValueError on anything else
    CarveEngine.radius_r2(settings.get("hull_open_mm", _settings["hull_open_mm"]))   # ... on a negative or non-finite radius
    CarveEngine._dist_flags(settings.get("hull_border", _settings["hull_border"]))
    CarveEngine.radius_r2(settings.get("hull_close_mm", _settings["hull_close_mm"]))
    if settings.get("normal_radius_mm", _settings["normal_radius_mm"]) is not None:
        CarveEngine.radius_r2(settings.get("normal_radius_mm", _settings["normal_radius_mm"]))
    k = settings.get("clusters", _settings["clusters"])
    if not isinstance(k, (int, np.integer)) or not 0 <= k <= 16:
        raise ValueError("clusters %r, expected an integer in 0..16" % (k,))
    if int(settings.get("cluster_min_column", _settings["cluster_min_column"])) < 0:
        raise ValueError("cluster_min_column %r is negative" % (settings["cluster_min_column"],))
    k = settings.get("extremities", _settings["extremities"])
    if not isinstance(k, (int, np.integer)) or not 0 <= k <= 32:
        raise ValueError("extremities %r, expected an integer in 0..32" % (k,))
    if settings.get("geodesic_paint", _settings["geodesic_paint"]) not in GEODESIC_PAINTS:
        raise ValueError("geodesic_paint %r, expected one of %s" % (settings["geodesic_paint"], GEODESIC_PAINTS))
    g = settings.get("geodesic_seeds", _settings["geodesic_seeds"])
    if isinstance(g, str) and g not in ("floor", "top"):
        raise ValueError("geodesic_seeds %r, expected \"floor\", \"top\" or an array of voxel indices" % (g,))
    t = settings.get("temporal_window", _settings["temporal_window"])
    if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0:
        raise ValueError("temporal_window %r, expected an integer in 0..15" % (t,))
    CarveEngine.temporal_thresholds(t if t > 0 else 1, settings.get("temporal_keep", _settings["temporal_keep"]) if t > 0 else None,
                                    settings.get("temporal_keep_off", _settings["temporal_keep_off"]) if t > 0 else None)
    for name in ("hull_subtract", "hull_clip"):
        h = settings.get(name, _settings[name])
        if h is not None and not isinstance(h, (str, os.PathLike, np.ndarray)):
            raise ValueError("%s %r, expected a path, an array or None" % (name, h))
    m = settings.get("measure", _settings["measure"])
    if m not in MEASURES:
        raise ValueError("measure %r, expected one of %s" % (m, MEASURES))
    if not isinstance(settings.get("measure_profile", _settings["measure_profile"]), (bool, np.bool_)):
        raise ValueError("measure_profile %r, expected True or False" % (settings["measure_profile"],))
    merged = dict(_settings, **settings)
    if m == "clusters" and not merged["clusters"] > 0:
        raise ValueError('measure="clusters" needs clusters=K')
    if m == "geodesic" and not merged["extremities"] > 0:
        raise ValueError('measure="geodesic" needs extremities=K')
    if m == "components" and not (merged["min_component_voxels"] or merged["keep_components"]):
        raise ValueError('measure="components" needs the component filter: min_component_voxels or keep_components')
    if merged["skeleton"] not in SKELETONS:
        raise ValueError("skeleton %r, expected one of %s" % (merged["skeleton"], SKELETONS))
    if merged["skeleton_anchors"] not in (None, "extrema"):
        raise ValueError('skeleton_anchors %r, expected None or "extrema"' % (merged["skeleton_anchors"],))
    if merged["skeleton"] is not None and merged["skeleton_anchors"] == "extrema" and not merged["extremities"] > 0:
        raise ValueError('skeleton_anchors="extrema" needs extremities=K')
    if merged["output"] not in OUTPUTS:
        raise ValueError("output %r, expected one of %s" % (merged["output"], OUTPUTS))
    lv = merged["output_level"]
    if isinstance(lv, bool) or not isinstance(lv, (int, np.integer)) or not 0 <= lv <= 6:
        raise ValueError("output_level %r, expected an integer in 0..6" % (lv,))
    if lv != 0 and merged["output"] != "shell":
        raise ValueError('output_level=%d needs output="shell"' % lv)
    _settings.update(settings)
    _shell_state.update(last=None)
    _measure_state.update(last=None, centroids_mm=None)
    _skeleton_state.update(last=None)
    _temporal_state.update(last=None)
    _hull_ops_state.update(last=None)
    _cluster_state.update(centres_mm=None, references=None, last=None)
    _geodesic_state.update(last=None)
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
    global initialized, frame_count, _engine, _source
    if not initialized:
        if _source is None:
            _source = ReferenceVideoSource(_settings["data_path"], _settings["num_cameras"])
        _engine = CarveEngine(_settings["device"])
        _engine.set_grid(width, height * 2, depth, _settings["bounds"])        # assignment.py:85
        _engine._cameras = load_cameras(_settings["data_path"], _settings["num_cameras"])   # :88
        _engine._sized = None
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
    if _engine._sized != (H, W):
        _engine.set_cameras(_engine._cameras, H, W)
        if getattr(_source, "post_on_device", False):
            n = _settings["num_cameras"]
            _engine.set_mask_postfilter([cam_bg_model_params[c][4] for c in range(n)],
                                        [cam_bg_model_params[c][5] for c in range(n)])
        if _settings["mode"] == "lut":
            _engine.build_lut()
        _engine._sized = (H, W)
        _engine._operands = False                                               # (new cameras empty the registers)
    if not getattr(_engine, "_operands", False):
        _upload_operands()
    cc = _settings["color_camera"]
    photo = _settings["hull"] == "photo"
    visible = _settings["color_mode"] == "visible" or photo
    if device_source:
        if not _source.fill_slot(_engine, 0):                                   # masks and images made on the device
            return [], []
        frame_count += 1
    else:
        _engine.upload_masks(masks, slot=0)
        for c in (range(len(frames)) if visible else (cc,)):                   # "visible": every camera's image
            _engine.upload_frame(c, frames[c], slot=0)
    _engine.carve(slot=0, min_views=_settings["views_threshold"], color_cam=cc, mode=_settings["mode"],
                  footprint=_settings["footprint"])
    if _settings["hull_subtract"] is not None or _settings["hull_clip"] is not None:
        ops = {}
        if _settings["hull_subtract"] is not None:
            ops["subtract"] = _engine.combine_hull("andnot", HULL_SUBTRACT_REG)
        if _settings["hull_clip"] is not None:
            ops["clip"] = _engine.combine_hull("and", HULL_CLIP_REG)
        _hull_ops_state["last"] = ops
    if _settings["temporal_window"] > 0:
        _temporal_state["last"] = _engine.temporal_filter(_settings["temporal_window"], _settings["temporal_keep"],
                                                          _settings["temporal_keep_off"])
    if _settings["hull_close_mm"] > 0:
        _engine.close_hull(_settings["hull_close_mm"])
    if _settings["hull_open_mm"] > 0:
        _engine.open_hull(_settings["hull_open_mm"], border=_settings["hull_border"])
    if _settings["min_component_voxels"] or _settings["keep_components"]:
        _engine.filter_components(connectivity=_settings["component_connectivity"], min_voxels=_settings["min_component_voxels"],
                                  keep_largest=_settings["keep_components"])
    if photo:
        _engine.photo_carve(slot=0, var_threshold=_settings["photo_var_threshold"])
    elif visible:
        _engine.color_visible(slot=0)
    if _settings["clusters"] > 0:
        _cluster_frame()
    if _settings["extremities"] > 0:
        _geodesic_frame()
    if _settings["measure"] is not None:
        _measure_frame()
    if _settings["skeleton"] is not None:
        _skeleton_frame()
    if _settings["output"] == "shell":
        _shell_state["last"] = _engine.hull_shell(int(_settings["output_level"]))
        return _engine.fetch_shell_viewer()
    idx, rgb, _ = _engine.fetch()
    keys = voxel_keys(idx, _engine.grid, _engine.axes())
    return viewer_positions(keys), viewer_colors(rgb)


def _upload_operands():
    """The operands of hull_subtract and hull_clip into their registers (see configure): once per camera set."""
    for name, reg in (("hull_subtract", HULL_SUBTRACT_REG), ("hull_clip", HULL_CLIP_REG)):
        h = _settings[name]
        if h is None:
            continue
        if isinstance(h, (str, os.PathLike)):
            _engine.load_hull(h, reg)
        else:
            _engine.upload_hull(h, reg)
    _engine._operands = True


def hull_ops():
    """The stats of the last set_voxel_positions call's set operations (configure(hull_subtract=..., hull_clip=...)): a dict
    with "subtract" and / or "clip", each the dict of CarveEngine.combine_hull."""
    if _engine is None or not initialized or _hull_ops_state["last"] is None:
        raise RuntimeError("no hull operations: configure(hull_subtract=... or hull_clip=...) and set_voxel_positions have not run")
    return _hull_ops_state["last"]


def _cluster_frame():
    """The frame's split into figures, warm-started from the previous frame's centres (see configure)."""
    from .clusters import MATCH_MAX_K, match
    K = int(_settings["clusters"])
    out = _engine.cluster_hull(K, min_column=int(_settings["cluster_min_column"]), init_mm=_cluster_state["centres_mm"])
    out["figures"] = _engine.fetch_clusters()
    out["histograms"] = _engine.fetch_cluster_histograms()
    if _cluster_state["references"] is None:
        _cluster_state["references"] = out["histograms"].copy()
    out["identity"] = match(_cluster_state["references"], out["histograms"]) if K <= MATCH_MAX_K else None
    _cluster_state["centres_mm"] = out["centres_mm"]
    _cluster_state["last"] = out
    if _settings["cluster_paint"]:
        _engine.paint_clusters()


def _geodesic_frame():
    """The frame's geodesic distances and extremities (see configure)."""
    out = _engine.hull_geodesic(seeds=_settings["geodesic_seeds"], extrema=int(_settings["extremities"]), paths=True)
    out["extrema"] = _engine.fetch_extrema()
    out["paths"] = _engine.stick_figure()
    _geodesic_state["last"] = out
    if _settings["geodesic_paint"] is not None:
        _engine.paint_geodesic(_settings["geodesic_paint"])


def _skeleton_frame():
    """The frame's skeleton (see configure)."""
    from . import skeleton as sk
    stats = _engine.thin_hull(_settings["skeleton"], anchors=_settings["skeleton_anchors"])
    rows = _engine.fetch_skeleton()
    _skeleton_state["last"] = {"stats": stats, "skeleton": rows, "description": sk.describe(rows, _engine.grid, _engine.bounds)}


def skeleton():
    """The skeleton of the last set_voxel_positions call's hull (configure(skeleton=...)): stats, the dict of
    CarveEngine.thin_hull; skeleton, the dict of CarveEngine.fetch_skeleton (voxel, record, degree, index); description, the
    dict of voxcarve.skeleton.describe (positions_mm, edges, edge_mm, length_mm, endpoints, junctions)."""
    if _engine is None or not initialized or _skeleton_state["last"] is None:
        raise RuntimeError("no skeleton: configure(skeleton=...) and set_voxel_positions have not run")
    return _skeleton_state["last"]


def shell():
    """The stats of the last set_voxel_positions call's shell (configure(output="shell")): the dict of CarveEngine.hull_shell
    (survivors, cells_on, shell, faces, level, cube_scale, dims, shell_ms)."""
    if _engine is None or not initialized or _shell_state["last"] is None:
        raise RuntimeError("no shell: configure(output=\"shell\") and set_voxel_positions have not run")
    return _shell_state["last"]


def _measure_frame():
    """The frame's measurements (see configure); with "clusters", label k is the same figure from frame to frame, so the
    centroid's step since the previous frame is the figure's displacement."""
    from . import measure
    source = _settings["measure"]
    if source == "components":
        try:
            _engine.component_ranks()
        except ValueError:                                       # the filter removed something: label its output
            _engine.filter_components(connectivity=_settings["component_connectivity"])
    out = _engine.measure_hull(labels=source, profile=bool(_settings["measure_profile"]))
    out["source"] = source
    out["integers"] = _engine.fetch_measure()
    out["world"] = measure.describe(out["integers"], _engine.grid, _engine.bounds)
    if _settings["measure_profile"]:
        out["profile"] = _engine.fetch_measure_profile()
    if source == "clusters":
        c = out["world"]["centroid_mm"]
        prev = _measure_state["centroids_mm"]
        out["velocity_mm"] = None if prev is None or prev.shape != c.shape else c - prev
        _measure_state["centroids_mm"] = c.copy()
    _measure_state["last"] = out


def measurements():
    """The measurements of the last set_voxel_positions call's hull (configure(measure=...)): the dict of
    CarveEngine.measure_hull (survivors, groups, measured, unlabelled, measure_ms) with source; integers: the dict of
    CarveEngine.fetch_measure; world: the dict of voxcarve.measure.describe (volume_mm3, area_mm2 -- the voxel boundary's, which
    overstates a smooth surface --, centroid_mm, covariance_mm2, std_mm, axes, lean_deg, height_mm, top_mm, mean_rgb); profile:
    u64 [G, nz, 3] with measure_profile=True; and, with measure="clusters", velocity_mm: float64 [K, 3], each figure's centroid
    minus the previous frame's (None on the first frame; NaN rows for a figure that is empty in either)."""
    if _engine is None or not initialized or _measure_state["last"] is None:
        raise RuntimeError("no measurements: configure(measure=...) and set_voxel_positions have not run")
    return _measure_state["last"]


def temporal():
    """The stats of the last set_voxel_positions call's vote over the last frames' hulls (configure(temporal_window=T)): the dict
    of CarveEngine.temporal_filter."""
    if _engine is None or not initialized or _temporal_state["last"] is None:
        raise RuntimeError("no temporal vote: configure(temporal_window=T) and set_voxel_positions have not run")
    return _temporal_state["last"]


def extremities():
    """The extremities of the last set_voxel_positions call's hull (configure(extremities=K)): the dict of
    CarveEngine.hull_geodesic (survivors, seeds, reached, unreached, max_d, extremities, ...) with extrema: the dict of
    CarveEngine.fetch_extrema (label, voxel, record, d, d_mm, index, world_mm, in the order they were picked) and paths: the list
    of CarveEngine.stick_figure (world mm, one per extremity)."""
    if _engine is None or not initialized or _geodesic_state["last"] is None:
        raise RuntimeError("no extremities: configure(extremities=K) and set_voxel_positions have not run")
    return _geodesic_state["last"]


def clusters():
    """The split of the last set_voxel_positions call's hull into figures (configure(clusters=K)): the dict of
    CarveEngine.cluster_hull (survivors, columns, weight, iterations, converged, q, clusters_ms, k, centres_mm) with figures: the
    dict of CarveEngine.fetch_clusters (per figure centre_um, centre_mm, voxels, weight, columns, lo, hi), histograms u32
    [K, 512] and identity: the permutation voxcarve.clusters.match finds between the first frame's colour signatures and this
    frame's (identity[k] = the label that looks like the first frame's figure k; None above 8 figures)."""
    if _engine is None or not initialized or _cluster_state["last"] is None:
        raise RuntimeError("no clusters: configure(clusters=K) and set_voxel_positions have not run")
    return _cluster_state["last"]


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


def render_views(views=None, width=None, height=None, shade=None, smooth=False, ambient=64, textured=False, texture_steps=8):
    """Images of the hull of the last set_voxel_positions call, after whatever configure(...) asked for (component filter,
    photo carve, colouring), ray-cast on the device (CarveEngine.render): views = a list of camera.Camera (default: the
    calibrated cameras), width x height pixels (default: the mask size).  Returns the dict of CarveEngine.render: rgb
    [V, H, W, 3], depth, index, face and stats.  smooth=True shades every hit by the hull's surface normal under a headlight
    per view instead of the six face brightnesses of `shade` (CarveEngine.render_shaded: rgb is the shaded image, rgb_flat the
    unshaded one; ambient 0..255 is the brightness of a surface that faces away).  textured=True colours every hit from the
    frame's camera images instead of its voxel, after texture_steps bisection steps along the ray against the silhouettes
    (CarveEngine.render_textured: rgb is the textured image, rgb_voxels the render's own, depth the refined one); it needs
    configure(color_mode="visible"), whose depth maps say which cameras see a point, and excludes smooth and shade."""
    if _engine is None or not initialized or _engine._sized is None:
        raise RuntimeError("set_voxel_positions has not run")
    H, W = _engine.image_size
    views = _engine._cameras if views is None else views
    H, W = H if height is None else height, W if width is None else width
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
    if _engine is None or not initialized or _engine._sized is None:
        raise RuntimeError("set_voxel_positions has not run")
    mesh = _engine.surface_mesh(refine_steps)
    if normals:
        _ensure_normals()
        v = _engine.surface_normals()[:, :3].astype(np.float64)
        l = np.sqrt((v * v).sum(axis=1))
        mesh["normals"] = v / np.where(l == 0.0, 1.0, l)[:, None]
    return mesh
